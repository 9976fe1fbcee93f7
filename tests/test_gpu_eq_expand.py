"""GPU tests of the eq-indicator expansion (bn_eq_expand_device / _host / _device_split). The
reference is the level recursion of include/binius_ntt_amd.h written out over the oracle's products
(hi = A[y]*r_k, lo = A[y] ^ hi; usable up to n = 13); the larger sizes are pinned by the tensor
structure, the sum and multilinear-extension identities, a zerocheck run through the sumcheck
prover and the FRI fold's end-to-end identity. Every comparison is bit-exact."""
import functools

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu

ONE = np.array([1, 0, 0, 0], np.uint32)
# every case takes a prefix or a slice of these challenges
CH = np.random.default_rng(0xE9E9).integers(0, 2**32, size=(30, 4), dtype=np.uint64).astype(np.uint32)
CH.setflags(write=False)
SCALE = np.array([0x5CA1E001, 0x0BADF00D, 0x13579BDF, 0xFEDCBA98], np.uint32)
SCALE.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _ref13(scaled):
    """The recursion at n = 13 on CH[:13], once per scale; every level of it is the table of a smaller n."""
    tables = [[O._from_words(SCALE if scaled else ONE)]]
    for k in range(13):
        r = O._from_words(CH[k])
        nxt = []
        for a in tables[-1]:
            hi = O.mul128(a, r)
            nxt += [a ^ hi, hi]
        tables.append(nxt)
    out = []
    for t in tables:
        a = np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(4)] for v in t], dtype=np.uint32)
        a.setflags(write=False)
        out.append(a)
    return out


def _ref(n, scaled=False):
    return _ref13(scaled)[n]


def _expand(n, ch, dev, scale=None, bitsliced=False, max_levels=0, stream=None, fill=0x5A):
    """eq_expand into a fresh device tensor pre-filled with a pattern; returns the tensor."""
    import torch
    out = torch.full((4 << n,), fill * 0x01010101, dtype=torch.int32, device=dev)
    B.eq_expand(n, ch, out, scale=scale, bitsliced=bitsliced, stream=stream, max_levels=max_levels)
    return out


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4)


def _xor_sum(a):
    return np.bitwise_xor.reduce(a.reshape(-1, 4), axis=0)


# n < 3 has fewer levels than the register stage; 12 and 13 sit around one tile
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 12, 13])
def test_compact_default_split(n, dev):
    T = B.eq_expand_passes(30)[-1]
    assert T == 12  # the sizes above are chosen around it
    assert np.array_equal(_np(_expand(n, CH[:n], dev)), _ref(n))


# 2 + 3 + 3, three full passes, four passes (1 + 3 + 3 + 3), uneven first passes
@pytest.mark.parametrize("n,max_levels", [(8, 3), (9, 3), (10, 3), (11, 4), (13, 5)])
def test_forced_splits(n, max_levels, dev):
    assert len(B.eq_expand_passes(n, max_levels)) >= 3
    assert np.array_equal(_np(_expand(n, CH[:n], dev, max_levels=max_levels)), _ref(n))


@pytest.mark.parametrize("n", [7, 13])
def test_scale(n, dev):
    assert np.array_equal(_np(_expand(n, CH[:n], dev, scale=SCALE)), _ref(n, scaled=True))
    assert np.array_equal(_np(_expand(n, CH[:n], dev, scale=ONE)), _ref(n))


@pytest.mark.parametrize("n", [7, 13])
def test_scale_zero(n, dev):
    assert not _np(_expand(n, CH[:n], dev, scale=np.zeros(4, np.uint32))).any()


@pytest.mark.parametrize("pattern", [0, (1 << 13) - 1, 0b1011001110001])
def test_boolean_challenges_select_one_index(pattern, dev):
    n = 13
    ch = np.zeros((n, 4), np.uint32)
    ch[:, 0] = [(pattern >> (n - 1 - i)) & 1 for i in range(n)]  # challenge i pairs with index bit n-1-i
    want = np.zeros((1 << n, 4), np.uint32)
    want[pattern] = SCALE
    assert np.array_equal(_np(_expand(n, ch, dev, scale=SCALE)), want)


@pytest.mark.parametrize("n", [5, 6, 12, 13])
def test_bitsliced(n, dev):
    got = _np(_expand(n, CH[:n], dev, bitsliced=True)).reshape(-1)
    assert np.array_equal(got, O.bitslice128(_ref(n)))
    compact = _expand(n, CH[:n], dev)
    B.bitslice(compact)
    assert np.array_equal(got, _np(compact).reshape(-1))


@pytest.mark.parametrize("n", [16, 20, 25])
def test_large_sizes_are_the_tensor_product_of_small_ones(n, dev):
    import torch
    T = B.eq_expand_passes(30)[-1]
    if n == 25:
        n = 2 * T + 1  # three passes with a one-level first
    if n > 26:
        pytest.skip("2T + 1 = %d: above 2^26 elements" % n)
    k = 13  # E_n = E_hi (x) E_lo with both at sizes test_compact_default_split covers
    assert n - k in (3, 7, 12)
    e_n = _expand(n, CH[:n], dev)
    e_hi = _expand(n - k, CH[:n - k], dev).view(-1, 4)
    e_lo = _expand(k, CH[n - k:n], dev).view(-1, 4)
    a = e_hi.repeat_interleave(1 << k, dim=0).reshape(-1)
    b = e_lo.repeat(1 << (n - k), 1).reshape(-1)
    B.gf128_mul(a, b, a)
    torch.cuda.synchronize()
    assert torch.equal(e_n, a)
    assert int(e_n.view(-1, 4)[-1].abs().sum().item()) != 0


@pytest.mark.parametrize("n", [16, 20])
def test_elements_sum_to_the_scale(n, dev):
    assert np.array_equal(_xor_sum(_np(_expand(n, CH[:n], dev, scale=SCALE))), SCALE)
    assert np.array_equal(_xor_sum(_np(_expand(n, CH[30 - n:], dev))), ONE)


def test_multilinear_extension_identity(dev):
    import torch
    n = 16
    f = O.fill128(0xF00D, 0x0DDBA110, 1 << n)
    d_f = torch.from_numpy(f.reshape(-1).view(np.int32)).to(dev)
    e = _expand(n, CH[:n], dev)
    B.gf128_mul(d_f, e, e)
    assert np.array_equal(_xor_sum(_np(e)), B.evaluate_multilinear_composition(f, n, 1, False, CH[:n]))


def test_zerocheck_flow(dev):
    """Sumcheck over [E_r, a, b] with E_r bitsliced from the call: round 0's sum is the multilinear
    extension of a*b at r, the last claim eq(r, rho) * a(rho) * b(rho), both against the oracle."""
    import torch
    n = 10
    r = CH[:n]
    a = O.fill128(0xAAAA, 0x0A000000, 1 << n)
    b = O.fill128(0xBBBB, 0x0B000000, 1 << n)
    rho = O.fill128(0xCCCC, 0x0C000000, n)
    cols = torch.empty(3 * (4 << n), dtype=torch.int32, device=dev)
    B.eq_expand(n, r, cols[:4 << n], bitsliced=True)
    ab_bs = O.bitslice128(np.concatenate([a.reshape(-1), b.reshape(-1)]))
    cols[4 << n:] = torch.from_numpy(ab_bs.view(np.int32)).to(dev)
    sc = B.Sumcheck(n, 3, True, cols)
    ab = np.array([O._to_words(O.mul128(O._from_words(x), O._from_words(y))) for x, y in zip(a, b)], dtype=np.uint32)
    claim = None
    for rnd in range(n):
        s, p = sc.this_round_messages()
        if rnd == 0:
            assert np.array_equal(s, O.multilinear_composition(ab, n, 1, r))
        else:
            assert np.array_equal(s, claim)
        assert np.array_equal(s, p[0] ^ p[1])
        claim = B.evaluate_univariate_given_points(rho[rnd], p)
        sc.move_to_next_round(rho[rnd])
    s, _ = sc.this_round_messages()
    sc.close()
    assert np.array_equal(s, claim)
    fg = O.multilinear_composition(np.concatenate([a.reshape(-1), b.reshape(-1)]), n, 2, rho)
    want = O.mul128(O._from_words(B.eq_eval(r, rho)), O._from_words(fg))
    assert np.array_equal(s, O._to_words(want))


def test_fri_fold_identity(dev):
    """The codeword of x folded through all rounds is XOR_x x[x]*E[x] with the fold's challenges reversed."""
    import torch
    log_h, rate = 12, 1
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, rate, B.FanPaarTowerField(7)))
    x = O.fill128(0xDEADBEEF + log_h + rate, 0x5EED0000, 1 << log_h)
    ch = CH[5:5 + log_h]
    d_x = torch.from_numpy(x.reshape(-1).view(np.int32)).to(dev)
    cw = torch.empty(4 << (log_h + rate), dtype=torch.int32, device=dev)
    ntt.forward_device(d_x, cw)
    for at, k in ((0, 8), (8, 4)):
        nxt = torch.empty(cw.numel() >> k, dtype=torch.int32, device=dev)
        ntt.fri_fold_device(cw, nxt, at, ch[at:at + k])
        cw = nxt
    folded = _np(cw)
    assert folded.shape == (1 << rate, 4) and (folded == folded[0]).all()
    e = _expand(log_h, np.ascontiguousarray(ch[::-1]), dev)
    B.gf128_mul(d_x, e, e)
    assert np.array_equal(_xor_sum(_np(e)), folded[0])


def test_non_default_stream_and_back_to_back_calls(dev):
    import torch
    n = 13
    want_a, want_b = _np(_expand(n, CH[:n], dev)), _np(_expand(n, CH[10:10 + n], dev, scale=SCALE))
    out_a = torch.zeros(4 << n, dtype=torch.int32, device=dev)
    out_b = torch.zeros(4 << n, dtype=torch.int32, device=dev)
    busy = torch.zeros(1 << 26, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        for _ in range(4):  # work queued ahead of the calls
            busy.add_(1)
        B.eq_expand(n, CH[:n], out_a, stream=st)
        B.eq_expand(n, CH[10:10 + n], out_b, scale=SCALE, stream=st)
    st.synchronize()
    assert np.array_equal(_np(out_a), want_a)
    assert np.array_equal(_np(out_b), want_b)
    assert int(busy[0].item()) == 4


@pytest.mark.parametrize("n,bitsliced", [(0, False), (7, False), (13, True)])
def test_host_call_equals_device_call(n, bitsliced, dev):
    got = B.eq_expand_host(n, CH[:n], scale=SCALE, bitsliced=bitsliced)
    assert got.shape == (1 << n, 4)
    assert np.array_equal(got, _np(_expand(n, CH[:n], dev, scale=SCALE, bitsliced=bitsliced)))


def test_rejected_calls_leave_the_buffer_alone(dev):
    import torch
    n = 8
    out = torch.full((4 << n,), 0x11111111, dtype=torch.int32, device=dev)
    before = out.clone()
    T = B.eq_expand_passes(30)[-1]
    for ml in (1, 2, T + 1, -3):
        with pytest.raises(B.BnError) as e:
            B.eq_expand(n, CH[:n], out, max_levels=ml)
        assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(B.BnError) as e:
        B.eq_expand(4, CH[:4], out, bitsliced=True)
    assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(ValueError):
        B.eq_expand(n, CH[:n], out[:-4])  # short output
    with pytest.raises(ValueError):
        B.eq_expand(n, CH[:n - 1], out)  # one challenge short
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    B.eq_expand(n, CH[:n], out)
    assert np.array_equal(_np(out), _ref(n))
