"""GPU tests of the FRI-Binius fold (bn_antt_fri_fold_device / bn_antt_fri_fold_host). The reference
is the per-pair rule of include/binius_ntt_amd.h written out over the oracle's field arithmetic and
the plan's subspace table; the end-to-end identity pins it against the multilinear extension. Every
comparison is bit-exact."""
import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


def _to_np(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4)


def _ntt(log_h, r, bits=128):
    return B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(7 if bits == 128 else 5)))


def _challenges(seed, k):
    return O.fill128(0xF01D0000 + seed, 0xC4A11E00 + seed, k)


def _fold(ntt, d_in, rnd, ch, dev, batch=1):
    """fri_fold_device on a device tensor; returns the device tensor of the folded codeword(s)."""
    import torch
    out = torch.empty(d_in.numel() >> len(ch), dtype=torch.int32, device=dev)
    ntt.fri_fold_device(d_in, out, rnd, ch, batch=batch)
    torch.cuda.synchronize()
    return out


def _fold_schedule(ntt, d_in, rnd, schedule, ch, dev):
    at = 0
    for k in schedule:
        d_in = _fold(ntt, d_in, rnd, ch[at:at + k], dev)
        rnd, at = rnd + k, at + k
    return d_in


def _ref_round(state, s, log_h, r, i, ch):
    """One round of the per-pair rule on a (2^(log_h+r-i), 4) codeword of round i."""
    m = 1 << (log_h - i)
    nbits = log_h + r - 1 - i
    rr = O._from_words(ch)
    out = np.zeros((state.shape[0] // 2, 4), np.uint32)
    for c in range(1 << r):
        for j in range(m // 2):
            ind = (c << (log_h - 1 - i)) | j
            t = 0
            for k in range(nbits):
                if (ind >> k) & 1:
                    t ^= int(s[i][k])
            u = [int(x) for x in state[c * m + 2 * j]]
            v = [int(x) for x in state[c * m + 2 * j + 1]]
            v1 = [a ^ b for a, b in zip(u, v)]
            u1 = [a ^ O.mul(t, b, 5) for a, b in zip(u, v1)]
            d = O._from_words([a ^ b for a, b in zip(u1, v1)])
            out[c * (m // 2) + j] = O._to_words(O._from_words(u1) ^ O.mul128(rr, d))
    return out


def _state(log_h, r, rnd, seed):
    """A round-`rnd` state: the per-pair rule holds for any input of that shape."""
    return O.fill128(0xF01D + 64 * log_h + 8 * r + rnd + seed, 0x5EED0000, 1 << (log_h + r - rnd))


# one pair in all (1,0); cosets (2,1), (5,2); the last round, twiddle bits from the coset alone (5,2,4);
# less than a tile, a tile and more, eight tiles with three coset bits
@pytest.mark.parametrize("log_h,r,rnd", [(1, 0, 0), (2, 1, 0), (5, 2, 0), (5, 2, 4), (10, 1, 0), (12, 0, 0), (12, 3, 0)])
def test_arity1_matches_per_pair_rule(log_h, r, rnd, dev):
    ntt = _ntt(log_h, r)
    x = _state(log_h, r, rnd, 0)
    ch = _challenges(log_h + r + rnd, 1)
    got = _to_np(_fold(ntt, _to_dev(x, dev), rnd, ch, dev))
    assert np.array_equal(got, _ref_round(x, ntt.subspace_evals(), log_h, r, rnd, ch[0]))


def test_degenerate_challenges(dev):
    log_h, r = 12, 1
    ntt = _ntt(log_h, r)
    s = ntt.subspace_evals()
    x = _state(log_h, r, 0, 1)
    one = np.array([[1, 0, 0, 0]], np.uint32)
    got = _to_np(_fold(ntt, _to_dev(x, dev), 0, one, dev))
    assert np.array_equal(got, x[0::2] ^ x[1::2])  # r = 1: the odd part
    zero = np.zeros((1, 4), np.uint32)
    got = _to_np(_fold(ntt, _to_dev(x, dev), 0, zero, dev))
    n_pairs, nbits = x.shape[0] // 2, log_h + r - 1
    want = np.zeros((n_pairs, 4), np.uint32)
    for p in range(n_pairs):  # the pair index is (coset << (log_h - 1)) | j already
        t = 0
        for k in range(nbits):
            if (p >> k) & 1:
                t ^= int(s[0][k])
        for l in range(4):
            want[p, l] = int(x[2 * p, l]) ^ O.mul(t, int(x[2 * p, l]) ^ int(x[2 * p + 1, l]), 5)
    assert np.array_equal(got, want)  # r = 0: the even part


def _arity_equals_singles(log_h, r, rnd, k, d_in, dev, seed=0):
    ntt = _ntt(log_h, r)
    ch = _challenges(16 * log_h + k + seed, k)
    multi = _fold(ntt, d_in, rnd, ch, dev)
    single = _fold_schedule(ntt, d_in, rnd, [1] * k, ch, dev)
    assert multi.numel() == 4 << (log_h + r - rnd - k)
    assert np.array_equal(_to_np(multi), _to_np(single))


@pytest.mark.parametrize("k", range(1, 9))
def test_arity_k_equals_k_single_rounds(k, dev):
    _arity_equals_singles(12, 1, 0, k, _to_dev(_state(12, 1, 0, 2), dev), dev)


# a middle chunk with cosets; the last chunk of a large plan (one output element); the whole
# codeword one chunk
@pytest.mark.parametrize("log_h,r,rnd,k", [(14, 2, 3, 4), (20, 0, 12, 8), (3, 0, 0, 3)])
def test_arity_k_equals_k_single_rounds_at_other_rounds(log_h, r, rnd, k, dev):
    _arity_equals_singles(log_h, r, rnd, k, _to_dev(_state(log_h, r, rnd, 3), dev), dev, seed=rnd)


def _full_fold(log_h, r, schedule, dev):
    """The codeword of x folded through all log_h rounds, and what every element must equal."""
    assert sum(schedule) == log_h
    ntt = _ntt(log_h, r)
    x = O.fill128(0xDEADBEEF + log_h + r, 0x5EED0000, 1 << log_h)
    ch = _challenges(32 * log_h + r, log_h)
    import torch
    cw = torch.empty(4 << (log_h + r), dtype=torch.int32, device=dev)
    ntt.forward_device(_to_dev(x, dev), cw)
    got = _to_np(_fold_schedule(ntt, cw, 0, schedule, ch, dev))
    return x, ch, got


@pytest.mark.parametrize("log_h,r,schedule", [(1, 0, [1]), (8, 2, [3, 4, 1]), (12, 4, [8, 4]), (20, 1, [4, 4, 4, 4, 4])])
def test_full_fold_is_the_multilinear_extension(log_h, r, schedule, dev):
    x, ch, got = _full_fold(log_h, r, schedule, dev)
    assert got.shape == (1 << r, 4)
    assert (got == got[0]).all()
    # the oracle folds the highest variable first: bit i of the index pairs with ch[i]. Its
    # O(n 2^n) form takes 17 s at 2^20, so that size takes the oracle's O(2^n) form of the same
    # value, which the smaller sizes check against the first
    want = O.multilinear_composition_fold(x, log_h, 1, False, ch[::-1])
    if log_h <= 12:
        assert np.array_equal(want, O.multilinear_composition(x, log_h, 1, ch[::-1]))
    assert np.array_equal(got[0], want)


def test_full_fold_against_the_gpu_multilinear_evaluation(dev):
    log_h, r = 12, 1
    x, ch, got = _full_fold(log_h, r, [4, 8], dev)
    want = B.evaluate_multilinear_composition(x, log_h, 1, False, np.ascontiguousarray(ch[::-1]))
    assert (got == want).all()


@pytest.mark.parametrize("log_h,r,rnd,k,batch", [(12, 1, 0, 4, 3), (8, 0, 2, 3, 2)])
def test_batched_fold(log_h, r, rnd, k, batch, dev):
    ntt = _ntt(log_h, r)
    ch = _challenges(batch, k)
    xs = np.stack([_state(log_h, r, rnd, 16 + b) for b in range(batch)])
    got = _to_np(_fold(ntt, _to_dev(xs, dev), rnd, ch, dev, batch=batch)).reshape(batch, -1, 4)
    assert got.shape[1] == 1 << (log_h + r - rnd - k)
    for b in range(batch):
        assert np.array_equal(got[b], _to_np(_fold(ntt, _to_dev(xs[b], dev), rnd, ch, dev))), b


@pytest.mark.parametrize("k", [1, 5])
def test_input_left_untouched(k, dev):
    import torch
    log_h, r = 12, 1
    d_in = _to_dev(_state(log_h, r, 0, 4), dev)
    before = d_in.clone()
    out = _fold(_ntt(log_h, r), d_in, 0, _challenges(k, k), dev)
    assert torch.equal(d_in, before)
    assert out.abs().sum().item() != 0


def test_argument_errors(dev):
    import torch
    log_h, r = 12, 1
    ntt = _ntt(log_h, r)
    x = _state(log_h, r, 0, 5)
    d_in = _to_dev(x, dev)
    ch = _challenges(9, 9)
    out = torch.empty(d_in.numel() >> 1, dtype=torch.int32, device=dev)
    want = _to_np(_fold_schedule(ntt, d_in, 0, [1, 1], ch, dev))

    def good_call_still_works():
        out.zero_()
        ntt.fri_fold_device(d_in, out, 0, ch[:2])
        torch.cuda.synchronize()
        assert np.array_equal(_to_np(out)[:want.shape[0]], want)

    good_call_still_works()
    # round + arity > log_h, arity 0, arity 9, negative round
    for rnd, c in ((log_h - 1, ch[:2]), (log_h, ch[:1]), (0, np.zeros((0, 4), np.uint32)), (0, ch[:9]), (-1, ch[:1])):
        with pytest.raises(B.BnError) as e:
            ntt.fri_fold_device(d_in, out, rnd, c)
        assert e.value.code == B.BN_ERR_INVALID
        good_call_still_works()
    with pytest.raises(B.BnError) as e:
        ntt.fri_fold_device(d_in, d_in, 0, ch[:1])
    assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(B.BnError) as e:  # the output in the input's second half
        ntt.fri_fold_device(d_in, d_in[d_in.numel() // 2:], 0, ch[:1])
    assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(B.BnError) as e:
        ntt.fri_fold_device(d_in, out, 0, ch[:1], batch=0)
    assert e.value.code == B.BN_ERR_INVALID
    good_call_still_works()
    ntt32 = _ntt(log_h, r, 32)
    with pytest.raises(B.BnError) as e:
        ntt32.fri_fold_device(d_in, out, 0, ch[:1])
    assert e.value.code == B.BN_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ntt.fri_fold_device(d_in[:-1], out, 0, ch[:1])
    with pytest.raises(ValueError):
        ntt.fri_fold_device(d_in, out[:(d_in.numel() >> 1) - 1], 0, ch[:1])
    with pytest.raises(ValueError):
        ntt.fri_fold_device(d_in, out, 0, ch[:1], batch=2)
    with pytest.raises(ValueError):
        ntt.fri_fold_device(d_in, out, 0, ch[:2].reshape(-1))  # not (arity, 4)
    good_call_still_works()


def test_host_fold_semantics(dev):
    log_h, r, rnd, k = 10, 1, 2, 3
    ntt = _ntt(log_h, r)
    n, n_out = 1 << (log_h + r - rnd), 1 << (log_h + r - rnd - k)
    x = _state(log_h, r, rnd, 6)
    ch = _challenges(7, k)
    out = B.NTTData(n_out, field_bits=128)
    sentinel = np.full((n_out, 4), 0xA5A5A5A5, np.uint32)
    out.data = sentinel.copy()
    bad = B.NTTData(n >> 1, B.DataOrder.IN_ORDER, 128)
    assert ntt.fri_fold(bad, out, rnd, ch) is False  # wrong size -> False, no other effect
    assert np.array_equal(out.data, sentinel) and out.order == B.DataOrder.INVALID
    wrong_order = B.NTTData(n, B.DataOrder.BIT_REVERSED, 128, x)
    assert ntt.fri_fold(wrong_order, out, rnd, ch) is False
    assert np.array_equal(out.data, sentinel) and out.order == B.DataOrder.INVALID
    good = B.NTTData(n, B.DataOrder.IN_ORDER, 128, x)
    assert ntt.fri_fold(good, out, rnd, ch) is True
    assert out.order == B.DataOrder.IN_ORDER and out.size == n_out
    assert np.array_equal(out.data, _to_np(_fold(ntt, _to_dev(x, dev), rnd, ch, dev)))
    # an output of another size is resized
    small = B.NTTData(4, field_bits=128)
    assert ntt.fri_fold(good, small, rnd, ch) is True
    assert small.size == n_out and np.array_equal(small.data, out.data)
    # the library's own size check
    L = B.lib()
    chp = np.ascontiguousarray(ch).ctypes.data_as(B.ctypes.POINTER(B.ctypes.c_uint32))
    assert L.bn_antt_fri_fold_host(ntt._plan, x.ctypes.data, n >> 1, rnd, k, chp, out.data.ctypes.data) == B.BN_ERR_INVALID
    assert L.bn_last_error()


@pytest.mark.slow
def test_full_fold_of_a_2p24_codeword(dev):
    x, ch, got = _full_fold(22, 2, [4, 4, 4, 4, 4, 2], dev)
    assert got.shape == (4, 4)
    assert (got == got[0]).all()
    assert np.array_equal(got[0], O.multilinear_composition_fold(x, 22, 1, False, ch[::-1]))
