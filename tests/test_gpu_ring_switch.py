"""GPU tests of the two ring-switching kernels, bit-exact against numpy (tests/_rs_ref.py): the partial
evaluations s^_v = XOR over w with bit_v(t'[w]) = 1 of E[w] of two bitsliced columns, through one and
several work-groups, and the GF(2)-linear map out[w] = XOR over u with bit_u(in[w]) = 1 of matrix[u],
compact and bitsliced, in place and out of place."""
import functools

import numpy as np
import pytest

import _oracle as O
import _rs_ref as S
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


def _to_np(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _columns(log_n):
    """Random t' and E of 2^log_n elements and their partial evaluations (read-only)."""
    tp = O.fill128(0x7A57 + log_n, 0x5EED0000, 1 << log_n)
    E = O.fill128(0xE9E9 + log_n, 0xC0FFEE00, 1 << log_n)
    return tp, E, S.partial_evals(tp, E)


def _partial_evals(tp, E, log_n, dev, **kw):
    import torch
    out = torch.full((512,), 0x5A5A5A5A, dtype=torch.int32, device=dev)  # the call zeroes it itself
    B.rs_partial_evals(_to_dev(O.bitslice128(tp), dev), _to_dev(O.bitslice128(E), dev), log_n, out, **kw)
    torch.cuda.synchronize()
    return _to_np(out)


@pytest.mark.parametrize("log_n", [5, 6, 10])
def test_partial_evals_random(log_n, dev):
    tp, E, want = _columns(log_n)
    assert np.array_equal(_partial_evals(tp, E, log_n, dev), want)


# 2^13 elements are 256 blocks: 2 work-groups, 3 (100 + 100 + 56) and 37 (the last one of 4 blocks)
@pytest.mark.parametrize("log_n,per_group", [(6, 1), (10, 5), (13, 128), (13, 100), (13, 7)])
def test_partial_evals_through_several_work_groups(log_n, per_group, dev):
    tp, E, want = _columns(log_n)
    assert ((1 << (log_n - 5)) + per_group - 1) // per_group > 1
    assert np.array_equal(_partial_evals(tp, E, log_n, dev, max_blocks_per_group=per_group), want)


def test_partial_evals_default_plan_equals_the_split_one_at_2_to_the_13(dev):
    tp, E, want = _columns(13)
    assert np.array_equal(_partial_evals(tp, E, 13, dev), want)


@pytest.mark.parametrize("log_n", [5, 10])
def test_partial_evals_of_all_ones_is_the_sum_of_the_eq_column(log_n, dev):
    _, E, _ = _columns(log_n)
    tp = np.full((1 << log_n, 4), 0xFFFFFFFF, np.uint32)
    got = _partial_evals(tp, E, log_n, dev)
    assert np.array_equal(got, np.tile(np.bitwise_xor.reduce(E, axis=0), (128, 1)))


@pytest.mark.parametrize("v", [0, 31, 32, 127])
@pytest.mark.parametrize("w", [0, 17, (1 << 10) - 32, (1 << 10) - 1])
def test_partial_evals_of_one_set_bit_is_that_element_of_the_eq_column(w, v, dev):
    """Bit v of t'[w] alone: s^_v = E[w], every other s^ is 0 (limb order, bit order, block order)."""
    log_n = 10
    _, E, _ = _columns(log_n)
    tp = np.zeros((1 << log_n, 4), np.uint32)
    tp[w, v >> 5] = np.uint32(1) << np.uint32(v & 31)
    want = np.zeros((128, 4), np.uint32)
    want[v] = E[w]
    assert np.array_equal(_partial_evals(tp, E, log_n, dev), want)


def test_partial_evals_host_staging_and_inputs_untouched(dev):
    import torch
    tp, E, want = _columns(10)
    bt, be = O.bitslice128(tp), O.bitslice128(E)
    assert np.array_equal(B.rs_partial_evals_host(bt, be), want)
    dt, de = _to_dev(bt, dev), _to_dev(be, dev)
    out = torch.empty(512, dtype=torch.int32, device=dev)
    B.rs_partial_evals(dt, de, 10, out)
    torch.cuda.synchronize()
    assert np.array_equal(dt.cpu().numpy().view(np.uint32), bt) and np.array_equal(de.cpu().numpy().view(np.uint32), be)


def _matrix(kind):
    if kind == "identity":
        return S.words([1 << u for u in range(128)])
    if kind == "reversal":
        return S.words([1 << (127 - u) for u in range(128)])
    return O.fill128(0x3A7, 0x77770000, 128)


@functools.lru_cache(maxsize=None)
def _mapped(kind, n):
    x = O.fill128(0x11AE + n, 0x5EED0000, n)
    return x, S.linear_map(x, _matrix(kind))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4097])
@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
def test_linear_map_compact(kind, n, in_place, dev):
    import torch
    x, want = _mapped(kind, n)
    if kind == "identity":
        assert np.array_equal(want, x)
    src = _to_dev(x, dev)
    dst = src if in_place else torch.full_like(src, 0x5A5A5A5A)
    B.gf128_linear_map(src, dst, _matrix(kind))
    torch.cuda.synchronize()
    assert np.array_equal(_to_np(dst), want)
    if not in_place:
        assert np.array_equal(_to_np(src), x)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("blocks", [1, 3, 129])
@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
def test_linear_map_bitsliced(kind, blocks, in_place, dev):
    import torch
    x, want = _mapped(kind, 32 * blocks)
    src = _to_dev(O.bitslice128(x), dev)
    dst = src if in_place else torch.full_like(src, 0x5A5A5A5A)
    B.gf128_linear_map(src, dst, _matrix(kind), bitsliced=True)
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), O.bitslice128(want))
    if not in_place:
        assert np.array_equal(src.cpu().numpy().view(np.uint32), O.bitslice128(x))


def test_linear_map_host_staging(dev):
    x, want = _mapped("random", 4097)
    assert np.array_equal(B.gf128_linear_map_host(x, _matrix("random")), want)
    x, want = _mapped("random", 96)
    got = B.gf128_linear_map_host(O.bitslice128(x).reshape(-1, 4), _matrix("random"), bitsliced=True)
    assert np.array_equal(got.reshape(-1), O.bitslice128(want))


def test_the_map_of_the_eq_column_satisfies_the_sumcheck_s_identity(dev):
    """Both kernels and the host arithmetic together at 2^10: sum_w A[w] t'[w] == s_0."""
    import torch
    n = 10
    tp, _, _ = _columns(n)
    r_high, r2 = O.fill128(0xA1, 0x1111, n), O.fill128(0xA2, 0x2222, 7)
    cols = torch.empty(2, 4 << n, dtype=torch.int32, device=dev)
    B.eq_expand(n, r_high, cols[0], bitsliced=True)
    cols[1].copy_(_to_dev(O.bitslice128(tp[[int(format(y, "010b")[::-1], 2) for y in range(1 << n)]]), dev))
    shat = torch.empty(512, dtype=torch.int32, device=dev)
    B.rs_partial_evals(cols[1], cols[0], n, shat)
    B.gf128_linear_map(cols[0], cols[0], B.rs_batch_table(r2), bitsliced=True)
    torch.cuda.synchronize()
    shat = _to_np(shat)
    assert np.array_equal(shat, S.partial_evals(tp, S.eq_table_high(r_high)))
    sc =B.Sumcheck(n, 2, True, cols, device=0)
    s0, _ = sc.this_round_messages()
    sc.close()
    assert np.array_equal(s0, B.rs_sumcheck_claim(shat, r2))
