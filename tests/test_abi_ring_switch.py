"""CPU: the ring-switching entry points are declared, exported, bound, and validate their arguments
without touching a GPU (fake aligned device pointers, never dereferenced: every call fails its checks
first)."""
import ctypes

import numpy as np
import pytest

import binius_ntt_amd as B

NAMES = ("bn_rs_partial_evals_device", "bn_rs_partial_evals_host", "bn_rs_partial_evals_device_split",
         "bn_gf128_linear_map_device", "bn_gf128_linear_map_host", "bn_rs_batch_table", "bn_rs_row_check", "bn_rs_sumcheck_claim",
         "bn_rs_eq_eval")


def _invalid(rc):
    assert rc == B.BN_ERR_INVALID
    assert B.lib().bn_last_error()


def test_entry_points_declared_exported_and_bound():
    L = B.lib()
    declared = B.exported_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n  # bound in lib(), not just resolvable
    for n in ("rs_partial_evals", "rs_partial_evals_host", "gf128_linear_map", "gf128_linear_map_host", "rs_batch_table",
              "rs_row_check", "rs_sumcheck_claim", "rs_eq_eval"):
        assert callable(getattr(B, n))
    from binius_ntt_amd import fri_pcs
    assert callable(fri_pcs.prove_eval_packed) and callable(fri_pcs.verify_eval_packed)


def test_partial_evals_device_argument_errors():
    L = B.lib()
    t, e, out = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000), ctypes.c_void_p(0x1100000)  # 2^10 elements are 16 KiB
    for fn in (lambda *a: L.bn_rs_partial_evals_device(*a, None), lambda *a: L.bn_rs_partial_evals_device_split(*a, 0, None),
               lambda *a: L.bn_rs_partial_evals_device_split(*a, 3, None)):
        _invalid(fn(None, e, 10, out))
        _invalid(fn(t, None, 10, out))
        _invalid(fn(t, e, 10, None))
        _invalid(fn(ctypes.c_void_p(0x100008), e, 10, out))  # misaligned
        _invalid(fn(t, ctypes.c_void_p(0x900004), 10, out))
        _invalid(fn(t, e, 10, ctypes.c_void_p(0x1100008)))
        _invalid(fn(t, e, 4, out))  # below one 32-element block
        _invalid(fn(t, e, 0, out))
        _invalid(fn(t, e, -1, out))
        _invalid(fn(t, e, 31, out))
        # the result inside an input: its first byte on the column's last element, and the column inside the result
        _invalid(fn(t, e, 10, ctypes.c_void_p(0x100000 + 0x4000 - 16)))
        _invalid(fn(t, e, 10, ctypes.c_void_p(0x900000)))
        _invalid(fn(t, ctypes.c_void_p(0x1100000 + 2048 - 16), 10, out))


def test_partial_evals_host_argument_errors():
    L = B.lib()
    buf = (ctypes.c_uint32 * 512)()
    _invalid(L.bn_rs_partial_evals_host(0, None, buf, 5, buf))
    _invalid(L.bn_rs_partial_evals_host(0, buf, None, 5, buf))
    _invalid(L.bn_rs_partial_evals_host(0, buf, buf, 5, None))
    _invalid(L.bn_rs_partial_evals_host(0, buf, buf, 4, buf))
    _invalid(L.bn_rs_partial_evals_host(0, buf, buf, 31, buf))
    with pytest.raises(ValueError):
        B.rs_partial_evals_host(np.zeros((48, 4), np.uint32), np.zeros((48, 4), np.uint32))
    with pytest.raises(ValueError):
        B.rs_partial_evals_host(np.zeros((32, 4), np.uint32), np.zeros((64, 4), np.uint32))


def test_linear_map_argument_errors():
    L = B.lib()
    m = (ctypes.c_uint32 * 512)()
    src, dst = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)
    for bs in (0, 1):
        size = 100 * (512 if bs else 16)
        _invalid(L.bn_gf128_linear_map_device(None, dst, 100, m, bs, None))
        _invalid(L.bn_gf128_linear_map_device(src, None, 100, m, bs, None))
        _invalid(L.bn_gf128_linear_map_device(src, dst, 100, None, bs, None))
        _invalid(L.bn_gf128_linear_map_device(ctypes.c_void_p(0x100008), dst, 100, m, bs, None))
        _invalid(L.bn_gf128_linear_map_device(src, ctypes.c_void_p(0x900004), 100, m, bs, None))
        _invalid(L.bn_gf128_linear_map_device(src, dst, 0, m, bs, None))
        # partial overlap, either way round (in place, d_out == d_in, is allowed and would launch)
        _invalid(L.bn_gf128_linear_map_device(src, ctypes.c_void_p(0x100000 + size - 16), 100, m, bs, None))
        _invalid(L.bn_gf128_linear_map_device(ctypes.c_void_p(0x900000 + 16), dst, 100, m, bs, None))
    _invalid(L.bn_gf128_linear_map_device(src, dst, (1 << 32) + 1, m, 0, None))
    _invalid(L.bn_gf128_linear_map_device(src, dst, (1 << 27) + 1, m, 1, None))
    buf = (ctypes.c_uint32 * 128)()
    _invalid(L.bn_gf128_linear_map_host(0, None, 1, m, 0, buf))
    _invalid(L.bn_gf128_linear_map_host(0, buf, 1, None, 0, buf))
    _invalid(L.bn_gf128_linear_map_host(0, buf, 1, m, 0, None))
    _invalid(L.bn_gf128_linear_map_host(0, buf, 0, m, 0, buf))
    with pytest.raises(ValueError):
        B.gf128_linear_map_host(np.zeros((4, 4), np.uint32), np.zeros((127, 4), np.uint32))
    with pytest.raises(ValueError):
        B.gf128_linear_map_host(np.zeros((33, 4), np.uint32), np.zeros((128, 4), np.uint32), bitsliced=True)


def test_verifier_functions_argument_errors():
    L = B.lib()
    r7, tab, one = (ctypes.c_uint32 * 28)(), (ctypes.c_uint32 * 512)(), (ctypes.c_uint32 * 4)()
    pts = (ctypes.c_uint32 * (4 * 122))()
    assert L.bn_rs_batch_table(r7, tab) == B.BN_OK
    _invalid(L.bn_rs_batch_table(None, tab))
    _invalid(L.bn_rs_batch_table(r7, None))
    for fn in (L.bn_rs_row_check, L.bn_rs_sumcheck_claim):
        assert fn(tab, r7, one) == B.BN_OK
        _invalid(fn(None, r7, one))
        _invalid(fn(tab, None, one))
        _invalid(fn(tab, r7, None))
    assert L.bn_rs_eq_eval(0, None, None, r7, one) == B.BN_OK
    assert L.bn_rs_eq_eval(121, pts, pts, r7, one) == B.BN_OK
    _invalid(L.bn_rs_eq_eval(-1, pts, pts, r7, one))
    _invalid(L.bn_rs_eq_eval(122, pts, pts, r7, one))
    _invalid(L.bn_rs_eq_eval(3, None, pts, r7, one))
    _invalid(L.bn_rs_eq_eval(3, pts, None, r7, one))
    _invalid(L.bn_rs_eq_eval(3, pts, pts, None, one))
    _invalid(L.bn_rs_eq_eval(3, pts, pts, r7, None))
    with pytest.raises(ValueError):
        B.rs_batch_table(np.zeros((6, 4), np.uint32))
    with pytest.raises(ValueError):
        B.rs_row_check(np.zeros((128, 4), np.uint32), np.zeros((8, 4), np.uint32))
    with pytest.raises(ValueError):
        B.rs_eq_eval(np.zeros((3, 4), np.uint32), np.zeros((2, 4), np.uint32), np.zeros((7, 4), np.uint32))
