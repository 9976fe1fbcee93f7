"""CPU: the bit-reversal permutation's and the verifier fold's entry points are declared, exported,
bound, and validate their arguments without touching a GPU (fake aligned device pointers, never
dereferenced: every call fails its checks first)."""
import ctypes

import numpy as np
import pytest

import binius_ntt_amd as B

NAMES = ("bn_bit_reverse_device", "bn_bit_reverse_host", "bn_bit_reverse_device_split", "bn_antt_fri_fold_leaf")


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
    for n in ("bit_reverse", "bit_reverse_host", "fri_fold_leaf"):
        assert callable(getattr(B, n))


def test_bit_reverse_device_argument_errors():
    L = B.lib()
    src, dst = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x900000)  # 2^10 elements are 16 KiB
    for fn in (lambda *a: L.bn_bit_reverse_device(*a, None), lambda *a: L.bn_bit_reverse_device_split(*a, 0, None),
               lambda *a: L.bn_bit_reverse_device_split(*a, 3, None)):
        _invalid(fn(None, dst, 10, 1, 0))
        _invalid(fn(src, None, 10, 1, 0))
        _invalid(fn(ctypes.c_void_p(0x100008), dst, 10, 1, 0))  # misaligned
        _invalid(fn(src, ctypes.c_void_p(0x900004), 10, 1, 0))
        _invalid(fn(src, dst, -1, 1, 0))
        _invalid(fn(src, dst, 31, 1, 0))
        _invalid(fn(src, dst, 4, 1, 1))  # bitsliced needs whole 32-element blocks
        _invalid(fn(src, dst, 0, 1, 1))
        _invalid(fn(src, dst, 10, 0, 0))  # no transform
        _invalid(fn(src, dst, 10, (1 << 22) + 1, 0))  # above 2^32 elements
        _invalid(fn(src, dst, 30, 5, 0))
        _invalid(fn(src, dst, 0, (1 << 32) + 1, 0))
        _invalid(fn(src, dst, 10, (1 << 64) - 1, 0))  # a batch whose element count wraps
        # overlapping ranges: in place, the output's first byte on the input's last element, and the reverse
        _invalid(fn(src, src, 10, 1, 0))
        _invalid(fn(src, ctypes.c_void_p(0x100000 + 0x4000 - 16), 10, 1, 0))
        _invalid(fn(ctypes.c_void_p(0x900000 + 0x4000 - 16), dst, 10, 1, 0))
        _invalid(fn(src, ctypes.c_void_p(0x100000 + 3 * 0x4000 - 16), 10, 3, 0))  # the batch counts
    for tl in (-1, 7, 12):
        _invalid(L.bn_bit_reverse_device_split(src, dst, 10, 1, 0, tl, None))


def test_bit_reverse_host_argument_errors():
    L = B.lib()
    buf = (ctypes.c_uint32 * 128)()
    _invalid(L.bn_bit_reverse_host(0, None, 3, 0, buf))
    _invalid(L.bn_bit_reverse_host(0, buf, 3, 0, None))
    _invalid(L.bn_bit_reverse_host(0, buf, -1, 0, buf))
    _invalid(L.bn_bit_reverse_host(0, buf, 31, 0, buf))
    _invalid(L.bn_bit_reverse_host(0, buf, 4, 1, buf))
    with pytest.raises(ValueError):
        B.bit_reverse_host(np.zeros((3, 4), np.uint32))


def test_fri_fold_leaf_argument_errors():
    L = B.lib()
    leaf = (ctypes.c_uint32 * 1024)()
    ch = (ctypes.c_uint32 * 32)()
    out = (ctypes.c_uint32 * 4)()
    assert L.bn_antt_fri_fold_leaf(12, 1, 0, 4, 0, leaf, ch, out) == B.BN_OK
    assert L.bn_antt_fri_fold_leaf(12, 1, 0, 4, (1 << 9) - 1, leaf, ch, out) == B.BN_OK
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 4, 0, None, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 4, 0, leaf, None, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 4, 0, leaf, ch, None))
    _invalid(L.bn_antt_fri_fold_leaf(0, 1, 0, 1, 0, leaf, ch, out))  # the plan's ranges
    _invalid(L.bn_antt_fri_fold_leaf(12, -1, 0, 4, 0, leaf, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 5, 0, 4, 0, leaf, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(30, 3, 0, 4, 0, leaf, ch, out))  # log_h + log_rate > 32
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, -1, 4, 0, leaf, ch, out))  # the fold's ranges
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 0, 0, leaf, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 9, 0, leaf, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 9, 4, 0, leaf, ch, out))  # round + arity > log_h
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 13, 1, 0, leaf, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 4, 1 << 9, leaf, ch, out))  # index >= 2^(13 - 4)
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 8, 4, 2, leaf, ch, out))
    _invalid(L.bn_antt_fri_fold_leaf(12, 1, 0, 4, (1 << 64) - 1, leaf, ch, out))
    with pytest.raises(ValueError):
        B.fri_fold_leaf(12, 1, 0, 0, np.zeros((8, 4), np.uint32), np.zeros((4, 4), np.uint32))  # a short leaf
    with pytest.raises(ValueError):
        B.fri_fold_leaf(12, 1, 0, 0, np.zeros((16, 4), np.uint32), np.zeros(16, np.uint32))  # not (arity, 4)
