"""CPU: the eq-indicator expansion's entry points are declared, exported and validate their
arguments without touching a GPU; bn_eq_eval against its formula over the oracle's products; the
host planner's split for every size and cap."""
import ctypes

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

NAMES = ("bn_eq_expand_device", "bn_eq_expand_host", "bn_eq_eval", "bn_eq_expand_device_split", "bn_eq_expand_passes")
U32P = ctypes.POINTER(ctypes.c_uint32)


def test_eq_entry_points_declared_and_exported():
    L = B.lib()
    declared = B.exported_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(L, n), n


def _invalid(rc):
    assert rc == B.BN_ERR_INVALID
    assert B.lib().bn_last_error()


def test_eq_expand_argument_errors():
    L = B.lib()
    ch = (ctypes.c_uint32 * (4 * 31))(*range(4 * 31))
    host = (ctypes.c_uint32 * 64)()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks first
    for n in (-1, 31):  # num_vars out of range
        _invalid(L.bn_eq_expand_device(n, ch, None, fake, 0, None))
        _invalid(L.bn_eq_expand_device_split(n, ch, None, fake, 0, 0, None))
        _invalid(L.bn_eq_expand_host(0, n, ch, None, 0, host))
    _invalid(L.bn_eq_expand_device(4, ch, None, None, 0, None))  # NULL output
    _invalid(L.bn_eq_expand_host(0, 2, ch, None, 0, None))
    _invalid(L.bn_eq_expand_device(3, None, None, fake, 0, None))  # NULL challenges with num_vars > 0
    _invalid(L.bn_eq_expand_host(0, 3, None, None, 0, host))
    for n in (0, 4):  # bitsliced below one block
        _invalid(L.bn_eq_expand_device(n, ch, None, fake, 1, None))
        _invalid(L.bn_eq_expand_host(0, n, ch, None, 1, host))
    T = B.eq_expand_passes(30)[-1]
    for cap in (-1, 1, 2, T + 1):  # the forced cap is 3 up to the default
        _invalid(L.bn_eq_expand_device_split(8, ch, None, fake, 0, cap, None))


def test_eq_expand_passes_argument_errors():
    L = B.lib()
    lv = (ctypes.c_int32 * 32)()
    k = ctypes.c_int()
    _invalid(L.bn_eq_expand_passes(-1, 0, lv, 32, ctypes.byref(k)))
    _invalid(L.bn_eq_expand_passes(31, 0, lv, 32, ctypes.byref(k)))
    _invalid(L.bn_eq_expand_passes(10, 2, lv, 32, ctypes.byref(k)))
    _invalid(L.bn_eq_expand_passes(10, 13, lv, 32, ctypes.byref(k)))
    _invalid(L.bn_eq_expand_passes(10, 3, lv, 3, ctypes.byref(k)))  # four passes, room for three
    _invalid(L.bn_eq_expand_passes(10, 3, None, 32, ctypes.byref(k)))
    _invalid(L.bn_eq_expand_passes(10, 3, lv, 32, None))


def test_eq_expand_passes_split():
    T = B.eq_expand_passes(30)[-1]
    assert T == 12
    assert B.eq_expand_passes(30) == [6, 12, 12]
    assert B.eq_expand_passes(0) == []
    for n in range(31):
        for ml in [0] + list(range(3, T + 1)):
            cap = ml or T
            lv = B.eq_expand_passes(n, ml)
            assert sum(lv) == n, (n, ml, lv)
            assert all(1 <= l <= cap for l in lv), (n, ml, lv)
            if n:
                # the planner has no small-n rule: the last pass is always the full one
                assert lv[-1] == min(n, cap), (n, ml, lv)
                assert all(l == cap for l in lv[1:]), (n, ml, lv)
                assert len(lv) == -(-n // cap)
    assert B.eq_expand_passes(8, 3) == [2, 3, 3]
    assert B.eq_expand_passes(9, 3) == [3, 3, 3]
    assert B.eq_expand_passes(10, 3) == [1, 3, 3, 3]
    assert B.eq_expand_passes(11, 4) == [3, 4, 4]
    assert B.eq_expand_passes(13, 5) == [3, 5, 5]


def _eq_ref(a, b):
    acc = 1
    for x, y in zip(a, b):
        x, y = O._from_words(x), O._from_words(y)
        acc = O.mul128(acc, O.mul128(x, y) ^ O.mul128(1 ^ x, 1 ^ y))
    return O._to_words(acc)


@pytest.mark.parametrize("n", [0, 1, 7, 128])
def test_eq_eval_matches_the_formula(n):
    a = O.fill128(0xE0E0 + n, 0xA0000000, max(n, 1))[:n]
    b = O.fill128(0xE1E1 + n, 0xB0000000, max(n, 1))[:n]
    got = B.eq_eval(a, b)
    assert np.array_equal(got, _eq_ref(a, b))
    assert np.array_equal(got, B.eq_eval(b, a))  # symmetric
    if n == 0:
        assert list(got) == [1, 0, 0, 0]


def _boolean(bits):
    p = np.zeros((len(bits), 4), np.uint32)
    p[:, 0] = bits
    return p


def test_eq_eval_on_boolean_points():
    bits = [(0x5A3C96E1 >> (i % 32)) & 1 for i in range(40)]
    a = _boolean(bits)
    assert list(B.eq_eval(a, a)) == [1, 0, 0, 0]
    for flip in (0, 17, 39):
        other = list(bits)
        other[flip] ^= 1
        assert list(B.eq_eval(a, _boolean(other))) == [0, 0, 0, 0]
        assert list(B.eq_eval(_boolean(other), a)) == [0, 0, 0, 0]


def test_eq_eval_argument_errors():
    L = B.lib()
    w = (ctypes.c_uint32 * 4)()
    _invalid(L.bn_eq_eval(-1, w, w, w))
    _invalid(L.bn_eq_eval(129, w, w, w))
    _invalid(L.bn_eq_eval(1, None, w, w))
    _invalid(L.bn_eq_eval(1, w, None, w))
    _invalid(L.bn_eq_eval(1, w, w, None))
