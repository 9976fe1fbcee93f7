"""CPU: the sub-field classes of the register-tile pass tables (bn_antt_stage_classes, host only)
against an independent computation from the oracle's subspace evaluations.

The twiddle of a butterfly block of stage s is an XOR of entries of row s of the table, up to the
plan's width (log_h + log_rate - 1), so the stage's class is the smallest of 0, 2, 4, 8, 16, 32 bits
that holds every entry of that row: 0 when all are zero. The first pass's GF(2^8) register-tile
kernels run a class-0 stage without a product and classes 2 / 4 on the GF(2^2) / GF(2^4) circuits
(DESIGN.md section 5.2)."""
import ctypes

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

BOTTOM = 12  # stages 0..11 belong to the bottom pass


def _classes(log_h, log_rate, n=None):
    n = log_h - BOTTOM if n is None else n
    out = np.full(max(n, 1), -1, np.int32)
    rc = B.lib().bn_antt_stage_classes(log_h, log_rate, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n)
    return rc, [int(v) for v in out[:n]]


def _expected(log_h, log_rate):
    S = O.subspace_evals(log_h, log_rate)
    width = log_h + log_rate - 1
    out = []
    for s in range(BOTTOM, log_h):
        acc = 0
        for kk in range(width - s):
            acc |= int(S[s][kk])
        out.append(next(c for c in (0, 2, 4, 8, 16, 32) if acc < (1 << c)))
    return out


@pytest.mark.parametrize("log_rate", [0, 1, 2, 3])
@pytest.mark.parametrize("log_h", list(range(13, 27)))
def test_stage_classes_match_the_oracles_table(log_h, log_rate):
    rc, got = _classes(log_h, log_rate)
    assert rc == B.BN_OK, B.lib().bn_last_error()
    assert got == _expected(log_h, log_rate)


@pytest.mark.parametrize("log_h,want", [
    (13, [0]),
    (14, [2, 0]),
    (16, [4, 4, 2, 0]),
    (20, [16, 16, 16, 16, 4, 4, 2, 0]),
    (24, [32, 32, 32, 32, 8, 8, 8, 8, 4, 4, 2, 0]),
])
def test_rate_0_classes_are_the_documented_ones(log_h, want):
    rc, got = _classes(log_h, 0)
    assert rc == B.BN_OK, B.lib().bn_last_error()
    assert got == want
    assert _expected(log_h, 0) == want


def test_rate_1_raises_the_classes():
    # the coset bits' table entries are wider: at 2^16 every upper stage needs GF(2^16), and at 2^24
    # stages 16..20 do and the top stage needs GF(2^8)
    assert _classes(16, 1)[1] == [16] * 4
    c = _classes(24, 1)[1]
    assert c[4:9] == [16] * 5 and c[11] == 8


def test_stage_classes_rejects_bad_arguments():
    assert _classes(11, 0, 4)[0] == B.BN_ERR_UNSUPPORTED
    assert _classes(16, 0, 3)[0] == B.BN_ERR_INVALID
    assert _classes(16, 5, 4)[0] == B.BN_ERR_INVALID
    assert B.lib().bn_antt_stage_classes(16, 0, None, 4) == B.BN_ERR_INVALID
    rc, got = _classes(12, 0)  # one pass: no upper stage, nothing written
    assert rc == B.BN_OK and got == []
