"""CPU: the FRI-Binius fold entry points are declared, exported and validate their arguments
without touching a GPU."""
import ctypes

import binius_ntt_amd as B

NAMES = ("bn_antt_fri_fold_device", "bn_antt_fri_fold_host")


def test_fold_entry_points_declared_and_exported():
    L = B.lib()
    declared = B.exported_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(L, n), n


def test_fold_null_arguments_rejected():
    L = B.lib()
    ch = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    assert L.bn_antt_fri_fold_device(None, None, None, 0, 1, None, 1, None) == B.BN_ERR_INVALID
    assert L.bn_last_error()
    assert L.bn_antt_fri_fold_device(None, None, None, 0, 1, ch, 1, None) == B.BN_ERR_INVALID
    assert L.bn_last_error()
    assert L.bn_antt_fri_fold_host(None, None, 0, 0, 1, None, None) == B.BN_ERR_INVALID
    assert L.bn_last_error()
    assert L.bn_antt_fri_fold_host(None, None, 0, 0, 1, ch, None) == B.BN_ERR_INVALID
    assert L.bn_last_error()
