"""CPU: the inverse additive-NTT entry points are declared, exported and validate their arguments
without touching a GPU."""
import binius_ntt_amd as B

NAMES = ("bn_antt_inverse_device", "bn_antt_inverse_host")


def test_inverse_entry_points_declared_and_exported():
    L = B.lib()
    declared = B.exported_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(L, n), n


def test_inverse_null_arguments_rejected():
    L = B.lib()
    assert L.bn_antt_inverse_device(None, None, None, 0, 1, None) == B.BN_ERR_INVALID
    assert L.bn_last_error()
    assert L.bn_antt_inverse_host(None, None, 0, 0, None) == B.BN_ERR_INVALID
    assert L.bn_last_error()
