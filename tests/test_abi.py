"""CPU: the C-ABI library loads, exports every symbol include/binius_ntt_amd.h declares, and
validates arguments without touching a GPU (no compute calls here)."""
import ctypes

import pytest

import binius_ntt_amd as B


def test_library_exports_every_declared_symbol():
    L = B.lib()
    names = B.exported_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), n


def test_version_and_error_strings():
    L = B.lib()
    assert b"gfx950" in L.bn_version()
    assert isinstance(L.bn_last_error(), bytes)


@pytest.mark.parametrize("field,log_h,log_rate", [(64, 10, 0), (128, 0, 0), (32, 10, 5), (32, 30, 3)])
def test_plan_create_rejects_bad_parameters(field, log_h, log_rate):
    # AdditiveNTTConf asserts (nttconf.cuh:55-60): log_h >= 1, log_h+log_rate <= N_BITS, 0 <= log_rate <= 4
    p = ctypes.c_void_p()
    rc = B.lib().bn_antt_plan_create(0, field, log_h, log_rate, ctypes.byref(p))
    assert rc == B.BN_ERR_INVALID
    assert not p.value
    assert B.lib().bn_last_error()


def test_plan_create_unsupported_sizes():
    # GF(2^128) with log_h + log_rate > 32 is valid for the reference surface but not built here
    p = ctypes.c_void_p()
    assert B.lib().bn_antt_plan_create(0, 128, 31, 2, ctypes.byref(p)) == B.BN_ERR_UNSUPPORTED


def test_conf_mirror_raises_like_reference_asserts():
    with pytest.raises(ValueError):
        B.AdditiveNTTConf(0, 0)
    with pytest.raises(ValueError):
        B.AdditiveNTTConf(10, 5)
    with pytest.raises(ValueError):
        B.AdditiveNTTConf(30, 3, B.FanPaarTowerField(5))


def test_null_arguments_rejected():
    L = B.lib()
    assert L.bn_antt_forward_device(None, None, None, 1, None) == B.BN_ERR_INVALID
    assert L.bn_antt_plan_destroy(None) == B.BN_OK
    assert L.bn_sumcheck_destroy(None) == B.BN_OK
    assert L.bn_gf128_mul_device(None, None, None, 4, None) == B.BN_ERR_INVALID


def test_product_library_has_no_experiment_kernels():
    """Experiments measured and not kept live only in the development build (BN_DEV) or, like the
    fused sumcheck fold + messages kernel sc_fold_msgs, have left the tree:
    the product library the driver loads carries none of their kernels."""
    with open(B.LIB_PATH, "rb") as f:
        blob = f.read()
    # positive control: kernel names are stored as plain text in this file, so a name that is
    # absent below is absent from the library and not merely compressed or bundled out of sight
    # (sc_messagesILi0ELi4E: the mangled sc_messages<0, 4>, a kept sumcheck instantiation)
    for name in (b"antt_bs_pass", b"antt_rr_pass", b"k_gf128_mul_bs", b"sc_messagesILi0ELi4E"):
        assert name in blob, name
    for name in (b"antt_bs_persist3", b"antt_rr_mid_pf", b"antt_rr_pass_persist", b"sc_fold_msgs"):
        assert name not in blob, name
    # sumcheck instantiations that no round shape selects (tests/cpp/test_host_asan.cpp sweeps the
    # planner): sc_fold<2, *>, sc_fold<0, 4>, sc_messages<1, 4>, sc_messages<2, 16>
    for name in (b"sc_foldILi2E", b"sc_foldILi0ELi4E", b"sc_messagesILi1ELi4E", b"sc_messagesILi2ELi16E"):
        assert name not in blob, name
    # additive-NTT pass instantiations that no plan selects (the same program sweeps ntt_plan_launch
    # over every plan): only a first pass (roles: 0 first, 1 mid, 2 last, 3 single; the inverse's
    # last) has every twiddle in GF(2^8), and a single pass (log_h 12) lies in GF(2^16).
    # Template arguments <limbs, role, fmax[, waves bound]>; a kept instance of each family first
    for name in (b"antt_bs_passILi4ELi2ELi32E", b"antt_bs_passILi1ELi0ELi8E", b"antt_bs3_passILi1E", b"antt_inv_bs_passILi4ELi2ELi8E",
                 b"antt_inv_bs_passILi1ELi0ELi32E", b"antt_rr_passILi4ELi0ELi8ELi1E", b"antt_rr_passILi1ELi3ELi16ELi3E",
                 b"antt_rr_passILi4ELi2ELi32ELi1E"):
        assert name in blob, name
    gone = [b"antt_bs_passILi%dELi%dELi8E" % (l, role) for l in (1, 4) for role in (1, 2, 3)]
    gone += [b"antt_inv_bs_passILi%dELi%dELi8E" % (l, role) for l in (1, 4) for role in (0, 1, 3)]
    gone += [b"antt_rr_passILi%dELi%sE" % (l, args) for l in (1, 4)
             for args in (b"1ELi8ELi1", b"2ELi8ELi3", b"3ELi8ELi3", b"3ELi32ELi3")]
    gone += [b"antt_rr_passILi4ELi2ELi8ELi1E"]
    assert len(gone) == 21
    for name in gone:
        assert name not in blob, name
    # BabyBear NTT: the multi-pass roles 0 and 1 run on bb_pass_r<role, m> alone (the same program
    # sweeps bb_plan_launch over log_n 1..27), so the LDS-tile kernel bb_pass has no role 0 / 1 forms
    assert b"bb_pass_rILi0ELi6E" in blob
    for name in (b"bb_passILi0E", b"bb_passILi1E"):
        assert name not in blob, name
