"""The register-tile first pass's small-sub-field stages (csrc/antt_rr.hip):
a stage whose twiddles are all zero runs without a product, stages with GF(2^2) / GF(2^4) twiddles
on bsm1x16_fma_tw / bsm2x8_fma_tw. Forward transforms against the oracle, full outputs, at the
smallest sizes that reach each class mix:

* 2^13, rate 0: a first pass that is one zero-twiddle stage; rate 1 and 2: the same pass at class
  2, then class 4;
* 2^14, rate 0: classes 2, 0;
* 2^16, rate 0: classes 4, 4, 2, 0, at batch 1 and at a batch of more than two tiles per CU (the
  bottom pass then runs its other kernel instance);
* 2^16, rate 1: every upper stage needs GF(2^16), so no pass takes the GF(2^8) register-tile kernel;
* 2^20, rate 0: the 4, 4, 2, 0 first pass in front of a GF(2^16) pass.

Each at kernel variants 5 (the default plan), 4 (register tiles everywhere) and 1 (LDS tiles: its
kernels round the small classes up and share the tables), for GF(2^128) and GF(2^32) elements. At
2^16 and 2^20 limb 0 is also pinned by the reference's MD5 table, and the inverse at 2^16 (kernels
unchanged, tables shared) must still return the input."""
import ctypes

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu

BIG_BATCH = 40  # 16 tiles per 2^16 transform: 640 tiles, above two per CU on 256 CUs
# (log_h, log_rate, batch) -> classes of stages 12 .. log_h - 1, and how many of them (from the top)
# the first pass runs
SHAPES = {
    (13, 0, 1): ([0], 1),
    (13, 1, 1): ([2], 1),
    (13, 2, 1): ([4], 1),
    (14, 0, 1): ([2, 0], 2),
    (16, 0, 1): ([4, 4, 2, 0], 4),
    (16, 0, BIG_BATCH): ([4, 4, 2, 0], 4),
    (16, 1, 1): ([16, 16, 16, 16], 4),
    (20, 0, 1): ([16, 16, 16, 16, 4, 4, 2, 0], 4),
}


def _field(bits):
    return B.FanPaarTowerField(7 if bits == 128 else 5)


_cache = {}


def _case(bits, log_h, r, batch):
    """Input and oracle output of a shape, computed once and read-only."""
    key = (bits, log_h, r, batch)
    if key not in _cache:
        n = 1 << log_h
        if bits == 128:
            # transform 0 is the reference's input (limb 0 = its mt19937 stream)
            x = np.stack([O.fill128(0xDEADBEEF + log_h + 977 * b, 0x5EED0000 + b, n) for b in range(batch)])
            want = O.antt128_batch(x, log_h, r)
        else:
            x = np.stack([O.mt_fill(0xDEADBEEF + log_h + 977 * b, n) for b in range(batch)])
            want = np.stack([O.antt32(x[b], log_h, r) for b in range(batch)])
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (x, want)
    return _cache[key]


def _forward(ntt, x, batch, dev):
    import torch
    d_in = torch.from_numpy(x.reshape(-1).view(np.int32).copy()).to(dev)  # the cached input stays read-only
    d_out = torch.empty(d_in.numel() << ntt.conf.log_rate, dtype=torch.int32, device=dev)
    ntt.forward_device(d_in, d_out, batch=batch)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)


def _classes(log_h, r):
    out = np.zeros(log_h - 12, np.int32)
    assert B.lib().bn_antt_stage_classes(log_h, r, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), out.size) == B.BN_OK
    return [int(v) for v in out]


@pytest.mark.parametrize("bits", [128, 32])
@pytest.mark.parametrize("variant", [5, 4, 1])
@pytest.mark.parametrize("log_h,r,batch", sorted(SHAPES))
def test_forward_matches_oracle(log_h, r, batch, variant, bits, ntt_md5, dev):
    classes, k_first = SHAPES[(log_h, r, batch)]
    assert _classes(log_h, r) == classes
    x, want = _case(bits, log_h, r, batch)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, _field(bits)))
    ntt.set_variant(variant)
    first = ntt.pass_kernel_name(0)
    by_class = "antt_rr_pass<%d, 0, 8" % ntt.limbs  # the instance that runs its stages by class
    if variant != 1 and max(classes[-k_first:]) <= 8:
        assert by_class in first, first
    else:
        assert by_class not in first, first
    got = _forward(ntt, x, batch, dev).reshape(want.shape)
    assert np.array_equal(got, want)
    if r == 0 and log_h in (16, 20):
        md5 = O.md5_limb(got[0], 0) if bits == 128 else O.md5(got[0])
        assert md5 == ntt_md5["0"][log_h]


@pytest.mark.parametrize("bits", [128, 32])
def test_inverse_round_trip_at_2p16(bits, dev):
    import torch
    log_h = 16
    x, want = _case(bits, log_h, 0, 1)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, 0, _field(bits)))
    y = _forward(ntt, x, 1, dev)
    assert np.array_equal(y.reshape(want.shape), want)
    d_y = torch.from_numpy(y.view(np.int32)).to(dev)
    d_x = torch.empty_like(d_y)
    ntt.inverse_device(d_y, d_x, coset=0, batch=1)
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint32), x.reshape(-1))
