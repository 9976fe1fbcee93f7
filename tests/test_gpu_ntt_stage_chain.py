"""The block stages of the LDS-tile forward passes request words of U from LDS next to V, ahead of
the multiply circuit (early_u_words, csrc/antt_bs_dev.hpp: all 32 in the bottom pass and with the
GF(2^8) circuits, 16 early and 16 after the circuit in the other GF(2^32) kernels), and the packed
in-word stages of the bottom pass and the scalar top stage run the same body (bs_pass_body,
csrc/antt_bs.hip). Parity with the oracle at the smallest
launches that are not small launches: at least two tiles per CU, below which the default plan
takes the lane-split and register-tile kernels instead (ntt_plan_launch, csrc/antt_passes.cpp).

* 2^13 at log_rate 1, 128 transforms: 2 tiles x 2 cosets x 128 = 512 bottom tiles. A one-stage upper
  pass over the packed bottom kernel (GF(2^16) twiddles on the FMAX 32 kernel; the LDS-tile plan
  runs the upper stage on antt_bs_pass<., 0, 8>, all of U early).
* 2^19 at log_rate 1, 2 transforms: 128 x 2 x 2 = 512 bottom tiles. GF(2^32) twiddles in every
  bottom stage, the scalar top stage (ntt_mul32_w), and a seven-stage upper GF(2^16/32) LDS-tile
  pass (antt_bs_pass<., 0, 32>: 16 words of U early, 16 late).
* 2^21 at log_rate 0, one GF(2^32) transform of the reference's input stream (512 tiles), against
  the reference's MD5 table.

log_rate 1 and several transforms make the coset and outer parts of every twiddle non-zero. Each
case runs on the default plan and on the LDS-tile plan (variant 1), for GF(2^128) (four limbs) and
GF(2^32) (one limb).

All of these are two-pass transforms, so the upper kernel here is ROLE_FIRST; it shares its count
of early words with ROLE_MID. antt_bs_pass<4, 1, 32> itself runs in three-pass transforms:
tests/test_gpu_ntt_circuit_sites.py at 2^20 (1024 tiles in the default plan) and the 2^24 tests of
tests/test_gpu_ntt.py."""
import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

gpu = pytest.mark.gpu

# log_h -> (log_rate, transforms): 512 bottom tiles each
CASES = {13: (1, 128), 19: (1, 2)}
TILE_LOG = 12


def _tiles(log_h, r, batch):
    return (batch << r) << (log_h - TILE_LOG)


def _inputs(log_h, limbs):
    r, batch = CASES[log_h]
    if limbs == 4:
        return np.stack([O.fill128(0x57A6E + 16 * log_h + b, 0xC4A10 + b, 1 << log_h) for b in range(batch)])
    return np.stack([O.mt_fill(0x57A6E + 64 * log_h + b, 1 << log_h) for b in range(batch)])


_want = {}


def _oracle(log_h, limbs):
    """The oracle's transforms of _inputs, computed once and shared read-only."""
    key = (log_h, limbs)
    if key not in _want:
        r, _ = CASES[log_h]
        x = _inputs(log_h, limbs)
        w = O.antt128_batch(x, log_h, r) if limbs == 4 else np.stack([O.antt32(xb, log_h, r) for xb in x])
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def _plan(log_h, r, limbs, variant):
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(7 if limbs == 4 else 5)))
    assert ntt.variant() == 5
    if variant != 5:
        ntt.set_variant(variant)
    return ntt


def _forward(ntt, x_np, batch, dev):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(x_np).reshape(-1).view(np.int32)).to(dev)
    y = torch.empty(x.numel() << ntt.conf.log_rate, dtype=torch.int32, device=dev)
    ntt.forward_device(x, y, batch=batch)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint32)


def _not_a_small_launch(tiles, dev):
    import torch
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert tiles >= 2 * cus, "the launch of %d tiles is a small launch on %d CUs: the LDS-tile kernels would not run" % (tiles, cus)


# The LDS-tile plan's kernels by pass. pass_kernel_name answers for ONE transform, which is a small
# launch: in the default plan it says nothing about these batched launches, and in the LDS-tile plan
# the upper GF(2^32) pass of one four-limb 2^19 transform is the lane-split kernel (None: not
# asserted; the 512-tile launch here runs antt_bs_pass<4, 0, 32>).
LDS_TILE_KERNELS = {(13, 4): ["antt_bs_pass<4, 0, 8", "antt_bs_pass<4, 2, 32"],
                    (13, 1): ["antt_bs_pass<1, 0, 8", "antt_bs_pass<1, 2, 32"],
                    (19, 4): [None, "antt_bs_pass<4, 2, 32"],
                    (19, 1): ["antt_bs_pass<1, 0, 32", "antt_bs_pass<1, 2, 32"]}


@gpu
@pytest.mark.parametrize("variant", [5, 1])
@pytest.mark.parametrize("limbs", [4, 1])
@pytest.mark.parametrize("log_h", sorted(CASES))
def test_early_u_reads_match_oracle(log_h, limbs, variant, dev):
    r, batch = CASES[log_h]
    _not_a_small_launch(_tiles(log_h, r, batch), dev)
    ntt = _plan(log_h, r, limbs, variant)
    if variant == 1:
        for i, want in enumerate(LDS_TILE_KERNELS[log_h, limbs]):
            assert want is None or want in ntt.pass_kernel_name(i)
    got = _forward(ntt, _inputs(log_h, limbs), batch, dev)
    want = _oracle(log_h, limbs)
    assert np.array_equal(got.reshape(want.shape), want)


def _bottom_kernel_name(ntt):
    """Name of the plan's last pass (the plan exposes no pass count: the first index it rejects ends it)."""
    name = None
    for i in range(8):
        try:
            name = ntt.pass_kernel_name(i)
        except B.BnError:
            break
    return name


@gpu
@pytest.mark.parametrize("variant", [5, 1])
def test_rate0_reference_stream_md5(ntt_md5, variant, dev):
    log_h, r = 21, 0
    _not_a_small_launch(_tiles(log_h, r, 1), dev)
    x = O.mt_fill(0xDEADBEEF + log_h + r, 1 << log_h)
    ntt = _plan(log_h, r, 1, variant)
    if variant == 1:
        assert "antt_bs_pass<1, 2, 32" in _bottom_kernel_name(ntt)
    assert O.md5(_forward(ntt, x, 1, dev)) == ntt_md5[str(r)][log_h]
