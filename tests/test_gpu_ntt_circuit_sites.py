"""The forward NTT's call sites of the passes' own GF(2^32) circuits (ntt_mul32 through mul_tw,
ntt_mul32_w on the scalar top stage; bitsliced_ntt_gen.hpp) and of the sub-field circuits beside
them in the same kernels, against the oracle, at the smallest sizes that reach each of them, with
two transforms and log_rate 1 so that the coset and outer parts of the twiddles are non-zero:

* 2^12: one pass, the single-pass kernel with the per-stage in-word path (mul_tw in place);
* 2^13: two passes, a one-stage upper pass over the packed ROLE_LAST bottom kernel;
* 2^18: still two passes (six upper stages fit one tile): the lane-split upper pass (bsm3_mul /
  bsm4_mul) over a bottom pass whose stages 0..10 need the GF(2^32) circuit, in the block stages
  and in the packed in-word stages; its top stage (11) has GF(2^16) twiddles;
* 2^20: the smallest size with three passes, FIRST over GF(2^8) stages 16..19 (LDS tiles in the
  LDS-tile plan, register tiles with bsm3x4_fma_tw in the default plan), ROLE_MID
  antt_bs_pass<4, 1, 32> over stages 12..15, and the bottom pass, whose top stage now has GF(2^32)
  twiddles and so takes the scalar branch (ntt_mul32_w).

Which circuit a stage runs is decided by its twiddles' field (plan_passes, csrc/antt_passes.cpp: the
smallest of GF(2^8), GF(2^16), GF(2^32) that holds every subspace evaluation of the stage); the
tests assert those fields from the oracle's subspace evaluations, and the kernels of each plan by
name.

The circuits on their own are tests/test_circuits.py and tests/test_ntt_circuits_host.py."""
import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

gpu = pytest.mark.gpu
BATCH, RATE = 2, 1


def _inputs(log_h):
    return np.stack([O.fill128(0xC1C0 + 16 * log_h + b, 0x5170 + b, 1 << log_h) for b in range(BATCH)])


_want = {}


def _oracle(log_h):
    if log_h not in _want:
        w = O.antt128_batch(_inputs(log_h), log_h, RATE)
        w.setflags(write=False)
        _want[log_h] = w
    return _want[log_h]


def _forward(ntt, log_h, dev):
    import torch
    x = torch.from_numpy(_inputs(log_h).reshape(-1).view(np.int32)).to(dev)
    y = torch.empty(x.numel() << RATE, dtype=torch.int32, device=dev)
    ntt.forward_device(x, y, batch=BATCH)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint32).reshape(BATCH, -1, 4)


def _stage_fields(log_h):
    """Field (8, 16 or 32 bits) of every stage's twiddles, by plan_passes' rule."""
    S = O.subspace_evals(log_h, RATE)
    width = log_h + RATE - 1
    out = []
    for s in range(log_h):
        acc = 0
        for kk in range(width - s):
            acc |= int(S[s][kk])
        out.append(8 if acc < 256 else 16 if acc < 65536 else 32)
    return out


# the bottom pass's top stage (tile bit 6 = stage 11) takes the scalar branch iff its field is 32
TOP = 11


def test_stage_fields_put_each_size_on_the_intended_circuits():
    f = {n: _stage_fields(n) for n in (12, 13, 18, 20)}
    assert set(f[12]) == set(f[13]) == {8, 16}            # sub-field circuits only
    assert f[18][:TOP] == [32] * TOP and f[18][TOP] == 16  # ntt_mul32, no scalar top stage yet
    assert f[20][:TOP + 2] == [32] * (TOP + 2)             # ntt_mul32 and ntt_mul32_w (stage 11), stage 12 in the MID pass
    assert f[20][16:] == [8] * 4                           # the FIRST pass's stages: GF(2^8)


def _kernels(ntt):
    names = []
    while len(names) < 8:
        try:
            names.append(ntt.pass_kernel_name(len(names)))
        except B.BnError:
            break
    return names


@gpu
@pytest.mark.parametrize("log_h,kernels", [
    (12, ["antt_bs_pass<4, 3, 32"]),
    (13, ["antt_bs_pass<4, 0, 8", "antt_bs_pass<4, 2, 32"]),
    (18, ["antt_bs3_pass<0>", "antt_bs_pass<4, 2, 32"]),  # lane-split upper pass: bsm3_mul / bsm4_mul
    (20, ["antt_bs_pass<4, 0, 8", "antt_bs_pass<4, 1, 32", "antt_bs_pass<4, 2, 32"]),
])
def test_lds_tile_plan_matches_oracle(log_h, kernels, dev):
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, RATE, B.FanPaarTowerField(7)))
    ntt.set_variant(1)
    names = _kernels(ntt)
    print(log_h, names)
    assert len(names) == len(kernels), names
    for want, got in zip(kernels, names):
        assert want in got, (want, got)
    assert np.array_equal(_forward(ntt, log_h, dev), _oracle(log_h))


@gpu
@pytest.mark.parametrize("log_h", [12, 13, 18, 20])
def test_default_plan_matches_oracle(log_h, dev):
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, RATE, B.FanPaarTowerField(7)))
    assert ntt.variant() == 5
    names = _kernels(ntt)
    print(log_h, names)
    # GF(2^8) passes run on register tiles in the default plan, and so do bottom passes of fewer
    # than two tiles per CU (2^12 .. 2^18 here; at 2^20 the launch has 1024 tiles)
    want = {12: ["antt_bs_pass<4, 3, 32"],
            13: ["antt_rr_pass<4, 0, 8", "antt_rr_pass<4, 2, 16"],
            18: ["antt_bs3_pass<0>", "antt_rr_pass<4, 2, 32"],
            20: ["antt_rr_pass<4, 0, 8", "antt_bs_pass<4, 1, 32", "antt_bs_pass<4, 2, 32"]}[log_h]
    assert len(names) == len(want), names
    for w, got in zip(want, names):
        assert w in got, (w, got)
    assert np.array_equal(_forward(ntt, log_h, dev), _oracle(log_h))
