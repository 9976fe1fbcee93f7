"""The start of a tile in the additive NTT's pass kernels: the outer offset in closed form (two masks
and shifts from the pass's TileStart) and the work-group-uniform twiddle parts as the XOR of one
chunk-table row per six outer / coset bits (plan_tile_starts, csrc/antt_passes.cpp; tile_addr and
uniform_tw_rows, csrc/antt_bs_dev.hpp). tests/test_tile_tables_host.py checks the tables on the CPU;
here every kernel family runs them at the smallest shapes that reach each path, and every case
compares the whole output with the oracle bit for bit:

  log_h 12, rates 0 and 2, batch 3   no outer bits; coset and batch in the tile index
  log_h 13                           one outer bit; the first use of both runs of outer bits
  log_h 18 and 19, rate 0            six and seven outer bits: one chunk against two
  log_h 17, rate 2, batch 2          coset bits in the last chunk, the batch above them
  log_h 20, rate 0, variant 5        the lane-split middle pass
  inverse                            (13, 0), (17, 2, coset 3), (19, 0): what it returns must go forward
                                     through the oracle to the evaluations given (tests/test_gpu_intt.py)
"""
import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu

# (log_h, log_rate, batch, limbs, variant)
FORWARD = ([(12, r, 3, l, v) for r in (0, 2) for l in (4, 1) for v in (1, 4)]
           + [(13, 0, 1, l, v) for l in (4, 1) for v in (1, 4)]
           + [(log_h, 0, 1, 4, v) for log_h in (18, 19) for v in (1, 4, 5)]
           + [(17, 2, 2, 4, v) for v in (1, 4, 5)]
           + [(20, 0, 1, 4, 5)])
# (log_h, log_rate, coset, limbs)
INVERSE = [(log_h, r, coset, l) for (log_h, r, coset) in ((13, 0, 0), (17, 2, 3), (19, 0, 0)) for l in (4, 1)]


def _plan(limbs, variant, log_h, r):
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(7 if limbs == 4 else 5)))
    if variant != ntt.variant():
        ntt.set_variant(variant)
    assert ntt.variant() == variant
    return ntt


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


_cache = {}


def _case(limbs, log_h, r, batch):
    """Inputs and the oracle's transforms of them, computed once per shape and shared read-only."""
    key = (limbs, log_h, r, batch)
    if key not in _cache:
        n = 1 << log_h
        if limbs == 4:
            x = np.stack([O.fill128(0x711E0000 + 16 * log_h + r + 0x1000 * b, 0x5EED0000 + b, n) for b in range(batch)])
            want = O.antt128_batch(x, log_h, r)
        else:
            x = np.stack([O.mt_fill(0x711E0000 + 16 * log_h + r + 0x1000 * b, n) for b in range(batch)])
            want = np.stack([O.antt32(xb, log_h, r) for xb in x])
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (x, want)
    return _cache[key]


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: "2^%d-r%d-x%d-L%d-v%d" % c)
def test_forward_matches_oracle(case, dev):
    import torch
    log_h, r, batch, limbs, variant = case
    x_np, want = _case(limbs, log_h, r, batch)
    ntt = _plan(limbs, variant, log_h, r)
    x = _to_dev(x_np, dev)
    y = torch.empty(x.numel() << r, dtype=torch.int32, device=dev)
    ntt.forward_device(x, y, batch=batch)
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint32).reshape(want.shape)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", INVERSE, ids=lambda c: "2^%d-r%d-c%d-L%d" % c)
def test_inverse_undoes_oracle_forward(case, dev):
    import torch
    log_h, r, coset, limbs = case
    n = 1 << log_h
    ntt = _plan(limbs, 5, log_h, r)
    if limbs == 4:
        y_np = O.fill128(0x711E1A7E + 64 * log_h + 8 * r + coset, 0x5EED0000, n)
    else:
        y_np = O.mt_fill(0x711E1A7E + 64 * log_h + 8 * r + coset, n)
    y = _to_dev(y_np, dev)
    x = torch.empty_like(y)
    ntt.inverse_device(y, x, coset=coset)
    torch.cuda.synchronize()
    x_np = x.cpu().numpy().view(np.uint32).reshape(y_np.shape)
    fw = O.antt128(x_np, log_h, r) if limbs == 4 else O.antt32(x_np, log_h, r)
    assert np.array_equal(fw[coset * n:(coset + 1) * n], y_np)
