"""One parity run per pass-kernel instance of the additive NTT (kNttInstances, csrc/antt_passes.hpp:
the 40 instantiations the library carries, each at the smallest launch that selects it).

A case is a plan (limbs, variant, log_h, log_rate), a batch and the instances its passes launch. The
forward cases compare the whole output with the oracle bit for bit, and the GF(2^32) cases at rates 0
and 2 run the reference's input stream and compare with its MD5 table as well. The inverse cases use
the check of tests/test_gpu_intt.py: what the inverse returns must go forward, through the oracle, to
the evaluations it was given.

Which kernel runs: pass_kernel_name answers for the forward pass of ONE transform, and every case
asserts it. That is the launched kernel itself wherever the choice does not depend on the tile count
(every GF(2^32) plan, every first and middle register-tile pass, the single pass) or the case is one
transform. The cases of 512 tiles are the launches at two tiles per CU of a 256-CU device, where the
lane-split and unbounded bottom kernels hand over to the others; (19,2) and (21,0) reach 512 tiles
with one transform, so their names are direct too. Two kinds of case are named through the planner's
host-side rules, which tests/cpp/test_host_asan.cpp pins on the CPU: antt_rr_pass<4, 2, 16, 3> runs
only in a batch (256 transforms of 2^13 here; one transform is named <4, 2, 16, 1>), and the inverse
has no name query, so its cases assert the LDS-tile forward names of the same passes, whose roles
the inverse mirrors (forward first pass = inverse last pass)."""
import re

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

gpu = pytest.mark.gpu
TILE_LOG = 12

BS, BS3, INV, RR = "antt_bs_pass<%d, %d, %d>", "antt_bs3_pass<%d>", "antt_inv_bs_pass<%d, %d, %d>", "antt_rr_pass<%d, %d, %d, %d>"

# every instance of the list, as pass_kernel_name spells it
INSTANCES = ([BS % (l, role, f) for l in (1, 4) for role, f in ((0, 8), (0, 32), (1, 32), (2, 32), (3, 32))]
             + [BS3 % 0, BS3 % 1]
             + [INV % (l, role, f) for l in (1, 4) for role, f in ((2, 8), (2, 32), (1, 32), (0, 32), (3, 32))]
             + [RR % (l, role, f, occ) for l in (1, 4)
                for role, f, occ in ((0, 8, 1), (0, 16, 1), (0, 32, 1), (1, 16, 1), (1, 32, 1), (2, 16, 3), (2, 32, 3), (3, 16, 3))]
             + [RR % (4, 2, 16, 1), RR % (4, 2, 32, 1)])

# (limbs, variant, log_h, log_rate, batch) -> the instance each pass launches, in launch order.
# Plans (passes as role/fmax): 12 = single/16; 13 = first/8, last/16; (15,2) = first/16, last/32;
# (19,2) = first/32, last/32; (20,0) = first/8, mid/16, last/32; (21,0) = first/8, mid/32, last/32.
FORWARD = {
    # GF(2^128), small launches: the lane-split upper passes and the unbounded register-tile bottom pass
    (4, 5, 12, 2, 3): [BS % (4, 3, 32)],
    (4, 4, 12, 2, 3): [RR % (4, 3, 16, 3)],
    (4, 1, 13, 1, 3): [BS % (4, 0, 8), BS % (4, 2, 32)],
    (4, 5, 13, 0, 1): [RR % (4, 0, 8, 1), RR % (4, 2, 16, 1)],
    (4, 5, 15, 2, 1): [BS3 % 0, RR % (4, 2, 32, 1)],
    (4, 4, 15, 2, 1): [RR % (4, 0, 16, 1), RR % (4, 2, 32, 1)],
    (4, 5, 20, 0, 1): [RR % (4, 0, 8, 1), BS3 % 1, RR % (4, 2, 32, 1)],
    (4, 4, 20, 0, 1): [RR % (4, 0, 8, 1), RR % (4, 1, 16, 1), RR % (4, 2, 32, 1)],
    # GF(2^128) at 512 tiles
    (4, 4, 13, 0, 256): [RR % (4, 0, 8, 1), RR % (4, 2, 16, 3)],
    (4, 1, 19, 2, 1): [BS % (4, 0, 32), BS % (4, 2, 32)],
    (4, 4, 19, 2, 1): [RR % (4, 0, 32, 1), RR % (4, 2, 32, 3)],
    (4, 5, 21, 0, 1): [RR % (4, 0, 8, 1), BS % (4, 1, 32), BS % (4, 2, 32)],
    (4, 4, 21, 0, 1): [RR % (4, 0, 8, 1), RR % (4, 1, 32, 1), RR % (4, 2, 32, 3)],
    # GF(2^32): one wave per tile, no kernel depends on the tile count
    (1, 1, 12, 2, 1): [BS % (1, 3, 32)],
    (1, 4, 12, 2, 1): [RR % (1, 3, 16, 3)],
    (1, 1, 13, 0, 1): [BS % (1, 0, 8), BS % (1, 2, 32)],
    (1, 4, 13, 0, 1): [RR % (1, 0, 8, 1), RR % (1, 2, 16, 3)],
    (1, 1, 15, 2, 1): [BS % (1, 0, 32), BS % (1, 2, 32)],
    (1, 4, 15, 2, 1): [RR % (1, 0, 16, 1), RR % (1, 2, 32, 3)],
    (1, 4, 19, 2, 1): [RR % (1, 0, 32, 1), RR % (1, 2, 32, 3)],
    (1, 1, 20, 0, 1): [BS % (1, 0, 8), BS % (1, 1, 32), BS % (1, 2, 32)],
    (1, 4, 20, 0, 1): [RR % (1, 0, 8, 1), RR % (1, 1, 16, 1), RR % (1, 2, 32, 3)],
    (1, 4, 21, 0, 1): [RR % (1, 0, 8, 1), RR % (1, 1, 32, 1), RR % (1, 2, 32, 3)],
}
# what pass_kernel_name says where the batch, and not one transform, selects the launched instance
NAMED = {(4, 4, 13, 0, 256): [RR % (4, 0, 8, 1), RR % (4, 2, 16, 1)]}

# (limbs, log_h, log_rate, coset, batch) -> the inverse's instances in ITS launch order (bottom pass first)
INVERSE = {
    (l, log_h, r, coset, batch): [INV % ((l,) + p) for p in passes]
    for l in (1, 4)
    for (log_h, r, coset, batch), passes in {
        (12, 2, 3, 3): [(3, 32)],
        (13, 0, 0, 2): [(0, 32), (2, 8)],
        (15, 2, 2, 1): [(0, 32), (2, 32)],
        (20, 0, 0, 1): [(0, 32), (1, 32), (2, 8)],
    }.items()
}


def test_the_cases_launch_every_instance_of_the_list():
    launched = {n for names in list(FORWARD.values()) + list(INVERSE.values()) for n in names}
    assert len(INSTANCES) == 40 and len(set(INSTANCES)) == 40
    assert launched == set(INSTANCES), (sorted(set(INSTANCES) - launched), sorted(launched - set(INSTANCES)))


def _plan(limbs, variant, log_h, r):
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(7 if limbs == 4 else 5)))
    assert ntt.variant() == 5
    if variant != 5:
        ntt.set_variant(variant)
    return ntt


def _names(ntt, n_passes):
    names = [ntt.pass_kernel_name(i) for i in range(n_passes)]
    with pytest.raises(B.BnError):
        ntt.pass_kernel_name(n_passes)
    return names


def _inputs(limbs, log_h, r, batch):
    """GF(2^32), one transform: the reference's input stream of (log_h, log_rate)."""
    if limbs == 1:
        return np.stack([O.mt_fill(0xDEADBEEF + log_h + r + 0x1000 * b, 1 << log_h) for b in range(batch)])
    return np.stack([O.fill128(0x1257A + 16 * log_h + r + 0x1000 * b, 0x5EED0000 + b, 1 << log_h) for b in range(batch)])


_want = {}


def _oracle(limbs, log_h, r, batch):
    """The oracle's transforms of _inputs, computed once per shape and shared read-only."""
    key = (limbs, log_h, r, batch)
    if key not in _want:
        x = _inputs(limbs, log_h, r, batch)
        w = O.antt128_batch(x, log_h, r) if limbs == 4 else np.stack([O.antt32(xb, log_h, r) for xb in x])
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


@gpu
@pytest.mark.parametrize("case", sorted(FORWARD), ids=lambda c: "L%d-v%d-2^%d-r%d-x%d" % c)
def test_forward_instance_matches_oracle(case, ntt_md5, dev):
    import torch
    limbs, variant, log_h, r, batch = case
    launched = FORWARD[case]
    ntt = _plan(limbs, variant, log_h, r)
    names = _names(ntt, len(launched))
    for name, want in zip(names, NAMED.get(case, launched)):
        assert want + "(" in name, (names, launched)
    tiles = (batch << r) << (log_h - TILE_LOG)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if limbs == 4 and (case in NAMED or tiles >= 512):
        assert tiles >= 2 * cus, "%d tiles are a small launch on %d CUs: other kernels would run" % (tiles, cus)
    elif limbs == 4:
        assert tiles < 2 * cus
    x = _to_dev(_inputs(limbs, log_h, r, batch), dev)
    y = torch.empty(x.numel() << r, dtype=torch.int32, device=dev)
    ntt.forward_device(x, y, batch=batch)
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint32)
    want = _oracle(limbs, log_h, r, batch)
    assert np.array_equal(got.reshape(want.shape), want)
    if limbs == 1 and batch == 1 and r in (0, 2):
        assert O.md5(got) == ntt_md5[str(r)][log_h]


@gpu
@pytest.mark.parametrize("case", sorted(INVERSE), ids=lambda c: "L%d-2^%d-r%d-c%d-x%d" % c)
def test_inverse_instance_undoes_oracle_forward(case, dev):
    import torch
    limbs, log_h, r, coset, batch = case
    launched = INVERSE[case]
    n = 1 << log_h
    # the LDS-tile forward names of the same passes, mirrored: forward pass i is the inverse's pass
    # n_passes - 1 - i, first <-> last, and both families have the GF(2^8) and the GF(2^32) form.
    # (One GF(2^128) transform of these sizes is a small launch: its upper GF(2^16/32) forward passes
    # are named lane-split.)
    ntt = _plan(limbs, 1, log_h, r)
    mirror = {0: 2, 1: 1, 2: 0, 3: 3}
    fwd = []
    for name in reversed(launched):
        l, role, f = map(int, re.match(r"antt_inv_bs_pass<(\d+), (\d+), (\d+)>", name).groups())
        role = mirror[role]
        fwd.append(BS3 % role if l == 4 and f == 32 and role in (0, 1) else BS % (l, role, f))
    for name, want in zip(_names(ntt, len(fwd)), fwd):
        assert want + "(" in name, (name, fwd)
    ntt.set_variant(5)
    if limbs == 4:
        ys = np.stack([O.fill128(0x1A7E1257 + 64 * log_h + 8 * r + coset + 0x1000 * b, 0x5EED0000 + b, n) for b in range(batch)])
    else:
        ys = np.stack([O.mt_fill(0x1A7E1257 + 64 * log_h + 8 * r + coset + 0x1000 * b, n) for b in range(batch)])
    y = _to_dev(ys, dev)
    x = torch.empty_like(y)
    ntt.inverse_device(y, x, coset=coset, batch=batch)
    torch.cuda.synchronize()
    xs = x.cpu().numpy().view(np.uint32).reshape(ys.shape)
    for b in range(batch):
        fw = O.antt128(xs[b], log_h, r) if limbs == 4 else O.antt32(xs[b], log_h, r)
        assert np.array_equal(fw[coset * n:(coset + 1) * n], ys[b]), b
