"""GPU tests of the opening protocol (binius_ntt_amd.fri_pcs): commit and prove_eval on the device,
verify_eval on the host. The value v comes from the multilinear evaluation, not from the prover; the
proof is accepted, every single tampering is rejected, the verifier's leaf fold reproduces the device
fold at every query and round, and the verifier runs in a process that sees no GPU."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B
from binius_ntt_amd import fri_pcs

pytestmark = pytest.mark.gpu

SHAPES = [(8, 2, (3, 4, 1)), (12, 1, (4, 4, 4))]
NQ = 8
LABEL = b"gpu test"


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


def _to_np(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _proved(log_h, rate, schedule):
    """One commitment and one proof per shape, shared by the tests (read-only)."""
    import torch
    dev = torch.device("cuda:0")
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, rate, B.FanPaarTowerField(7)))
    x = O.fill128(0xFC5 + 64 * log_h + rate, 0x5EED0000, 1 << log_h)
    z = O.fill128(0x2E2E + log_h, 0x9017, log_h)
    com, state = fri_pcs.commit(ntt, _to_dev(x, dev), list(schedule))
    proof = fri_pcs.prove_eval(state, z, NQ, fri_pcs.Transcript(LABEL))
    torch.cuda.synchronize()
    v = B.evaluate_multilinear_composition(x, log_h, 1, False, np.ascontiguousarray(z[::-1]))
    return dict(ntt=ntt, x=x, z=z, com=com, state=state, proof=proof, v=v)


def _copy(proof):
    return fri_pcs.Proof(proof.round_points.copy(), list(proof.roots), proof.final.copy(), [o.copy() for o in proof.openings])


def _verify(p, log_h, rate, schedule, proof=None, v=None, root0=None):
    return fri_pcs.verify_eval(log_h, rate, list(schedule), p["com"].root if root0 is None else root0, p["z"],
                               p["v"] if v is None else v, _copy(p["proof"]) if proof is None else proof, NQ,
                               fri_pcs.Transcript(LABEL))


def _flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@pytest.mark.parametrize("log_h,rate,schedule", SHAPES)
def test_proof_is_accepted(log_h, rate, schedule, dev):
    p = _proved(log_h, rate, schedule)
    assert np.array_equal(p["proof"].v, p["v"])  # the prover's round-0 sum is x~(z)
    assert p["com"].root == p["state"].tree[-32:].cpu().numpy().tobytes()
    assert _verify(p, log_h, rate, schedule) is True


@pytest.mark.parametrize("log_h,rate,schedule", SHAPES)
def test_final_codeword_is_constant(log_h, rate, schedule, dev):
    f = _proved(log_h, rate, schedule)["proof"].final
    assert f.shape == (1 << rate, 4)
    assert (f == f[0]).all()


@pytest.mark.parametrize("what", ["v", "round_point", "root", "leaf", "sibling", "final"])
@pytest.mark.parametrize("log_h,rate,schedule", SHAPES)
def test_tampering_is_rejected(log_h, rate, schedule, what, dev):
    p = _proved(log_h, rate, schedule)
    proof, kw = _copy(p["proof"]), {}
    if what == "v":
        kw["v"] = p["v"] ^ np.array([1, 0, 0, 0], np.uint32)
    elif what == "round_point":
        proof.round_points[log_h // 2, 1, 2] ^= 1 << 9
    elif what == "root":
        proof.roots[-1] = _flip(proof.roots[-1], 255)
    elif what == "leaf":
        proof.openings[1][NQ - 1, 3] ^= 0x40
    elif what == "sibling":
        proof.openings[0][0, (16 << schedule[0]) + 7] ^= 1
    elif what == "final":
        proof.final[0, 3] ^= 1 << 31
    assert _verify(p, log_h, rate, schedule, proof=proof, **kw) is False
    assert _verify(p, log_h, rate, schedule, root0=_flip(p["com"].root, 0)) is False


@pytest.mark.parametrize("log_h,rate,schedule", SHAPES)
def test_leaf_fold_equals_the_device_fold_at_every_query_and_round(log_h, rate, schedule, dev):
    import torch
    p = _proved(log_h, rate, schedule)
    ntt, proof = p["ntt"], p["proof"]
    # the transcript replayed: the challenges and the queries
    t = fri_pcs.Transcript(LABEL)
    t.absorb(fri_pcs._header(log_h, rate, NQ, list(schedule)))
    t.absorb(p["com"].root + p["z"].astype("<u4").tobytes() + p["v"].astype("<u4").tobytes())
    rho, ends = [], np.cumsum(schedule).tolist()
    for k in range(log_h):
        t.absorb(proof.round_points[k].astype("<u4").tobytes())
        rho.append(t.challenge())
        if k + 1 in ends:
            i = ends.index(k + 1)
            t.absorb(proof.roots[i] if i + 1 < len(schedule) else proof.final.astype("<u4").tobytes())
    rho = np.stack(rho)
    queries = [t.query(log_h + rate - schedule[0]) for _ in range(NQ)]
    # the device folds of the committed codeword
    cw = [p["state"].codeword]
    rnd = 0
    for a in schedule:
        out = torch.empty(cw[-1].numel() >> a, dtype=torch.int32, device=dev)
        ntt.fri_fold_device(cw[-1], out, rnd, rho[rnd:rnd + a])
        cw.append(out)
        rnd += a
    torch.cuda.synchronize()
    cw = [_to_np(c) for c in cw]
    assert np.array_equal(cw[-1], proof.final)
    for q, j in enumerate(queries):
        rnd = 0
        for i, a in enumerate(schedule):
            if i:
                j >>= a
            leaf = np.frombuffer(proof.openings[i][q, :16 << a].tobytes(), dtype=np.uint32).reshape(-1, 4)
            assert np.array_equal(leaf, cw[i][j << a:(j + 1) << a]), (q, i)
            assert np.array_equal(B.fri_fold_leaf(log_h, rate, rnd, j, leaf, rho[rnd:rnd + a]), cw[i + 1][j]), (q, i)
            rnd += a


_CHILD = r"""
import os, pickle, sys
sys.path[:0] = [%r, %r]
import binius_ntt_amd as B
from binius_ntt_amd import fri_pcs
with open(sys.argv[1], "rb") as f:
    a = pickle.load(f)
proof = fri_pcs.Proof(*a["proof"])
ok = fri_pcs.verify_eval(a["log_h"], a["rate"], a["schedule"], a["root"], a["z"], a["v"], proof, a["nq"], fri_pcs.Transcript(a["label"]))
proof.final[0, 0] ^= 1
bad = fri_pcs.verify_eval(a["log_h"], a["rate"], a["schedule"], a["root"], a["z"], a["v"], proof, a["nq"], fri_pcs.Transcript(a["label"]))
import torch
print("RESULT", ok, bad, torch.cuda.is_available())
"""


def test_verifier_runs_in_a_process_without_a_gpu(dev, tmp_path):
    log_h, rate, schedule = SHAPES[0]
    p = _proved(log_h, rate, schedule)
    pr = p["proof"]
    arg = tmp_path / "proof.pkl"
    with open(arg, "wb") as f:
        pickle.dump(dict(log_h=log_h, rate=rate, schedule=list(schedule), root=p["com"].root, z=p["z"], v=p["v"], nq=NQ, label=LABEL,
                         proof=(pr.round_points, pr.roots, pr.final, pr.openings)), f)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CHILD % (os.path.join(root, "binius-ntt_amd", "python"), os.path.join(root, "tests")), str(arg)],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # accepted, the tampered one rejected, and the process saw no device
    assert out.stdout.strip().splitlines()[-1] == "RESULT True False False"
