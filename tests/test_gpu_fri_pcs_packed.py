"""GPU tests of the packed opening protocol (binius_ntt_amd.fri_pcs): a GF(2) witness of 2^l bits,
commit and prove_eval_packed on the device, verify_eval_packed on the host. The value s comes from the
multilinear evaluation of the unpacked bits embedded as 0/1 elements, not from the prover; the proof is
accepted, every single tampering is rejected, a forged s^ that still passes the row check is rejected
by the sumcheck's claim, and the verifier runs in a process that sees no GPU."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
import _rs_ref as S
import binius_ntt_amd as B
from binius_ntt_amd import fri_pcs

pytestmark = pytest.mark.gpu

SHAPES = [(12, 1, (2, 3)), (15, 2, (3, 4, 1)), (19, 1, (4, 4, 4))]
NQ = 8
LABEL = b"gpu packed test"


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


@functools.lru_cache(maxsize=None)
def _proved(log_bits, rate, schedule):
    """One commitment and one proof per shape, shared by the tests (read-only)."""
    import torch
    dev = torch.device("cuda:0")
    n = log_bits - 7
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(n, rate, B.FanPaarTowerField(7)))
    tp = O.fill128(0xB175 + 64 * log_bits + rate, 0x5EED0000, 1 << n)  # the packed column: random bits
    r = O.fill128(0x2E2E + log_bits, 0x9017, log_bits)
    com, state = fri_pcs.commit(ntt, _to_dev(tp, dev), list(schedule))
    proof = fri_pcs.prove_eval_packed(state, r, NQ, fri_pcs.Transcript(LABEL))
    torch.cuda.synchronize()
    # t~(r) of the 2^l bits as 0/1 elements of GF(2^128), variable i with bit i of the bit index
    bits = np.zeros((1 << log_bits, 4), np.uint32)
    bits[:, 0] = S.unpack_bits(tp)
    s = B.evaluate_multilinear_composition(bits, log_bits, 1, False, np.ascontiguousarray(r[::-1]))
    return dict(ntt=ntt, tp=tp, r=r, com=com, state=state, proof=proof, s=s)


def _copy(proof):
    return fri_pcs.Proof(proof.round_points.copy(), list(proof.roots), proof.final.copy(), [o.copy() for o in proof.openings],
                         shat=proof.shat.copy())


def _verify(p, log_bits, rate, schedule, proof=None, s=None, root0=None):
    return fri_pcs.verify_eval_packed(log_bits, rate, list(schedule), p["com"].root if root0 is None else root0, p["r"],
                                      p["s"] if s is None else s, _copy(p["proof"]) if proof is None else proof, NQ,
                                      fri_pcs.Transcript(LABEL))


def _flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@pytest.mark.parametrize("log_bits,rate,schedule", SHAPES)
def test_proof_is_accepted(log_bits, rate, schedule, dev):
    p = _proved(log_bits, rate, schedule)
    assert np.array_equal(p["proof"].v, p["s"])  # the prover's row-check value is t~(r)
    assert p["proof"].shat.shape == (128, 4)
    f = p["proof"].final
    assert f.shape == (1 << rate, 4) and (f == f[0]).all()
    assert _verify(p, log_bits, rate, schedule) is True


@pytest.mark.parametrize("log_bits,rate,schedule", SHAPES[:2])
def test_partial_evals_in_the_proof_equal_the_reference(log_bits, rate, schedule, dev):
    p = _proved(log_bits, rate, schedule)
    assert np.array_equal(p["proof"].shat, S.partial_evals(p["tp"], S.eq_table_high(p["r"][7:])))


@pytest.mark.parametrize("what", ["s", "shat", "round_point", "root", "leaf", "sibling", "final"])
@pytest.mark.parametrize("log_bits,rate,schedule", SHAPES)
def test_tampering_is_rejected(log_bits, rate, schedule, what, dev):
    p = _proved(log_bits, rate, schedule)
    proof, kw = _copy(p["proof"]), {}
    if what == "s":
        kw["s"] = p["s"] ^ np.array([1, 0, 0, 0], np.uint32)
    elif what == "shat":
        proof.shat[77, 2] ^= 1 << 13
    elif what == "round_point":
        proof.round_points[(log_bits - 7) // 2, 1, 2] ^= 1 << 9
    elif what == "root":
        proof.roots[-1] = _flip(proof.roots[-1], 255)
    elif what == "leaf":
        proof.openings[1][NQ - 1, 3] ^= 0x40
    elif what == "sibling":
        proof.openings[0][0, (16 << schedule[0]) + 7] ^= 1
    elif what == "final":
        proof.final[0, 3] ^= 1 << 31
    assert _verify(p, log_bits, rate, schedule, proof=proof, **kw) is False
    assert _verify(p, log_bits, rate, schedule, root0=_flip(p["com"].root, 0)) is False


@pytest.mark.parametrize("log_bits,rate,schedule", SHAPES)
def test_a_forged_shat_that_passes_the_row_check_is_rejected_by_the_sumcheck_claim(log_bits, rate, schedule, dev):
    p = _proved(log_bits, rate, schedule)
    low = S.ints(p["r"][:7])
    delta = 0xD0D0CAFE << 64 | 5
    # s^_0 ^= d, s^_1 ^= d * eq(r_low, 0) * eq(r_low, 1)^-1: the row check's sum does not move
    d1 = O.mul128(O.mul128(delta, S.eq_low_first(low, 0)), O.inv128(S.eq_low_first(low, 1)))
    proof = _copy(p["proof"])
    proof.shat[0] ^= O._to_words(delta)
    proof.shat[1] ^= O._to_words(d1)
    assert np.array_equal(B.rs_row_check(proof.shat, p["r"][:7]), p["s"])
    assert _verify(p, log_bits, rate, schedule, proof=proof) is False


_CHILD = r"""
import os, pickle, sys
sys.path[:0] = [%r, %r]
import binius_ntt_amd as B
from binius_ntt_amd import fri_pcs
with open(sys.argv[1], "rb") as f:
    a = pickle.load(f)
def run(proof):
    return fri_pcs.verify_eval_packed(a["log_bits"], a["rate"], a["schedule"], a["root"], a["r"], a["s"], proof, a["nq"],
                                      fri_pcs.Transcript(a["label"]))
proof = fri_pcs.Proof(*a["proof"], shat=a["shat"])
ok = run(proof)
proof.shat[5, 0] ^= 1
bad = run(proof)
import torch
print("RESULT", ok, bad, torch.cuda.is_available())
"""


def test_verifier_runs_in_a_process_without_a_gpu(dev, tmp_path):
    log_bits, rate, schedule = SHAPES[0]
    p = _proved(log_bits, rate, schedule)
    pr = p["proof"]
    arg = tmp_path / "proof.pkl"
    with open(arg, "wb") as f:
        pickle.dump(dict(log_bits=log_bits, rate=rate, schedule=list(schedule), root=p["com"].root, r=p["r"], s=p["s"], nq=NQ,
                         label=LABEL, proof=(pr.round_points, pr.roots, pr.final, pr.openings), shat=pr.shat), f)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CHILD % (os.path.join(root, "binius-ntt_amd", "python"), os.path.join(root, "tests")), str(arg)],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # accepted, the tampered one rejected, and the process saw no device
    assert out.stdout.strip().splitlines()[-1] == "RESULT True False False"
