"""CPU: the opening protocol's verifier (binius_ntt_amd.fri_pcs.verify_eval: host arithmetic, no
device, no plan) on a proof built on the host by the reference rules of tests/_fri_ref.py (the
oracle's sumcheck and NTT, the per-pair fold rule, tests/_merkle_ref.py, the transcript from its byte
specification). The proof is accepted; one flipped bit anywhere in it is rejected."""
import functools

import numpy as np
import pytest

import _fri_ref as F
import _oracle as O
from binius_ntt_amd import fri_pcs

LOG_H, RATE, SCHEDULE, NQ, LABEL = 5, 1, [2, 3], 4, b"host fixture"


@functools.lru_cache(maxsize=None)
def _fixture():
    x = O.fill128(0xC0FFEE + LOG_H, 0x5EED0000, 1 << LOG_H)
    z = O.fill128(0x2E2E, 0x9017, LOG_H)
    return x, z, F.host_proof(x, LOG_H, RATE, SCHEDULE, z, NQ, LABEL)


def _proof(p):
    return fri_pcs.Proof(p["round_points"].copy(), list(p["roots"]), p["final"].copy(), [o.copy() for o in p["openings"]])


def _verify(p, proof, v=None, root0=None, z=None, label=LABEL):
    _, z0, _ = _fixture()
    return fri_pcs.verify_eval(LOG_H, RATE, SCHEDULE, p["root0"] if root0 is None else root0, z0 if z is None else z,
                               p["v"] if v is None else v, proof, NQ, fri_pcs.Transcript(label))


def _flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def test_the_fixture_is_an_evaluation_proof():
    x, z, p = _fixture()
    # the round-0 sum is x~(z), z_i with bit i of the index: the oracle takes the highest variable first
    assert np.array_equal(p["v"], O.multilinear_composition(x, LOG_H, 1, z[::-1]))
    assert p["final"].shape == (1 << RATE, 4) and (p["final"] == p["final"][0]).all()
    assert np.array_equal(p["final"][0], O.multilinear_composition(x, LOG_H, 1, p["rho"][::-1]))
    assert len(set(p["queries"])) > 1


def test_host_proof_is_accepted():
    _, _, p = _fixture()
    assert _verify(p, _proof(p)) is True


def test_transcript_class_follows_the_byte_specification():
    a, b = fri_pcs.Transcript(b"x"), F.RefTranscript(b"x")
    for m in (b"", b"abc", bytes(range(48))):
        a.absorb(m)
        b.absorb(m)
        assert np.array_equal(a.challenge(), b.challenge())
        assert a.query(13) == b.query(13)
    assert a.state == b.state


@pytest.mark.parametrize("what", ["v", "round_point", "last_round_point", "root0", "root", "leaf", "last_leaf", "sibling", "final",
                                  "final_both", "z", "label"])
def test_one_flipped_bit_is_rejected(what):
    _, z, p = _fixture()
    proof = _proof(p)
    kw = {}
    if what == "v":
        kw["v"] = p["v"] ^ np.array([0, 0, 1 << 7, 0], np.uint32)
    elif what == "round_point":
        proof.round_points[1, 2, 3] ^= 1 << 30
    elif what == "last_round_point":
        proof.round_points[LOG_H - 1, 0, 0] ^= 1
    elif what == "root0":
        kw["root0"] = _flip(p["root0"], 100)
    elif what == "root":
        proof.roots[0] = _flip(proof.roots[0], 3)
    elif what == "leaf":
        proof.openings[0][2, 5] ^= 0x10  # an element of query 2's first leaf
    elif what == "last_leaf":
        proof.openings[1][0, 16 * 7 + 1] ^= 1
    elif what == "sibling":
        proof.openings[0][1, (16 << SCHEDULE[0]) + 32 * 2 + 9] ^= 0x80
    elif what == "final":
        proof.final[1, 0] ^= 1
    elif what == "final_both":  # still 2^rate equal elements, but not the folded value
        proof.final[:, 2] ^= 1 << 5
    elif what == "z":
        kw["z"] = z ^ np.array([[0, 1, 0, 0]] + [[0, 0, 0, 0]] * (LOG_H - 1), np.uint32)
    elif what == "label":
        kw["label"] = b"another session"
    assert _verify(p, proof, **kw) is False


def test_malformed_proofs_are_rejected_not_errors():
    _, _, p = _fixture()
    bad = _proof(p)
    bad.roots = []
    assert _verify(p, bad) is False
    bad = _proof(p)
    bad.openings[0] = bad.openings[0][:, :-1]
    assert _verify(p, bad) is False
    bad = _proof(p)
    bad.round_points = bad.round_points[:-1]
    assert _verify(p, bad) is False
    bad = _proof(p)
    bad.final = bad.final[:1]
    assert _verify(p, bad) is False
    with pytest.raises(ValueError):  # the caller's own parameters
        fri_pcs.verify_eval(LOG_H, RATE, [2, 2], p["root0"], _fixture()[1], p["v"], _proof(p), NQ, fri_pcs.Transcript(LABEL))
