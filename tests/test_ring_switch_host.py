"""CPU: the verifier's side of ring-switching (bn_rs_batch_table, bn_rs_row_check,
bn_rs_sumcheck_claim, bn_rs_eq_eval: host arithmetic, no device) against the brute-force restatement
of tests/_rs_ref.py, the identity the sumcheck proves, and fri_pcs.verify_eval_packed on a proof built
on the host by the reference rules: accepted, and every single tampering rejected."""
import functools

import numpy as np
import pytest

import _oracle as O
import _rs_ref as S
import binius_ntt_amd as B
from binius_ntt_amd import fri_pcs

NQ, LABEL = 4, b"packed host fixture"
SHAPES = [(12, 1, (2, 3)), (15, 2, (3, 4, 1))]


@functools.lru_cache(maxsize=None)
def _point(n):
    """r_high, rho (n, 4), r_low, r2 (7, 4) and a packed column of 2^n elements."""
    r_high = O.fill128(0x4150 + n, 0x1111, n) if n else np.zeros((0, 4), np.uint32)
    rho = O.fill128(0x4151 + n, 0x2222, n) if n else np.zeros((0, 4), np.uint32)
    r_low, r2 = O.fill128(0x4152 + n, 0x3333, 7), O.fill128(0x4153 + n, 0x4444, 7)
    tp = O.fill128(0x4154 + n, 0x5555, 1 << n)
    return r_high, rho, r_low, r2, tp


@pytest.mark.parametrize("n", [1, 5, 8])
def test_host_functions_equal_the_brute_force(n):
    r_high, rho, r_low, r2, tp = _point(n)
    shat = S.partial_evals(tp, S.eq_table_high(r_high))
    assert np.array_equal(B.rs_batch_table(r2), S.batch_table(r2))
    assert np.array_equal(B.rs_row_check(shat, r_low), S.row_check(shat, r_low))
    assert np.array_equal(B.rs_sumcheck_claim(shat, r2), S.sumcheck_claim(shat, r2))
    assert np.array_equal(B.rs_eq_eval(r_high, rho, r2), S.eq_eval_brute(r_high, rho, r2))


def test_eq_eval_of_no_variables_is_the_table_s_first_entry():
    _, _, _, r2, _ = _point(1)
    none = np.zeros((0, 4), np.uint32)
    # e = 1 (x) 1: A~() = B[0]
    assert np.array_equal(B.rs_eq_eval(none, none, r2), B.rs_batch_table(r2)[0])


@pytest.mark.parametrize("n", [1, 5, 8])
def test_the_sumcheck_s_identity(n):
    """sum_w A[w] t'[w] == s_0, and the row check's right-hand side is t~(r)."""
    r_high, _, r_low, r2, tp = _point(n)
    E = S.eq_table_high(r_high)
    shat = S.partial_evals(tp, E)
    A = S.linear_map(E, B.rs_batch_table(r2))
    assert np.array_equal(S.inner(A, tp), B.rs_sumcheck_claim(shat, r2))
    assert np.array_equal(B.rs_row_check(shat, r_low), S.evaluate_bits(S.unpack_bits(tp), np.concatenate([r_low, r_high])))


@functools.lru_cache(maxsize=None)
def _fixture(log_bits, rate, schedule):
    bits = (O.mt_fill(0xB175 + log_bits, (1 << log_bits) // 32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1
    bits = bits.reshape(-1).astype(np.uint8)
    r = O.fill128(0x2E2E + log_bits, 0x9017, log_bits)
    return bits, r, S.host_proof_packed(bits, log_bits, rate, list(schedule), r, NQ, LABEL)


def _proof(p):
    return fri_pcs.Proof(p["round_points"].copy(), list(p["roots"]), p["final"].copy(), [o.copy() for o in p["openings"]],
                         shat=p["shat"].copy())


def _verify(shape, proof, s=None, root0=None, r=None, label=LABEL):
    log_bits, rate, schedule = shape
    _, r0, p = _fixture(*shape)
    return fri_pcs.verify_eval_packed(log_bits, rate, list(schedule), p["root0"] if root0 is None else root0,
                                      r0 if r is None else r, p["s"] if s is None else s, proof, NQ, fri_pcs.Transcript(label))


def _flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_fixture_is_an_evaluation_proof_of_the_bits(shape):
    bits, r, p = _fixture(*shape)
    assert np.array_equal(p["s"], S.evaluate_bits(bits, r))
    assert np.array_equal(p["s0"], S.sumcheck_claim(p["shat"], p["r2"]))
    assert (p["final"] == p["final"][0]).all()
    assert len(set(p["queries"])) > 1


@pytest.mark.parametrize("shape", SHAPES)
def test_host_proof_is_accepted(shape):
    p = _fixture(*shape)[2]
    assert _verify(shape, _proof(p)) is True


@pytest.mark.parametrize("what", ["s", "shat", "shat_last", "round_point", "last_round_point", "root0", "root", "leaf", "sibling",
                                  "final", "final_both", "r_low", "r_high", "label"])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_tampering_is_rejected(shape, what):
    log_bits, rate, schedule = shape
    _, r, p = _fixture(*shape)
    proof, kw = _proof(p), {}
    if what == "s":
        kw["s"] = p["s"] ^ np.array([0, 0, 1 << 7, 0], np.uint32)
    elif what == "shat":
        proof.shat[0, 0] ^= 1
    elif what == "shat_last":
        proof.shat[127, 3] ^= 1 << 31
    elif what == "round_point":
        proof.round_points[1, 2, 3] ^= 1 << 30
    elif what == "last_round_point":
        proof.round_points[log_bits - 8, 0, 0] ^= 1
    elif what == "root0":
        kw["root0"] = _flip(p["root0"], 100)
    elif what == "root":
        proof.roots[0] = _flip(proof.roots[0], 3)
    elif what == "leaf":
        proof.openings[0][2, 5] ^= 0x10
    elif what == "sibling":
        proof.openings[0][1, (16 << schedule[0]) + 32 * 2 + 9] ^= 0x80
    elif what == "final":
        proof.final[1, 0] ^= 1
    elif what == "final_both":
        proof.final[:, 2] ^= 1 << 5
    elif what == "r_low":
        r2 = r.copy()
        r2[3, 1] ^= 1
        kw["r"] = r2
    elif what == "r_high":
        r2 = r.copy()
        r2[log_bits - 1, 0] ^= 2
        kw["r"] = r2
    elif what == "label":
        kw["label"] = b"another session"
    assert _verify(shape, proof, **kw) is False


def test_a_forged_shat_that_passes_the_row_check_fails_the_sumcheck_claim():
    shape = SHAPES[0]
    _, r, p = _fixture(*shape)
    low = S.ints(r[:7])
    delta = 0x1234567
    # s^_0 ^= d, s^_1 ^= d * eq(r_low, 0) / eq(r_low, 1): the row check's sum does not move
    d1 = O.mul128(O.mul128(delta, S.eq_low_first(low, 0)), O.inv128(S.eq_low_first(low, 1)))
    proof = _proof(p)
    proof.shat[0] ^= O._to_words(delta)
    proof.shat[1] ^= O._to_words(d1)
    assert np.array_equal(B.rs_row_check(proof.shat, r[:7]), p["s"])
    assert _verify(shape, proof) is False


def test_malformed_proofs_are_rejected_not_errors():
    shape = SHAPES[0]
    log_bits, rate, schedule = shape
    _, r, p = _fixture(*shape)
    bad = _proof(p)
    bad.shat = None
    assert _verify(shape, bad) is False
    bad = _proof(p)
    bad.shat = bad.shat[:127]
    assert _verify(shape, bad) is False
    bad = _proof(p)
    bad.roots = []
    assert _verify(shape, bad) is False
    bad = _proof(p)
    bad.round_points = bad.round_points[:-1]
    assert _verify(shape, bad) is False
    with pytest.raises(ValueError):  # the caller's own parameters: the schedule sums to log_bits - 7
        fri_pcs.verify_eval_packed(log_bits, rate, [2, 2], p["root0"], r, p["s"], _proof(p), NQ, fri_pcs.Transcript(LABEL))
