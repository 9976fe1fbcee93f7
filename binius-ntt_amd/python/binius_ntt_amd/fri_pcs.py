"""A FRI-Binius opening proof over the C ABI: a reference protocol driver, no kernels of its own.

It joins the device calls of the package into one evaluation proof for a multilinear polynomial with
2^log_h GF(2^128) coefficients x[w]: "x~(z) = v", where z_i goes with bit i of w, and, by ring-switching
(below), into one for a GF(2)-valued multilinear committed 128 bits to an element. Query count,
grinding and the security level are the caller's business; packed GF(2^8) and GF(2^32) witnesses and
multi-GPU are out of scope.

The construction. The sumcheck binds the highest variable first, the fold the lowest index bit first,
and round k of both must take the same challenge rho_k. So the sumcheck runs over the coefficient
column in bit-reversed index order, x'[y] = x[rev(y)] (bit_reverse), against E' = eq_expand(log_h, z)
with z's coordinates in natural order: round k of the sumcheck then binds bit k of w, as fold round k
does. With claim_0 = v, every round satisfies p_k(0) ^ p_k(1) == claim_k and claim_{k+1} = p_k(rho_k),
and the last claim is eq(z, rho) * c, where c is the value of every element of the fully folded
codeword.

  commit(ntt, coeffs_dev, schedule)      forward NTT, Merkle tree with leaves of 2^schedule[0] elements
  prove_eval(state, z, n_queries, t)     sumcheck rounds interleaved with folds and commitments, then
                                         the query openings
  verify_eval(...)                       host only: no device, no plan
  prove_eval_packed(state, r, n_queries, t), verify_eval_packed(...)
                                         the same for a GF(2) witness (ring-switching, below)

`schedule` is the list of fold arities: it sums to log_h, every arity is in 1..8, log_h >= 5 (the
bitsliced sumcheck column needs whole 32-element blocks). Codeword i (i = 0 .. len(schedule) - 1) is
the codeword after schedule[:i] rounds, 2^(log_h + log_rate - sum(schedule[:i])) elements, committed
with leaves of 2^schedule[i] elements: the elements one fold call of that arity takes to one output
element. The last fold leaves 2^log_rate elements, sent in the clear.

The transcript, byte for byte. The state is 32 bytes.
  start        state = SHA-256("binius-ntt-amd/fri-pcs/v1" || label)
  absorb(m)    state = SHA-256(state || 0x00 || m)
  draw         state = SHA-256(state || 0x01); the draw is the new state
  challenge    a draw; its first 16 bytes as four little-endian uint32 words (limb 0 first)
  query(L)     a draw; its first 8 bytes as a little-endian integer, masked to the low L bits
Both sides absorb and draw in this order:
  1. absorb the header: the little-endian uint32 words log_h, log_rate, n_queries, len(schedule) and
     the schedule's entries
  2. absorb root_0 (32 bytes), z (log_h x 16 bytes, z_0 first, four little-endian limbs each), v (16 bytes)
  3. for k = 0 .. log_h - 1: absorb the round's points p_k(0), p_k(1), p_k(2) (48 bytes); rho_k = challenge.
     When k + 1 completes schedule entry i (k + 1 == sum(schedule[:i+1])): absorb root_{i+1}, or for
     the last entry the final codeword (2^log_rate x 16 bytes)
  4. n_queries times: j = query(log_h + log_rate - schedule[0]), a leaf index of codeword 0
Query j opens leaf j >> sum(schedule[1:i+1]) of codeword i; folding that leaf gives the element at
slot (index & (2^schedule[i+1] - 1)) of the next codeword's opened leaf, and for the last codeword
element `index` of the final codeword.

Ring-switching for GF(2) witnesses (Diamond-Posen, "Polylogarithmic Proofs for Multilinears over
Binary Towers", section 4). L = GF(2^128); beta_v is the element whose only set bit is bit v (bit
v % 32 of limb v / 32, limb 0 first; beta_0 = 1): the bit basis of L over GF(2).
  witness      t has 2^l bits, l >= 12; variable i goes with bit i of the bit index
  packing      t'[w] = sum_v t[128 w + v] beta_v (little-endian bit packing): 2^n elements, n = l - 7,
               variable 7 + j with bit j of w. commit() commits t' as it is, with a plan of log_h = n
  point        r = (r_0 .. r_{l-1}), r_low = r[0:7], r_high = r[7:l]; E[w] = eq(r_high, w) =
               prod_j (bit_j(w) ? r_high,j : 1 ^ r_high,j); the claim is s = t~(r)
  1. the prover sends s^_v = XOR over w with bit_v(t'[w]) = 1 of E[w], v = 0 .. 127 (rs_partial_evals)
  2. row check: s == sum_v eq(r_low, v) s^_v, r_low,i with bit i of v (rs_row_check)
  3. the verifier draws r'' in L^7; B[u] = eq(r'', u), r''_i with bit i of u (rs_batch_table). With
     s^row_u = sum_v bit_u(s^_v) beta_v (the transpose of s^ as a 128 x 128 bit matrix), the sumcheck's
     claim is s_0 = sum_u B[u] s^row_u (rs_sumcheck_claim)
  4. the sumcheck runs over [A, t'], A[w] = XOR over u with bit_u(E[w]) = 1 of B[u] (gf128_linear_map
     of the eq column with matrix B): sum_w A[w] t'[w] = s_0. It is interleaved with the folds as
     above; in the driver's order the columns are A' = map(eq_expand(n, r_high)) and bit_reverse(t')
  5. the last claim is A~(rho) * c with A~(rho) = sum_u B[u] e_u, where e = sum_u beta_u (x) e_u is the
     tensor-algebra element prod_j (1 (x) (1 ^ rho_j) + r_high,j (x) 1) (rs_eq_eval)
The packed protocol's transcript, with the same Transcript class:
  1. absorb b"ring-switch/gf2" followed by the little-endian uint32 words l, log_rate, n_queries,
     len(schedule) and the schedule's entries (one message); the schedule sums to n = l - 7
  2. absorb root_0 (32 bytes), r (l x 16 bytes, r_0 first), s (16 bytes) (one message)
  3. absorb s^ (128 x 16 bytes, s^_0 first); r''_0 .. r''_6 = seven challenge draws
  4. the rounds k = 0 .. n - 1 exactly as step 3 above, with claim_0 = s_0
  5. the queries exactly as step 4 above
The verifier performs, in order: the row check, the sumcheck chain from s_0, claim_n ==
rs_eq_eval(r_high, rho, r'') * final[0] with a constant final codeword, the queries.
"""
import hashlib

import numpy as np

from . import (Sumcheck, bit_reverse, eq_eval, eq_expand, evaluate_univariate_given_points, fri_fold_leaf, gf128_linear_map,
               merkle_commit, merkle_open, merkle_open_bytes, merkle_tree_digests, merkle_verify, rs_batch_table, rs_eq_eval,
               rs_partial_evals, rs_row_check, rs_sumcheck_claim)

DOMAIN = b"binius-ntt-amd/fri-pcs/v1"
PACKED_TAG = b"ring-switch/gf2"
LOG_PACK = 7  # 128 bits to a GF(2^128) element


class Transcript:
    """The SHA-256 chain of the module docstring."""

    def __init__(self, label=b""):
        self.state = hashlib.sha256(DOMAIN + bytes(label)).digest()

    def absorb(self, data):
        self.state = hashlib.sha256(self.state + b"\x00" + bytes(data)).digest()

    def _draw(self):
        self.state = hashlib.sha256(self.state + b"\x01").digest()
        return self.state

    def challenge(self):
        return np.frombuffer(self._draw()[:16], dtype="<u4").astype(np.uint32)

    def query(self, log_range):
        return int.from_bytes(self._draw()[:8], "little") & ((1 << log_range) - 1)


class Commitment:
    def __init__(self, root, log_h, log_rate, schedule):
        self.root, self.log_h, self.log_rate, self.schedule = bytes(root), log_h, log_rate, list(schedule)


class ProverState:
    """What the prover keeps between commit and prove_eval: the plan, the coefficients, codeword 0 and
    its tree (device tensors)."""

    def __init__(self, ntt, coeffs, codeword, tree, schedule, root):
        self.ntt, self.coeffs, self.codeword, self.tree, self.schedule, self.root = ntt, coeffs, codeword, tree, list(schedule), root
        self.timing = {}  # seconds of the last prove_eval: sumcheck, folds, commits, opens


class Proof:
    """round_points: (log_h, 3, 4) uint32, p_k(0), p_k(1), p_k(2); roots: the 32-byte roots of codewords
    1 .. len(schedule) - 1; final: (2^log_rate, 4) uint32, the last codeword; openings[i]: (n_queries,
    merkle_open_bytes) uint8, the records of codeword i in query order; shat (the packed protocol
    only): (128, 4) uint32, the partial evaluations."""

    def __init__(self, round_points, roots, final, openings, v=None, shat=None):
        self.round_points, self.roots, self.final, self.openings = round_points, list(roots), final, list(openings)
        self.v = v  # the prover's value of x~(z) (the round-0 sum; packed: of t~(r)); the verifier takes it as an argument
        self.shat = shat


def check_schedule(log_h, log_rate, schedule):
    sch = [int(a) for a in schedule]
    if not sch or any(a < 1 or a > 8 for a in sch) or sum(sch) != log_h:
        raise ValueError("the schedule's arities must be in 1..8 and sum to log_h = %d (got %s)" % (log_h, sch))
    if log_h < 5 or log_h + log_rate > 30 or not 0 <= log_rate <= 4:
        raise ValueError("need 5 <= log_h, 0 <= log_rate <= 4, log_h + log_rate <= 30")
    return sch


def _header(log_h, log_rate, n_queries, schedule):
    return np.array([log_h, log_rate, n_queries, len(schedule)] + list(schedule), dtype="<u4").tobytes()


def _words(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(shape)).astype("<u4")


def _mul(a, b):
    """a * b in GF(2^128) by the library's host arithmetic: the line through (0, 0) and (1, a) at b."""
    return evaluate_univariate_given_points(b, np.stack([np.zeros(4, np.uint32), np.asarray(a, np.uint32)]))


def _tree_root(tree):
    return tree[-32:].cpu().numpy().tobytes()


def commit(ntt, coeffs_dev, schedule):
    """Encodes the 2^log_h coefficients in the device tensor `coeffs_dev` (4 * 2^log_h words) with the
    GF(2^128) plan `ntt` and commits to the codeword. Returns (Commitment, ProverState)."""
    import torch
    log_h, log_rate = ntt.conf.log_h, ntt.conf.log_rate
    sch = check_schedule(log_h, log_rate, schedule)
    dev = coeffs_dev.device
    with torch.cuda.device(dev):
        codeword = torch.empty(4 << (log_h + log_rate), dtype=torch.int32, device=dev)
        ntt.forward_device(coeffs_dev, codeword)
        log_leaves = log_h + log_rate - sch[0]
        tree = torch.empty(32 * merkle_tree_digests(log_leaves), dtype=torch.uint8, device=dev)
        merkle_commit(codeword, log_leaves, sch[0], tree)
        root = _tree_root(tree)
    return Commitment(root, log_h, log_rate, sch), ProverState(ntt, coeffs_dev, codeword, tree, sch, root)


def _prove_rounds(state, sc, pts, n_queries, transcript, timing, last_factor, what):
    """Steps 3 and 4 for the prover `sc`, whose round-0 points are `pts`: the sumcheck rounds
    interleaved with the folds and commitments, the prover's own check of the identity the verifier
    ends on (the last sum is last_factor(rho) times the folded codeword's value), and the query
    openings. Adds its seconds to `timing`; returns (round_points, roots, final, openings)."""
    import time

    import torch
    ntt, sch = state.ntt, state.schedule
    log_h, log_rate = ntt.conf.log_h, ntt.conf.log_rate
    dev = state.coeffs.device
    t_sum = t_fold = t_commit = t_open = 0.0
    round_points, rho, roots = [], [], []
    committed = [(state.codeword, state.tree)]  # codeword i and its tree
    cur, entry, entry_end = state.codeword, 0, sch[0]
    final = None
    for k in range(log_h):
        t0 = time.perf_counter()
        if k:
            _, pts = sc.this_round_messages()
        round_points.append(pts)
        transcript.absorb(pts.astype("<u4").tobytes())
        rho.append(transcript.challenge())
        sc.move_to_next_round(rho[k])
        t_sum += time.perf_counter() - t0
        if k + 1 != entry_end:
            continue
        t0 = time.perf_counter()
        a = sch[entry]
        log_out = log_h + log_rate - entry_end
        out = torch.empty(4 << log_out, dtype=torch.int32, device=dev)
        ntt.fri_fold_device(cur, out, entry_end - a, np.stack(rho[entry_end - a:entry_end]))
        torch.cuda.current_stream().synchronize()
        t_fold += time.perf_counter() - t0
        t0 = time.perf_counter()
        if entry + 1 < len(sch):
            a_next = sch[entry + 1]
            tree = torch.empty(32 * merkle_tree_digests(log_out - a_next), dtype=torch.uint8, device=dev)
            merkle_commit(out, log_out - a_next, a_next, tree)
            roots.append(_tree_root(tree))
            transcript.absorb(roots[-1])
            committed.append((out, tree))
            entry_end += a_next
        else:
            final = out.cpu().numpy().view(np.uint32).reshape(-1, 4)
            transcript.absorb(final.astype("<u4").tobytes())
        t_commit += time.perf_counter() - t0
        cur, entry = out, entry + 1
    t0 = time.perf_counter()
    last_sum, _ = sc.this_round_messages()
    sc.close()
    t_sum += time.perf_counter() - t0
    if not np.array_equal(last_sum, _mul(last_factor(np.stack(rho)), final[0])):
        raise RuntimeError(what)

    t0 = time.perf_counter()
    log_leaves0 = log_h + log_rate - sch[0]
    queries = np.array([transcript.query(log_leaves0) for _ in range(n_queries)], dtype=np.int64)
    openings, shift = [], 0
    for i, (data, tree) in enumerate(committed):
        shift += sch[i] if i else 0
        log_leaves = log_h + log_rate - sum(sch[:i + 1])
        idx = torch.from_numpy((queries >> shift).astype(np.int32)).to(dev)
        rec = torch.empty(n_queries * merkle_open_bytes(log_leaves, sch[i]), dtype=torch.uint8, device=dev)
        merkle_open(data, tree, log_leaves, sch[i], idx, rec)
        openings.append(rec.cpu().numpy().reshape(n_queries, -1))
    t_open += time.perf_counter() - t0
    for key, sec in (("sumcheck", t_sum), ("folds", t_fold), ("commits", t_commit), ("opens", t_open)):
        timing[key] = timing.get(key, 0.0) + sec
    return np.stack(round_points), roots, final, openings


def prove_eval(state, z, n_queries, transcript):
    """The opening proof of x~(z) for the committed coefficients; z is a (log_h, 4) uint32 host array.
    Returns the Proof; its `v` is x~(z) as the prover computed it (the sumcheck's round-0 sum)."""
    import time

    import torch
    ntt, sch = state.ntt, state.schedule
    log_h, log_rate = ntt.conf.log_h, ntt.conf.log_rate
    z = _words(z, (log_h, 4))
    dev = state.coeffs.device
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        cols = torch.empty(2, 4 << log_h, dtype=torch.int32, device=dev)
        eq_expand(log_h, z, cols[0], bitsliced=True)
        bit_reverse(state.coeffs, cols[1], log_h, bitsliced=True)
        sc = Sumcheck(log_h, 2, True, cols, device=dev.index)
        v, pts = sc.this_round_messages()
        timing = {"sumcheck": time.perf_counter() - t0}

        transcript.absorb(_header(log_h, log_rate, n_queries, sch))
        transcript.absorb(state.root + z.tobytes() + v.astype("<u4").tobytes())
        round_points, roots, final, openings = _prove_rounds(
            state, sc, pts, n_queries, transcript, timing, lambda rho: eq_eval(z.astype(np.uint32), rho),
            "prove_eval: the last sumcheck claim is not eq(z, rho) times the folded codeword's value")
    state.timing = timing
    return Proof(round_points, roots, final, openings, v)


def prove_eval_packed(state, r, n_queries, transcript):
    """The opening proof of t~(r) for a GF(2) witness t of 2^l bits whose packed column t' (2^(l-7)
    elements) `state` commits to; r is an (l, 4) uint32 host array. Returns the Proof with `shat`;
    its `v` is s = t~(r) as the prover computed it (the row check's right-hand side). state.timing
    gains "ring_switch": the seconds of the partial evaluations and the linear map."""
    import time

    import torch
    ntt, sch = state.ntt, state.schedule
    n, log_rate = ntt.conf.log_h, ntt.conf.log_rate
    r = _words(r, (n + LOG_PACK, 4))
    r_low, r_high = r[:LOG_PACK].astype(np.uint32), r[LOG_PACK:].astype(np.uint32)
    dev = state.coeffs.device
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        cols = torch.empty(2, 4 << n, dtype=torch.int32, device=dev)
        eq_expand(n, r_high, cols[0], bitsliced=True)
        bit_reverse(state.coeffs, cols[1], n, bitsliced=True)
        timing = {"sumcheck": time.perf_counter() - t0}
        t0 = time.perf_counter()
        shat_dev = torch.empty(512, dtype=torch.int32, device=dev)
        rs_partial_evals(cols[1], cols[0], n, shat_dev)
        shat = shat_dev.cpu().numpy().view(np.uint32).reshape(128, 4)
        s = rs_row_check(shat, r_low)
        timing["ring_switch"] = time.perf_counter() - t0

        transcript.absorb(PACKED_TAG + _header(n + LOG_PACK, log_rate, n_queries, sch))
        transcript.absorb(state.root + r.tobytes() + s.astype("<u4").tobytes())
        transcript.absorb(shat.astype("<u4").tobytes())
        r2 = np.stack([transcript.challenge() for _ in range(LOG_PACK)])

        t0 = time.perf_counter()
        gf128_linear_map(cols[0], cols[0], rs_batch_table(r2), bitsliced=True)
        torch.cuda.current_stream().synchronize()
        timing["ring_switch"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        sc = Sumcheck(n, 2, True, cols, device=dev.index)
        s0, pts = sc.this_round_messages()
        timing["sumcheck"] += time.perf_counter() - t0
        if not np.array_equal(s0, rs_sumcheck_claim(shat, r2)):
            sc.close()
            raise RuntimeError("prove_eval_packed: the sum of A * t' is not the claim s_0 of the partial evaluations")
        round_points, roots, final, openings = _prove_rounds(
            state, sc, pts, n_queries, transcript, timing, lambda rho: rs_eq_eval(r_high, rho, r2),
            "prove_eval_packed: the last sumcheck claim is not A~(rho) times the folded codeword's value")
    state.timing = timing
    return Proof(round_points, roots, final, openings, s, shat)


def _parse_proof(log_h, log_rate, sch, root0, proof, n_queries):
    """The proof's parts in the verifier's types, or None if one is malformed: (pts, final, roots,
    log_leaves, recs)."""
    try:
        pts = _words(proof.round_points, (log_h, 3, 4))
        final = _words(proof.final, (1 << log_rate, 4))
        roots = [bytes(root0)] + [bytes(r) for r in proof.roots]
        if len(roots) != len(sch) or any(len(r) != 32 for r in roots) or len(proof.openings) != len(sch):
            return None
        log_leaves = [log_h + log_rate - sum(sch[:i + 1]) for i in range(len(sch))]
        recs = []
        for i, o in enumerate(proof.openings):
            o = np.ascontiguousarray(o, dtype=np.uint8)
            if o.shape != (n_queries, merkle_open_bytes(log_leaves[i], sch[i])):
                return None
            recs.append(o)
    except (ValueError, TypeError, AttributeError):
        return None
    return pts, final, roots, log_leaves, recs


def _verify_rounds(log_h, log_rate, sch, parsed, claim, n_queries, transcript, last_factor):
    """Steps 3 and 4 for the verifier: the sumcheck chain from `claim`, the last claim ==
    last_factor(rho) * final[0] with a constant final codeword, the queries."""
    pts, final, roots, log_leaves, recs = parsed
    claim, rho, entry, entry_end = claim.astype(np.uint32), [], 0, sch[0]
    for k in range(log_h):
        p = pts[k].astype(np.uint32)
        if not np.array_equal(p[0] ^ p[1], claim):
            return False
        transcript.absorb(pts[k].tobytes())
        rho.append(transcript.challenge())
        claim = evaluate_univariate_given_points(rho[k], p)
        if k + 1 == entry_end:
            entry += 1
            if entry < len(sch):
                transcript.absorb(roots[entry])
                entry_end += sch[entry]
            else:
                transcript.absorb(final.tobytes())
    rho = np.stack(rho)
    final = final.astype(np.uint32)
    if not (final == final[0]).all():
        return False
    if not np.array_equal(claim, _mul(last_factor(rho), final[0])):
        return False

    # ---- the queries
    for q in range(n_queries):
        j = transcript.query(log_leaves[0])
        want = None  # what the previous codeword's leaf folded to
        rnd = 0
        for i, a in enumerate(sch):
            if i:
                j >>= a
            rec = recs[i][q]
            if not merkle_verify(roots[i], log_leaves[i], a, j, rec):
                return False
            leaf = np.frombuffer(rec[:16 << a].tobytes(), dtype="<u4").astype(np.uint32).reshape(-1, 4)
            if want is not None and not np.array_equal(leaf[want[0]], want[1]):
                return False
            folded = fri_fold_leaf(log_h, log_rate, rnd, j, leaf, rho[rnd:rnd + a])
            rnd += a
            if i + 1 < len(sch):
                want = (j & ((1 << sch[i + 1]) - 1), folded)
            elif not np.array_equal(final[j], folded):
                return False
    return True


def verify_eval(log_h, log_rate, schedule, root0, z, v, proof, n_queries, transcript):
    """True if `proof` shows x~(z) = v for the polynomial committed to by root0. Host arithmetic only:
    no device, no plan. A malformed proof is rejected, not an error."""
    sch = check_schedule(log_h, log_rate, schedule)
    try:
        z = _words(z, (log_h, 4))
        v = _words(v, (4,))
    except (ValueError, TypeError, AttributeError):
        return False
    parsed = _parse_proof(log_h, log_rate, sch, root0, proof, n_queries)
    if parsed is None:
        return False
    transcript.absorb(_header(log_h, log_rate, n_queries, sch))
    transcript.absorb(parsed[2][0] + z.tobytes() + v.tobytes())
    return _verify_rounds(log_h, log_rate, sch, parsed, v, n_queries, transcript, lambda rho: eq_eval(z.astype(np.uint32), rho))


def verify_eval_packed(log_bits, log_rate, schedule, root0, r, s, proof, n_queries, transcript):
    """True if `proof` shows t~(r) = s for the GF(2) multilinear t of 2^log_bits bits whose packed
    column root0 commits to; the schedule sums to log_bits - 7. Host arithmetic only: no device, no
    plan. A malformed proof is rejected, not an error."""
    n = log_bits - LOG_PACK
    sch = check_schedule(n, log_rate, schedule)
    try:
        r = _words(r, (log_bits, 4))
        s = _words(s, (4,))
        shat = _words(proof.shat, (128, 4))
    except (ValueError, TypeError, AttributeError):
        return False
    parsed = _parse_proof(n, log_rate, sch, root0, proof, n_queries)
    if parsed is None:
        return False
    r_low, r_high = r[:LOG_PACK].astype(np.uint32), r[LOG_PACK:].astype(np.uint32)
    transcript.absorb(PACKED_TAG + _header(log_bits, log_rate, n_queries, sch))
    transcript.absorb(parsed[2][0] + r.tobytes() + s.tobytes())
    transcript.absorb(shat.tobytes())
    r2 = np.stack([transcript.challenge() for _ in range(LOG_PACK)])
    if not np.array_equal(s.astype(np.uint32), rs_row_check(shat.astype(np.uint32), r_low)):
        return False
    s0 = rs_sumcheck_claim(shat.astype(np.uint32), r2)
    return _verify_rounds(n, log_rate, sch, parsed, s0, n_queries, transcript, lambda rho: rs_eq_eval(r_high, rho, r2))
