"""A FRI-Binius opening proof over the C ABI: a reference protocol driver, no kernels of its own.

It joins the device calls of the package into one evaluation proof for a multilinear polynomial with
2^log_h GF(2^128) coefficients x[w]: "x~(z) = v", where z_i goes with bit i of w. Query count, grinding
and the security level are the caller's business; ring-switching for small-field witnesses and
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
"""
import hashlib

import numpy as np

from . import (Sumcheck, bit_reverse, eq_eval, eq_expand, evaluate_univariate_given_points, fri_fold_leaf,
               merkle_commit, merkle_open, merkle_open_bytes, merkle_tree_digests, merkle_verify)

DOMAIN = b"binius-ntt-amd/fri-pcs/v1"


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
    merkle_open_bytes) uint8, the records of codeword i in query order."""

    def __init__(self, round_points, roots, final, openings, v=None):
        self.round_points, self.roots, self.final, self.openings = round_points, list(roots), final, list(openings)
        self.v = v  # the prover's value of x~(z) (the round-0 sum); the verifier takes v as an argument


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


def prove_eval(state, z, n_queries, transcript):
    """The opening proof of x~(z) for the committed coefficients; z is a (log_h, 4) uint32 host array.
    Returns the Proof; its `v` is x~(z) as the prover computed it (the sumcheck's round-0 sum)."""
    import time

    import torch
    ntt, sch = state.ntt, state.schedule
    log_h, log_rate = ntt.conf.log_h, ntt.conf.log_rate
    z = _words(z, (log_h, 4))
    dev = state.coeffs.device
    t_sum = t_fold = t_commit = t_open = 0.0
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        cols = torch.empty(2, 4 << log_h, dtype=torch.int32, device=dev)
        eq_expand(log_h, z, cols[0], bitsliced=True)
        bit_reverse(state.coeffs, cols[1], log_h, bitsliced=True)
        sc = Sumcheck(log_h, 2, True, cols, device=dev.index)
        v, pts = sc.this_round_messages()
        t_sum += time.perf_counter() - t0

        transcript.absorb(_header(log_h, log_rate, n_queries, sch))
        transcript.absorb(state.root + z.tobytes() + v.astype("<u4").tobytes())

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
        # the prover's own check of the identity the verifier ends on: the last sum is eq(z, rho) * c
        t0 = time.perf_counter()
        last_sum, _ = sc.this_round_messages()
        sc.close()
        t_sum += time.perf_counter() - t0
        if not np.array_equal(last_sum, _mul(eq_eval(z.astype(np.uint32), np.stack(rho)), final[0])):
            raise RuntimeError("prove_eval: the last sumcheck claim is not eq(z, rho) times the folded codeword's value")

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
    state.timing = {"sumcheck": t_sum, "folds": t_fold, "commits": t_commit, "opens": t_open}
    return Proof(np.stack(round_points), roots, final, openings, v)


def verify_eval(log_h, log_rate, schedule, root0, z, v, proof, n_queries, transcript):
    """True if `proof` shows x~(z) = v for the polynomial committed to by root0. Host arithmetic only:
    no device, no plan. A malformed proof is rejected, not an error."""
    sch = check_schedule(log_h, log_rate, schedule)
    try:
        z = _words(z, (log_h, 4))
        v = _words(v, (4,))
        pts = _words(proof.round_points, (log_h, 3, 4))
        final = _words(proof.final, (1 << log_rate, 4))
        roots = [bytes(root0)] + [bytes(r) for r in proof.roots]
        if len(roots) != len(sch) or any(len(r) != 32 for r in roots) or len(proof.openings) != len(sch):
            return False
        log_leaves = [log_h + log_rate - sum(sch[:i + 1]) for i in range(len(sch))]
        recs = []
        for i, o in enumerate(proof.openings):
            o = np.ascontiguousarray(o, dtype=np.uint8)
            if o.shape != (n_queries, merkle_open_bytes(log_leaves[i], sch[i])):
                return False
            recs.append(o)
    except (ValueError, TypeError, AttributeError):
        return False

    # ---- the transcript and the sumcheck chain
    transcript.absorb(_header(log_h, log_rate, n_queries, sch))
    transcript.absorb(roots[0] + z.tobytes() + v.tobytes())
    claim, rho, entry, entry_end = v.astype(np.uint32), [], 0, sch[0]
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
    if not np.array_equal(claim, _mul(eq_eval(z.astype(np.uint32), rho), final[0])):
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
