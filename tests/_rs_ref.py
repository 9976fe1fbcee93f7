"""Reference of ring-switching for GF(2) witnesses for the tests, on the host: steps 1-5 of
binius_ntt_amd/fri_pcs.py's docstring restated over the oracle's field arithmetic with brute-force
tables (no table doubling, and no tensor trick for A~(rho): it sums A[w] * eq(rho, w)), and a host
proof of the packed protocol from tests/_fri_ref.py's pieces, the oracle's sumcheck and
tests/_merkle_ref.py. Elements are Python integers (bit v of the integer is beta_v's bit) or (n, 4)
uint32 arrays, limb 0 first."""
import numpy as np

import _fri_ref as F
import _merkle_ref as R
import _oracle as O

TAG = b"ring-switch/gf2"


def ints(a):
    return [O._from_words(w) for w in np.asarray(a, dtype=np.uint32).reshape(-1, 4)]


def words(xs):
    return np.stack([O._to_words(x) for x in xs]) if len(xs) else np.zeros((0, 4), np.uint32)


def eq_low_first(r, x):
    """prod_i (bit_i(x) ? r_i : 1 ^ r_i), r a list of integers."""
    acc = 1
    for i, ri in enumerate(r):
        acc = O.mul128(acc, ri if (x >> i) & 1 else ri ^ 1)
    return acc


def eq_table_low_first(r):
    return [eq_low_first(r, x) for x in range(1 << len(r))]


def pack_bits(bits):
    """t'[w] = sum_v t[128 w + v] beta_v for a 0/1 array of 2^l entries: (2^(l-7), 4) uint32."""
    b = np.asarray(bits, dtype=np.uint8).reshape(-1, 128)
    return np.packbits(b, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def unpack_bits(tp):
    return np.unpackbits(np.ascontiguousarray(tp, dtype="<u4").view(np.uint8), axis=1, bitorder="little").reshape(-1)


def _bit_mask(a, v):
    """Boolean per element: bit v of the (n, 4) uint32 array's elements."""
    return ((a[:, v >> 5] >> np.uint32(v & 31)) & np.uint32(1)).astype(bool)


def partial_evals(tp, E):
    """s^_v = XOR over w with bit_v(t'[w]) = 1 of E[w]: (128, 4) uint32 from two (n, 4) arrays."""
    tp, E = np.asarray(tp, np.uint32).reshape(-1, 4), np.asarray(E, np.uint32).reshape(-1, 4)
    out = np.zeros((128, 4), np.uint32)
    for v in range(128):
        sel = E[_bit_mask(tp, v)]
        if len(sel):
            out[v] = np.bitwise_xor.reduce(sel, axis=0)
    return out


def linear_map(x, matrix):
    """out[w] = XOR over u with bit_u(x[w]) = 1 of matrix[u]."""
    x, m = np.asarray(x, np.uint32).reshape(-1, 4), np.asarray(matrix, np.uint32).reshape(128, 4)
    out = np.zeros_like(x)
    for u in range(128):
        out[_bit_mask(x, u)] ^= m[u]
    return out


def batch_table(r2):
    return words(eq_table_low_first(ints(r2)))


def row_check(shat, r_low):
    T, s, acc = eq_table_low_first(ints(r_low)), ints(shat), 0
    for v in range(128):
        acc ^= O.mul128(T[v], s[v])
    return O._to_words(acc)


def sumcheck_claim(shat, r2):
    B, s, acc = eq_table_low_first(ints(r2)), ints(shat), 0
    for u in range(128):
        row = sum(((s[v] >> u) & 1) << v for v in range(128))
        acc ^= O.mul128(B[u], row)
    return O._to_words(acc)


def eq_table_high(r_high):
    """E[w] = eq(r_high, w), r_high,j with bit j of w: (2^n, 4)."""
    return words(eq_table_low_first(ints(r_high)))


def eq_eval_brute(r_high, rho, r2):
    """A~(rho) = sum_w A[w] eq(rho, w), rho_j with bit j of w."""
    A = ints(linear_map(eq_table_high(r_high), batch_table(r2)))
    P, acc = eq_table_low_first(ints(rho)), 0
    for w in range(len(A)):
        acc ^= O.mul128(A[w], P[w])
    return O._to_words(acc)


def inner(a, b):
    acc = 0
    for x, y in zip(ints(a), ints(b)):
        acc ^= O.mul128(x, y)
    return O._to_words(acc)


def evaluate_bits(bits, r):
    """t~(r) of the GF(2) multilinear by brute force over the packed form: the row check's two sides
    are tested against each other elsewhere, so this sums t[i] eq(r, i) limb by limb instead:
    sum_w sum_v t[128 w + v] eq(r_low, v) eq(r_high, w)."""
    r = ints(r)
    low, high = eq_table_low_first(r[:7]), eq_table_low_first(r[7:])
    t = np.asarray(bits, np.uint8).reshape(-1, 128)
    acc = 0
    for w in range(t.shape[0]):
        inner_sum = 0
        for v in np.nonzero(t[w])[0]:
            inner_sum ^= low[int(v)]
        acc ^= O.mul128(inner_sum, high[w])
    return O._to_words(acc)


def host_proof_packed(bits, log_bits, log_rate, schedule, r, n_queries, label):
    """The packed protocol's opening proof of t~(r) built on the host. Returns a dict: root0, s, shat,
    r2, round_points (n, 3, 4), roots, final, openings, rho, queries."""
    n = log_bits - 7
    tp = pack_bits(bits)
    r = np.asarray(r, np.uint32).reshape(log_bits, 4)
    E = eq_table_high(r[7:])
    shat = partial_evals(tp, E)
    s = row_check(shat, r[:7])
    t = F.RefTranscript(label)
    cws = [O.antt128(tp, n, log_rate)]
    log_leaves = [n + log_rate - sum(schedule[:i + 1]) for i in range(len(schedule))]
    trees = [R.tree_of(cws[0], log_leaves[0], schedule[0])]
    root0 = trees[0][-1].tobytes()
    t.absorb(TAG + F._le([log_bits, log_rate, n_queries, len(schedule)] + list(schedule)))
    t.absorb(root0 + F._le(r) + F._le(s))
    t.absorb(F._le(shat))
    r2 = np.stack([t.challenge() for _ in range(7)])
    A = linear_map(E, batch_table(r2))
    order = [F.rev(y, n) for y in range(1 << n)]
    cols = np.stack([A[order], tp[order]])
    rho = np.zeros((n, 4), np.uint32)
    sums, _ = O.sumcheck_run(cols, n, 2, False, rho)
    s0 = sums[0].copy()
    points, roots, final = [], [], None
    entry, entry_end = 0, schedule[0]
    for k in range(n):
        _, pts = O.sumcheck_run(cols, n, 2, False, rho)
        points.append(pts[k].copy())
        t.absorb(F._le(pts[k]))
        rho[k] = t.challenge()
        if k + 1 == entry_end:
            a = schedule[entry]
            cws.append(F.ref_fold(cws[-1], n, log_rate, entry_end - a, rho[entry_end - a:entry_end]))
            entry += 1
            if entry < len(schedule):
                trees.append(R.tree_of(cws[-1], log_leaves[entry], schedule[entry]))
                roots.append(trees[-1][-1].tobytes())
                t.absorb(roots[-1])
                entry_end += schedule[entry]
            else:
                final = cws[-1]
                t.absorb(F._le(final))
    queries = [t.query(log_leaves[0]) for _ in range(n_queries)]
    openings = []
    for i, a in enumerate(schedule):
        shift = sum(schedule[1:i + 1])
        recs = [R.record_of(cws[i], trees[i], log_leaves[i], a, j >> shift) for j in queries]
        openings.append(np.frombuffer(b"".join(recs), np.uint8).reshape(n_queries, -1).copy())
    return dict(root0=root0, s=s, s0=s0, shat=shat, r2=r2, round_points=np.stack(points), roots=roots, final=final.copy(),
                openings=openings, rho=rho, queries=queries, packed=tp)
