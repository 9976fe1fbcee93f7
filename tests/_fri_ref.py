"""Reference of the FRI-Binius fold and of the opening protocol for the tests, on the host: the
per-pair rule of include/binius_ntt_amd.h over the oracle's field arithmetic and subspace table, the
oracle's sumcheck, tests/_merkle_ref.py, and the transcript written out from its byte-level
specification (binius_ntt_amd/fri_pcs.py's docstring) over hashlib, not through the package's class."""
import hashlib

import numpy as np

import _merkle_ref as R
import _oracle as O


def ref_round(state, s, log_h, r, i, ch):
    """One round of the per-pair rule on a (2^(log_h+r-i), 4) codeword of round i."""
    m = 1 << (log_h - i)
    nbits = log_h + r - 1 - i
    rr = O._from_words(ch)
    out = np.zeros((state.shape[0] // 2, 4), np.uint32)
    for c in range(1 << r):
        for j in range(m // 2):
            ind = (c << (log_h - 1 - i)) | j
            t = 0
            for k in range(nbits):
                if (ind >> k) & 1:
                    t ^= int(s[i][k])
            u = [int(x) for x in state[c * m + 2 * j]]
            v = [int(x) for x in state[c * m + 2 * j + 1]]
            v1 = [a ^ b for a, b in zip(u, v)]
            u1 = [a ^ O.mul(t, b, 5) for a, b in zip(u, v1)]
            d = O._from_words([a ^ b for a, b in zip(u1, v1)])
            out[c * (m // 2) + j] = O._to_words(O._from_words(u1) ^ O.mul128(rr, d))
    return out


def ref_fold(state, log_h, r, rnd, ch):
    """Rounds rnd .. rnd+len(ch)-1 on the whole codeword of round rnd."""
    s = O.subspace_evals(log_h, r)
    for l in range(len(ch)):
        state = ref_round(state, s, log_h, r, rnd + l, ch[l])
    return state


def rev(y, n):
    return int(format(y, "0%db" % n)[::-1], 2) if n else 0


def eq_table(z):
    """E[y] = prod_i (bit_{n-1-i}(y) ? z_i : 1 ^ z_i), the convention of bn_eq_expand_device."""
    n = len(z)
    zz = [O._from_words(w) for w in z]
    out = np.zeros((1 << n, 4), np.uint32)
    for y in range(1 << n):
        acc = 1
        for i in range(n):
            acc = O.mul128(acc, zz[i] if (y >> (n - 1 - i)) & 1 else zz[i] ^ 1)
        out[y] = O._to_words(acc)
    return out


class RefTranscript:
    def __init__(self, label=b""):
        self.state = hashlib.sha256(b"binius-ntt-amd/fri-pcs/v1" + label).digest()

    def absorb(self, m):
        self.state = hashlib.sha256(self.state + b"\x00" + m).digest()

    def draw(self):
        self.state = hashlib.sha256(self.state + b"\x01").digest()
        return self.state

    def challenge(self):
        d = self.draw()
        return np.array([int.from_bytes(d[4 * i:4 * i + 4], "little") for i in range(4)], np.uint32)

    def query(self, bits):
        return int.from_bytes(self.draw()[:8], "little") % (1 << bits)


def _le(a):
    return np.ascontiguousarray(a, dtype=np.uint32).astype("<u4").tobytes()


def host_proof(x, log_h, log_rate, schedule, z, n_queries, label):
    """The opening proof of x~(z) built on the host. Returns a dict: root0, v, round_points (n, 3, 4),
    roots (of codewords 1..), final (2^rate, 4), openings (per codeword: (n_queries, record bytes) uint8),
    rho (n, 4), queries, codewords."""
    n = log_h
    t = RefTranscript(label)
    cws = [O.antt128(x, log_h, log_rate)]
    log_leaves = [log_h + log_rate - sum(schedule[:i + 1]) for i in range(len(schedule))]
    trees = [R.tree_of(cws[0], log_leaves[0], schedule[0])]
    root0 = trees[0][-1].tobytes()
    xr = x[[rev(y, n) for y in range(1 << n)]]
    cols = np.stack([eq_table(z), xr])
    rho = np.zeros((n, 4), np.uint32)
    sums, _ = O.sumcheck_run(cols, n, 2, False, rho)
    v = sums[0].copy()
    t.absorb(_le([log_h, log_rate, n_queries, len(schedule)] + list(schedule)))
    t.absorb(root0 + _le(z) + _le(v))
    points, roots, final = [], [], None
    entry, entry_end = 0, schedule[0]
    for k in range(n):
        # the oracle takes every challenge up front: round k's points depend on rho[:k] only
        _, pts = O.sumcheck_run(cols, n, 2, False, rho)
        points.append(pts[k].copy())
        t.absorb(_le(pts[k]))
        rho[k] = t.challenge()
        if k + 1 == entry_end:
            a = schedule[entry]
            cws.append(ref_fold(cws[-1], log_h, log_rate, entry_end - a, rho[entry_end - a:entry_end]))
            entry += 1
            if entry < len(schedule):
                trees.append(R.tree_of(cws[-1], log_leaves[entry], schedule[entry]))
                roots.append(trees[-1][-1].tobytes())
                t.absorb(roots[-1])
                entry_end += schedule[entry]
            else:
                final = cws[-1]
                t.absorb(_le(final))
    queries = [t.query(log_leaves[0]) for _ in range(n_queries)]
    openings = []
    for i, a in enumerate(schedule):
        shift = sum(schedule[1:i + 1])
        recs = [R.record_of(cws[i], trees[i], log_leaves[i], a, j >> shift) for j in queries]
        openings.append(np.frombuffer(b"".join(recs), np.uint8).reshape(n_queries, -1).copy())
    return dict(root0=root0, v=v, round_points=np.stack(points), roots=roots, final=final.copy(), openings=openings, rho=rho,
                queries=queries, codewords=cws)
