"""CPU: the verifier's fold of one leaf (bn_antt_fri_fold_leaf: host arithmetic, no plan, no device)
against the per-pair rule of include/binius_ntt_amd.h written over the oracle's field arithmetic and
subspace table (tests/_fri_ref.py), applied round by round to the whole codeword with its (coset, block) indexing; and the
end-to-end identity: leaf folds chained through every round end at the multilinear extension. Every
comparison is bit-exact."""
import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B
from _fri_ref import ref_fold as _ref_fold


def _challenges(seed, k):
    return O.fill128(0xF01D0000 + seed, 0xC4A11E00 + seed, k)


# every index of a middle round with a coset; the widest leaf; the last round of a rate-16 plan (the
# twiddle bits are the coset's alone); the whole codeword one leaf
@pytest.mark.parametrize("log_h,r,rnd,k", [(5, 1, 1, 3), (8, 2, 0, 8), (12, 4, 11, 1), (3, 0, 0, 3)])
def test_leaf_fold_matches_per_pair_rule(log_h, r, rnd, k):
    state = O.fill128(0x1EAF + 64 * log_h + 8 * r + rnd, 0x5EED0000, 1 << (log_h + r - rnd))
    ch = _challenges(16 * log_h + k, k)
    want = _ref_fold(state, log_h, r, rnd, ch)
    assert want.shape[0] == 1 << (log_h + r - rnd - k)
    for j in range(want.shape[0]):
        leaf = state[j << k:(j + 1) << k]
        assert np.array_equal(B.fri_fold_leaf(log_h, r, rnd, j, leaf, ch), want[j]), j
        assert np.array_equal(B.fri_fold_leaf(log_h, r, rnd, j, leaf.tobytes(), ch), want[j]), j


def test_leaf_fold_alternating_shapes_use_their_own_table():
    """The per-thread table follows (log_h, log_rate): two shapes taken in turn."""
    shapes = [(5, 1, 1, 3), (6, 0, 2, 2)]
    cases = []
    for log_h, r, rnd, k in shapes:
        state = O.fill128(0xA17 + log_h, 0x5EED0000, 1 << (log_h + r - rnd))
        ch = _challenges(log_h, k)
        cases.append((log_h, r, rnd, k, state, ch, _ref_fold(state, log_h, r, rnd, ch)))
    for j in range(4):
        for log_h, r, rnd, k, state, ch, want in cases:
            assert np.array_equal(B.fri_fold_leaf(log_h, r, rnd, j, state[j << k:(j + 1) << k], ch), want[j])


@pytest.mark.parametrize("schedule", [[2, 3], [1, 1, 1, 1, 1], [5]])
def test_chain_of_leaf_folds_ends_at_the_multilinear_extension(schedule):
    log_h, r = 5, 1
    x = O.fill128(0xDEADBEEF + log_h + r, 0x5EED0000, 1 << log_h)
    rho = _challenges(32 * log_h + r, log_h)
    cw = O.antt128(x, log_h, r)
    rnd = 0
    for k in schedule:
        n_out = cw.shape[0] >> k
        cw = np.stack([B.fri_fold_leaf(log_h, r, rnd, j, cw[j << k:(j + 1) << k], rho[rnd:rnd + k]) for j in range(n_out)])
        rnd += k
    assert cw.shape == (1 << r, 4)
    assert (cw == cw[0]).all()
    # bit i of the index pairs with rho[i]; the oracle takes the highest variable first
    assert np.array_equal(cw[0], O.multilinear_composition(x, log_h, 1, rho[::-1]))
