"""GPU tests of the SHA-256 Merkle commitment (bn_merkle_commit_device / _split / _host) and its
openings (bn_merkle_open_device). The reference is tests/_merkle_ref.py: hashlib.sha256 for the leaf
digests, a numpy compression (checked against hashlib in test_abi_merkle.py) for the node rows.
Every comparison is bit-exact."""
import numpy as np
import pytest

import _merkle_ref as R
import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu

# fewer leaves than a wave (0, 1, 2, 5), than a work-group (6, 7), one work-group (8), two (9), 32 (13);
# the one-block leaf classes (0, 1), the multi-block ones (2: one chunk of one block, 3: one chunk of
# two, 4: two chunks) and the 65-block leaf (8)
SIZES = [(L, a) for L in (0, 1, 2, 5, 6, 7, 8, 9, 13) for a in (0, 1, 2, 3, 4, 8) if L + a <= 17]


def _dev_data(L, a, dev, data=None):
    import torch
    x = R.codeword(L + a) if data is None else data
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.int32).copy()).to(dev)


def _new_tree(L, dev, fill=0x5A):
    import torch
    return torch.full((32 * B.merkle_tree_digests(L),), fill, dtype=torch.uint8, device=dev)


def _commit(L, a, dev, data=None, max_rows=0, stream=None):
    """merkle_commit into a fresh tree tensor pre-filled with a pattern; returns (data, tree) tensors."""
    d = _dev_data(L, a, dev, data)
    tree = _new_tree(L, dev)
    B.merkle_commit(d, L, a, tree, stream=stream, max_rows=max_rows)
    return d, tree


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8).reshape(-1, 32)


def _first_difference(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return "%d digests differ, the first at index %d" % (bad.size, bad[0]) if bad.size else ""


@pytest.mark.parametrize("L,a", SIZES)
def test_whole_tree_equals_the_reference(L, a, dev):
    d, tree = _commit(L, a, dev)
    got, want = _np(tree), R.ref_tree(L, a)
    assert got.shape == want.shape == ((2 << L) - 1, 32)
    assert np.array_equal(got, want), _first_difference(got, want)
    assert np.array_equal(d.cpu().numpy().view(np.uint32).reshape(-1, 4), R.codeword(L + a))  # the data is not written


@pytest.mark.parametrize("max_rows", [1, 2, 3])
def test_forced_splits(max_rows, dev):
    L, a = 10, 2
    ps = B.merkle_commit_passes(L, a, max_rows)
    rows = [n for k, _, n in ps if k == B.MERKLE_ROW]
    if max_rows == 1:
        assert rows == [1] * 9
    elif max_rows == 2:
        assert rows == [1, 2, 2, 2]  # at least three row passes, the first uneven
    else:
        assert rows == [2, 3]
    assert max_rows == 3 or len(rows) >= 3
    _, tree = _commit(L, a, dev, max_rows=max_rows)
    got, want = _np(tree), R.ref_tree(L, a)
    assert np.array_equal(got, want), _first_difference(got, want)


def _default_plan_L(a):
    for L in range(31 - a):
        kinds = [k for k, _, _ in B.merkle_commit_passes(L, a)]
        if kinds.count(B.MERKLE_ROW) >= 2 and B.MERKLE_TAIL in kinds:
            return L
    return None


def test_default_plan_with_all_three_pass_kinds(dev):
    a = 2
    L = _default_plan_L(a)
    assert L is not None and L <= 20
    assert L == 15
    ps = B.merkle_commit_passes(L, a)
    kinds = [k for k, _, _ in ps]
    assert kinds[0] == B.MERKLE_LEAF and kinds[-1] == B.MERKLE_TAIL and kinds.count(B.MERKLE_ROW) >= 2
    _, tree = _commit(L, a, dev)
    got, want = _np(tree), R.ref_tree(L, a)
    assert np.array_equal(got, want), _first_difference(got, want)


@pytest.mark.parametrize("a", [0, 4])
def test_one_flipped_bit_changes_exactly_the_path(a, dev):
    L = 9
    base = R.ref_tree(L, a)
    n = 1 << a
    for leaf, slot, bit in ((0, 0, 0), (333, n // 2, 77), ((1 << L) - 1, n - 1, 127)):  # first, middle, last position of a leaf
        x = R.codeword(L + a).copy()
        x[leaf * n + slot, bit // 32] ^= np.uint32(1 << (bit % 32))
        _, tree = _commit(L, a, dev, data=x)
        changed = set(np.flatnonzero((_np(tree) != base).any(axis=1)).tolist())
        assert changed == {R.row_offset(L, h) + (leaf >> h) for h in range(L + 1)}


@pytest.mark.parametrize("a", [0, 2, 4])
def test_openings(a, dev):
    import torch
    L = 9
    d, tree = _commit(L, a, dev)
    want_tree = R.ref_tree(L, a)
    rng = np.random.default_rng(0x09E7 + a)
    idx = np.concatenate([[0, (1 << L) - 1, 17, 17], rng.integers(0, 1 << L, 300), [1 << L]]).astype(np.uint32)
    rb = B.merkle_open_bytes(L, a)
    assert rb == (16 << a) + 32 * L
    out = torch.full((idx.size * rb,), 0xA5, dtype=torch.uint8, device=dev)
    B.merkle_open(d, tree, L, a, torch.from_numpy(idx.view(np.int32)).to(dev), out)
    torch.cuda.synchronize()
    recs = out.cpu().numpy().reshape(idx.size, rb)
    root = want_tree[-1].tobytes()
    for q, j in enumerate(idx.tolist()):
        rec = recs[q].tobytes()
        if j >= 1 << L:
            assert rec == bytes(rb)  # out of range: all zero
            assert not B.merkle_verify(root, L, a, j, rec)
            continue
        assert rec == R.record_of(R.codeword(L + a), want_tree, L, a, j), (q, j)
        assert B.merkle_verify(root, L, a, j, rec)
        if q < 8:
            for at in (0, (16 << a) - 1, (16 << a) + 3, rb - 1):  # the leaf's ends, the first and the last sibling
                bad = bytearray(rec)
                bad[at] ^= 0x40
                assert not B.merkle_verify(root, L, a, j, bytes(bad))


def test_commit_phase_end_to_end(dev):
    """forward_device -> commit -> fold -> commit -> fold -> commit -> fold at log_h = 10, rate 1; the
    opened leaves verify against each round's root, equal the codeword's slices, and element j of the
    next codeword lies at slot j & (2^a' - 1) of leaf j >> a' of the next tree."""
    import torch
    log_h, rate = 10, 1
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, rate, B.FanPaarTowerField(7)))
    x = O.fill128(0xC0DE0000 + log_h, 0x5EED0000, 1 << log_h)
    ch = O.fill128(0xCA11, 0x0C000000, log_h)
    cw = torch.empty(4 << (log_h + rate), dtype=torch.int32, device=dev)
    ntt.forward_device(torch.from_numpy(x.reshape(-1).view(np.int32)).to(dev), cw)
    rounds = []  # (codeword, tree, L, a) of every commitment
    at = 0
    for arity in (4, 4, 2):
        log_n = log_h + rate - at
        L = log_n - arity
        tree = _new_tree(L, dev)
        B.merkle_commit(cw, L, arity, tree)
        rounds.append((cw, tree, L, arity))
        nxt = torch.empty(cw.numel() >> arity, dtype=torch.int32, device=dev)
        ntt.fri_fold_device(cw, nxt, at, ch[at:at + arity])
        cw, at = nxt, at + arity
    last = cw.cpu().numpy().view(np.uint32).reshape(-1, 4)
    assert last.shape == (1 << rate, 4) and (last == last[0]).all()
    queries = np.random.default_rng(0xF121).integers(0, 1 << rounds[0][2], 16).astype(np.uint32)
    host = [(c.cpu().numpy().view(np.uint32).reshape(-1, 4), _np(t)) for c, t, _, _ in rounds]
    for i, (c, t, L, a) in enumerate(rounds):
        if i:
            # element j of this codeword, the fold of leaf j of the round before, lies in leaf j >> a at slot j & (2^a - 1)
            slots, queries = queries & ((1 << a) - 1), queries >> a
        rb = B.merkle_open_bytes(L, a)
        out = torch.zeros(queries.size * rb, dtype=torch.uint8, device=dev)
        B.merkle_open(c, t, L, a, torch.from_numpy(queries.view(np.int32).copy()).to(dev), out)
        torch.cuda.synchronize()
        recs = out.cpu().numpy().reshape(queries.size, rb)
        cw_host, tree_host = host[i]
        assert np.array_equal(tree_host, R.tree_of(cw_host, L, a))
        for q, j in enumerate(queries.tolist()):
            assert B.merkle_verify(tree_host[-1], L, a, j, recs[q])
            leaf = recs[q][:16 << a].view(np.uint32).reshape(-1, 4)
            assert np.array_equal(leaf, cw_host[j << a:(j + 1) << a])
            if i:
                assert np.array_equal(leaf[slots[q]], cw_host[prev[q]])
        prev = queries.copy()


def test_streams(dev):
    """A non-default stream behind queued work, two back-to-back commits, and an opening queued right
    behind its commit with no host synchronisation between them."""
    import torch
    L, a = 13, 2
    d1 = _dev_data(L, a, dev)
    other = R.codeword(L + a + 1)[1 << (L + a):]
    d2 = _dev_data(L, a, dev, other)
    t1, t2 = _new_tree(L, dev), _new_tree(L, dev)
    idx = np.array([5, 4097, (1 << L) - 1], np.uint32)
    d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    rb = B.merkle_open_bytes(L, a)
    out = torch.zeros(idx.size * rb, dtype=torch.uint8, device=dev)
    busy = torch.zeros(1 << 26, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        for _ in range(4):  # work queued ahead of the calls
            busy.add_(1)
        B.merkle_commit(d1, L, a, t1, stream=st)
        B.merkle_commit(d2, L, a, t2, stream=st)
        B.merkle_open(d2, t2, L, a, d_idx, out, stream=st)
    st.synchronize()
    want2 = R.tree_of(other, L, a)
    assert np.array_equal(_np(t1), R.ref_tree(L, a))
    assert np.array_equal(_np(t2), want2)
    recs = out.cpu().numpy().reshape(idx.size, rb)
    for q, j in enumerate(idx.tolist()):
        assert recs[q].tobytes() == R.record_of(other, want2, L, a, j)
    assert int(busy[0].item()) == 4


@pytest.mark.parametrize("L,a", [(0, 0), (7, 4), (13, 2)])
def test_host_call_equals_device_call(L, a, dev):
    got = B.merkle_commit_host(R.codeword(L + a), a)
    assert got.shape == ((2 << L) - 1, 32)
    _, tree = _commit(L, a, dev)
    assert np.array_equal(got, _np(tree))
    assert np.array_equal(got, R.ref_tree(L, a))


def test_rejected_calls_leave_the_buffers_alone(dev):
    import torch
    L, a = 8, 2
    d = _dev_data(L, a, dev)
    tree = _new_tree(L, dev, fill=0x11)
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    rb = B.merkle_open_bytes(L, a)
    out = torch.full((4 * rb,), 0x22, dtype=torch.uint8, device=dev)
    d0, tree0, out0 = d.clone(), tree.clone(), out.clone()

    def invalid(f, *args, **kw):
        with pytest.raises(B.BnError) as e:
            f(*args, **kw)
        assert e.value.code == B.BN_ERR_INVALID

    for cap in (-1, 4, 9):
        invalid(B.merkle_commit, d, L, a, tree, max_rows=cap)
    invalid(B.merkle_commit, d, L, 9, tree)
    invalid(B.merkle_commit, d, -1, a, tree)
    invalid(B.merkle_commit, d, 27, 4, tree)
    bytes_view = d.view(torch.uint8)
    invalid(B.merkle_commit, d, L - 1, a, bytes_view[16 << (L - 1 + a - 1):])  # the tree inside the data
    invalid(B.merkle_commit, bytes_view[8:], L - 1, a, tree)  # misaligned data
    invalid(B.merkle_open, d, tree, L, a, idx[:0], out)  # no query
    invalid(B.merkle_open, d, tree, L, a, idx, tree.view(torch.uint8)[:4 * rb])  # the output on the tree
    invalid(B.merkle_open, d, tree, L, a, idx, bytes_view[:4 * rb])  # the output on the data
    with pytest.raises(ValueError):
        B.merkle_commit(d[:-4], L, a, tree)  # short data
    with pytest.raises(ValueError):
        B.merkle_commit(d, L, a, tree[:-32])  # short tree
    with pytest.raises(ValueError):
        B.merkle_commit(d.cpu(), L, a, tree)  # a host tensor
    with pytest.raises(ValueError):
        B.merkle_open(d, tree, L, a, idx, out[:-1])  # short output
    with pytest.raises(ValueError):
        B.merkle_open(d, tree, L, a, idx.to(torch.int64), out)  # 64-bit indices
    torch.cuda.synchronize()
    assert torch.equal(d, d0) and torch.equal(tree, tree0) and torch.equal(out, out0)
    B.merkle_commit(d, L, a, tree)
    assert np.array_equal(_np(tree), R.ref_tree(L, a))
