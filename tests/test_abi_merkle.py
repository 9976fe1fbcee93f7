"""CPU: the Merkle commitment's entry points are declared, exported and validate their arguments
without touching a GPU; the host-only hashes and the verifier against hashlib and the numpy
compression of tests/_merkle_ref.py (itself checked against hashlib here); the sizes, the row offsets
and the host planner's split for every size and cap."""
import ctypes
import hashlib

import numpy as np
import pytest

import _merkle_ref as R
import binius_ntt_amd as B

NAMES = ("bn_merkle_tree_digests", "bn_merkle_open_bytes", "bn_merkle_row_offset", "bn_merkle_commit_device",
         "bn_merkle_commit_device_split", "bn_merkle_commit_host", "bn_merkle_open_device", "bn_merkle_hash_leaf",
         "bn_merkle_hash_node", "bn_merkle_verify", "bn_merkle_commit_passes")
CAPS = (0, 1, 2, 3)  # the caps the planner accepts (0: the default)


def test_merkle_entry_points_declared_and_exported():
    L = B.lib()
    declared = B.exported_symbols()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(L, n), n


def _invalid(rc):
    assert rc == B.BN_ERR_INVALID
    assert B.lib().bn_last_error()


def test_reference_compression_against_hashlib():
    rng = np.random.default_rng(0x5A256)
    for n in (0, 1, 31, 55):  # one padded block
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        block = msg + b"\x80" + bytes(55 - n) + (8 * n).to_bytes(8, "big")
        assert R.state_bytes(R.compress(R.IV, np.frombuffer(block, np.uint8)))[0].tobytes() == hashlib.sha256(msg).digest()
    msgs = rng.integers(0, 256, (5, 64), dtype=np.uint8)  # 64 bytes: the data block, then a block of padding
    pad = np.frombuffer(b"\x80" + bytes(55) + (512).to_bytes(8, "big"), np.uint8)
    st = R.compress(R.compress(R.IV, msgs), np.broadcast_to(pad, (5, 64)))
    for i in range(5):
        assert R.state_bytes(st)[i].tobytes() == hashlib.sha256(msgs[i].tobytes()).digest()


def test_hash_node_known_answer_and_random_pairs():
    assert B.merkle_hash_node(bytes(32), bytes(32)) == R.ZERO_NODE
    assert R.hash_node(bytes(32), bytes(32)) == R.ZERO_NODE
    pairs = np.random.default_rng(0x90DE).integers(0, 256, (64, 32), dtype=np.uint8)
    want = R.node_row(pairs)
    for k in range(32):
        assert B.merkle_hash_node(pairs[2 * k], pairs[2 * k + 1]) == want[k].tobytes()
    assert B.merkle_hash_node(pairs[0], pairs[1]) != B.merkle_hash_node(pairs[1], pairs[0])


@pytest.mark.parametrize("a", range(9))
def test_hash_leaf_equals_hashlib(a):
    leaf = R.codeword(9)[3:3 + (1 << a)]
    assert B.merkle_hash_leaf(leaf, a) == hashlib.sha256(leaf.tobytes()).digest()
    assert B.merkle_hash_leaf(leaf.tobytes(), a) == hashlib.sha256(leaf.tobytes()).digest()


def _flip(rec, bit):
    b = bytearray(rec)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@pytest.mark.parametrize("L", [0, 1, 5, 10])
@pytest.mark.parametrize("a", [0, 2, 4])
def test_verify_accepts_reference_records_and_rejects_tampered_ones(L, a):
    data, tree = R.codeword(L + a), R.ref_tree(L, a)
    root = tree[-1].tobytes()
    nb = 16 << a
    assert B.merkle_open_bytes(L, a) == nb + 32 * L
    for j in sorted({0, (1 << L) - 1, (1 << L) // 2, (1 << L) // 3}):
        rec = R.record_of(data, tree, L, a, j)
        assert len(rec) == nb + 32 * L
        assert B.merkle_verify(root, L, a, j, rec)
        for bit in (0, 8 * nb - 1, 4 * nb + 3):  # one flipped bit in the leaf
            assert not B.merkle_verify(root, L, a, j, _flip(rec, bit))
        for h in range(L):  # one flipped bit in each sibling
            assert not B.merkle_verify(root, L, a, j, _flip(rec, 8 * (nb + 32 * h) + 5 + 17 * h))
        if L:
            assert not B.merkle_verify(root, L, a, j ^ 1, rec)  # a wrong index
            assert not B.merkle_verify(root, L, a, j ^ (1 << (L - 1)), rec)
        assert not B.merkle_verify(root, L, a, j + (1 << L), rec)  # out of range
        assert not B.merkle_verify(_flip(root, 77), L, a, j, rec)  # a wrong root


def test_sizes_and_row_offsets():
    for L in range(31):
        assert B.merkle_tree_digests(L) == 2 ** (L + 1) - 1
        for h in range(L + 1):
            assert B.merkle_row_offset(L, h) == 2 ** (L + 1) - 2 ** (L - h + 1)
        assert B.merkle_row_offset(L, 0) == 0
        assert B.merkle_row_offset(L, L) == 2 ** (L + 1) - 2  # the root is the last digest
        for a in range(9):
            if L + a <= 30:
                assert B.merkle_open_bytes(L, a) == 16 * 2 ** a + 32 * L
    sz = ctypes.c_size_t()
    L_ = B.lib()
    _invalid(L_.bn_merkle_tree_digests(-1, ctypes.byref(sz)))
    _invalid(L_.bn_merkle_tree_digests(31, ctypes.byref(sz)))
    _invalid(L_.bn_merkle_tree_digests(4, None))
    _invalid(L_.bn_merkle_row_offset(4, 5, ctypes.byref(sz)))
    _invalid(L_.bn_merkle_row_offset(4, -1, ctypes.byref(sz)))
    _invalid(L_.bn_merkle_open_bytes(4, 9, ctypes.byref(sz)))
    _invalid(L_.bn_merkle_open_bytes(23, 8, ctypes.byref(sz)))
    _invalid(L_.bn_merkle_open_bytes(4, 2, None))


def test_commit_passes_cover_the_rows_once_and_in_order():
    for L in range(31):
        for cap in CAPS:
            ps = B.merkle_commit_passes(L, 0, cap)
            rows = [r for _, first, n in ps for r in range(first, first + n)]
            assert rows == list(range(L + 1)), (L, cap, ps)
            kinds = [k for k, _, _ in ps]
            assert kinds[0] == B.MERKLE_LEAF and kinds.count(B.MERKLE_LEAF) == 1, (L, cap, ps)
            assert kinds.count(B.MERKLE_TAIL) <= 1, (L, cap, ps)
            if B.MERKLE_TAIL in kinds:
                assert kinds[-1] == B.MERKLE_TAIL
            assert all(k == B.MERKLE_ROW for k in kinds[1:-1]), (L, cap, ps)
            lim = cap or 3
            assert all(1 <= n <= lim for k, _, n in ps if k != B.MERKLE_TAIL), (L, cap, ps)
            assert all(1 <= n <= (cap or 9) for k, _, n in ps if k == B.MERKLE_TAIL), (L, cap, ps)
            # the split does not depend on the leaf size
            for a in (4, 8):
                if L + a <= 30:
                    assert B.merkle_commit_passes(L, a, cap) == ps
    assert B.merkle_commit_passes(0, 4) == [(0, 0, 1)]
    assert B.merkle_commit_passes(5, 4) == [(0, 0, 1), (2, 1, 5)]  # fewer leaves than a work-group: no fused rows
    assert B.merkle_commit_passes(10, 2) == [(0, 0, 3), (2, 3, 8)]
    assert B.merkle_commit_passes(15, 2) == [(0, 0, 3), (1, 3, 1), (1, 4, 3), (2, 7, 9)]
    assert B.merkle_commit_passes(20, 4) == [(0, 0, 3), (1, 3, 3), (1, 6, 3), (1, 9, 3), (2, 12, 9)]
    assert B.merkle_commit_passes(10, 2, 2) == [(0, 0, 2), (1, 2, 1), (1, 3, 2), (1, 5, 2), (1, 7, 2), (2, 9, 2)]


def test_commit_passes_argument_errors():
    L = B.lib()
    out = (ctypes.c_int32 * 96)()
    k = ctypes.c_int()
    _invalid(L.bn_merkle_commit_passes(-1, 0, 0, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(31, 0, 0, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(27, 4, 0, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(10, 9, 0, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(10, -1, 0, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(10, 2, 4, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(10, 2, -1, out, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(10, 2, 2, out, 5, ctypes.byref(k)))  # six passes, room for five
    _invalid(L.bn_merkle_commit_passes(10, 2, 0, None, 32, ctypes.byref(k)))
    _invalid(L.bn_merkle_commit_passes(10, 2, 0, out, 32, None))


def test_commit_and_open_argument_errors():
    L = B.lib()
    # fake device pointers, never dereferenced: every call below fails its checks first. At L = 10,
    # a = 2 the data is 64 KiB and the tree just under 64 KiB
    data, tree, idx, out = (ctypes.c_void_p(v) for v in (0x100000, 0x200000, 0x300000, 0x400000))
    host = (ctypes.c_uint32 * 64)()
    host8 = (ctypes.c_uint8 * 64)()
    for la, a in ((-1, 2), (10, -1), (10, 9), (23, 8), (31, 0)):
        _invalid(L.bn_merkle_commit_device(data, la, a, tree, None))
        _invalid(L.bn_merkle_commit_device_split(data, la, a, tree, 0, None))
        _invalid(L.bn_merkle_commit_host(0, host, la, a, host8))
        _invalid(L.bn_merkle_open_device(data, tree, la, a, idx, 4, out, None))
    _invalid(L.bn_merkle_commit_device(None, 10, 2, tree, None))
    _invalid(L.bn_merkle_commit_device(data, 10, 2, None, None))
    _invalid(L.bn_merkle_commit_host(0, None, 0, 0, host8))
    _invalid(L.bn_merkle_commit_host(0, host, 0, 0, None))
    for cap in (-1, 4, 9):
        _invalid(L.bn_merkle_commit_device_split(data, 10, 2, tree, cap, None))
    _invalid(L.bn_merkle_commit_device(ctypes.c_void_p(0x100008), 10, 2, tree, None))  # misaligned
    # overlapping ranges: the tree inside the data, the data's last byte on the tree's first
    _invalid(L.bn_merkle_commit_device(data, 10, 2, ctypes.c_void_p(0x100000 + 0x8000), None))
    _invalid(L.bn_merkle_commit_device(data, 10, 2, ctypes.c_void_p(0x100000 + 0x10000 - 16), None))
    _invalid(L.bn_merkle_commit_device(ctypes.c_void_p(0x200000 + 0x10000 - 64), 10, 2, tree, None))
    for bad in ((None, tree, idx, out), (data, None, idx, out), (data, tree, None, out), (data, tree, idx, None)):
        _invalid(L.bn_merkle_open_device(bad[0], bad[1], 10, 2, bad[2], 4, bad[3], None))
    _invalid(L.bn_merkle_open_device(data, tree, 10, 2, idx, 0, out, None))  # no query
    _invalid(L.bn_merkle_open_device(data, tree, 10, 2, idx, 4, ctypes.c_void_p(0x100000 + 0x10000 - 16), None))  # out on the data
    _invalid(L.bn_merkle_open_device(data, tree, 10, 2, idx, 4, ctypes.c_void_p(0x200000 - 16), None))  # out runs into the tree
    _invalid(L.bn_merkle_open_device(data, tree, 10, 2, idx, 4, idx, None))  # out on the indices
    _invalid(L.bn_merkle_open_device(data, data, 10, 2, idx, 4, out, None))  # the tree on the data


def test_host_hash_argument_errors():
    L = B.lib()
    b = (ctypes.c_uint8 * 4096)()
    ok = ctypes.c_int()
    _invalid(L.bn_merkle_hash_leaf(None, 0, b))
    _invalid(L.bn_merkle_hash_leaf(b, 0, None))
    _invalid(L.bn_merkle_hash_leaf(b, 9, b))
    _invalid(L.bn_merkle_hash_leaf(b, -1, b))
    _invalid(L.bn_merkle_hash_node(None, b, b))
    _invalid(L.bn_merkle_hash_node(b, None, b))
    _invalid(L.bn_merkle_hash_node(b, b, None))
    _invalid(L.bn_merkle_verify(None, 3, 2, 0, b, ctypes.byref(ok)))
    _invalid(L.bn_merkle_verify(b, 3, 2, 0, None, ctypes.byref(ok)))
    _invalid(L.bn_merkle_verify(b, 3, 2, 0, b, None))
    _invalid(L.bn_merkle_verify(b, 3, 9, 0, b, ctypes.byref(ok)))
    _invalid(L.bn_merkle_verify(b, 27, 4, 0, b, ctypes.byref(ok)))
    with pytest.raises(ValueError):
        B.merkle_verify(bytes(32), 3, 2, 0, bytes(10))  # a short record
    with pytest.raises(ValueError):
        B.merkle_hash_leaf(bytes(16), 2)
