"""Reference of the Merkle commitment for the tests: hashlib.sha256 for the leaf digests and a
numpy-vectorised SHA-256 compression over arrays of blocks for the node rows (a pure-Python one
takes seconds per 2^16 nodes). The compression is itself checked against hashlib in
tests/test_abi_merkle.py. Inputs come from the oracle's fill128."""
import functools
import hashlib

import numpy as np

import _oracle as O

IV = np.array([0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19], np.uint32)
K = np.array([
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2], np.uint32)
ZERO_NODE = bytes.fromhex("da5698be17b9b46962335799779fbeca8ce5d491c0d26243bafef9ea1837a9d8")


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def compress(state, blocks):
    """One SHA-256 compression per row: state (n, 8) uint32, blocks (n, 64) uint8 -> new state (n, 8)."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 64)
    n = blocks.shape[0]
    w = np.zeros((64, n), np.uint32)
    w[:16] = blocks.view(">u4").astype(np.uint32).T
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> np.uint32(3))
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> np.uint32(10))
        w[t] = w[t - 16] + s0 + w[t - 7] + s1
    st = np.ascontiguousarray(np.broadcast_to(state, (n, 8)).T).astype(np.uint32)
    a, b, c, d, e, f, g, h = (st[i].copy() for i in range(8))
    for t in range(64):
        t1 = h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t]
        t2 = (_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))
        h, g, f, e, d, c, b, a = g, f, e, d + t1, c, b, a, t1 + t2
    return (st + np.stack([a, b, c, d, e, f, g, h])).T.copy()


def state_bytes(state):
    """(n, 8) uint32 state words -> (n, 32) uint8 digests (big-endian words)."""
    return np.ascontiguousarray(state.astype(">u4")).view(np.uint8).reshape(-1, 32)


def node_row(children):
    """(2n, 32) uint8 child digests -> (n, 32) uint8 node digests."""
    return state_bytes(compress(IV, np.ascontiguousarray(children).reshape(-1, 64)))


def hash_node(left, right):
    return node_row(np.frombuffer(bytes(left) + bytes(right), np.uint8).reshape(2, 32))[0].tobytes()


def tree_of(data, log_leaves, log_leaf_elems):
    """The whole tree buffer, (2^(L+1) - 1, 32) uint8, of the (2^(L+a), 4) uint32 array `data`."""
    raw = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1).view(np.uint8)
    nb = 16 << log_leaf_elems
    assert raw.size == nb << log_leaves
    buf = raw.tobytes()
    row = np.frombuffer(b"".join(hashlib.sha256(buf[j * nb:(j + 1) * nb]).digest() for j in range(1 << log_leaves)),
                        np.uint8).reshape(-1, 32)
    rows = [row]
    for _ in range(log_leaves):
        row = node_row(row)
        rows.append(row)
    return np.concatenate(rows)


def row_offset(log_leaves, row):
    return (2 << log_leaves) - (2 << (log_leaves - row))


def record_of(data, tree, log_leaves, log_leaf_elems, j):
    """The opening record of leaf j as bytes: the leaf, then the L siblings from the bottom up."""
    raw = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1).view(np.uint8)
    nb = 16 << log_leaf_elems
    sib = [tree[row_offset(log_leaves, h) + ((j >> h) ^ 1)].tobytes() for h in range(log_leaves)]
    return raw[j * nb:(j + 1) * nb].tobytes() + b"".join(sib)


@functools.lru_cache(maxsize=None)
def codeword(log_elems):
    """The shared input of 2^log_elems elements (read-only), seeded by fill128."""
    x = O.fill128(0x3E4B1E00 + log_elems, 0x4D4B0000, 1 << log_elems)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_tree(log_leaves, log_leaf_elems):
    """The reference tree of codeword(L + a), computed once (read-only)."""
    t = tree_of(codeword(log_leaves + log_leaf_elems), log_leaves, log_leaf_elems)
    t.setflags(write=False)
    return t
