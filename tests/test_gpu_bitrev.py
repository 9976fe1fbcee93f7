"""GPU tests of the bit-reversal permutation (bn_bit_reverse_device / _split / _host) against a numpy
index permutation of the oracle's fill128 data. Every comparison is bit-exact."""
import functools

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _data(log_n, batch=1):
    """The shared input of batch * 2^log_n elements (read-only)."""
    x = O.fill128(0xB17E0000 + 64 * batch + log_n, 0xB17E5EED, batch << log_n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _perm(log_n):
    """rev_n of every index, by reversing the bits of the index array."""
    i = np.arange(1 << log_n, dtype=np.uint64)
    r = np.zeros_like(i)
    for b in range(log_n):
        r |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(log_n - 1 - b)
    r = r.astype(np.int64)
    r.setflags(write=False)
    return r


def _want(x, log_n, batch=1):
    """out[b, rev(i)] = in[b, i]; rev is an involution, so out[b, j] = in[b, rev(j)]."""
    return x.reshape(batch, 1 << log_n, 4)[:, _perm(log_n)].reshape(-1, 4)


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


def _to_np(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 4)


def _run(x, log_n, dev, batch=1, bitsliced=False, tile_log=0):
    import torch
    d_in = _to_dev(x, dev)
    before = d_in.clone()
    out = torch.full_like(d_in, 0x5A5A5A5A)
    B.bit_reverse(d_in, out, log_n, batch=batch, bitsliced=bitsliced, tile_log=tile_log)
    torch.cuda.synchronize()
    assert torch.equal(d_in, before)  # the input is left untouched
    return out


def test_reference_permutation_is_the_bit_reversal():
    assert _perm(3).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    assert _perm(0).tolist() == [0]
    p = _perm(11)
    assert np.array_equal(p[p], np.arange(1 << 11))


# a copy (0, 1); one tile with no mid bit and with one (2, 5, 6, 11, 12); two tiles, four tiles (13, 14)
@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 6, 11, 12, 13, 14])
def test_default_tile(log_n, dev):
    x = _data(log_n)
    assert np.array_equal(_to_np(_run(x, log_n, dev)), _want(x, log_n))


# odd and even n - 2q, one tile and many tiles (up to 2^11 at 2^13 elements in runs of 2)
@pytest.mark.parametrize("tile_log", range(1, 7))
@pytest.mark.parametrize("log_n", [4, 7, 9, 13])
def test_forced_tile(log_n, tile_log, dev):
    x = _data(log_n)
    assert np.array_equal(_to_np(_run(x, log_n, dev, tile_log=tile_log)), _want(x, log_n))


@pytest.mark.parametrize("log_n", [6, 13])
def test_batch_of_three(log_n, dev):
    x = _data(log_n, 3)
    assert np.array_equal(_to_np(_run(x, log_n, dev, batch=3)), _want(x, log_n, 3))


@pytest.mark.parametrize("log_n", [1, 6, 13])
def test_twice_is_the_identity(log_n, dev):
    x = _data(log_n)
    once = _run(x, log_n, dev)
    assert np.array_equal(_to_np(_run(_to_np(once), log_n, dev)), x)


@pytest.mark.parametrize("log_n", [5, 6, 10, 13])
def test_bitsliced_equals_compact_then_bitslice(log_n, dev):
    import torch
    x = _data(log_n)
    compact = _run(x, log_n, dev)
    B.bitslice(compact)
    torch.cuda.synchronize()
    got = _run(x, log_n, dev, bitsliced=True)
    assert torch.equal(got, compact)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), O.bitslice128(_want(x, log_n)))


def test_bitsliced_batch(dev):
    x = _data(6, 3)
    got = _run(x, 6, dev, batch=3, bitsliced=True)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), O.bitslice128(_want(x, 6, 3)))


def test_host_entry(dev):
    x = _data(10)
    assert np.array_equal(B.bit_reverse_host(x), _want(x, 10))
    assert np.array_equal(B.bit_reverse_host(x, bitsliced=True).reshape(-1), O.bitslice128(_want(x, 10)))


def test_argument_errors_leave_the_output_alone(dev):
    import torch
    x = _data(10)
    d_in = _to_dev(x, dev)
    out = torch.full_like(d_in, 0x5A5A5A5A)
    for kw in (dict(log_n=10, batch=0), dict(log_n=4, bitsliced=True), dict(log_n=10, tile_log=7), dict(log_n=31)):
        with pytest.raises(B.BnError) as e:
            B.bit_reverse(d_in, out, **kw)
        assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(B.BnError) as e:
        B.bit_reverse(d_in, d_in, 10)
    assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(B.BnError) as e:  # the output starts in the input's second half
        B.bit_reverse(d_in, d_in[d_in.numel() // 4:], 9)
    assert e.value.code == B.BN_ERR_INVALID
    with pytest.raises(ValueError):
        B.bit_reverse(d_in, out[:-4], 10)
    with pytest.raises(ValueError):
        B.bit_reverse(d_in, out, 10, batch=2)
    torch.cuda.synchronize()
    assert (out == 0x5A5A5A5A).all().item()
    B.bit_reverse(d_in, out, 10)
    torch.cuda.synchronize()
    assert np.array_equal(_to_np(out), _want(x, 10))


@pytest.mark.slow
def test_2p24_by_md5(dev):
    import torch
    log_n = 24
    x = O.fill128(0xB17E0024, 0xB17E5EED, 1 << log_n)
    d_in = _to_dev(x, dev)
    out = torch.empty_like(d_in)
    B.bit_reverse(d_in, out, log_n)
    torch.cuda.synchronize()
    assert O.md5(_to_np(out)) == O.md5(_want(x, log_n))
