"""GPU tests of the inverse additive NTT (bn_antt_inverse_device / bn_antt_inverse_host). The
oracle has no inverse, so the inverse is pinned through the forward transform: what it returns
must go forward (oracle, or the MD5-pinned GPU forward) to the evaluations it was given. Every
comparison is bit-exact."""
import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

pytestmark = pytest.mark.gpu


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)


def _to_np(t, limbs):
    a = t.cpu().numpy().view(np.uint32)
    return a if limbs == 1 else a.reshape(-1, limbs)


def _inverse(ntt, y_np, dev, coset=0, batch=1):
    """inverse_device on host data; returns the coefficients as numpy (n*batch [, 4])."""
    import torch
    y = _to_dev(y_np, dev)
    x = torch.empty_like(y)
    ntt.inverse_device(y, x, coset=coset, batch=batch)
    torch.cuda.synchronize()
    return _to_np(x, ntt.limbs)


def _forward(ntt, x_np, dev, batch=1):
    import torch
    x = _to_dev(x_np, dev)
    y = torch.empty(x.numel() << ntt.conf.log_rate, dtype=torch.int32, device=dev)
    ntt.forward_device(x, y, batch=batch)
    torch.cuda.synchronize()
    return _to_np(y, ntt.limbs)


def _ntt(log_h, r, bits):
    return B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(7 if bits == 128 else 5)))


# compact kernel (1-11), single pass (12), 1-stage upper pass with six batch bits in the tile (13),
# full 7-stage upper pass (19), FIRST + MID + LAST (20)
@pytest.mark.parametrize("log_h,r,coset", [(1, 0, 0), (2, 1, 1), (3, 0, 0), (5, 2, 3), (8, 0, 0), (11, 1, 1),
                                           (12, 0, 0), (12, 3, 5), (13, 0, 0), (13, 2, 2), (14, 4, 15), (16, 0, 0),
                                           (17, 2, 3), (19, 1, 1), (20, 0, 0), (20, 1, 1)])
def test_gf128_inverse_undoes_oracle_forward(log_h, r, coset, dev):
    n = 1 << log_h
    y = O.fill128(0x1A7E0000 + 64 * log_h + 8 * r + coset, 0x5EED0000, n)
    x = _inverse(_ntt(log_h, r, 128), y, dev, coset)
    assert np.array_equal(O.antt128(x, log_h, r)[coset * n:(coset + 1) * n], y)


@pytest.mark.parametrize("log_h,r,coset", [(4, 0, 0), (10, 2, 2), (12, 0, 0), (12, 2, 3), (13, 1, 1), (15, 0, 0),
                                           (20, 0, 0), (20, 1, 1)])
def test_gf32_inverse_undoes_oracle_forward(log_h, r, coset, dev):
    n = 1 << log_h
    y = O.mt_fill(0x1A7E0000 + 64 * log_h + 8 * r + coset, n)
    x = _inverse(_ntt(log_h, r, 32), y, dev, coset)
    assert np.array_equal(O.antt32(x, log_h, r)[coset * n:(coset + 1) * n], y)


@pytest.mark.parametrize("log_h", [12, 13, 20])
def test_every_coset_round_trips(log_h, dev):
    r, n = 2, 1 << log_h
    ntt = _ntt(log_h, r, 128)
    x = O.fill128(0xC05E7 + log_h, 0x5EED0000, n)
    Y = _forward(ntt, x, dev)
    for c in range(1 << r):
        assert np.array_equal(_inverse(ntt, Y[c * n:(c + 1) * n], dev, c), x), c
        # the coset must matter: block c read as coset c ^ 1 is another polynomial
        assert not np.array_equal(_inverse(ntt, Y[c * n:(c + 1) * n], dev, c ^ 1), x), c


@pytest.mark.parametrize("log_h,r,coset,batch", [(12, 1, 1, 5), (13, 0, 0, 3), (20, 0, 0, 2)])
def test_batched_inverse(log_h, r, coset, batch, dev):
    n = 1 << log_h
    ntt = _ntt(log_h, r, 128)
    xs = np.stack([O.fill128(0xBA7C4 + 16 * log_h + b, 0x5EED0000 + b, n) for b in range(batch)])
    Y = _forward(ntt, xs, dev, batch=batch).reshape(batch, n << r, 4)
    ys = np.ascontiguousarray(Y[:, coset * n:(coset + 1) * n])
    got = _inverse(ntt, ys, dev, coset, batch=batch).reshape(batch, n, 4)
    for b in range(batch):
        assert np.array_equal(got[b], xs[b]), b


# the compact kernel at GF(2^128) and the bitsliced tiles at GF(2^32) (one limb plane, L = 1): single
# pass with a coset, and an upper pass with batch bits in the tile index
@pytest.mark.parametrize("bits,log_h,r,coset,batch", [(128, 8, 1, 1, 3), (32, 12, 1, 1, 3), (32, 13, 0, 0, 2)])
def test_batched_inverse_compact_and_gf32(bits, log_h, r, coset, batch, dev):
    n, limbs = 1 << log_h, bits // 32
    ntt = _ntt(log_h, r, bits)
    if bits == 128:
        xs = np.stack([O.fill128(0xBA7C4 + 16 * log_h + b, 0x5EED0000 + b, n) for b in range(batch)])
    else:
        xs = np.stack([O.mt_fill(0xBA7C4 + 16 * log_h + b, n) for b in range(batch)])
    Y = _forward(ntt, xs, dev, batch=batch).reshape(batch, n << r, limbs)
    ys = np.ascontiguousarray(Y[:, coset * n:(coset + 1) * n])
    got = _inverse(ntt, ys, dev, coset, batch=batch).reshape(batch, n, limbs)
    for b in range(batch):
        assert np.array_equal(got[b], xs[b].reshape(n, limbs)), b


@pytest.mark.parametrize("log_h", [13, 20])
def test_variants_agree(log_h, dev):
    # variant 0 at 13 runs the multi-group compact inverse; 1, 4 and 5 the bitsliced LDS tiles
    r, coset, n = 1, 1, 1 << log_h
    ntt = _ntt(log_h, r, 128)
    x = O.fill128(0x7A81A + log_h, 0x5EED0000, n)
    y = np.ascontiguousarray(_forward(ntt, x, dev)[coset * n:(coset + 1) * n])
    for v in (0, 1, 4, 5):
        ntt.set_variant(v)
        assert ntt.variant() == v
        assert np.array_equal(_inverse(ntt, y, dev, coset), x), v


@pytest.mark.parametrize("log_h", [12, 20])
def test_input_left_untouched(log_h, dev):
    import torch
    n = 1 << log_h
    ntt = _ntt(log_h, 0, 128)
    y = _to_dev(O.fill128(0x0DD + log_h, 0x5EED0000, n), dev)
    before = y.clone()
    x = torch.empty_like(y)
    ntt.inverse_device(y, x)
    torch.cuda.synchronize()
    assert torch.equal(y, before)
    assert not torch.equal(x, y)


def test_host_inverse_semantics(dev):
    log_h, r, coset, n = 10, 1, 1, 1 << 10
    ntt = _ntt(log_h, r, 128)
    y = O.fill128(0x4057, 0x5EED0000, n)
    out = B.NTTData(n, field_bits=128)
    sentinel = np.full((n, 4), 0xA5A5A5A5, np.uint32)
    out.data = sentinel.copy()
    bad = B.NTTData(n >> 1, B.DataOrder.IN_ORDER, 128)
    assert ntt.inverse(bad, out, coset) is False  # wrong size -> False, no other effect
    assert np.array_equal(out.data, sentinel) and out.order == B.DataOrder.INVALID
    wrong_order = B.NTTData(n, B.DataOrder.BIT_REVERSED, 128, y)
    assert ntt.inverse(wrong_order, out, coset) is False
    assert np.array_equal(out.data, sentinel) and out.order == B.DataOrder.INVALID
    good = B.NTTData(n, B.DataOrder.IN_ORDER, 128, y)
    assert ntt.inverse(good, out, coset) is True
    assert out.order == B.DataOrder.IN_ORDER
    assert np.array_equal(O.antt128(out.data, log_h, r)[coset * n:(coset + 1) * n], y)
    # an output of another size is resized to n elements
    small = B.NTTData(4, field_bits=128)
    assert ntt.inverse(good, small, coset) is True
    assert small.size == n and np.array_equal(small.data, out.data)


def test_argument_errors(dev):
    import torch
    log_h, r, n = 12, 1, 1 << 12
    ntt = _ntt(log_h, r, 128)
    x = O.fill128(0xE44, 0x5EED0000, n)
    Y = _forward(ntt, x, dev)
    y = _to_dev(Y[n:], dev)
    out = torch.empty_like(y)

    def good_call_still_works():
        out.zero_()
        ntt.inverse_device(y, out, coset=1)
        torch.cuda.synchronize()
        assert np.array_equal(_to_np(out, 4), x)

    good_call_still_works()
    for coset in (1 << r, -1):
        with pytest.raises(B.BnError) as e:
            ntt.inverse_device(y, out, coset=coset)
        assert e.value.code == B.BN_ERR_INVALID
        good_call_still_works()
    with pytest.raises(B.BnError) as e:
        ntt.inverse_device(y, y, coset=1)
    assert e.value.code == B.BN_ERR_INVALID
    good_call_still_works()
    with pytest.raises(ValueError):
        ntt.inverse_device(y, out[:-1], coset=1)
    with pytest.raises(ValueError):
        ntt.inverse_device(y[:-1], out, coset=1)
    good_call_still_works()


@pytest.mark.slow
def test_headline_size_round_trip(ntt_md5, dev):
    import torch
    log_h = 24
    x_np = O.fill128(0xDEADBEEF + log_h, 0x5EED0000, 1 << log_h)
    ntt = _ntt(log_h, 0, 128)
    x = _to_dev(x_np, dev)
    Y = torch.empty_like(x)
    ntt.forward_device(x, Y)
    torch.cuda.synchronize()
    assert O.md5_limb(_to_np(Y, 4), 0) == ntt_md5["0"][log_h]  # the reference table pins the forward
    back = torch.empty_like(x)
    ntt.inverse_device(Y, back)
    torch.cuda.synchronize()
    assert torch.equal(back, x)
