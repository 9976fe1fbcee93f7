"""The bottom pass of the LDS-tile additive NTT (antt_bs_pass, kernel variant 1; the default
variant 5 uses it for launches of two tiles per CU and more) runs its in-word stages 4..0 as
block stages on a packed pair of blocks when the transform has two and more passes; the
single-pass kernel keeps the per-stage form. Both address the tile as
one contiguous run. GPU parity at the sizes where those paths change, and a host-only check of
the packed path's twiddle table (BsPass::pat2)."""
import ctypes

import numpy as np
import pytest

import _oracle as O
import binius_ntt_amd as B

gpu = pytest.mark.gpu

# log_h, log_rate: single pass and one tile with the in-word stages on the GF(2^16) circuit; two
# passes with coset bits in the twiddles; the smallest size whose stages 0..4 need the GF(2^32)
# circuit; the same with cosets
SHAPES = [(12, 0), (13, 2), (17, 0), (15, 2)]


def _run_device(ntt, x_np, dev, batch=1):
    import torch
    x = torch.from_numpy(x_np.astype(np.uint32).view(np.int32)).to(dev)
    y = torch.empty(x_np.size << ntt.conf.log_rate, dtype=torch.int32, device=dev)
    ntt.forward_device(x, y, batch=batch)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint32)


@gpu
@pytest.mark.parametrize("log_h,r", SHAPES)
def test_variant1_gf128_matches_oracle(log_h, r, dev):
    x = O.fill128(0xDEADBEEF + log_h + r, 0x5EED0000, 1 << log_h)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(7)))
    ntt.set_variant(1)
    # 2^12 is one pass (the single-pass kernel keeps the per-stage in-word path), the others end in
    # the two-pass bottom kernel with the packed stages
    assert ("antt_bs_pass<4, 3" if log_h == 12 else "antt_bs_pass<4, 2") in ntt.pass_kernel_name(0 if log_h == 12 else 1)
    y = _run_device(ntt, x.reshape(-1), dev).reshape(-1, 4)
    assert np.array_equal(y, O.antt128(x, log_h, r))


@gpu
@pytest.mark.parametrize("log_h,r", SHAPES)
def test_variant1_gf32_reference_md5(ntt_md5, log_h, r, dev):
    # one limb per element: the reference's own inputs and MD5 table (both rows hold these sizes)
    x = O.mt_fill(0xDEADBEEF + log_h + r, 1 << log_h)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, r, B.FanPaarTowerField(5)))
    ntt.set_variant(1)
    assert ("antt_bs_pass<1, 3" if log_h == 12 else "antt_bs_pass<1, 2") in ntt.pass_kernel_name(0 if log_h == 12 else 1)
    assert O.md5(_run_device(ntt, x, dev)) == ntt_md5[str(r)][log_h]


@gpu
def test_variant1_gf128_batched(dev):
    log_h, batch = 12, 3
    xs = np.stack([O.fill128(0x1200 + b, 0x3400 + b, 1 << log_h) for b in range(batch)])
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, 0, B.FanPaarTowerField(7)))
    ntt.set_variant(1)
    y = _run_device(ntt, xs.reshape(-1), dev, batch=batch).reshape(batch, -1, 4)
    for b in range(batch):
        assert np.array_equal(y[b], O.antt128(xs[b], log_h, 0)), b


@gpu
def test_default_variant_512_tiles(dev):
    # 512 tiles: the smallest launch for which the default plan keeps the bottom pass on LDS tiles
    import torch
    log_h, batch = 12, 512
    g = torch.Generator(device=dev)
    g.manual_seed(0x512)
    x = torch.randint(-2**31, 2**31 - 1, (batch, 1 << log_h, 4), dtype=torch.int32, device=dev, generator=g)
    y = torch.empty_like(x)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, 0, B.FanPaarTowerField(7)))
    assert ntt.variant() == 5
    assert "antt_bs_pass<4, 3" in ntt.pass_kernel_name(0)  # LDS tiles, not register tiles
    ntt.forward_device(x.view(-1), y.view(-1), batch=batch)
    torch.cuda.synchronize()
    for b in (0, 1, 63, 256, 511):
        xb = x[b].cpu().numpy().view(np.uint32)
        assert np.array_equal(y[b].cpu().numpy().view(np.uint32), O.antt128(xb, log_h, 0)), b


# ---------------------------------------------------------------- host only: the pattern table
BUF_WORDS = 1024  # the library states the layout in the first four words it writes


def _inword_tables(log_h, r):
    out = np.zeros(BUF_WORDS, np.uint32)
    rc = B.lib().bn_antt_inword_tables(log_h, r, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out.size)
    assert rc == B.BN_OK, B.lib().bn_last_error()
    words, nb, no, nr = (int(v) for v in out[:4])
    stage_words = 32 + nb + no + nr + 1
    assert words == 4 + 1 + no + 5 * stage_words and nb == 7
    assert not out[words:].any()
    n_outer, ob = int(out[4]), [int(v) for v in out[5:5 + no]]
    stages = []
    for s in range(5):
        w = out[5 + no + s * stage_words:][:stage_words]
        stages.append(dict(pat2=w[:32], twt=w[32:32 + nb], two=w[32 + nb:32 + nb + no],
                           twc=w[32 + nb + no:32 + nb + no + nr], field=int(w[-1])))
    return n_outer, ob[:n_outer], stages


def _twiddle32(s_tab, log_h, r, coset, stage, blk):
    # oracle/antt.c twiddle32 over the oracle's own subspace table
    ind = (coset << (log_h - 1 - stage)) | blk
    w = 0
    for k in range(log_h + r - 1 - stage):
        if (ind >> k) & 1:
            w ^= int(s_tab[stage, k])
    return w


@pytest.mark.parametrize("log_h,r", [(17, 0), (15, 2)])
def test_packed_pattern_table_rebuilds_every_twiddle(log_h, r):
    n_outer, ob, stages = _inword_tables(log_h, r)
    assert ob == list(range(12, log_h))
    s_tab = O.subspace_evals(log_h, r)
    outer = (1 << n_outer) - 1 - 2  # a tile with several fixed bits set
    coset = (1 << r) - 1
    base = sum(((outer >> m) & 1) << ob[m] for m in range(n_outer))
    fields = []
    for s in range(5):
        t = stages[s]
        uni = 0
        for m in range(n_outer):
            if (outer >> m) & 1:
                uni ^= int(t["two"][m])
        for c in range(r):
            if (coset >> c) & 1:
                uni ^= int(t["twc"][c])
        top = 0
        for lane in range(64):
            lane_part = uni
            for m in range(6):
                if (lane >> m) & 1:
                    lane_part ^= int(t["twt"][m])
            for p in range(32):
                got = lane_part
                for i in range(32):
                    got ^= ((int(t["pat2"][i]) >> p) & 1) << i
                # bit-lane p of the pair (X, Y) at stage s: index bits 0..s-1 = p's, index bits
                # s+1..4 = p's bits s..3, index bit 11 = p's bit 4; the lane is index bits 5..10
                low = p & ((1 << s) - 1)
                high = (p >> s) & ((1 << (4 - s)) - 1)
                idx = base | ((p >> 4) << 11) | (lane << 5) | (high << (s + 1)) | low
                want = _twiddle32(s_tab, log_h, r, coset, s, idx >> (s + 1))
                assert got == want, (s, lane, p)
                top |= want
        assert t["field"] == (8 if top < 256 else 16 if top < 65536 else 32)
        fields.append(t["field"])
    assert 32 in fields  # these sizes run the GF(2^32) circuit in the in-word stages


def test_inword_tables_rejects_small_sizes():
    out = np.zeros(BUF_WORDS, np.uint32)
    p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert B.lib().bn_antt_inword_tables(11, 0, p, out.size) == B.BN_ERR_UNSUPPORTED
    assert B.lib().bn_antt_inword_tables(12, 0, p, 10) == B.BN_ERR_INVALID
