#!/usr/bin/env python3
"""Secondary benchmark lines for BASELINE.json configs 2-5 (bench.py keeps the headline NTT).

  python tools/bench_configs.py [--only c2,c3,c4,c5,bb,qm] [--sc-vars 24] [--out FILE]

c2  GF(2^128) multiply microbench, register-resident repeat loops (bitsliced_repeat style):
    compact (one element per lane) and bitsliced (32 products per lane-block), products/s.
c3  2^20-point GF(2^128) additive NTT, device-resident, elements/s.
c4  Sumcheck over GF(2^128), 2^N evals, bitsliced input (DATA_IS_TRANSPOSED = true),
    d in {2,3,4}: all N rounds (messages + fold) plus the final messages, device-resident
    columns; evals/s = 2^N / t.  Synthetic evals (numpy PCG64, fixed seed) and challenges.
c5  one GPU's share of the 256 x 2^20 batched NTT (32 transforms), elements/s; and one GPU's
    shard (rank 0 of 8) of the 2^28-eval d=3 sumcheck: the sharded rounds up to the endgame
    gather (the per-round all-gather of (d+2)x16 B partials is not included).
bb  BabyBear radix-2 NTT (prime-field sibling): 2^24 single transform and
    16 x 2^20 batched, device-resident, elements/s and algorithmic GB/s (4 B read + 4 B written
    per element).
qm  QM31 sumcheck (prime-field sibling), two columns of 2^N QM31, product
    composition: all N rounds (round messages + fold, one host round trip per round as in
    sumcheck.cuh:46-96) on device-resident columns; evals/s = 2^N / t (wall clock, setup upload
    excluded as the reference's benchmarking timer does).
intt (only with --only intt) inverse additive NTT, GF(2^128), r = 0, 2^20 and 2^24: the inverse
    next to the forward under set_variant(1) (the same products and LDS traffic) and the forward
    default, all three in one process, ms per transform.
fold (only with --only fold) FRI-Binius fold of a 2^24-element GF(2^128) codeword (log_h 22, log_rate
    2): round 0 at arity 1 and arity 4, rounds 0-3 singly, the full schedule 4+4+4+4+4+2, and
    bn_gf128_mul_device on 2^23 products (the arity-1 round's traffic and full-product count) in the
    same process; ms per call, the two ratios DESIGN.md section 5.8 states bounds for, and the
    fractions of HBM peak.
eq  (only with --only eq) eq-indicator expansion of n GF(2^128) challenges, n = 24 (compact, and
    bitsliced next to compact + bn_bitslice_device in alternating pairs) and n = 20, with
    bn_gf128_mul_device on 2^n products first and last in the same process (the yardstick DESIGN.md
    section 6.1 states the bound for) and a plain device fill of the same bytes (the write floor).
merkle (only with --only merkle) SHA-256 Merkle commitment of the fold line's codeword (log_h 22,
    log_rate 2, 2^24 elements): the commit at a = 1 and a = 4, bn_antt_forward_device on the same plan
    (the encode that produces this codeword; the yardstick DESIGN.md section 5.9 states the bound
    for), a device-to-device copy of the same 256 MiB, and the six commits of the 4+4+4+4+4+2
    schedule next to its six folds, all in one process; ms, leaves/s, compressions/s, the share of
    the HBM peak and the share of the v_bitop3 issue ceiling from the static VALU count per compression.
bitrev (only with --only bitrev) bit-reversal permutation of a GF(2^128) column, 2^24 and 2^20 elements,
    compact and bitsliced (at 2^24 next to the compact call + bn_bitslice_device in alternating pairs),
    with a device-to-device copy of the same bytes timed first and last in the same process (the
    smaller reading counts: the yardstick DESIGN.md section 5.10 states the bound for).
pcs (only with --only pcs) wall time of fri_pcs.prove_eval at log_h 20, log_rate 2, schedule 4+4+4+4+4,
    32 queries, with its split into sumcheck, folds, commits and opens. For the record: no bound.
rs  (only with --only rs) the two ring-switching kernels (bn_rs_partial_evals_device on bitsliced columns,
    bn_gf128_linear_map_device compact and bitsliced in place) at 2^24 and 2^20 packed elements, next
    to bn_gf128_mul_device and bn_eq_expand_device on as many elements and a device copy of the same
    bytes, all in one process; then fri_pcs.prove_eval_packed at n = 20 (2^27 bits), log_rate 2, schedule
    4+4+4+4+4, 32 queries, next to prove_eval at the same shape, with the share of the ring-switching
    steps in the whole opening. For the record: no bound.
Every line is one JSON object.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "binius-ntt_amd", "python"))

import numpy as np  # noqa: E402


def ev_time(fn, reps, stream):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def c2(dev, out):
    import torch
    import binius_ntt_amd as B
    st = torch.cuda.current_stream(dev)
    g = np.random.default_rng(2)
    # kind 2 is the product behind the boundary's multiply_unrolled<7> (bn_multiply_unrolled_device(7),
    # bn_gf128_mul_bitsliced_device); kind 1 keeps the reference's structure (one 32-product block
    # per lane, binary_tower_unrolled7.cu) for comparison only
    for kind, name, words, per in ((0, "compact", 4, 1),
                                   (2, "bitsliced multiply_unrolled<7>, quad-lane product (the boundary's path)", 128, 32),
                                   (1, "bitsliced, one 9712-gate multiply_unrolled<7> circuit per lane (reference "
                                       "structure, not the boundary's path)", 128, 32)):
        threads = 256 * 2048 if kind == 0 else 256 * 1024
        iters = 2000 if kind == 0 else 20 if kind == 1 else 200
        state = torch.from_numpy(g.integers(0, 2**32, size=threads * words, dtype=np.uint64).astype(np.uint32)
                                 .view(np.int32)).to(dev)
        opnd = torch.from_numpy(g.integers(0, 2**32, size=threads * words, dtype=np.uint64).astype(np.uint32)
                                .view(np.int32)).to(dev)  # one multiplier per lane, same shape as state
        ms = ev_time(lambda: B.gf128_mul_repeat(kind, state, opnd, threads, iters, stream=st), 3, st)
        prods = threads * iters * per
        out({"config": "c2", "workload": "GF(2^128) multiply repeat loop, %s" % name, "value": prods / (ms * 1e-3),
             "unit": "products/s", "ms": ms, "threads": threads, "iters": iters,
             "kernel": ("bn::k_repeat_compact", "bn::k_repeat_bitsliced", "bn::k_repeat_quad")[kind]})
    # the boundary entry itself on HBM-resident operands: dst = a * b over 2^20 blocks (32 Mi products;
    # 48 B of HBM traffic per product: two operands read, one product written)
    nblk = 1 << 20
    a = torch.from_numpy(g.integers(0, 2**32, size=128 * nblk, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    b = torch.from_numpy(g.integers(0, 2**32, size=128 * nblk, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    o = torch.empty_like(a)
    ms = ev_time(lambda: B.multiply_unrolled_device(7, a, b, o, stream=st), 5, st)
    prods = 32 * nblk
    out({"config": "c2", "workload": "GF(2^128) bitsliced products through bn_multiply_unrolled_device(7), 2^20 "
                                     "HBM-resident 128-word blocks", "value": prods / (ms * 1e-3), "unit": "products/s",
         "ms": ms, "hbm_gbps_algorithmic": 3 * 512.0 * nblk / (ms * 1e-3) / 1e9, "kernel": "bn::k_gf128_mul_bs"})
    del a, b, o
    # the compact entry on HBM-resident operands: dst = a * b over 2^25 compact elements
    # (tower_height_7_mul semantics; 48 B of HBM traffic per product)
    n = 1 << 25
    a = torch.randint(-2**31, 2**31, (4 * n,), dtype=torch.int32, device=dev)
    b = torch.randint(-2**31, 2**31, (4 * n,), dtype=torch.int32, device=dev)
    o = torch.empty_like(a)
    ms = ev_time(lambda: B.gf128_mul(a, b, o, stream=st), 5, st)
    out({"config": "c2", "workload": "GF(2^128) compact products through bn_gf128_mul_device, 2^25 HBM-resident "
                                     "elements", "value": n / (ms * 1e-3), "unit": "products/s", "ms": ms,
         "hbm_gbps_algorithmic": 48.0 * n / (ms * 1e-3) / 1e9, "kernel": "bn::k_gf128_mul"})
    del a, b, o


def ntt_line(dev, out, cfg, log_h, batch):
    import torch
    import binius_ntt_amd as B
    n = 1 << log_h
    g = np.random.default_rng(3)
    x = torch.from_numpy(g.integers(0, 2**32, size=4 * n * batch, dtype=np.uint64).astype(np.uint32)
                         .view(np.int32)).to(dev)
    y = torch.empty_like(x)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, 0, B.FanPaarTowerField(7), device=dev.index or 0))
    st = torch.cuda.current_stream(dev)
    ms = ev_time(lambda: ntt.forward_device(x, y, batch=batch, stream=st), 10, st)
    elems = n * batch
    out({"config": cfg, "workload": "%d x 2^%d-point GF(2^128) additive NTT (r=0)" % (batch, log_h),
         "value": elems / (ms * 1e-3), "unit": "elements/s", "ms": ms,
         "hbm_gbps_algorithmic": 32.0 * elems / (ms * 1e-3) / 1e9})


def intt_line(dev, out, log_h):
    import torch
    import binius_ntt_amd as B
    n = 1 << log_h
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.integers(0, 2**32, size=4 * n, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
    y = torch.empty_like(x)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, 0, B.FanPaarTowerField(7), device=dev.index or 0))
    st = torch.cuda.current_stream(dev)
    default = ntt.variant()
    ms_inv = ev_time(lambda: ntt.inverse_device(x, y, stream=st), 10, st)
    ntt.set_variant(1)
    ms_fwd1 = ev_time(lambda: ntt.forward_device(x, y, stream=st), 10, st)
    ntt.set_variant(default)
    ms_fwd = ev_time(lambda: ntt.forward_device(x, y, stream=st), 10, st)
    out({"config": "intt", "workload": "2^%d-point GF(2^128) inverse additive NTT (r=0, coset 0)" % log_h,
         "value": n / (ms_inv * 1e-3), "unit": "elements/s", "ms": ms_inv, "ms_forward_variant1": ms_fwd1,
         "ms_forward_default": ms_fwd, "forward_default_variant": default,
         "inverse_over_forward_variant1": ms_inv / ms_fwd1,
         "hbm_gbps_algorithmic": 32.0 * n / (ms_inv * 1e-3) / 1e9})


HBM_PEAK = 8.0e12  # bytes/s, MI355X specification


def fold_line(dev, out, log_h=22, log_rate=2, reps=30):
    """FRI-Binius fold of a 2^(log_h+log_rate)-element GF(2^128) codeword: round 0 at arity 1 and 4,
    rounds 0..3 singly, the full schedule 4+4+...+rest, and bn_gf128_mul_device on half as many
    products as the codeword has elements (the traffic and full-product count of the arity-1 round)
    as the yardstick, all in one process; ms per call, device events after a warm-up call."""
    import torch
    import binius_ntt_amd as B
    n = 1 << (log_h + log_rate)
    g = np.random.default_rng(7)
    st = torch.cuda.current_stream(dev)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, log_rate, B.FanPaarTowerField(7), device=dev.index or 0))
    ch = g.integers(0, 2**32, size=(log_h, 4), dtype=np.uint64).astype(np.uint32)
    bufs = [torch.randint(-2**31, 2**31, (4 * n,), dtype=torch.int32, device=dev),
            torch.empty(2 * n, dtype=torch.int32, device=dev)]

    def fold(src, dst, rnd, k):
        ntt.fri_fold_device(src, dst, rnd, ch[rnd:rnd + k], stream=st)

    def run(schedule, rnd=0):
        src = 0
        for k in schedule:
            fold(bufs[src], bufs[1 - src], rnd, k)
            rnd, src = rnd + k, 1 - src

    def hbm_bytes(schedule, rnd=0):
        b = 0
        for k in schedule:
            b += 16 * (n >> rnd) + 16 * (n >> (rnd + k))
            rnd += k
        return b

    # the yardstick first and last: the spread of the same call within the run
    a, b, o = bufs[0][:2 * n], bufs[0][2 * n:], bufs[1]
    ms_mul = [ev_time(lambda: B.gf128_mul(a, b, o, stream=st), reps, st)]
    ms_a1 = ev_time(lambda: run([1]), reps, st)
    ms_a4 = ev_time(lambda: run([4]), reps, st)
    # rounds 0..3 singly, each on a state of its own size (the values do not matter to the time)
    ms_single = [ev_time(lambda r=r: fold(bufs[0], bufs[1], r, 1), reps, st) for r in range(4)]
    full = [4] * (log_h // 4) + ([log_h % 4] if log_h % 4 else [])
    ms_full = ev_time(lambda: run(full), reps, st)
    ms_mul.append(ev_time(lambda: B.gf128_mul(a, b, o, stream=st), reps, st))
    mul = min(ms_mul)

    def peak(schedule, ms):
        return hbm_bytes(schedule) / (ms * 1e-3) / HBM_PEAK

    out({"config": "fold", "workload": "FRI-Binius fold of a 2^%d-element GF(2^128) codeword (log_h %d, log_rate %d)"
         % (log_h + log_rate, log_h, log_rate), "kernel": "bn::antt_fold",
         "value": n / (ms_full * 1e-3), "unit": "codeword elements/s (full schedule)",
         "ms_arity1_round0": ms_a1, "ms_arity4_round0": ms_a4, "ms_single_rounds_0_3": ms_single,
         "ms_full_schedule": ms_full, "full_schedule": full,
         "ms_gf128_mul_2p%d" % (log_h + log_rate - 1): ms_mul,
         "arity1_over_gf128_mul": ms_a1 / mul, "bound_arity1_over_gf128_mul": 1.5,
         "arity4_over_four_single_rounds": ms_a4 / sum(ms_single), "bound_arity4_over_four_single_rounds": 1.0,
         "hbm_peak_fraction_arity1": peak([1], ms_a1), "hbm_peak_fraction_arity4": peak([4], ms_a4),
         "hbm_peak_fraction_full_schedule": peak(full, ms_full),
         "hbm_peak_fraction_gf128_mul": 24.0 * n / (mul * 1e-3) / HBM_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK})


def eq_line(dev, out, n, bitsliced_too, reps=30):
    """The eq-indicator expansion at 2^n elements: the compact call (and, if asked, the bitsliced call
    next to the compact call followed by bn_bitslice_device), with bn_gf128_mul_device on 2^n products
    timed first and last as the yardstick (the smaller reading counts) and a plain device fill of the
    same 2^n x 16 B as the write floor, all in one process; ms per call, device events after a
    warm-up call."""
    import torch
    import binius_ntt_amd as B
    g = np.random.default_rng(11)
    st = torch.cuda.current_stream(dev)
    ch = g.integers(0, 2**32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    e = torch.empty(4 << n, dtype=torch.int32, device=dev)
    a = torch.randint(-2**31, 2**31, (4 << n,), dtype=torch.int32, device=dev)
    b = torch.randint(-2**31, 2**31, (4 << n,), dtype=torch.int32, device=dev)

    def then_bitslice():
        B.eq_expand(n, ch, e, stream=st)
        B.bitslice(e, stream=st)

    ms_mul = [ev_time(lambda: B.gf128_mul(a, b, e, stream=st), reps, st)]
    ms_fill = ev_time(lambda: e.fill_(0x5A5A5A5A), reps, st)
    ms_eq = ev_time(lambda: B.eq_expand(n, ch, e, stream=st), reps, st)
    line = {"config": "eq", "workload": "eq-indicator expansion of %d GF(2^128) challenges (2^%d elements)" % (n, n),
            "kernel": "bn::eq_expand_pass", "passes": B.eq_expand_passes(n), "value": (1 << n) / (ms_eq * 1e-3),
            "unit": "elements/s", "ms": ms_eq, "ms_fill": ms_fill}
    if bitsliced_too:
        # alternating pairs: the library's bitsliced call against the compact call plus bn_bitslice_device
        pairs = [(ev_time(lambda: B.eq_expand(n, ch, e, bitsliced=True, stream=st), reps, st), ev_time(then_bitslice, reps, st))
                 for _ in range(3)]
        line["ms_bitsliced_vs_compact_then_bitslice"] = pairs
    ms_mul.append(ev_time(lambda: B.gf128_mul(a, b, e, stream=st), reps, st))
    mul = min(ms_mul)
    line.update({"ms_gf128_mul_2p%d" % n: ms_mul, "over_gf128_mul": ms_eq / mul, "bound_over_gf128_mul": 1.0,
                 "over_fill": ms_eq / ms_fill, "hbm_peak_fraction": (16 << n) / (ms_eq * 1e-3) / HBM_PEAK,
                 "hbm_peak_bytes_per_s": HBM_PEAK})
    out(line)


def bitrev_line(dev, out, n, pairs_too, reps=30):
    """The bit-reversal permutation at 2^n elements: the compact and the bitsliced call (and, if asked,
    the bitsliced call next to the compact call followed by bn_bitslice_device, in alternating pairs),
    with a device-to-device copy of the same 2^n x 16 B timed first and last as the yardstick (the
    smaller reading counts), all in one process; ms per call, device events after a warm-up call."""
    import torch
    import binius_ntt_amd as B
    st = torch.cuda.current_stream(dev)
    a = torch.randint(-2**31, 2**31, (4 << n,), dtype=torch.int32, device=dev)
    o = torch.empty(4 << n, dtype=torch.int32, device=dev)

    def then_bitslice():
        B.bit_reverse(a, o, n, stream=st)
        B.bitslice(o, stream=st)

    ms_copy = [ev_time(lambda: o.copy_(a), reps, st)]
    ms = ev_time(lambda: B.bit_reverse(a, o, n, stream=st), reps, st)
    ms_bs = ev_time(lambda: B.bit_reverse(a, o, n, bitsliced=True, stream=st), reps, st)
    line = {"config": "bitrev", "workload": "bit-reversal permutation of 2^%d GF(2^128) elements" % n,
            "kernel": "bn::bit_reverse_tiles", "value": (1 << n) / (ms * 1e-3), "unit": "elements/s", "ms": ms,
            "ms_bitsliced": ms_bs}
    if pairs_too:
        line["ms_bitsliced_vs_compact_then_bitslice"] = [
            (ev_time(lambda: B.bit_reverse(a, o, n, bitsliced=True, stream=st), reps, st), ev_time(then_bitslice, reps, st))
            for _ in range(3)]
    ms_copy.append(ev_time(lambda: o.copy_(a), reps, st))
    cp = min(ms_copy)
    line.update({"ms_copy": ms_copy, "over_copy": ms / cp, "hbm_peak_fraction": (32 << n) / (ms * 1e-3) / HBM_PEAK,
                 "hbm_peak_fraction_copy": (32 << n) / (cp * 1e-3) / HBM_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK})
    if pairs_too:
        line["bound_over_copy"] = 1.5
    out(line)


def pcs_line(dev, out, log_h=20, log_rate=2, schedule=(4, 4, 4, 4, 4), n_queries=32, runs=3):
    """Wall time of the opening proof (fri_pcs.prove_eval) of a committed 2^log_h-coefficient
    polynomial and its split, the best of `runs` after a warm-up proof; commit and verify_eval once."""
    import torch
    import binius_ntt_amd as B
    from binius_ntt_amd import fri_pcs
    g = np.random.default_rng(13)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, log_rate, B.FanPaarTowerField(7), device=dev.index or 0))
    x = torch.randint(-2**31, 2**31, (4 << log_h,), dtype=torch.int32, device=dev)
    z = g.integers(0, 2**32, size=(log_h, 4), dtype=np.uint64).astype(np.uint32)
    t0 = time.perf_counter()
    com, state = fri_pcs.commit(ntt, x, list(schedule))
    torch.cuda.synchronize()
    s_commit = time.perf_counter() - t0
    best = None
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        proof = fri_pcs.prove_eval(state, z, n_queries, fri_pcs.Transcript(b"bench"))
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        if best is None or s < best[0]:
            best = (s, dict(state.timing))
    t0 = time.perf_counter()
    ok = fri_pcs.verify_eval(log_h, log_rate, list(schedule), com.root, z, proof.v, proof, n_queries, fri_pcs.Transcript(b"bench"))
    s_verify = time.perf_counter() - t0
    out({"config": "pcs", "workload": "FRI-Binius opening proof, log_h %d, log_rate %d, schedule %s, %d queries"
         % (log_h, log_rate, "+".join(str(a) for a in schedule), n_queries), "value": best[0] * 1e3, "unit": "ms per prove_eval (wall)",
         "ms_split": {k: v * 1e3 for k, v in best[1].items()}, "ms_commit": s_commit * 1e3, "ms_verify_host": s_verify * 1e3,
         "accepted": bool(ok)})


def rs_line(dev, out, n, reps=30):
    """The two ring-switching kernels on 2^n packed elements: the partial evaluations of two bitsliced
    columns and the linear map (compact, and bitsliced in place), next to bn_gf128_mul_device and
    bn_eq_expand_device on as many elements and a device copy of the same 2^n x 16 B (timed first and
    last, the smaller reading counts), all in one process; ms per call, device events after a warm-up
    call."""
    import torch
    import binius_ntt_amd as B
    st = torch.cuda.current_stream(dev)
    g = np.random.default_rng(17)
    a = torch.randint(-2**31, 2**31, (4 << n,), dtype=torch.int32, device=dev)
    b = torch.randint(-2**31, 2**31, (4 << n,), dtype=torch.int32, device=dev)
    o = torch.empty(4 << n, dtype=torch.int32, device=dev)
    shat = torch.empty(512, dtype=torch.int32, device=dev)
    m = g.integers(0, 2**32, size=(128, 4), dtype=np.uint64).astype(np.uint32)
    ch = g.integers(0, 2**32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    ms_copy = [ev_time(lambda: o.copy_(a), reps, st)]
    ms_pe = ev_time(lambda: B.rs_partial_evals(a, b, n, shat, stream=st), reps, st)
    ms_map = ev_time(lambda: B.gf128_linear_map(a, o, m, stream=st), reps, st)
    ms_map_bs = ev_time(lambda: B.gf128_linear_map(o, o, m, bitsliced=True, stream=st), reps, st)
    ms_mul = ev_time(lambda: B.gf128_mul(a, b, o, stream=st), reps, st)
    ms_eq = ev_time(lambda: B.eq_expand(n, ch, o, bitsliced=True, stream=st), reps, st)
    ms_copy.append(ev_time(lambda: o.copy_(a), reps, st))
    cp = min(ms_copy)
    out({"config": "rs", "workload": "ring-switching kernels on 2^%d packed GF(2^128) elements" % n,
         "kernel": "bn::rs_partial_evals, bn::gf128_linear_map", "value": (1 << n) / (ms_pe * 1e-3), "unit": "elements/s (partial evals)",
         "ms_partial_evals": ms_pe, "ms_linear_map": ms_map, "ms_linear_map_bitsliced_in_place": ms_map_bs, "ms_gf128_mul": ms_mul,
         "ms_eq_expand_bitsliced": ms_eq, "ms_copy": ms_copy,
         "partial_evals_over_copy": ms_pe / cp, "linear_map_over_copy": ms_map / cp,
         "partial_evals_hbm_peak_fraction": (32 << n) / (ms_pe * 1e-3) / HBM_PEAK,
         # 128 x 128 word pairs per 32-element block, one v_bitop3 lane-operation each: 64 per wave-instruction
         "partial_evals_bitop3_ceiling_fraction": ((1 << n) / 32 * 16384 / 64) / (ms_pe * 1e-3) / BITOP3_CEILING,
         "linear_map_hbm_peak_fraction": (32 << n) / (ms_map * 1e-3) / HBM_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK})


def rs_pcs_line(dev, out, n=20, log_rate=2, schedule=(4, 4, 4, 4, 4), n_queries=32, runs=3):
    """Wall time of the packed opening (fri_pcs.prove_eval_packed) of a GF(2) witness of 2^(n+7) bits
    next to prove_eval of the same committed column in the same process, the best of `runs` each after
    a warm-up proof, with the splits; verify_eval_packed once."""
    import torch
    import binius_ntt_amd as B
    from binius_ntt_amd import fri_pcs
    g = np.random.default_rng(19)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(n, log_rate, B.FanPaarTowerField(7), device=dev.index or 0))
    x = torch.randint(-2**31, 2**31, (4 << n,), dtype=torch.int32, device=dev)
    r = g.integers(0, 2**32, size=(n + 7, 4), dtype=np.uint64).astype(np.uint32)
    com, state = fri_pcs.commit(ntt, x, list(schedule))
    torch.cuda.synchronize()
    best = {}
    for name, prove in (("packed", lambda: fri_pcs.prove_eval_packed(state, r, n_queries, fri_pcs.Transcript(b"bench"))),
                        ("plain", lambda: fri_pcs.prove_eval(state, r[7:], n_queries, fri_pcs.Transcript(b"bench")))):
        for _ in range(runs + 1):
            t0 = time.perf_counter()
            proof = prove()
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            if name not in best or s < best[name][0]:
                best[name] = (s, dict(state.timing), proof)
    proof = best["packed"][2]
    t0 = time.perf_counter()
    ok = fri_pcs.verify_eval_packed(n + 7, log_rate, list(schedule), com.root, r, proof.v, proof, n_queries, fri_pcs.Transcript(b"bench"))
    s_verify = time.perf_counter() - t0
    out({"config": "rs", "workload": "packed FRI-Binius opening, 2^%d bits (n %d), log_rate %d, schedule %s, %d queries"
         % (n + 7, n, log_rate, "+".join(str(a) for a in schedule), n_queries), "value": best["packed"][0] * 1e3,
         "unit": "ms per prove_eval_packed (wall)", "ms_split": {k: v * 1e3 for k, v in best["packed"][1].items()},
         "ms_prove_eval": best["plain"][0] * 1e3, "ms_split_prove_eval": {k: v * 1e3 for k, v in best["plain"][1].items()},
         "ring_switch_share": best["packed"][1]["ring_switch"] / best["packed"][0], "ms_verify_host": s_verify * 1e3,
         "accepted": bool(ok)})


BITOP3_CEILING = 8.36e11    # wave-instructions/s chip-wide
SHA_VALU_PER_BLOCK = 1400   # static VALU count of one unrolled compression in the ISA
SHA_VALU_PER_PAD_BLOCK = 1000  # the all-padding block of a leaf of a >= 2: rounds only


def merkle_line(dev, out, log_h=22, log_rate=2, reps=30):
    """SHA-256 Merkle commitment of a 2^(log_h+log_rate)-element GF(2^128) codeword: a = 1 and a = 4,
    the encode of the same plan, a device copy of the same bytes, and the commits of the fold schedule
    next to its folds, all in one process; ms per call, device events after a warm-up call."""
    import torch
    import binius_ntt_amd as B
    log_n = log_h + log_rate
    n = 1 << log_n
    g = np.random.default_rng(13)
    st = torch.cuda.current_stream(dev)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, log_rate, B.FanPaarTowerField(7), device=dev.index or 0))
    ch = g.integers(0, 2**32, size=(log_h, 4), dtype=np.uint64).astype(np.uint32)
    msg = torch.randint(-2**31, 2**31, (4 << log_h,), dtype=torch.int32, device=dev)
    cw = torch.empty(4 * n, dtype=torch.int32, device=dev)
    other = torch.empty(4 * n, dtype=torch.int32, device=dev)
    tree = torch.empty(32 * B.merkle_tree_digests(log_n - 1), dtype=torch.uint8, device=dev)

    def blocks(log_elems, a):
        """(leaves, compressions, VALU lane-instructions) of a commit of 2^log_elems elements at leaf size a."""
        leaves = 1 << (log_elems - a)
        data = leaves * max(1, (16 << a) // 64)
        pad = leaves if a >= 2 else 0
        nodes = leaves - 1
        return leaves, data + pad + nodes, (data + nodes) * SHA_VALU_PER_BLOCK + pad * SHA_VALU_PER_PAD_BLOCK

    def stats(log_elems, a, ms):
        leaves, comp, valu = blocks(log_elems, a)
        t = ms * 1e-3
        return {"ms": ms, "leaves_per_s": leaves / t, "compressions_per_s": comp / t,
                "hbm_peak_fraction": ((16 << log_elems) + 32 * (2 * leaves - 1)) / t / HBM_PEAK,
                "bitop3_ceiling_fraction": valu / 64 / t / BITOP3_CEILING,
                "passes": B.merkle_commit_passes(log_elems - a, a)}

    ms_enc = [ev_time(lambda: ntt.forward_device(msg, cw, stream=st), reps, st)]
    ms_copy = ev_time(lambda: other.copy_(cw), reps, st)
    ms_a1 = ev_time(lambda: B.merkle_commit(cw, log_n - 1, 1, tree, stream=st), reps, st)
    ms_a4 = ev_time(lambda: B.merkle_commit(cw, log_n - 4, 4, tree, stream=st), reps, st)
    ms_enc.append(ev_time(lambda: ntt.forward_device(msg, cw, stream=st), reps, st))
    enc = min(ms_enc)
    # the schedule: commit i is of the codeword of round rnd at a = the arity of the fold that follows
    full = [4] * (log_h // 4) + ([log_h % 4] if log_h % 4 else [])
    bufs = [cw, other]
    sched = []
    rnd, src = 0, 0
    for k in full:
        le = log_n - rnd
        ms_c = ev_time(lambda le=le, k=k, src=src: B.merkle_commit(bufs[src], le - k, k, tree, stream=st), reps, st)
        ms_f = ev_time(lambda rnd=rnd, k=k, src=src: ntt.fri_fold_device(bufs[src], bufs[1 - src], rnd, ch[rnd:rnd + k], stream=st), reps, st)
        sched.append(dict(stats(le, k, ms_c), round=rnd, arity=k, log_elems=le, ms_fold=ms_f))
        rnd, src = rnd + k, 1 - src
    a1, a4 = stats(log_n, 1, ms_a1), stats(log_n, 4, ms_a4)
    # the bound: the a = 4 commit takes no longer than the encode timed in this
    # process. Measured on one MI355X: 0.307 ms against 0.636 ms, a ratio of 0.48.
    binding = "VALU" if a4["bitop3_ceiling_fraction"] > a4["hbm_peak_fraction"] else "HBM"
    out({"config": "merkle", "workload": "SHA-256 Merkle commitment of a 2^%d-element GF(2^128) codeword (log_h %d, log_rate %d)"
         % (log_n, log_h, log_rate), "kernel": "bn::merkle_leaf_pass / bn::merkle_row_pass",
         "value": a4["leaves_per_s"], "unit": "leaves/s (a = 4)", "commit_a1": a1, "commit_a4": a4,
         "ms_encode": ms_enc, "ms_copy_d2d": ms_copy, "a4_over_encode": ms_a4 / enc, "bound_a4_over_encode": 1.0,
         "a1_over_encode": ms_a1 / enc, "a4_over_copy": ms_a4 / ms_copy, "binding_resource_a4": binding,
         "schedule": sched, "ms_schedule_commits": sum(x["ms"] for x in sched), "ms_schedule_folds": sum(x["ms_fold"] for x in sched),
         "valu_per_compression": SHA_VALU_PER_BLOCK, "valu_per_padding_block": SHA_VALU_PER_PAD_BLOCK,
         "bitop3_ceiling_wave_instructions_per_s": BITOP3_CEILING, "hbm_peak_bytes_per_s": HBM_PEAK})


def c4(dev, out, nvars, ds):
    import torch
    import binius_ntt_amd as B
    for d in ds:
        g = np.random.default_rng(0x5C00 + d)
        words = 4 * (1 << nvars) * d
        ev = torch.from_numpy(g.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32)
                              .view(np.int32)).to(dev)
        ch = g.integers(0, 2**32, size=(nvars, 4), dtype=np.uint64).astype(np.uint32)
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):  # median of 3 whole protocol runs (the first also warms the kernels)
            sc = B.Sumcheck(nvars, d, True, ev)  # copies the columns (device to device)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r in range(nvars):
                sc.this_round_messages()
                sc.move_to_next_round(ch[r])
            sc.this_round_messages()
            runs.append(time.perf_counter() - t0)
            sc.close()
        dt = sorted(runs)[1]
        del ev
        torch.cuda.empty_cache()
        out({"config": "c4", "workload": "sumcheck GF(2^128), 2^%d evals, d=%d, bitsliced input" % (nvars, d),
             "value": (1 << nvars) / dt, "unit": "evals/s", "ms": dt * 1e3,
             "hbm_gbps_algorithmic": 3.0 * d * 16 * (1 << nvars) / dt / 1e9})


def c4_phases(dev, out, nvars, d, runs=3):
    """The reference's sumcheck benchmark shape (src/ulvt/sumcheck/bench/benchmark.cu:12-46, main at
    :71-85 runs N in {20, 24, 28} x d in {2, 3, 4}): DATA_IS_TRANSPOSED = false, timed as memcpy
    (compact host evals -> HBM; the reference copies from a pageable std::vector, reported as
    memcpy_ms, with the pinned-staging copy beside it), transpose (prover construction from the
    compact device columns: copy + bitslice transpose on the device) and raw (all rounds + the final
    messages); medians of `runs` after one warm-up. Inputs above 1 GiB repeat a random 64 MiB pattern
    (the reference feeds zeros; the kernels have no data-dependent control flow)."""
    import torch
    import binius_ntt_amd as B
    g = np.random.default_rng(0x5CF0 + d)
    words = 4 * (1 << nvars) * d
    if words <= (1 << 28):
        host = g.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32).view(np.int32)
    else:
        pat = g.integers(0, 2**32, size=1 << 24, dtype=np.uint64).astype(np.uint32).view(np.int32)
        host = np.tile(pat, words // pat.size)
    pinned = torch.from_numpy(host).pin_memory()
    ch = g.integers(0, 2**32, size=(nvars, 4), dtype=np.uint64).astype(np.uint32)
    res = []
    for it in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sc = B.Sumcheck(nvars, d, False, ev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for r in range(nvars):
            sc.this_round_messages()
            sc.move_to_next_round(ch[r])
        sc.this_round_messages()
        t3 = time.perf_counter()
        sc.close()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        ev.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        del ev
        if it:
            res.append((t1 - t0, t2 - t1, t3 - t2, t5 - t4))
    del pinned
    torch.cuda.empty_cache()
    med = [sorted(x)[len(x) // 2] * 1e3 for x in zip(*res)]
    out({"config": "c4", "workload": "sumcheck GF(2^128), 2^%d evals, d=%d, compact input "
                                     "(DATA_IS_TRANSPOSED=false): memcpy / transpose / raw" % (nvars, d),
         "memcpy_ms": med[0], "memcpy_pinned_ms": med[3], "transpose_ms": med[1], "raw_ms": med[2],
         "total_ms": med[0] + med[1] + med[2],
         "value": (1 << nvars) / (med[2] * 1e-3), "unit": "evals/s (raw)", "runs": runs,
         "memcpy_note": "memcpy_ms: pageable numpy -> HBM (the reference's std::vector source); "
                        "memcpy_pinned_ms: the same bytes from a pinned staging tensor"})


def c5_sumcheck_single(dev, out, nvars=28, d=3):
    """The whole 2^28-eval d=3 sumcheck on ONE GPU (12.9 GB of columns, fits in 288 GB)."""
    import torch
    import binius_ntt_amd as B
    g = torch.Generator(device=dev)
    g.manual_seed(0x5C00 + d)
    ev = torch.randint(-2**31, 2**31 - 1, (4 * (1 << nvars) * d,), dtype=torch.int32, device=dev, generator=g)
    ch = np.random.default_rng(1).integers(0, 2**32, size=(nvars, 4), dtype=np.uint64).astype(np.uint32)
    sc = B.Sumcheck(nvars, d, True, ev)
    del ev
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(nvars):
        sc.this_round_messages()
        sc.move_to_next_round(ch[r])
    sc.this_round_messages()
    dt = time.perf_counter() - t0
    sc.close()
    out({"config": "c5 (1 GPU, whole problem)", "workload": "sumcheck GF(2^128), 2^%d evals, d=%d, bitsliced input"
         % (nvars, d), "value": (1 << nvars) / dt, "unit": "evals/s", "ms": dt * 1e3})


def c5_sumcheck_shard(dev, out, nvars=28, d=3, world=8):
    import torch
    import binius_ntt_amd as B
    g = torch.Generator(device=dev)
    g.manual_seed(0x5C00 + d)
    ev = torch.randint(-2**31, 2**31 - 1, (4 * (1 << nvars) * d,), dtype=torch.int32, device=dev, generator=g)
    sc = B.Sumcheck(nvars, d, True, ev, shard=(0, world))  # keeps batches b % 8 == 0
    del ev
    torch.cuda.empty_cache()
    ch = np.random.default_rng(1).integers(0, 2**32, size=(nvars, 4), dtype=np.uint64).astype(np.uint32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = 0
    while not sc.needs_gather():
        sc.this_round_messages()
        sc.move_to_next_round(ch[r])
        r += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sc.close()
    out({"config": "c5 (per-GPU share)", "workload": "sumcheck GF(2^128), 2^%d evals, d=%d, shard 0 of %d: %d local rounds"
         % (nvars, d, world, r), "value": (1 << nvars) / world / dt, "unit": "evals/s (this shard)", "ms": dt * 1e3})


def bb_line(dev, out, log_n, batch):
    import torch
    import binius_ntt_amd as B
    st = torch.cuda.current_stream(dev)
    n = 1 << log_n
    x = torch.from_numpy(np.random.default_rng(9).integers(0, 2**32, size=n * batch, dtype=np.uint64)
                         .astype(np.uint32).view(np.int32)).to(dev)
    y = torch.empty_like(x)
    ntt = B.NTT(B.NTTConfRad2(B.BB31(137), 27, log_n))
    ms = ev_time(lambda: ntt.forward_device(x, y, batch=batch, stream=st), 20, st)
    out({"config": "bb", "workload": "BabyBear NTT 2^%d x %d (natural order in/out)" % (log_n, batch),
         "value": n * batch / (ms * 1e-3), "unit": "elements/s", "ms": ms,
         "hbm_gbps_algorithmic": 8 * n * batch / (ms * 1e-3) / 1e9})


def qm_line(dev, out, nvars, reps=3):
    import torch
    import binius_ntt_amd.prime_field as PF
    ev = np.random.default_rng(11).integers(0, 2**31 - 1, size=(2 << nvars, 4), dtype=np.uint64).astype(np.uint32)
    r = PF.QM31([32482843, 85864538, 8348234, 9544334])
    best = None
    for _ in range(reps):
        sc = PF.Sumcheck(nvars, ev, device=dev.index or 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nvars):
            sc.this_round_messages()
            sc.fold(r)
        sc.final_values()
        dt = time.perf_counter() - t0
        sc.close()
        best = dt if best is None else min(best, dt)
    out({"config": "qm", "workload": "QM31 sumcheck 2 x 2^%d, d=2, all rounds" % nvars,
         "value": (1 << nvars) / best, "unit": "evals/s", "ms": best * 1e3,
         # per round over cur evals: the fused fold+messages pass reads 2 x 16 B x cur and writes
         # half of that; sum of cur over rounds ~ 2 x 2^N  ->  96 B per eval
         "hbm_gbps_algorithmic": 96 * (1 << nvars) / best / 1e9})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c2,c3,c4,c5,bb,qm")
    ap.add_argument("--sc-vars", type=int, default=24)
    ap.add_argument("--sc-d", default="2,3,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    lines = []

    def out(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    only = set(a.only.split(","))
    if "c2" in only:
        c2(dev, out)
    if "c3" in only:
        ntt_line(dev, out, "c3", 20, 1)
    if "c4" in only:
        c4(dev, out, a.sc_vars, [int(x) for x in a.sc_d.split(",")])
        for d in [int(x) for x in a.sc_d.split(",")]:
            c4_phases(dev, out, a.sc_vars, d)
    if "c5" in only:
        ntt_line(dev, out, "c5 (per-GPU share)", 20, 32)
        c5_sumcheck_shard(dev, out)
        c5_sumcheck_single(dev, out)
    if "bb" in only:
        bb_line(dev, out, 24, 1)
        bb_line(dev, out, 20, 16)
    if "qm" in only:
        qm_line(dev, out, 24)
    if "intt" in only:
        intt_line(dev, out, 20)
        intt_line(dev, out, 24)
    if "fold" in only:
        fold_line(dev, out)
    if "eq" in only:
        eq_line(dev, out, 24, True)
        eq_line(dev, out, 20, False)
    if "merkle" in only:
        merkle_line(dev, out)
    if "bitrev" in only:
        bitrev_line(dev, out, 24, True)
        bitrev_line(dev, out, 20, False)
    if "pcs" in only:
        pcs_line(dev, out)
    if "rs" in only:
        rs_line(dev, out, 24)
        rs_line(dev, out, 20)
        rs_pcs_line(dev, out)
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
