#!/usr/bin/env python3
"""Headline benchmark: 2^24-point GF(2^128) additive NTT (BASELINE.json north star), plus the
config-5 multi-GPU workloads.

One "step" = one full forward transform (log_h = 24, log_rate = 0) of a device-resident,
synthetic GF(2^128) vector (numpy PCG64, seed 0xdeadbeef + 24 + rank) into a separate device
output buffer. The oracle (test infrastructure) is used only by the cpu_baseline leg.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--log-h 24] [--dump-outputs DIR]
                  [--full [--no-cpu] [--no-c5] [--no-configs]]

A plain run sets up, warms up, times the K transforms and prints the headline line (metric, value,
ms_per_step, ...). --dump-outputs DIR then writes the last timed transform's output (rank 0) as
DIR/additive_ntt_out.npy: float64 (exact for u32 limbs), shape (rows, 4), all rows up to 2^20 points and
a fixed seeded sample of 2^20 rows (ascending) above that. The inputs are seeded, so two builds can
be compared output for output. Everything else is measured only with --full: the per-pass timings
and rooflines, the limb-0 MD5 check against the reference table, the c5 and configs legs listed
below, apply_e2e and the CPU baseline.

--gpus N > 1 without a torch.distributed environment re-launches this script as a child
`python -m torch.distributed.run --nproc-per-node N` (before anything touches the GPU) and exits
with its status. Under torch.distributed every rank drives one GPU:
  * headline: every rank transforms its own 2^24 vector (independent transforms = batched
    sharding, weak scaling, no data-path collective); the timed region is bracketed by barriers +
    synchronize and the max over ranks is reported;
  * c5.batched_ntt: 256 x 2^20-point transforms split over the ranks (rank g owns a contiguous
    slice, no collective; strong scaling over the fixed batch);
  * configs (world 1 only): BASELINE.json configs 2-4 through tools/bench_configs.py -- the
    GF(2^128) multiply repeat loops, the 2^20-point NTT, and the 2^24-eval d = 3 sumcheck with
    bitsliced input and with compact input (memcpy / transpose / raw, the reference harness's
    phases);
  * c5.sumcheck: the 2^28-evaluation, d = 3 bitsliced sumcheck sharded by 32-element batch
    (b mod world == rank); every round all-gathers the (d + 2) x 16 B partial messages and XORs
    them (RCCL has no XOR reduction); the endgame gathers the last batches.
Rank 0 prints one JSON line. BENCH_DIST_BACKEND=gloo rehearses the multi-rank path on fewer
GPUs (ranks then share devices round-robin; collectives run on CPU tensors).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "binius-ntt_amd", "python"))

HBM_PEAK_GBPS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
# VALU issue peak: 256 CU x 4 SIMD x 0.5 wave64 instructions/cycle (SIMD-32) x 2.4 GHz
VALU_PEAK_WAVE_INSTS = 256 * 4 * 0.5 * 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-h", type=int, default=24)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed transform's output to DIR/additive_ntt_out.npy (float64, rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: per-pass timings and rooflines, the output "
                         "MD5 check, the c5 and configs legs, apply_e2e and the CPU baseline")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--no-c5", action="store_true", help="with --full: skip the config-5 legs")
    ap.add_argument("--no-configs", action="store_true",
                    help="with --full: skip the configs 2-4 leg (world 1 only)")
    ap.add_argument("--c5-log-n", type=int, default=20)
    ap.add_argument("--c5-batch", type=int, default=256)
    ap.add_argument("--c5-steps", type=int, default=3)
    ap.add_argument("--sc-log-n", type=int, default=28)
    ap.add_argument("--sc-d", type=int, default=3)
    ap.add_argument("--sc-runs", type=int, default=2)
    ap.add_argument("--sc-exchange", choices=("auto", "host", "device"), default="auto",
                    help="config-5 sumcheck message exchange: auto = device sink on nccl, host-staged "
                         "on gloo; device on gloo stages the sink through host memory")
    ap.add_argument("--variant", type=int, default=None, help="NTT kernel variant (default: the plan's choice)")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU rehearsal of the launch path: the --gpus relaunch, process-group setup (gloo), "
                         "barriers, max-over-ranks timing, batch slicing and the sharded message exchange, "
                         "with no GPU work; prints one JSON line")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


DUMP_ROWS = 1 << 20  # 2^20 rows x 4 limbs x 8 B = 32 MB of float64
SETTLE_SECONDS = 0.3  # untimed transforms before a plain run's timed steps (see main)


def dump_outputs(path, d_out, n, torch, np):
    """--dump-outputs: the timed transform's output (n GF(2^128) elements as u32 limbs) as float64,
    whole up to DUMP_ROWS elements, else the rows of a fixed seeded sample (ascending)."""
    rows = d_out.view(-1, 4)
    if n > DUMP_ROWS:
        idx = np.sort(np.random.default_rng(0xD0A7).choice(n, size=DUMP_ROWS, replace=False))
        rows = rows[torch.from_numpy(idx).to(d_out.device)]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "additive_ntt_out.npy"), rows.cpu().numpy().view(np.uint32).astype(np.float64))


def relaunch_if_needed(a):
    """--gpus N without a torch.distributed environment: run N ranks as a child process group
    (never exec: the parent has not touched the GPU, the child does) and exit with its status."""
    if "WORLD_SIZE" in os.environ:
        world = int(os.environ["WORLD_SIZE"])
        if world != a.gpus:
            raise SystemExit("bench.py: --gpus %d disagrees with WORLD_SIZE=%d" % (a.gpus, world))
        return
    if a.gpus <= 1:
        return
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def cpu_info():
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        allowed = len(os.sched_getaffinity(0))
    except AttributeError:
        allowed = os.cpu_count()
    threads = allowed
    cap = os.environ.get("OMP_NUM_THREADS")
    if cap and cap.isdigit() and int(cap) > 0:
        threads = min(threads, int(cap))  # the box's CPU share for one GPU
    return model, os.cpu_count(), allowed, threads


def cpu_baseline():
    """The oracle (a C restatement of the reference algorithm, oracle/antt.c) on the GPU box's
    own host cores: 1 thread and all usable threads, at 2^10, 2^20 and 2^24 points."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import _oracle as O
    model, nproc, allowed, threads = cpu_info()
    L = O.lib()
    per_size = {}
    total = 0.0
    for log_h in (10, 20, 24):
        x = O.fill128(0xDEADBEEF + log_h, 0x5EED0000, 1 << log_h)
        out = np.zeros_like(x)
        row = {}
        for nt in (1, threads):
            reps = max(1, min(200, (1 << 20) // (1 << log_h)))
            used = L.orc_antt_mt_threads(log_h, nt)  # at most one thread per 4096 butterflies of a stage
            t0 = time.perf_counter()
            for _ in range(reps):
                L.orc_antt128_limbwise_mt(x.reshape(-1), out.reshape(-1), log_h, 0, nt)
            dt = (time.perf_counter() - t0) / reps
            total += dt * reps
            row["threads_%d" % nt] = {"elements_per_s": (1 << log_h) / dt, "ms": dt * 1e3, "reps": reps,
                                      "threads_used": used}
        per_size["2^%d" % log_h] = row
    head = per_size["2^24"]["threads_%d" % threads]
    return {"value": head["elements_per_s"], "unit": "elements/s", "cores": threads, "kind": "port",
            "sample": "one 2^24-point GF(2^128) additive NTT (r=0) by oracle/antt.c (C port of the reference "
                      "algorithm, butterflies of each stage split over a persistent pool of %d threads); per_size has "
                      "1 thread and %d threads at 2^10/2^20/2^24, each row with the threads it used (at most "
                      "one per 4096 butterflies of a stage: 1 at 2^10) (%.1f s of CPU work in all)" % (threads, threads, total),
            "cpu_model": model, "nproc": nproc, "cpus_allowed": allowed, "per_size": per_size,
            "share": {"threads_used": threads,
                      "basis": "OMP_NUM_THREADS=%s: the GPU box's CPU share for one GPU" % os.environ.get("OMP_NUM_THREADS", "unset"),
                      "full_host_row": "not run: cpus_allowed (%d) is the whole host, which other jobs share; a run "
                                       "is held to its per-GPU thread share, so the baseline is a %d-thread share of "
                                       "the host, not the host" % (allowed, threads)}}


def limb0_check(d_out, log_h):
    """MD5 of the timed loop's output limb-0 plane against the reference table entry (the golden
    data file tests/golden/additive_ntt_md5.json holds test_ntt.cu:52-124 as data)."""
    import hashlib
    import numpy as np
    plane = d_out.view(-1, 4)[:, 0].contiguous().cpu().numpy().view(np.uint32)
    got = hashlib.md5(plane.tobytes()).hexdigest()
    want = None
    try:
        with open(os.path.join(ROOT, "tests", "golden", "additive_ntt_md5.json")) as f:
            want = json.load(f)["hashes"]["0"][log_h] or None  # list indexed by log_h
    except (OSError, ValueError, KeyError, IndexError):
        pass
    ok = want is not None and got == want
    if want is not None and not ok:
        print("bench.py: OUTPUT MISMATCH: limb-0 MD5 %s != reference %s" % (got, want), file=sys.stderr)
    return {"limb0_md5": got, "reference_md5": want, "match": ok,
            "source": "additive_ntt_hashes[0][%d] (src/ulvt/ntt/tests/test_ntt.cu:52-124)" % log_h}


PMC_FILE = os.path.join("profiles", "r06", "pmc_kernels.json")
# the practical VALU ceiling of these kernels: independent 3-VGPR-operand v_bitop3_b32 streams issue
# at ~0.34 per SIMD-cycle at any occupancy (binius-ntt_amd/tools/microbench4.hip)
BITOP3_CEILING = VALU_PEAK_WAVE_INSTS * 0.34 / 0.5
TARGET_HBM_FRAC = 0.60  # the north star's target fraction of the HBM roofline


def lib_sha256():
    import hashlib
    with open(os.path.join(ROOT, "binius-ntt_amd", "lib", "libbinius_ntt_amd.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def kernel_counters(name):
    """Committed rocprofv3 PMC counters (tools/pmc_summary.py --kernels) of the kernel `name`
    (demangled; a name without its argument list matches by prefix), or (None, reason) when the
    profiled library is not this one (SHA-256 of the .so) or the kernel was not profiled."""
    try:
        with open(os.path.join(ROOT, PMC_FILE)) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        return None, "no %s" % PMC_FILE
    if doc.get("lib_sha256") != lib_sha256():
        return None, "%s was profiled on another build of the library" % PMC_FILE
    ks = doc.get("kernels", {})
    if name in ks:
        return ks[name], None
    for k, v in ks.items():
        if "(" not in name and k.split("(")[0].replace("void ", "") == name:
            return v, None
    return None, "kernel %s not in %s" % (name, PMC_FILE)


def valu_transform(ntt, n_passes, ms_step, alg_bytes):
    """The roofline that binds the whole transform: its VALU wave-instructions (the sum over its
    passes, from the committed PMC counters of this library build) per transform time, against the
    nominal issue peak and the bitop3 ceiling; and the instruction budget the north star's 60 %-of-HBM
    target implies at that ceiling."""
    per_pass, total, why = [], 0, None
    for i in range(n_passes):
        name = ntt.pass_kernel_name(i)
        ctr, w = kernel_counters(name) if name else (None, "no kernel name")
        insts = ctr.get("SQ_INSTS_VALU") if ctr else None
        per_pass.append({"pass": i, "kernel": name, "valu_insts": insts})
        if insts is None:
            why = why or w
        else:
            total += insts
    if why is not None:
        return {"insts_per_transform": None, "note": why, "per_pass": per_pass}
    rate = total / (ms_step * 1e-3)
    t_target = alg_bytes / (TARGET_HBM_FRAC * HBM_PEAK_GBPS * 1e9)
    budget = BITOP3_CEILING * t_target
    return {"insts_per_transform": total, "per_pass": per_pass, "achieved": rate, "unit": "wave64 instructions/s",
            "frac_nominal_peak": rate / VALU_PEAK_WAVE_INSTS, "nominal_peak": VALU_PEAK_WAVE_INSTS,
            "frac_bitop3_ceiling": rate / BITOP3_CEILING, "bitop3_ceiling": BITOP3_CEILING,
            "floor_ms_at_ceiling": total / BITOP3_CEILING * 1e3,
            "hbm_frac_cap_at_ceiling": alg_bytes / (total / BITOP3_CEILING) / 1e9 / HBM_PEAK_GBPS,
            "target": {"hbm_frac": TARGET_HBM_FRAC, "ms": t_target * 1e3, "insts_budget_at_ceiling": budget,
                       "reduction_needed": total / budget},
            "source": PMC_FILE + " (library SHA-256 checked)",
            "note": "the transform is bound by VALU issue, not HBM: at the bitop3 ceiling its instructions take "
                    "floor_ms_at_ceiling, which caps the HBM fraction at hbm_frac_cap_at_ceiling; the 60 % target "
                    "needs insts_budget_at_ceiling instructions per transform"}


def limiter_of(valu, hbm_frac, ctr):
    """What bounds the dominant pass, from its committed counters: VALU issue when its VALU
    instruction rate is a larger fraction of the bitop3 issue ceiling than its algorithmic bytes are
    of the HBM peak, HBM otherwise; with the share of wave time parked on s_waitcnt (SQ_WAIT_ANY)."""
    v = valu.get("bitop3_ceiling_frac") if valu else None
    if v is None:
        return {"limiter": None, "why": "no PMC counters of this library build (%s)" % (valu or {}).get("note")}
    out = {"limiter": "valu-issue" if v >= hbm_frac else "hbm",
           "why": "VALU at %.2f of the bitop3 issue ceiling vs algorithmic HBM bytes at %.2f of peak" % (v, hbm_frac)}
    if ctr and ctr.get("SQ_WAVE_CYCLES") and ctr.get("SQ_WAIT_ANY") is not None:
        out["wait_share"] = ctr["SQ_WAIT_ANY"] / ctr["SQ_WAVE_CYCLES"]
    return out


def c5_sumcheck(a, B, D, torch, dev, local, rank, world, backend, barrier, max_over_ranks):
    """Config 5's 2^28-evaluation d = 3 sumcheck, sharded by 32-element batch over the ranks, with the
    per-round all-gather + XOR exchange (distributed.ShardedSumcheck); medians over a.sc_runs."""
    import numpy as np
    N, d = a.sc_log_n, a.sc_d
    local_words = d * (4 << N) // world
    chunks = []
    left = local_words
    while left:
        m = min(left, 1 << 30)
        chunks.append(torch.randint(-2**31, 2**31 - 1, (m,), dtype=torch.int32, device=dev))
        left -= m
    shard = torch.cat(chunks) if len(chunks) > 1 else chunks[0]
    del chunks
    rng = np.random.default_rng(0xC4A1)
    challenges = rng.integers(0, 2**32, size=(N, 4), dtype=np.uint64).astype(np.uint32)
    group = None

    exch = []

    def run_sumcheck(check):
        prover = B.Sumcheck.from_shard(N, d, shard, rank, world, device=local)
        dx = None if a.sc_exchange == "auto" else a.sc_exchange == "device"
        sc = D.ShardedSumcheck(prover, group, device_exchange=dx)
        exch.append(sc)
        barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        claim = None
        ok = True
        for i in range(N):
            s, pts = sc.this_round_messages()
            if check:
                if claim is not None and not np.array_equal(s, claim):
                    ok = False
                if not np.array_equal(s, pts[0] ^ pts[1]):
                    ok = False
                claim = B.evaluate_univariate_given_points(challenges[i], pts)
            sc.move_to_next_round(challenges[i])
        s, _ = sc.this_round_messages()  # final claim: prod_j f_j(r)
        if check and claim is not None and not np.array_equal(s, claim):
            ok = False
        torch.cuda.synchronize(dev)
        barrier()
        el = max_over_ranks(time.perf_counter() - t0)
        prover.close()
        return el, ok

    run_sumcheck(False)  # warm-up (kernels, allocator, collectives)
    times, oks = [], []
    for _ in range(max(1, a.sc_runs)):
        el, ok = run_sumcheck(True)
        times.append(el)
        oks.append(ok)
    tsc = sorted(times)[len(times) // 2]
    last = exch[-1]
    ex_ms = max_over_ranks(last.exchange_seconds * 1e3)
    alg = sum(d * 16 * ((1 << (N - i)) + (1 << (N - i - 1))) for i in range(N))
    res = {
        "workload": "GF(2^128) sumcheck, 2^%d evals, d=%d, bitsliced, sharded %d ways by 32-element batch; "
                    "all %d rounds incl. per-round all-gather+XOR of partial messages" % (N, d, world, N),
        "ms": tsc * 1e3, "evals_per_s": (1 << N) / tsc, "runs": len(times),
        "protocol_checks_pass": all(oks),
        "per_gpu_alg_gbps": alg / world / tsc / 1e9,
        "collective": "all_gather_into_tensor (%s) + XOR" % (backend if world > 1 else "none, world 1"),
        "exchange_ms": ex_ms, "exchange_rounds": last.exchange_rounds,
        "exchange_ms_per_round": ex_ms / last.exchange_rounds if last.exchange_rounds else None,
        "exchange_path": "device sink" if last.device_exchange else "host-staged",
        "messages_ms_per_round": max_over_ranks(last.round_seconds * 1e3) / N}
    del shard
    return res


def dry_run(a, json_out):
    """--dry-run: everything of the multi-rank path that does not need a GPU (tests/test_bench_cli.py)."""
    import numpy as np
    import torch.distributed as dist
    from binius_ntt_amd import distributed as D
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    res = {"dry_run": True, "n_gpus": world, "rank_checks": []}
    if world > 1:
        dist.barrier()
        ex = D.WordExchange(4 * (a.sc_d + 2))
        mine = np.random.default_rng(rank).integers(0, 2**32, size=ex.n, dtype=np.uint64).astype(np.uint32)
        want = np.bitwise_xor.reduce(np.stack([np.random.default_rng(r).integers(0, 2**32, size=ex.n, dtype=np.uint64)
                                               .astype(np.uint32) for r in range(world)]), axis=0)
        got = ex.xor(mine)
        t = __import__("torch").tensor([float(rank)], dtype=__import__("torch").float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        lo, hi = D.batch_slice(a.c5_batch, rank, world)
        sizes = [0] * world
        dist.all_gather_object(sizes, hi - lo)
        res["rank_checks"] = {"xor_exchange_ok": bool(np.array_equal(got, want)), "max_over_ranks": t.item(),
                              "batch_slices_cover": sum(sizes) == a.c5_batch}
        dist.barrier()
    if rank == 0:
        json_out.write(json.dumps(res) + "\n")
        json_out.flush()
    if world > 1:
        dist.destroy_process_group()


def main():
    a = parse()
    relaunch_if_needed(a)
    if a.dry_run:
        json_out = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
        return dry_run(a, json_out)
    # stdout carries exactly one JSON line (rank 0): library chatter (e.g. gloo's connection
    # messages on std::cout) is sent to stderr by pointing fd 1 there for the rest of the run
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    import numpy as np
    import torch
    import torch.distributed as dist
    import binius_ntt_amd as B
    from binius_ntt_amd import distributed as D

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    local = local % max(1, ndev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local)
    stream = torch.cuda.current_stream(dev)

    def barrier():
        if world > 1:
            dist.barrier()

    def max_over_ranks(v):
        if world == 1:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def timed(fn, reps):
        barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(dev)
        barrier()
        return max_over_ranks(time.perf_counter() - t0)

    # ---------------- headline: 2^24 GF(2^128) additive NTT, one transform per rank
    log_h = a.log_h
    n = 1 << log_h
    # limb 0 = the reference test's input stream, std::mt19937(0xdeadbeef + log_h) (test_ntt.cu:192-199;
    # numpy's legacy MT19937 seeding is the same generator), so the output limb-0 plane must hash to
    # additive_ntt_hashes[0][log_h] (test_ntt.cu:52-124) -- checked after the timed loop; limbs 1..3 =
    # numpy PCG64 words (independent per rank)
    x = np.random.default_rng(0xDEADBEEF + log_h + rank).integers(0, 2**32, size=(n, 4), dtype=np.uint64)
    x = x.astype(np.uint32)
    x[:, 0] = np.random.RandomState(0xDEADBEEF + log_h).randint(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    d_in = torch.from_numpy(x.reshape(-1).view(np.int32)).to(dev)
    del x
    d_out = torch.empty_like(d_in)
    ntt = B.AdditiveNTT(B.AdditiveNTTConf(log_h, 0, B.FanPaarTowerField(7), device=local))
    if a.variant is not None:
        ntt.set_variant(a.variant)
    for _ in range(a.warmup):
        ntt.forward_device(d_in, d_out, stream=stream)
    torch.cuda.synchronize(dev)

    if a.full:
        # per-pass durations inside the back-to-back transform loop: hipEvents recorded between the
        # pass launches of consecutive transforms (no host synchronisation between launches), averaged
        # per pass; profiles/r02 holds the rocprofv3 kernel trace of the same loop for comparison
        ntt.set_event_timing(True)
        for _ in range(max(5, min(a.steps, 20))):
            ntt.forward_device(d_in, d_out, stream=stream)
        torch.cuda.synchronize(dev)
        pass_ms_inloop = ntt.event_timing()
        ntt.set_event_timing(False)
        # steady-state duration per launch of each pass: the pass launched back to back between two
        # events only (bn_antt_time_passes), so no event sits between the timed launches; d_out is
        # scratch here and is overwritten by the timed loop below
        pass_ms = ntt.time_passes(d_in, d_out, reps=max(10, min(a.steps, 40)), stream=stream)
        torch.cuda.synchronize(dev)
    else:
        # the GPU's clocks reach their steady state only after tens of milliseconds of load: a few
        # warm-up transforms (0.7 ms each) do not get there, the per-pass loops above do. A plain
        # run keeps the device busy with untimed transforms for SETTLE_SECONDS instead, so that
        # ms_per_step is the same steady-state figure with and without --full
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < SETTLE_SECONDS:
            for _ in range(10):
                ntt.forward_device(d_in, d_out, stream=stream)
            torch.cuda.synchronize(dev)

    dt = timed(lambda: ntt.forward_device(d_in, d_out, stream=stream), a.steps)
    ms_step = dt / a.steps * 1e3
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, d_out, n, torch, np)
    elems_per_s = world * n / (dt / a.steps)
    alg_bytes = 2 * 16 * n  # read input once + write output once
    transform_gbps = alg_bytes / (ms_step * 1e-3) / 1e9

    res = None
    if rank == 0:
        res = {
            "metric": "GF(2^128) additive-NTT elements/sec (2^%d pts)" % log_h,
            "value": elems_per_s,
            "unit": "elements/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "gf2_128 (u32 limbs, bitwise)",
            "data": "synthetic: limb 0 = std::mt19937(0xdeadbeef + log_h) (the reference test stream), limbs 1-3 "
                    "numpy PCG64",
            "config": {"workload": "additive NTT over GF(2^128), log_h=%d, log_rate=0, one transform per GPU"
                                   % log_h, "log_h": log_h, "log_rate": 0, "field": "GF(2^128)",
                       "kernel_variant": ntt.variant(), "parallelism": "independent transform per rank"},
            "hbm_gbps_transform": transform_gbps,
        }
    if not a.full:
        if rank == 0:
            json_out.write(json.dumps(res) + "\n")
            json_out.flush()
        if world > 1:
            dist.destroy_process_group()
        return

    out_check = limb0_check(d_out, log_h)
    if rank == 0:
        # dominant kernel = the pass with the largest mean duration; every pass reads and writes
        # the whole vector once, so its algorithmic bytes are the same 32 B/element
        dom = max(range(len(pass_ms)), key=lambda i: pass_ms[i]) if pass_ms else None
        dom_ms = pass_ms[dom] if dom is not None else ms_step
        achieved = alg_bytes / (dom_ms * 1e-3) / 1e9
        dom_kernel = ntt.pass_kernel_name(dom) if dom is not None else None
        ctr, why = kernel_counters(dom_kernel) if dom_kernel else (None, "no pass")
        traffic = ctr.get("HBM_BYTES") if ctr else None
        valu = {"kernel": dom_kernel, "insts_per_launch": None, "note": why}
        if ctr and ctr.get("SQ_INSTS_VALU"):
            insts = ctr["SQ_INSTS_VALU"]
            rate = insts / (dom_ms * 1e-3)
            valu = {"kernel": dom_kernel, "insts_per_launch": insts, "achieved": rate, "peak": VALU_PEAK_WAVE_INSTS,
                    "unit": "wave64 instructions/s", "frac": rate / VALU_PEAK_WAVE_INSTS,
                    # practical ceiling of this instruction mix: independent 3-VGPR-operand v_bitop3_b32
                    # streams issue at ~0.34 per SIMD-cycle at any occupancy (binius-ntt_amd/tools/
                    # microbench4.hip), not the nominal 0.5
                    "bitop3_ceiling_frac": rate / BITOP3_CEILING,
                    "source": PMC_FILE + " (library SHA-256 checked)"}
        # kept in the driver's parsed record (the top-level output_check is not)
        res["config"]["output_check"] = ("limb-0 MD5 of the timed output %s additive_ntt_hashes[0][%d] (%s)"
                                         % ("==" if out_check["match"] else "!=", log_h, out_check["limb0_md5"]))
        res.update({
            "output_check": out_check,
            "roofline": {
                # the roofline the metric is priced against (the north star's HBM roofline); what
                # actually binds the kernel is binding_resource below (VALU issue), see valu_transform
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBPS,
                "traffic": traffic,
                "traffic_source": (PMC_FILE + ": FETCH_SIZE x 2 + WRITE_SIZE of this kernel") if traffic else why,
                "kernel": "pass %s of %d: %s" % (dom, len(pass_ms), dom_kernel),
                "kernel_ms": dom_ms,
                "pass_ms": pass_ms,
                "pass_ms_source": "each pass launched back to back between two hipEvents (bn_antt_time_passes)",
                "pass_ms_inloop": pass_ms_inloop,
                "transform_frac": transform_gbps / HBM_PEAK_GBPS,
                "binding_resource": limiter_of(valu, achieved / HBM_PEAK_GBPS, ctr),
                "duration_note": "kernel_ms / pass_ms are uninstrumented hipEvent timings of back-to-back "
                                 "launches; in the committed rocprofv3 traces (profiles/) the timed-loop "
                                 "launches agree within ~2 %, while the all-launch stats averages include "
                                 "warm-up and event-bracketed launches and run ~6-9 % longer, so frac "
                                 "recomputed from those is lower by that much",
            },
            "valu": valu,
            "valu_transform": valu_transform(ntt, len(pass_ms), ms_step, alg_bytes),
        })
    del d_in, d_out

    # ---------------- config 5: 256 x 2^20 batched NTT, sharded by transform
    c5 = None
    if not a.no_c5:
        c5 = {}
        lo, hi = D.batch_slice(a.c5_batch, rank, world)
        mine = hi - lo
        nb = 1 << a.c5_log_n
        bt_in = torch.randint(-2**31, 2**31 - 1, (max(mine, 1) * 4 * nb,), dtype=torch.int32, device=dev)
        # limb 0 of this rank's first transform = the reference stream std::mt19937(0xdeadbeef + log_n):
        # its output limb-0 plane must hash to additive_ntt_hashes[0][log_n] (checked after timing)
        mt = np.random.RandomState(0xDEADBEEF + a.c5_log_n).randint(0, 2**32, size=nb, dtype=np.uint64).astype(np.uint32)
        bt_in.view(-1, 4)[:nb, 0] = torch.from_numpy(mt.view(np.int32)).to(dev)
        del mt
        bt_out = torch.empty_like(bt_in)
        bplan = B.AdditiveNTT(B.AdditiveNTTConf(a.c5_log_n, 0, B.FanPaarTowerField(7), device=local))
        if a.variant is not None:
            bplan.set_variant(a.variant)

        def run_batch():
            if mine:
                bplan.forward_device(bt_in, bt_out, batch=mine, stream=stream)

        run_batch()
        torch.cuda.synchronize(dev)
        dtb = timed(run_batch, a.c5_steps) / a.c5_steps
        c5_check = limb0_check(bt_out[:4 * nb], a.c5_log_n) if mine else None
        c5["batched_ntt"] = {
            "workload": "%d x 2^%d-point GF(2^128) additive NTT, %d per rank (rank-contiguous slices, no collective)"
                        % (a.c5_batch, a.c5_log_n, -(-a.c5_batch // world)),
            "ms": dtb * 1e3, "elements_per_s": a.c5_batch * nb / dtb,
            "per_gpu_hbm_frac": (-(-a.c5_batch // world)) * 32 * nb / dtb / 1e9 / HBM_PEAK_GBPS,
            "scaling": "strong", "steps": a.c5_steps,
            "output_check": dict(c5_check, transform="this rank's first") if c5_check else None}
        del bt_in, bt_out, bplan
        torch.cuda.empty_cache()

        # ---------------- config 5: 2^28-eval d=3 sumcheck, sharded by 32-element batch
        try:
            c5["sumcheck"] = c5_sumcheck(a, B, D, torch, dev, local, rank, world, backend, barrier, max_over_ranks)
        except Exception as e:  # the headline line is still printed; the failure is in the record
            c5["sumcheck"] = {"error": "%s: %s" % (type(e).__name__, e)}
            print("bench.py: c5 sumcheck leg failed: %r" % (e,), file=sys.stderr)
        torch.cuda.empty_cache()

    configs = None
    if world == 1 and not a.no_configs:
        configs = configs_leg(dev)

    if rank == 0:
        res["c5"] = c5
        res["configs"] = configs
        if world == 1:
            res["apply_e2e"] = apply_e2e(B, ntt, n)
        res["cpu_baseline"] = cpu_baseline() if (not a.no_cpu and world == 1) else None
        json_out.write(json.dumps(res) + "\n")
        json_out.flush()
    if world > 1:
        dist.destroy_process_group()


def configs_leg(dev):
    """BASELINE.json configs 2-4 on this GPU (lines as tools/bench_configs.py prints them), each
    with its roofline fraction: algorithmic HBM bytes for the NTT and the sumcheck."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_configs as C
    lines = []
    C.c2(dev, lines.append)
    C.ntt_line(dev, lines.append, "c3", 20, 1)
    C.c4(dev, lines.append, 24, [3])
    # the reference harness's matrix (bench/benchmark.cu:71-85): N = 20 for d = 2..4, N = 24 and
    # N = 28 at d = 3 (12.9 GB of columns at N = 28: one timed run)
    for d in (2, 3, 4):
        C.c4_phases(dev, lines.append, 20, d)
    C.c4_phases(dev, lines.append, 24, 3)
    C.c4_phases(dev, lines.append, 28, 3, runs=1)
    # config 2 is VALU-bound (register-resident operands, no HBM traffic): its roofline is the
    # VALU issue peak, with the wave-instruction count per launch of the line's own kernel from the
    # committed PMC pass (PMC_FILE, matched by kernel name and library hash)
    for ln in lines:
        if "hbm_gbps_algorithmic" in ln:
            ln["hbm_frac_algorithmic"] = ln["hbm_gbps_algorithmic"] / HBM_PEAK_GBPS
        if ln.get("config") == "c2" and ln.get("kernel"):
            ctr, why = kernel_counters(ln["kernel"])
            insts = ctr.get("SQ_INSTS_VALU") if ctr else None
            if insts:
                rate = insts / (ln["ms"] * 1e-3)
                ln["valu"] = {"kernel": ln["kernel"], "insts_per_launch": insts, "frac": rate / VALU_PEAK_WAVE_INSTS,
                              "lane_insts_per_product": insts * 64 / (ln["value"] * ln["ms"] * 1e-3),
                              "source": PMC_FILE + " (library SHA-256 checked)"}
            else:
                ln["valu"] = {"kernel": ln["kernel"], "insts_per_launch": None, "note": why}
    return lines


def apply_e2e(B, ntt, n, reps=3):
    """Reference-semantics AdditiveNTT::apply (host buffers: H2D + transform + D2H, synchronous);
    reported beside `value`, never as it."""
    import numpy as np
    host = np.random.default_rng(7).integers(0, 2**32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    inp = B.NTTData(n, B.DataOrder.IN_ORDER, 128, host)
    out = B.NTTData(n, B.DataOrder.INVALID, 128)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        if not ntt.apply(inp, out):
            return None
        ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    return {"ms": t * 1e3, "elements_per_s": n / t, "reps": reps,
            "note": "AdditiveNTT.apply on pageable host buffers (PCIe-inclusive), median"}


if __name__ == "__main__":
    main()
