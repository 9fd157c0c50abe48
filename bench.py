#!/usr/bin/env python
"""Benchmark: KZG batch verification (BLS12-381, n = 2^20 tuples per GPU) on MI355X.

Metric (BASELINE.json:2): batch-verifies/sec + G1 MSM pts/sec at n=2^20, BLS12-381, 1/2/4/8 GPU.
`value` = batch-verifies/s where one batch = n tuples (default 2^20) per GPU; at N GPUs each
step verifies one global batch of N*n tuples sharded by point range (weak scaling), so
value = N*K / elapsed.  A "step" = one complete verification: input decoding, randomisers,
both G1 MSMs, the two-pairing check and the verdict back on the host.  Inputs are generated
on the device (valid toy-tau openings) and resident in HBM before the timed region.

Single GPU: steps are issued round-robin over `--slots` independent workspaces/streams, so
the latency-bound tail of one batch (bucket reduction, window combination, pairing) runs
beside the bucket accumulation of the next.  Every verdict is checked (must be True).
N GPUs: each rank computes its partial (A_k, B_k) over its shard, partials are all-gathered
over RCCL (torch.distributed 'nccl' backend) and every rank runs the pairing check; each rank
keeps `--slots` global batches in flight (kzgmi.distributed.ShardedPipeline).

Prints ONE JSON line on rank 0.  A plain run does only what the headline needs: set-up,
`--warmup` steps, `--steps` timed steps, the line.  `--full` adds every other leg (repeats, latencies, the other configs, MSM rates, the CPU verifiers, the
default-queue child run) and with them `roofline` for the dominant kernel (bucket
accumulation), `cpu_baseline` (the C oracle, timed on a bounded sample on this host's cores),
`secondary` and `headline`.

`--dump-outputs DIR` writes what the last timed step returned to its caller as DIR/<name>.npy
(float32): `verdict` (1 = batch accepted) and, on the unsharded path, `combination_A` /
`combination_B`, the bytes of the two combined G1 points the pairing check consumed.  Inputs
and randomisers are seeded, so two builds run with the same arguments must agree byte for byte.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "kzg-batch-verification-scheme_amd"))


def _launch_ranks():
    """`--gpus N` (N > 1) started directly, not by torchrun: run N rank processes of this script
    (kzgmi/launch.py) and exit with the job's status -- before anything here touches the GPU."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--gpus", type=int, default=1)
    a, _ = pre.parse_known_args()
    from kzgmi.launch import maybe_launch
    return maybe_launch([os.path.abspath(__file__)] + sys.argv[1:], a.gpus)


if __name__ == "__main__":
    _rc = _launch_ranks()
    if _rc is not None:
        sys.exit(_rc)

# HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues per stream priority (4 by
# default).  The slot pipeline needs about one queue per batch in flight -- batches whose streams
# share a queue serialise.  At HIP's default the library spreads its slot streams over the stream
# priorities (csrc/api.hip kzgmi_ctx_create_device) and reaches 0.96 of the 24-queue rate at 2^20
# (profiles/r05/ab_stream_prio.txt); the headline sets 24 queues, and secondary.default_hw_queues
# reports the same measurement at the default (a child process: the queue count is read when the
# HIP runtime initialises, so it is set here before torch touches the GPU).
os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("KZGMI_HW_QUEUES", "24")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import kzgmi  # noqa: E402
from kzgmi.distributed import ShardedMsmPipeline, ShardedPipeline  # noqa: E402

METRIC = "batch-verifies/sec + G1 MSM pts/sec at n=2^20, BLS12-381; 1/2/4/8 GPU"
HBM_PEAK = 8.0e12          # B/s, MI355X spec (MI355X_MICROARCH.md)
TAU = 0x2A1B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081
BYTES_PER_TUPLE = {"bls12_381": 256, "bn254": 192}
BYTES_PER_MSM_POINT = {"bls12_381": 128, "bn254": 96}
VALU_PER_ADD = 4528  # BLS12-381 k_accumulate, SQ_INSTS_VALU x 64 / 32n (profiles/r06/pmc_sq_accumulate.json)
PROFILE_ROUND = "r06"      # profiles/<round>/rocprof_single: the committed rocprofv3 summaries


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def gen_inputs(ctx, curve, n, seed, tau=None):
    g1b = 2 * kzgmi.FP_BYTES[curve]
    C = torch.empty(n * g1b, dtype=torch.uint8, device="cuda")
    P = torch.empty(n * g1b, dtype=torch.uint8, device="cuda")
    z = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    y = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    ctx.gen_tuples(curve, TAU if tau is None else tau, seed, n, C, z, y, P)
    return C, z, y, P


def pipelined_rate(ctx, slots, steps, submit, sync=None):
    """Batches per second of `steps` calls submit(slot) issued round-robin over `slots` slots (each
    slot's previous verdict collected -- and asserted -- before it is reused), after one warm-up
    pass over every slot; synchronize + host clock on both sides of the timed loop."""
    import torch
    pend = [False] * slots

    def go(count):
        for k in range(count):
            s = k % slots
            if pend[s]:
                assert ctx.wait(s), "batch rejected"
            submit(s)
            pend[s] = True
        for s in range(slots):
            if pend[s]:
                assert ctx.wait(s), "batch rejected"
                pend[s] = False

    go(min(slots, steps))
    (sync or torch.cuda.synchronize)()
    a = time.perf_counter()
    go(steps)
    (sync or torch.cuda.synchronize)()
    return steps / (time.perf_counter() - a)


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def _cpuset_count(spec):
    """Number of CPUs in a cpuset list such as '0-15,32-47'."""
    n = 0
    for part in (spec or "").split(","):
        part = part.strip()
        if not part:
            continue
        a, _, b = part.partition("-")
        n += (int(b) - int(a) + 1) if b else 1
    return n


def cpu_grant():
    """CPUs this process may really use, and what limits it: the affinity mask, the cgroup v2
    CPU quota (/sys/fs/cgroup/cpu.max = "quota period" or "max period"), the cgroup cpuset, and an
    explicit OMP_NUM_THREADS (the GPU box exports 16 = its per-GPU CPU share)."""
    try:
        affinity = len(os.sched_getaffinity(0))
    except Exception:
        affinity = os.cpu_count() or 1
    limits = {"sched_getaffinity": affinity}
    cpu_max = _read("/sys/fs/cgroup/cpu.max")
    quota = None
    if cpu_max:
        q, _, per = cpu_max.partition(" ")
        if q != "max" and per:
            quota = -(-int(q) // int(per))  # ceil: CPUs' worth of time per period
            limits["cgroup_cpu_max"] = quota
    cpuset = _read("/sys/fs/cgroup/cpuset.cpus.effective")
    if cpuset:
        limits["cgroup_cpuset"] = _cpuset_count(cpuset)
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp and omp.isdigit() and int(omp) > 0:
        limits["OMP_NUM_THREADS"] = int(omp)
    n = min(limits.values())
    binding = [k for k, v in limits.items() if v == n]
    info = {"nproc": os.cpu_count(), "sched_getaffinity": affinity, "cgroup_cpu_max_raw": cpu_max,
            "cgroup_quota_cpus": quota, "cgroup_cpuset_effective": cpuset, "OMP_NUM_THREADS": omp,
            "threads_used": max(1, n), "limited_by": binding,
            "grant": "%d of %d host CPUs (%s)" % (max(1, n), os.cpu_count() or 0, ", ".join(binding))}
    return max(1, n), info


def host_info():
    model = ""
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True).stdout
        for line in out.splitlines():
            if line.startswith("Model name"):
                model = line.split(":", 1)[1].strip()
    except Exception:
        pass
    _, grant = cpu_grant()
    return dict(grant, lscpu_model=model)


def cpu_baseline(curve, Cm, z, y, P, n_full, seed, target_s):
    """Time the CPU verifiers (OpenMP over this process's CPU grant) on the same tuples: the
    whole batch when it fits the time budget (no extrapolation), else the largest power-of-two
    prefix that does.  Two verifiers, both self-authored test infrastructure in oracle/:
      - "tuned" (the value): signed-window Pippenger with XYZZ buckets, fused MSMs and a
        mulx/adcx/adox Montgomery product (oracle/c/pippenger_tuned_tmpl.h), at the best of a
        few window widths -- the competent CPU verifier the GPU rate is quoted against;
      - "oracle": the plain correctness oracle (unsigned windows, Jacobian buckets).
    Plus a single-core tuned sample and configs[0] (n = 256) on both."""
    from oracle import oracle as O  # cpu_baseline leg only
    g1b = 2 * kzgmi.FP_BYTES[curve]
    threads, grant = cpu_grant()
    O.set_threads(threads)
    threads = O.threads()
    tg2_bytes = cpu_baseline.tg2
    g2 = kzgmi.G2_GENERATOR[curve]
    host = {}

    def host_bytes(m):
        if m not in host:
            host.clear()
            host[m] = [t[: m * w].cpu().numpy().tobytes() for t, w in ((Cm, g1b), (z, 32), (y, 32), (P, g1b))]
        return host[m]

    def run(m, tuned_c=None):
        hb = host_bytes(m)
        t0 = time.perf_counter()
        if tuned_c:  # -1: the verifier's own width for m
            ok, _, _ = O.batch_verify_tuned(curve, hb[0], hb[1], hb[2], hb[3], m, g2, tg2_bytes, seed,
                                            wbits=max(0, tuned_c))
        else:
            ok = O.batch_verify(curve, hb[0], hb[1], hb[2], hb[3], m, g2, tg2_bytes, seed)
        dt = time.perf_counter() - t0
        assert ok, "CPU verifier rejected a valid batch"
        return dt

    def sized_run(budget_s, tuned_c=None, m0=4096):
        # time = constant (pairing) + slope x m: two sample sizes give both
        m0 = max(1, min(m0, n_full // 4))
        dt0, dt1 = run(m0, tuned_c), run(4 * m0, tuned_c)
        slope = max(dt1 - dt0, 1e-9) / (3 * m0)
        m = 4 * m0
        while m * 2 <= n_full and dt1 + slope * (2 * m - 4 * m0) <= budget_s:
            m *= 2
        return m, (run(m, tuned_c) if m != 4 * m0 else dt1)

    def rate(m, dt):
        return 1.0 / dt if m == n_full else (m / dt) / n_full

    # tuned verifier: window width swept on the sample, best kept
    sweep = {}
    m_t = None
    for c in (13, 14, 16):
        m_c, dt_c = sized_run(target_s / 3, tuned_c=c)
        if m_t is None or m_c == m_t:
            m_t = m_c
            sweep[c] = dt_c
    best_c = min(sweep, key=sweep.get)
    dt_t = sweep[best_c]
    # the plain oracle (round 1-3's baseline) on its own sample
    m_o, dt_o = sized_run(target_s)
    # configs[0] (BASELINE.json:7): a 256-tuple batch, median of 5, both verifiers (the tuned one
    # with its window width for n = 256; its time there is the oracle's unoptimised pairing check)
    cfg0 = sorted(run(256, -1) for _ in range(5))
    cfg0_o = sorted(run(256) for _ in range(5))
    # single-core figure (SURVEY.md 8d "also record the single-core time"), tuned verifier
    O.set_threads(1)
    try:
        m1, dt1 = sized_run(min(target_s, 6.0), tuned_c=best_c)
    finally:
        O.set_threads(threads)
    whole = m_t == n_full
    return {
        "value": rate(m_t, dt_t),
        "unit": "batch-verifies/s of n=%d tuples%s" % (n_full, "" if whole else " (linear extrapolation from the sample)"),
        "cores": threads,
        "kind": "port",
        "sample": "tuned CPU verifier (oracle/c/pippenger_tuned_tmpl.h: signed %d-bit windows, XYZZ buckets, fused "
                  "MSMs, mulx/adcx/adox Montgomery products, OpenMP tasks) on %s of the %d tuples, %.2f s on %d "
                  "threads = %s; self-authored -- the reference has no CPU verifier"
                  % (best_c, "all" if whole else "the first %d" % m_t, n_full, dt_t, threads, grant["grant"]),
        "sample_tuples": m_t,
        "sample_seconds": dt_t,
        "sample_tuples_per_s": m_t / dt_t,
        "window_bits": best_c,
        "window_sweep_seconds": {str(c): v for c, v in sweep.items()},
        "oracle": {"value": rate(m_o, dt_o), "sample_tuples": m_o, "seconds": dt_o, "tuples_per_s": m_o / dt_o,
                   "note": "the unoptimised correctness oracle (unsigned-window Jacobian Pippenger, affine Miller "
                           "loop, plain-pow final exponentiation): rounds 1-3's cpu_baseline"},
        "single_core": {"value": (m1 / dt1) / n_full, "sample_tuples": m1, "seconds": dt1,
                        "tuples_per_s": m1 / dt1, "verifier": "tuned"},
        # the grant is 16 of the host's threads; the single-core rate x every
        # hardware thread of the host is what an unconstrained CPU verifier could at best reach
        # (linear scaling assumed: an extrapolation, labelled as such, not a measurement)
        "full_host_extrapolated": {"value": (m1 / dt1) / n_full * (os.cpu_count() or 1),
                                   "threads": os.cpu_count() or 1,
                                   "note": "EXTRAPOLATION: single-core tuned rate x os.cpu_count() host threads"},
        "cfg0_cpu_n256_ms": 1e3 * cfg0[len(cfg0) // 2],
        "cfg0_cpu_n256_runs_ms": [1e3 * t for t in cfg0],
        "cfg0_cpu_n256_ms_oracle": 1e3 * cfg0_o[len(cfg0_o) // 2],
    }


def _ensure_world1_pg(local):
    """A world-1 RCCL process group for the single-GPU run's sharded-path legs (the per-rank
    work of the N-GPU runs through the real collectives), created once and kept to the end of
    the run (one communicator, one set of RCCL streams); True if this call created it."""
    if dist.is_initialized():
        return False
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", local))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary leg (all the *-steps options below, the CPU baseline, the "
                         "roofline, the detail file); without it only the headline's warm-up and timed steps run")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned (verdict, combined points) as DIR/<name>.npy")
    ap.add_argument("--n", type=int, default=1 << 20, help="tuples per GPU")
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--slots", type=int, default=0,
                    help="batches in flight per GPU (default 16; sharded runs chain each combine on its slot)")
    ap.add_argument("--msm-steps", type=int, default=96,
                    help="configs[1]: pipelined 2^20 MSMs timed (the drain of the last in-flight MSMs is "
                         "inside the region: 24 steps read 356-358 M pts/s, 96 steps 372-374, tools/ab.py --key msm_pts_per_s; 0 = skip)")
    ap.add_argument("--trusted-steps", type=int, default=96,
                    help="secondary: pipelined batches with KZGMI_FLAG_TRUSTED_G1 (GLV on BLS12-381; 0 = skip)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0,
                    help="time budget of each multi-threaded CPU-baseline sample (whole batch if it fits)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--fs-steps", type=int, default=96,
                    help="secondary: pipelined batches in Fiat-Shamir mode (r_i = r^i, 0 = skip)")
    ap.add_argument("--commit-steps", type=int, default=24,
                    help="secondary: fixed-base prover commits of n coefficients (0 = skip)")
    ap.add_argument("--compressed-steps", type=int, default=36,
                    help="secondary: pipelined batches with compressed inputs + subgroup checks (0 = skip)")
    ap.add_argument("--cfg4-msms", type=int, default=6,
                    help="configs[3]: G1 MSMs of --cfg4-n points split over the ranks (strong scaling; 0 = skip)")
    ap.add_argument("--cfg4-n", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=10,
                    help="timed regions in a row (value = the first; their median in secondary)")
    ap.add_argument("--sharded", action="store_true",
                    help="run the multi-GPU pipeline (RCCL all-gather per batch) even at world size 1")
    ap.add_argument("--h2d-steps", type=int, default=48,
                    help="secondary.h2d_inclusive: pipelined batches from host buffers (pinned; the pageable "
                         "form runs half as many; 0 = skip)")
    ap.add_argument("--bn254-steps", type=int, default=48,
                    help="secondary.bn254_cfg4: pipelined BN254 batches at configs[4]'s per-GPU shard (2^19) "
                         "and a third as many at 2^22 (0 = skip)")
    ap.add_argument("--shard17-steps", type=int, default=240,
                    help="secondary.sharded_2e17_world1: 2^17-tuple batches (configs[2]'s 8-way per-rank share) "
                         "through ShardedPipeline + RCCL at world 1, and unsharded (0 = skip)")
    ap.add_argument("--default-queues-steps", type=int, default=60,
                    help="secondary.default_hw_queues: the configs[2] timed region again in a child process at HIP's "
                         "default GPU_MAX_HW_QUEUES = 4 (0 = skip)")
    ap.add_argument("--detail-file", default="gpurun_out/bench_detail.json",
                    help="where the full record goes (the printed line is the compact form; '' = nowhere)")
    ap.add_argument("--strong-steps", type=int, default=0,
                    help="sharded runs: batches of the strong-scaled leg (one --n batch split over the ranks; "
                         "default = --steps)")
    args = ap.parse_args()
    full = args.full

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log("warning: WORLD_SIZE=%d but --gpus=%d; using WORLD_SIZE" % (world, args.gpus))
    if os.environ.get("KZGMI_DIST_BACKEND", "nccl") != "nccl":  # rehearsal: ranks share the GPUs
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    sharded = world > 1 or args.sharded
    if sharded:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        # KZGMI_DIST_BACKEND=gloo: rehearsal of the N>1 orchestration with several ranks on
        # one GPU (RCCL refuses two ranks on one device); the driver's N>1 runs use RCCL
        backend = os.environ.get("KZGMI_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    curve, n = args.curve, args.n
    # 16 slots on 24 hardware queues (profiles/r01/prio_sweep.txt, r02/slots_sweep.txt).  Sharded
    # runs use the eager ShardedPipeline schedule (combine chained on each partial's slot, no
    # extra lanes): at world 1 over RCCL, 2^17-tuple shards run 968/s on 16 slots vs 832/s on 8
    # and 851/s with round 3's deferred 8 slots + 2 lanes (profiles/r04/bench_s1_legs_serial_h2d.json)
    slots = args.slots if args.slots else int(os.environ.get("KZGMI_BENCH_SLOTS", "16"))  # (A/B knob)
    lanes = 0  # the eager ShardedPipeline schedule chains each combine on its partial's slot
    ctx = kzgmi.Context(local, slots + lanes)  # + the combine lanes
    g2 = kzgmi.G2_GENERATOR[curve]
    tg2 = ctx.g2_mul(curve, g2, TAU)
    cpu_baseline.tg2 = tg2
    srs = ctx.load_srs(curve, g2, tg2)
    # every slot's workspace sized up front (kzgmi_ctx_reserve): the timed region allocates
    # nothing however few warm-up steps run (checked below with kzgmi_alloc_count)
    ctx.reserve(curve, n)
    gseed = hashlib.sha256(b"kzgmi-bench-%d" % rank).digest()
    vseed = hashlib.sha256(b"kzgmi-bench-verify").digest()
    t0 = time.perf_counter()
    Cm, z, y, P = gen_inputs(ctx, curve, n, gseed)
    torch.cuda.synchronize()
    log("[rank %d] generated %d tuples in %.2f s" % (rank, n, time.perf_counter() - t0))
    pipe = ShardedPipeline(ctx, srs, slots, lanes) if sharded else None
    # host copies of the batch (the H2D-inclusive leg and the CPU baseline)
    host_np = None

    def step_sharded():
        # every rank holds n tuples of a global batch of world*n; one RCCL all-gather per batch,
        # `slots` global batches in flight
        for ok in pipe.submit(Cm, z, y, P, n, rank * n, vseed):
            assert ok, "batch rejected"

    pending = [False] * slots
    newest = [None]  # slot of the latest step_single

    def step_single(k):
        s = k % slots
        if pending[s]:
            assert ctx.wait(s), "batch rejected"
        ctx.batch_verify_async(srs, s, Cm, z, y, P, n, seed=vseed)
        pending[s] = True
        newest[0] = s

    def drain():
        """Collect every batch in flight, each verdict asserted; returns the newest batch's verdict
        (the step before the drain ran on slot `newest`), None if nothing was in flight."""
        last = None
        if pipe is not None:
            for ok in pipe.drain():  # oldest first
                assert ok, "batch rejected"
                last = ok
            return last
        for s in range(slots):
            if pending[s]:
                ok = ctx.wait(s)
                assert ok, "batch rejected"
                pending[s] = False
                if s == newest[0]:
                    last = ok
        return last

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- warmup
    for k in range(args.warmup):
        if sharded:
            step_sharded()
        else:
            step_single(k)
    drain()
    barrier()
    # ---- timed region (phase events on the kernels' own streams)
    ctx.set_profiling(True)
    allocs0 = kzgmi.alloc_count()
    t0 = time.perf_counter()
    for k in range(args.steps):
        if sharded:
            step_sharded()
        else:
            step_single(k)
    last_verdict = drain()
    barrier()
    elapsed = time.perf_counter() - t0
    allocs_timed = kzgmi.alloc_count() - allocs0
    phases = ctx.phase_ms()
    ctx.set_profiling(False)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    value = world * args.steps / elapsed

    # ---- what the last timed step gave its caller (--dump-outputs): the verdict, and the combined
    # points (A, B) behind it.  kzgmi_last_combination reads slot 0, whose latest batch is one of
    # the timed steps; every step verifies the same tuples with the same randomisers, so that
    # pair is the last step's too.  Before any other leg, so nothing else has run on the slots.
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        dumped = {"verdict": np.array([float(bool(last_verdict))], dtype=np.float32)}
        if not sharded and args.steps > 0:
            for name, enc in zip(("combination_A", "combination_B"), ctx.last_combination(curve)):
                dumped[name] = np.frombuffer(enc, dtype=np.uint8).astype(np.float32)
        for name, arr in dumped.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)

    # ---- the same timed region repeated (median of >= 10 runs): value above is the
    # first run, as the contract asks; rep_values holds it and args.repeats - 1 more
    rep_values = [value]
    for _ in range(args.repeats - 1 if full else 0):
        barrier()
        a = time.perf_counter()
        for k in range(args.steps):
            if sharded:
                step_sharded()
            else:
                step_single(k)
        drain()
        barrier()
        dt = time.perf_counter() - a
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        rep_values.append(world * args.steps / dt)

    # ---- single-batch latency (not pipelined), rank 0 view
    lat = None
    phases_single = phases_single_split = None
    lat_runs = None
    if full and world == 1:
        ts = []
        for _ in range(10):  # median of >= 10 runs
            torch.cuda.synchronize()
            a = time.perf_counter()
            assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=n)
            ts.append(time.perf_counter() - a)
        ts.sort()
        lat = 1e3 * ts[len(ts) // 2]
        lat_runs = [1e3 * t for t in ts]
        # phases of the split accumulation these synchronous calls take (api.hip run_msm_core: the
        # marks follow the critical path), then of the single-launch form the pipeline runs -- the
        # dominant kernel the roofline prices
        ctx.set_profiling(True)
        for _ in range(6):  # phase means over 6 batches (2 read up to ~3 % apart run to run)
            assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=n)
        phases_single_split = ctx.phase_ms()
        ctx.set_split_acc(0)
        ctx.set_profiling(True)
        for _ in range(6):
            assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=n)
        phases_single = ctx.phase_ms()
        ctx.set_profiling(False)
        ctx.set_split_acc(-1)

    # ---- configs[0] (BASELINE.json:7): a 256-tuple batch (the CPU verifier's time is added by
    # cpu_baseline below); GPU latency of the same batch, median of 10 synchronous calls
    cfg0 = None
    if full and world == 1 and not sharded and n >= 256:
        ts = []
        for _ in range(10):
            torch.cuda.synchronize()
            a = time.perf_counter()
            assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=256)
            ts.append(time.perf_counter() - a)
        ts.sort()
        cfg0 = {"n": 256, "curve": curve, "gpu_latency_ms": 1e3 * ts[len(ts) // 2],
                "gpu_latency_runs_ms": [1e3 * t for t in ts],
                "note": "first 256 of the generated tuples; GPU: one synchronous kzgmi_batch_verify_device "
                        "(latency-bound: pairing + per-batch fixed costs); CPU: oracle/c batch_verify"}

    # ---- strong scaling (configs[2] as one batch over all ranks): ONE global batch of n tuples
    # split n/world per rank (shard_range), `slots` global batches in flight -- the per-rank
    # fixed costs (bucket reduction, window combination, pairing) do not shrink with the shard
    strong = None
    if full and sharded:
        from kzgmi.distributed import shard_range
        off_s, n_s = shard_range(n, world, rank)
        g1b = 2 * kzgmi.FP_BYTES[curve]
        views = (Cm[: n_s * g1b], z[: n_s * 32], y[: n_s * 32], P[: n_s * g1b])
        ssteps = args.strong_steps or args.steps

        def step_strong():
            for ok in pipe.submit(*views, n_s, off_s, vseed):
                assert ok, "batch rejected"

        for _ in range(min(slots, ssteps)):
            step_strong()
        drain()
        barrier()
        ctx.set_profiling(True)
        a = time.perf_counter()
        for _ in range(ssteps):
            step_strong()
        drain()
        barrier()
        dts = time.perf_counter() - a
        sph = ctx.phase_ms()
        ctx.set_profiling(False)
        if world > 1:
            t = torch.tensor([dts], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dts = float(t.item())
        strong = {"batch_verifies_per_s": ssteps / dts, "ms_per_batch": 1e3 * dts / ssteps, "steps": ssteps,
                  "n_total": n, "n_per_rank": n_s, "world": world, "scaling": "strong",
                  "phase_ms_avg_in_timed_region": sph,
                  "method": "one n-tuple batch split by point range (kzgmi.distributed.shard_range), partial "
                            "(A_k, B_k) per rank, RCCL all-gather, combine + pairing on every rank; %d batches "
                            "in flight" % slots}

    # ---- secondary: compressed inputs + subgroup checks, single GPU
    comp = None
    if full and world == 1 and not sharded and args.compressed_steps > 0:
        fb = kzgmi.FP_BYTES[curve]
        cc = torch.empty(n * fb, dtype=torch.uint8, device="cuda")
        pp = torch.empty(n * fb, dtype=torch.uint8, device="cuda")
        ctx.g1_compress(curve, Cm, n, cc)
        ctx.g1_compress(curve, P, n, pp)

        def cstep(k):
            s = k % slots
            if pending[s]:
                assert ctx.wait(s), "batch rejected"
            ctx.batch_verify_async(srs, s, cc, z, y, pp, n, seed=vseed, compressed=True, subgroup_check=True)
            pending[s] = True

        ctx.reserve(curve, n, compressed=True, subgroup_check=True)
        for k in range(min(slots, args.compressed_steps)):  # warm every slot's workspace (GLV sizes)
            cstep(k)
        drain()
        barrier()
        ctx.set_profiling(True)
        a = time.perf_counter()
        for k in range(args.compressed_steps):
            cstep(k)
        drain()
        barrier()
        dt = time.perf_counter() - a
        cph = ctx.phase_ms()
        ctx.set_profiling(False)
        ctx.set_profiling(True)
        assert ctx.batch_verify(srs, cc, z, y, pp, seed=vseed, n=n, compressed=True, subgroup_check=True)
        single = ctx.phase_ms()
        ctx.set_profiling(False)
        comp = {"batch_verifies_per_s": args.compressed_steps / dt, "steps": args.compressed_steps,
                "input": "48 B compressed C and pi, decompressed + subgroup-checked on the GPU",
                "phase_ms_single_batch": single, "phase_ms_avg_in_timed_region": cph}
        del cc, pp

    # ---- secondary: inputs declared G1 members (KZGMI_FLAG_TRUSTED_G1): the GLV split of s_i, t
    #  becomes exact on BLS12-381 and is used; single GPU
    trusted = None
    if full and world == 1 and not sharded and args.trusted_steps > 0:
        def tstep(k):
            s = k % slots
            if pending[s]:
                assert ctx.wait(s), "batch rejected"
            ctx.batch_verify_async(srs, s, Cm, z, y, P, n, seed=vseed, trusted_g1=True)
            pending[s] = True

        ctx.reserve(curve, n, trusted_g1=True)
        for k in range(min(slots, args.trusted_steps)):
            tstep(k)
        drain()
        barrier()
        a = time.perf_counter()
        for k in range(args.trusted_steps):
            tstep(k)
        drain()
        barrier()
        dt = time.perf_counter() - a
        ctx.set_profiling(True)
        assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=n, trusted_g1=True)
        trusted = {"batch_verifies_per_s": args.trusted_steps / dt, "steps": args.trusted_steps,
                   "flags": "KZGMI_FLAG_TRUSTED_G1 (caller guarantees G1 membership; enables GLV)",
                   "phase_ms_single_batch": ctx.phase_ms()}
        ctx.set_profiling(False)

    # ---- secondary: Fiat-Shamir randomisers, single GPU
    fsm = None
    if full and world == 1 and not sharded and args.fs_steps > 0:
        def fstep(k):
            s = k % slots
            if pending[s]:
                assert ctx.wait(s), "batch rejected"
            ctx.batch_verify_async(srs, s, Cm, z, y, P, n, fiat_shamir=True)
            pending[s] = True

        ctx.reserve(curve, n, fiat_shamir=True)
        for k in range(min(slots, args.fs_steps)):  # warm every slot's workspace
            fstep(k)
        drain()
        barrier()
        a = time.perf_counter()
        for k in range(args.fs_steps):
            fstep(k)
        drain()
        barrier()
        dt = time.perf_counter() - a
        ctx.set_profiling(True)
        assert ctx.batch_verify(srs, Cm, z, y, P, n=n, fiat_shamir=True)
        fsm = {"batch_verifies_per_s": args.fs_steps / dt, "steps": args.fs_steps,
               "randomisers": "counter-mode 127-bit r_i seeded with the Fiat-Shamir challenge r (GPU Merkle "
                              "transcript of the batch, KZGMI_FLAG_FIAT_SHAMIR)",
               "phase_ms_single_batch": ctx.phase_ms()}
        ctx.set_profiling(False)

    # ---- secondary: prover-side fixed-base commit, single GPU,
    # pipelined over the slots like the batches (kzgmi_commit_device_async)
    commit = None
    if full and world == 1 and not sharded and args.commit_steps > 0:
        a = time.perf_counter()
        ck = ctx.load_commit_key(curve, Cm.cpu().numpy().tobytes(), n)  # n points as a stand-in SRS
        load_s = time.perf_counter() - a
        ref = ctx.commit(ck, z, n)
        torch.cuda.synchronize()
        a = time.perf_counter()
        assert ctx.commit(ck, z, n) == ref
        commit_latency_ms = (time.perf_counter() - a) * 1e3
        got = []
        for k in range(min(slots, args.commit_steps)):  # warm every slot's workspace
            ctx.commit_async(ck, k, z, n)
        for k in range(min(slots, args.commit_steps)):
            got.append(ctx.msm_wait(k))
        barrier()
        a = time.perf_counter()
        for k in range(args.commit_steps):
            sl = k % slots
            if k >= slots:
                got.append(ctx.msm_wait(sl))
            ctx.commit_async(ck, sl, z, n)
        for i in range(min(args.commit_steps, slots)):
            k = max(0, args.commit_steps - slots) + i
            got.append(ctx.msm_wait(k % slots))
        barrier()
        dt = time.perf_counter() - a
        assert all(g == ref for g in got), "pipelined commitment differs"
        commit = {"commits_per_s": args.commit_steps / dt, "pts_per_s": n * args.commit_steps / dt,
                  "single_latency_ms": commit_latency_ms, "key_load_s": load_s, "n": n,
                  "method": "16 resident rows of 2^(16w)-shifted SRS points, one bucket set, "
                            "pipelined over the slots"}
        del ck

    # ---- secondary: the literal drop-in path -- batch_verify from HOST buffers (SURVEY.md 8d
    # "secondary: includes the H2D copy"; kzgmi_batch_verify_ex_async), pipelined over the slots:
    # the H2D DMA of one batch runs beside the kernels of the others.  Pinned host memory
    # (kzgmi_host_alloc) is DMA'd directly; pageable numpy arrays go through the slots' pinned
    # staging rings (host copy by the library's copy pool).
    h2d = None
    if full and world == 1 and not sharded and args.h2d_steps > 0:
        g1b = 2 * kzgmi.FP_BYTES[curve]
        host_np = [t.cpu().numpy() for t in (Cm, z, y, P)]
        batch_bytes = sum(a.nbytes for a in host_np)
        pinned = kzgmi.HostBuffer(batch_bytes)
        views, off = [], 0
        for a_ in host_np:
            v = pinned.view(off, a_.nbytes)
            v[:] = a_
            views.append(v)
            off += a_.nbytes
        # PCIe probe: one batch's bytes pinned -> HBM in one copy (torch, its own stream), median of 5
        hp = torch.empty(batch_bytes, dtype=torch.uint8, pin_memory=True)
        dp = torch.empty(batch_bytes, dtype=torch.uint8, device="cuda")
        cts = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dp.copy_(hp, non_blocking=True)
            e1.record()
            e1.synchronize()
            cts.append(e0.elapsed_time(e1))
        copy_ms = statistics.median(cts[1:])
        del hp, dp
        ctx.set_profiling(True)
        rate_pinned = pipelined_rate(ctx, slots, args.h2d_steps,
                                     lambda s_: ctx.batch_verify_host_async(srs, s_, *views, seed=vseed))
        ph_pipe_pin = ctx.phase_ms()
        ctx.set_profiling(False)
        rate_pageable = pipelined_rate(ctx, slots, max(1, args.h2d_steps // 2),
                                       lambda s_: ctx.batch_verify_host_async(srs, s_, *host_np, seed=vseed))
        # one synchronous host-buffer batch per kind, phases on the slot's stream (h2d = the copy)
        ctx.set_profiling(True)
        assert ctx.batch_verify(srs, *views, seed=vseed)
        ph_pin = ctx.phase_ms()
        ctx.set_profiling(False)
        ctx.set_profiling(True)
        a = time.perf_counter()
        assert ctx.batch_verify(srs, *host_np, seed=vseed)
        lat_pageable = 1e3 * (time.perf_counter() - a)
        ph_page = ctx.phase_ms()
        ctx.set_profiling(False)
        kernel_step_ms = 1e3 * elapsed / args.steps
        bound_ms = max(copy_ms, kernel_step_ms)
        h2d = {
            "batch_verifies_per_s_pinned": rate_pinned,
            "batch_verifies_per_s_pageable": rate_pageable,
            "steps_pinned": args.h2d_steps, "steps_pageable": max(1, args.h2d_steps // 2),
            "bytes_per_batch": batch_bytes,
            "pcie_h2d_GBps": batch_bytes / (copy_ms * 1e-3) / 1e9,
            "pcie_probe": "one %d-B pinned -> HBM copy (torch non_blocking copy, HIP events), median of 5" % batch_bytes,
            "copy_ms_per_batch_probe": copy_ms,
            "h2d_ms_single_batch_pinned": ph_pin.get("h2d"),
            "phase_ms_avg_in_timed_region_pinned": ph_pipe_pin,
            "h2d_ms_single_batch_pageable": ph_page.get("h2d"),
            "single_batch_latency_ms_pageable": lat_pageable,
            "kernel_ms_per_step_hbm_resident": kernel_step_ms,
            "bound_ms_per_batch": bound_ms,
            "bound_batch_verifies_per_s": 1e3 / bound_ms,
            "frac_of_bound_pinned": rate_pinned * bound_ms / 1e3,
            "bound_note": "pipelined host-buffer batches can run no faster than max(PCIe copy of one batch, the "
                          "HBM-resident pipelined step): the copy engine and the CUs overlap across slots",
            "method": "kzgmi_batch_verify_ex_async over %d slots (pinned: kzgmi_host_alloc block, DMA on the slot's "
                      "stream; pageable: numpy arrays staged through each slot's pinned ring by the library's copy "
                      "pool, %s threads), every verdict asserted" % (slots, os.environ.get("KZGMI_COPY_THREADS", "8")),
        }
        pinned.free()

    # ---- secondary: configs[2] split 8 ways -- 2^17-tuple batches at world 1 through the real
    # multi-GPU path (ShardedPipeline: partial + RCCL all-gather + combine per batch) and
    # unsharded; their ratio to `value` projects the 8-GPU strong speed-up of one 2^20 batch
    shard17 = None
    if full and world == 1 and not sharded and args.shard17_steps > 0 and n >= (1 << 17):
        n17 = 1 << 17
        g1b = 2 * kzgmi.FP_BYTES[curve]
        v17 = (Cm[: n17 * g1b], z[: n17 * 32], y[: n17 * 32], P[: n17 * g1b])
        rate_unsharded = pipelined_rate(ctx, slots, args.shard17_steps,
                                        lambda s_: ctx.batch_verify_async(srs, s_, *v17, n17, seed=vseed))
        _ensure_world1_pg(local)
        res17 = {}
        for mode, (sl17, ln17) in (("eager", (16, 0)), ("eager8", (8, 0)), ("deferred", (8, 2))):
            pipe17 = ShardedPipeline(ctx, srs, sl17, ln17, eager=mode != "deferred")

            def sub17():
                for ok in pipe17.submit(*v17, n17, 0, vseed):
                    assert ok, "batch rejected"
            for _ in range(sl17):
                sub17()
            assert all(pipe17.drain())
            torch.cuda.synchronize()
            a = time.perf_counter()
            for _ in range(args.shard17_steps):
                sub17()
            assert all(pipe17.drain())
            torch.cuda.synchronize()
            res17[mode] = args.shard17_steps / (time.perf_counter() - a)
            del pipe17
        shard17 = {
            "n_per_rank": n17, "steps": args.shard17_steps,
            "batch_verifies_per_s_sharded_rccl_world1": res17["eager"],
            "batch_verifies_per_s_sharded_eager_8_slots": res17["eager8"],
            "batch_verifies_per_s_sharded_deferred": res17["deferred"],
            "batch_verifies_per_s_unsharded": rate_unsharded,
            "projected_8gpu_strong_speedup": res17["eager"] / value,
            "projection_note": "one 2^20 batch split 8 ways runs one 2^17 shard per GPU plus an all-gather of 2 "
                               "partial records per rank; per-rank rate measured here through the same RCCL path at "
                               "world 1, over this run's 2^20 value",
            "method": "kzgmi.distributed.ShardedPipeline, eager schedule on all %d slots (the all-gather and the "
                      "combine + pairing of a batch enqueued right behind its partial, ordered on the GPU by "
                      "kzgmi_slot_signal, the combine chained on the partial's slot); also eager on 8 slots and the "
                      "deferred schedule (host waits each partial; 8 slots + 2 combine lanes); unsharded: "
                      "kzgmi_batch_verify_device_async over %d slots" % (slots, slots),
        }

    # ---- secondary: configs[4] (BASELINE.json:11) on one GPU: BN254 batches at the 8-GPU run's
    # per-GPU shard (2^19 tuples) and whole (2^22), pipelined over the slots, GLV (cofactor 1)
    bn = None
    if full and world == 1 and not sharded and args.bn254_steps > 0 and curve == "bls12_381":
        bn = {}
        g2b = kzgmi.G2_GENERATOR["bn254"]
        tg2b = ctx.g2_mul("bn254", g2b, TAU % (1 << 250))
        srs_b = ctx.load_srs("bn254", g2b, tg2b)
        nb = 1 << 22
        ctx.reserve("bn254", nb)
        Cb, zb, yb, Pb = gen_inputs(ctx, "bn254", nb, hashlib.sha256(b"kzgmi-bench-bn254").digest(), TAU % (1 << 250))
        for key, nn_, st_ in (("n2e19_per_gpu_shard", 1 << 19, args.bn254_steps),
                              ("n2e22_whole", nb, max(1, args.bn254_steps // 3))):
            vb = (Cb[: nn_ * 64], zb[: nn_ * 32], yb[: nn_ * 32], Pb[: nn_ * 64])
            rate_b = pipelined_rate(ctx, slots, st_, lambda s_: ctx.batch_verify_async(srs_b, s_, *vb, nn_, seed=vseed))
            a = time.perf_counter()
            assert ctx.batch_verify(srs_b, *vb, seed=vseed, n=nn_)
            lat_b = 1e3 * (time.perf_counter() - a)
            ctx.set_split_acc(0)  # the single-launch accumulation the pipeline runs
            ctx.set_profiling(True)
            for _ in range(2):
                assert ctx.batch_verify(srs_b, *vb, seed=vseed, n=nn_)
            phb = ctx.phase_ms()
            ctx.set_profiling(False)
            ctx.set_split_acc(-1)
            # BN254's compute floor as roofline.compute.hw_floor's: 32 nn mixed
            # additions x 10 products, 162 mads per 9-limb radix-2^29 product (9 x 9 a b + 9 x 9 m p)
            n_simd_b = 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
            floor_b = 0.4596e9 * n_simd_b * 64 / 162
            acc_b = phb.get("accumulate") or 0.0
            bn[key] = {"n": nn_, "steps": st_, "batch_verifies_per_s": rate_b, "tuples_per_s": rate_b * nn_,
                       "single_batch_latency_ms": lat_b, "phase_ms_single_batch": phb,
                       "accumulate_ms": acc_b, "hw_floor_fpmul_per_s": floor_b,
                       "hw_floor_frac": (32 * nn_ * 10 / (acc_b * 1e-3)) / floor_b if acc_b > 0 else None,
                       "pipeline_hw_floor_frac": 32 * nn_ * 10 * rate_b / floor_b}
        bn["method"] = ("BN254 toy-tau tuples generated on the GPU, kzgmi_batch_verify_device_async over %d slots "
                        "(GLV split: BN254's G1 has cofactor 1)" % slots)
        bn["projected_8gpu_whole_batch_per_s"] = bn["n2e19_per_gpu_shard"]["batch_verifies_per_s"]
        del Cb, zb, yb, Pb, srs_b

    # ---- secondary: G1 MSM pts/s at n points per GPU (commitments as points, z as scalars),
    # pipelined over the same slots as the batch verifications (configs[1] throughput); once as
    # plain on-curve inputs and once declared G1 members (GLV on BLS12-381)
    def msm_run(steps):
        torch.cuda.synchronize()
        a = time.perf_counter()
        msm_ref = ctx.msm_g1(curve, Cm, z, n=n)  # synchronous: single-MSM latency + reference
        latency_ms = (time.perf_counter() - a) * 1e3
        results = []
        if world > 1:
            mpipe = ShardedMsmPipeline(ctx, curve, slots, lanes)
            submit = lambda: results.extend(mpipe.submit(Cm, z, n))  # noqa: E731
            mdrain = lambda: results.extend(mpipe.drain())  # noqa: E731
        else:
            mk = [0]

            def submit():
                sl = mk[0] % slots
                if mk[0] >= slots:
                    results.append(ctx.msm_wait(sl))
                ctx.msm_g1_async(curve, sl, Cm, z, n)
                mk[0] += 1

            def mdrain():  # oldest first; fewer than `slots` submitted -> slots 0..mk-1
                first = mk[0] % slots if mk[0] >= slots else 0
                for i in range(min(mk[0], slots)):
                    results.append(ctx.msm_wait((first + i) % slots))
                mk[0] = 0
        for _ in range(min(slots, steps)):
            submit()
        mdrain()
        barrier()
        a = time.perf_counter()
        for _ in range(steps):
            submit()
        mdrain()
        barrier()
        dt = time.perf_counter() - a
        # every pipelined result equals the synchronous one (world 1) / the first global one
        want = msm_ref if world == 1 else results[0]
        assert len(results) == steps + min(slots, steps), len(results)
        assert all(r == want for r in results), "pipelined MSM result differs"
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return world * n * steps / dt, latency_ms, msm_ref

    msm_rate = msm_latency_ms = msm_rate_t = msm_latency_t = None
    if full and args.msm_steps > 0:
        msm_rate, msm_latency_ms, ref_u = msm_run(args.msm_steps)
        ctx.set_trusted_g1(True)
        msm_rate_t, msm_latency_t, ref_t = msm_run(args.msm_steps)
        ctx.set_trusted_g1(False)
        assert ref_u == ref_t, "GLV MSM differs from the plain MSM"

    # ---- configs[3]: one G1 MSM of cfg4_n points (2^24) split by point range over the ranks
    # (strong scaling: 2^21 per rank at 8 GPUs), partial sums all-gathered over RCCL; 2 MSMs in
    # flight per rank (each slot's workspace holds ~8 GB at 2^24 points)
    cfg4 = None
    if full and args.cfg4_msms > 0 and curve == "bls12_381":
        off4, m4 = (rank * args.cfg4_n // world, (rank + 1) * args.cfg4_n // world - rank * args.cfg4_n // world)
        gen = torch.Generator(device="cuda").manual_seed(1000 + rank)
        k4 = torch.randint(0, 256, (m4, 32), dtype=torch.uint8, device="cuda", generator=gen)
        k4[:, 0] &= 0x3F                               # < 2^254 < r
        s4 = torch.randint(0, 256, (m4, 32), dtype=torch.uint8, device="cuda", generator=gen)
        s4[:, 0] &= 0x3F
        p4 = torch.empty(m4 * 2 * kzgmi.FP_BYTES[curve], dtype=torch.uint8, device="cuda")
        ctx.gen_g1(curve, k4.reshape(-1), m4, p4)
        del k4
        s4 = s4.reshape(-1)
        res4, t4 = [], []  # results and the host time each one arrived (outliers name their MSM)

        def got4(rs):
            res4.extend(rs)
            t4.extend([time.perf_counter()] * len(rs))
        if world > 1 or sharded:
            mp4 = ShardedMsmPipeline(ctx, curve, slots=2, lanes=2)
            sub4 = lambda: got4(mp4.submit(p4, s4, m4))  # noqa: E731
            drain4 = lambda: got4(mp4.drain())  # noqa: E731
        else:
            q4 = [0]

            def sub4():
                sl = q4[0] % 2
                if q4[0] >= 2:
                    got4([ctx.msm_wait(sl)])
                ctx.msm_g1_async(curve, sl, p4, s4, m4)
                q4[0] += 1

            def drain4():
                first = q4[0] % 2 if q4[0] >= 2 else 0
                for i in range(min(q4[0], 2)):
                    got4([ctx.msm_wait((first + i) % 2)])
                q4[0] = 0
        sub4()
        drain4()                                        # warm both workspaces' allocation
        sub4()
        drain4()
        barrier()
        ctx.set_profiling(True)
        n_warm4 = len(t4)
        a = time.perf_counter()
        for _ in range(args.cfg4_msms):
            sub4()
        drain4()
        barrier()
        dt4 = time.perf_counter() - a
        ph4 = ctx.phase_ms()
        ctx.set_profiling(False)
        arrivals = [a] + t4[n_warm4:]
        gaps4 = [1e3 * (arrivals[i + 1] - arrivals[i]) for i in range(len(arrivals) - 1)]
        # one MSM alone, per phase (HIP events on its stream): the reference shape for the above
        ctx.set_profiling(True)
        if world > 1 or sharded:
            got4(mp4.submit(p4, s4, m4))
            got4(mp4.drain())
        else:
            ctx.msm_g1_async(curve, 0, p4, s4, m4)
            got4([ctx.msm_wait(0)])
        ph4_single = ctx.phase_ms()
        ctx.set_profiling(False)
        if world > 1:
            t = torch.tensor([dt4], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt4 = float(t.item())
        assert len(set(res4)) == 1, "configs[3] MSM results differ between runs"
        cfg4 = {"pts_per_s": args.cfg4_n * args.cfg4_msms / dt4, "ms_per_msm": 1e3 * dt4 / args.cfg4_msms,
                "n_total": args.cfg4_n, "n_per_rank": m4, "msms": args.cfg4_msms, "world": world,
                "result_gaps_ms": gaps4, "phase_ms_avg_in_timed_region": ph4, "phase_ms_single_msm": ph4_single,
                "timing_note": "result_gaps_ms: host time between consecutive results (first from the start of "
                               "the timed region; 2 MSMs in flight); phases: HIP events on the MSM's own stream",
                "scaling": "strong", "scalars": "uniform < 2^254 (16 windows of 16 bits)",
                "method": "point-range shards, kzgmi_msm_partial_device_async + RCCL all-gather of partial "
                          "sums + kzgmi_msm_combine_device_async, 2 MSMs in flight per rank" if world > 1 or sharded
                          else "one device, kzgmi_msm_g1_device_async, 2 MSMs in flight"}
        # per-rank share of the 8-GPU run (2^24 / 8 = 2^21 points) through the real sharded path
        # (ShardedMsmPipeline: partial + RCCL all-gather + combine, eager schedule) at world 1:
        # its rate x 2^24 over the one-GPU rate above projects configs[3]'s 8-GPU strong speed-up
        if world == 1 and not sharded and args.cfg4_n >= 8:
            m8 = args.cfg4_n // 8
            _ensure_world1_pg(local)
            mp8 = ShardedMsmPipeline(ctx, curve, slots=4, lanes=0)
            r8 = []
            for _ in range(4):
                r8.extend(mp8.submit(p4[: m8 * 2 * kzgmi.FP_BYTES[curve]], s4[: 32 * m8], m8))
            r8.extend(mp8.drain())
            torch.cuda.synchronize()
            n8 = 4 * args.cfg4_msms
            a = time.perf_counter()
            for _ in range(n8):
                r8.extend(mp8.submit(p4[: m8 * 2 * kzgmi.FP_BYTES[curve]], s4[: 32 * m8], m8))
            r8.extend(mp8.drain())
            torch.cuda.synchronize()
            dt8 = time.perf_counter() - a
            assert len(set(r8)) == 1, "sharded 2^21 MSM results differ"
            del mp8
            cfg4["per_rank_share_at_8_gpus"] = {
                "n_points": m8, "msms": n8, "msms_per_s": n8 / dt8, "ms_per_msm": 1e3 * dt8 / n8,
                "projected_8gpu_pts_per_s": n8 / dt8 * args.cfg4_n,
                "projected_8gpu_strong_speedup": (n8 / dt8 * args.cfg4_n) / cfg4["pts_per_s"],
                "method": "kzgmi.distributed.ShardedMsmPipeline (eager schedule, 4 MSMs in flight) over RCCL at "
                          "world 1 on the first 2^21 points: the per-rank work of the 8-GPU configs[3] run"}
        del p4, s4

    if rank != 0:
        dist.barrier()
        dist.destroy_process_group()
        return

    out = {
        "metric": METRIC,
        "value": value,
        "unit": "batch-verifies/s (n=%d tuples per GPU per batch)" % n,
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": ("Montgomery Fp, 381-bit modular integer (radix-2^29 limbs in the bucket accumulation)"
                  if curve == "bls12_381" else "Montgomery Fp, 254-bit modular integer"),
        "data": "synthetic: valid toy-tau KZG openings generated on the GPU (kzgmi_gen_tuples), HBM-resident",
        "config": {
            "workload": "batch_verify (configs[2]): n=%d %s tuples per GPU, two G1 MSMs + 2-pairing check" % (n, curve),
            "curve": curve,
            "tuples_per_gpu": n,
            "global_batch": world * n,
            "pipeline_slots": slots,
            "parallelism": "point-range shards" + (", RCCL all_gather of partial sums" if sharded else ""),
        },
        "full": full,
    }
    if not full:
        # the plain run: the headline alone, plus what its timed region measured along the way
        out["allocs_in_timed_region"] = allocs_timed
        out["phase_ms_avg_in_timed_region"] = {k: float("%.4g" % v) for k, v in phases.items() if v}
        out["hw_queues"] = os.environ.get("GPU_MAX_HW_QUEUES")
        print(json.dumps(out), flush=True)
        if sharded:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- roofline of the dominant kernel (bucket accumulation + fixup)
    # kernel_ms: the k_accumulate + k_fixup phase of a non-pipelined batch (HIP events on the
    # kernels' own stream, measured above in this run, same inputs) -- the execution time that
    # rocprof's begin-to-end duration measures.  Inside the 12-deep pipelined region the same
    # events also count the time a launch waits for CUs held by other batches, so that figure
    # is reported separately (kernel_ms_in_pipelined_region) and the pipeline's own efficiency
    # as compute.pipeline_frac.
    acc_ms_pipe = phases.get("accumulate", 0.0)
    acc_ms = (phases_single or {}).get("accumulate") or acc_ms_pipe
    alg_bytes = n * BYTES_PER_TUPLE[curve]
    achieved = alg_bytes / (acc_ms * 1e-3) if acc_ms > 0 else None
    fpmul_peak = ctx.probe_fpmul(curve)
    # algorithmic Fp products in the accumulation: 32 n window-terms x (8M + 2S) per mixed
    # addition (the kernel shares one reduction between two of them)
    acc_fpmuls = 32 * n * 10
    # PMC traffic of the same kernel and config from the committed profile (tools/prof.sh traffic:
    # separate FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE x 2 as MI355X_MICROARCH.md prescribes)
    traffic, traffic_src, rocprof_ms, rocprof_src, gather_bytes = None, None, None, None, None
    prof_dir = os.path.join("profiles", PROFILE_ROUND, "rocprof_single")
    pmc_path = os.path.join(ROOT, prof_dir, "pmc_accumulate_single.json")
    single_path = os.path.join(ROOT, prof_dir, "kernel_single.json")
    if curve == "bls12_381" and n == 1 << 20 and os.path.exists(pmc_path):
        with open(pmc_path) as f:
            pmc = json.load(f)
        # FETCH_SIZE x 2 + WRITE_SIZE (MI355X_MICROARCH.md HBM section; calibrated on k_pts_to29,
        # profiles/r02/pmc_sq_accumulate.json)
        traffic = (2 * pmc["FETCH_SIZE_KiB_per_launch_raw"] + pmc["WRITE_SIZE_KiB_per_launch"]) * 1024
        traffic_src = "%s/pmc_accumulate_single.json (%s; 2 x FETCH_SIZE + WRITE_SIZE)" % (prof_dir, pmc["command"])
        gather_bytes = pmc.get("gather_model_bytes_per_launch")
    if curve == "bls12_381" and n == 1 << 20 and os.path.exists(single_path):
        with open(single_path) as f:
            ks = json.load(f)
        rocprof_ms = ks["accumulate_phase_avg_ms"]
        rocprof_src = "%s/kernel_single.json (%s)" % (prof_dir, ks["command"])
    # hardware-derived compute floor: the measured v_mad_u64_u32 issue rate (8 independent chains,
    # 8 waves per SIMD: 0.4596 wave-instructions per SIMD per ns, profiles/r01/probes/mad_rate.txt)
    # x SIMDs x 64 lanes / 392 mads per radix-2^29 product (14 x 14 for a b + 14 x 14 for m p)
    n_simd = 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    mad_floor = 0.4596e9 * n_simd * 64 / 392 if curve == "bls12_381" else None
    valu_floor_ms = (32 * n * VALU_PER_ADD / 64) / (0.4474e6 * n_simd) if curve == "bls12_381" else None
    roofline = {
        "bound": "hbm",
        "achieved": achieved / 1e9 if achieved else None,
        "peak": HBM_PEAK / 1e9,
        "unit": "GB/s",
        "frac": (achieved / HBM_PEAK) if achieved else None,
        "traffic": traffic,
        "traffic_source": traffic_src,
        "gather_model_bytes": gather_bytes,
        "gather_note": "Pippenger accumulation gathers one 112-B radix-2^29 point (128-B stride) and streams one "
                       "4-B sorted value per window term (keys only at bucket starts), 32 terms per tuple: "
                       "traffic above the 256 B/tuple of unique input is inherent to the bucket method, not a "
                       "re-read to fix",
        "rocprof_kernel_avg_ms": rocprof_ms,
        "rocprof_source": rocprof_src,
        "timing_note": "kernel_ms = HIP events around k_accumulate + k_fixup of a non-pipelined "
                       "batch in this run (rocprof_kernel_avg_ms: the same kernels, rocprofv3 kernel trace of "
                       "single batches); kernel_ms_in_pipelined_region includes queueing behind other slots",
        "kernel": "k_accumulate+k_fixup (bucket accumulation, radix 2^29 on BLS12-381)",
        "kernel_ms": acc_ms,
        "kernel_ms_in_pipelined_region": acc_ms_pipe,
        "algorithmic_bytes": alg_bytes,
        "note": "integer-multiply (VALU) bound, not HBM: see compute",
        "compute": {
            "bound": "valu_mad_u64_u32",
            "model": "10 Fp products (8M + 2S) per mixed addition, 32 n additions per batch",
            "achieved_fpmul_per_s": acc_fpmuls / (acc_ms * 1e-3) if acc_ms > 0 else None,
            "peak_fpmul_per_s": fpmul_peak,
            "frac": (acc_fpmuls / (acc_ms * 1e-3)) / fpmul_peak if acc_ms > 0 else None,
            "peak_note": "peak_fpmul_per_s: kzgmi_probe_fpmul (32-bit-limb products, 8 chains per thread, whole "
                         "chip) measured in this run; hw_floor: the hardware mad issue rate",
            "hw_floor": {
                "mad_issue_rate_per_simd_ns": 0.4596, "simds": n_simd, "mads_per_product": 392,
                "source": "profiles/r01/probes/mad_rate.txt (tools/probes/mad_rate.hip, 8 waves/SIMD)",
                "peak_fpmul_per_s": mad_floor,
                "frac": (acc_fpmuls / (acc_ms * 1e-3)) / mad_floor if (mad_floor and acc_ms > 0) else None,
            },
            # every VALU instruction of the loop (SQ_INSTS_VALU per addition, profiles/r04/
            # pmc_sq_accumulate.json) at the issue rate a dependent mad chain reaches with the
            # kernel's 4 waves per SIMD (profiles/r02/probes/mad_rate_blocks.txt): the time the
            # kernel's instruction stream needs at that rate, over the measured accumulation phase
            "valu_issue_floor": {
                "valu_instr_per_addition": VALU_PER_ADD, "issue_rate_per_simd_ns": 0.4474, "simds": n_simd,
                "source": "profiles/r05/pmc_sq_accumulate.json + profiles/r02/probes/mad_rate_blocks.txt "
                          "('mad chain x8, 4/statement', 4 waves/SIMD)",
                "floor_ms": valu_floor_ms,
                "frac": valu_floor_ms / acc_ms if (valu_floor_ms and acc_ms > 0) else None,
            } if valu_floor_ms else None,
            # whole pipeline: accumulation products per second of wall time (batches/s x
            # products per batch) against the probe peak -- what the overlap actually sustains
            "pipeline_frac": acc_fpmuls * value / world / fpmul_peak,
        },
    }
    cpu = None
    if not args.no_cpu and world == 1:
        try:
            cpu = cpu_baseline(curve, Cm, z, y, P, n, vseed, args.cpu_seconds)
            cpu["host"] = host_info()
        except Exception as e:  # the baseline must not kill the GPU measurement
            cpu = {"error": repr(e)}
    # ---- the same timed region at HIP's default hardware-queue count (child process)
    dq = None
    if world == 1 and not sharded and args.default_queues_steps > 0:
        env = dict(os.environ, KZGMI_HW_QUEUES="4")
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.default_queues_steps),
               "--warmup", str(min(args.warmup, 5)), "--n", str(n), "--curve", curve, "--slots", str(slots),
               "--detail-file", "", "--no-cpu", "--repeats", "1", "--default-queues-steps", "0", "--msm-steps", "0",
               "--trusted-steps", "0", "--fs-steps", "0", "--commit-steps", "0", "--compressed-steps", "0",
               "--cfg4-msms", "0", "--h2d-steps", "0", "--bn254-steps", "0", "--shard17-steps", "0"]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            line = json.loads(p.stdout.strip().splitlines()[-1])
            dq = {"hw_queues": 4, "batch_verifies_per_s": line["value"], "ms_per_step": line["ms_per_step"],
                  "steps": args.default_queues_steps, "frac_of_value": line["value"] / value}
        except Exception as e:  # the child's failure must not kill the headline measurement
            dq = {"error": repr(e)[:300]}
    cfg0_cpu_ms = (cpu or {}).get("cfg0_cpu_n256_ms")
    if cfg0 is not None and cfg0_cpu_ms is not None:
        cfg0["cpu_ms"] = cfg0_cpu_ms
        cfg0["cpu_threads"] = cpu.get("cores")
    detail = {
        "tuples_per_s": value * n,
        "msm_pts_per_s": msm_rate,
        "msm_n_per_gpu": n,
        "msm_single_latency_ms": msm_latency_ms,
        "msm_method": "pipelined over the batch slots (kzgmi_msm_g1_device_async), 255-bit scalars",
        "msm_trusted_g1_glv": {"pts_per_s": msm_rate_t, "single_latency_ms": msm_latency_t,
                               "note": "points declared G1 members (kzgmi_set_trusted_g1): GLV split"},
        "trusted_g1": trusted,
        "single_batch_latency_ms": lat,
        "single_batch_latency_note": "median of 10 synchronous batches (host clock, HBM-resident inputs)",
        "repeats_median_batch_verifies_per_s": statistics.median(rep_values),
        "repeats_batch_verifies_per_s": rep_values,
        "repeats_note": "the timed region (warm pipeline, --steps batches, barrier + synchronize on both "
                        "sides, max over ranks) run --repeats times back to back; value is the first",
        "single_batch_latency_runs_ms": lat_runs,
        "strong_scaling_batch": strong,
        "allocs_in_timed_region": allocs_timed,
        "cfg0_n256": cfg0,
        "phase_ms_avg_in_timed_region": phases,
        "phase_ms_single_batch": phases_single,
        "phase_ms_single_batch_note": "single-launch accumulation (the pipelined form, kzgmi_set_split_acc 0); "
                                      "single_batch_latency_ms runs the default split form (phase_ms_single_batch_split)",
        "phase_ms_single_batch_split": phases_single_split,
        "compressed_subgroup": comp,
        "fiat_shamir": fsm,
        "prover_commit": commit,
        "cfg4_msm_2e24": cfg4,
        "h2d_inclusive": h2d,
        "sharded_2e17_world1": shard17,
        "bn254_cfg4": bn,
        "roofline": roofline,
        "cpu_baseline": cpu,
        "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
        "default_hw_queues": dq,
    }
    # The printed line stays short enough (< ~5 kB) for the driver's stdout tail to hold all of
    # it; the full record (per-run arrays, phase dicts, methods) goes to a side file.
    detail_path = os.path.join(ROOT, args.detail_file) if args.detail_file else None
    try:
        if detail_path:
            os.makedirs(os.path.dirname(detail_path), exist_ok=True)
            with open(detail_path, "w") as f:
                json.dump(detail, f, indent=1)
    except OSError:
        detail_path = None

    def r4(x):
        return float("%.4g" % x) if isinstance(x, (int, float)) and not isinstance(x, bool) else x

    def g(d, *keys):
        for k in keys:
            if not isinstance(d, dict):
                return None
            d = d.get(k)
        return r4(d)

    comp_cpu = cpu if cpu and "value" in cpu else None
    hw = roofline["compute"]["hw_floor"]
    vif = roofline["compute"].get("valu_issue_floor") or {}
    roof_out = {k: (r4(v) if not isinstance(v, str) else v) for k, v in roofline.items()
                if k not in ("compute", "gather_note", "timing_note", "traffic_source", "rocprof_source")}
    roof_out.update({
        "hw_floor_frac": r4(hw.get("frac")), "valu_issue_floor_frac": r4(vif.get("frac")),
        "traffic_source": "profiles/%s/rocprof_single/pmc_accumulate_single.json (2 FETCH_SIZE + WRITE_SIZE)" % PROFILE_ROUND,
        "rocprof_source": "profiles/%s/rocprof_single/kernel_single.json" % PROFILE_ROUND,
        "compute": {"bound": "valu_mad_u64_u32", "achieved_fpmul_per_s": r4(roofline["compute"]["achieved_fpmul_per_s"]),
                    "hw_floor_fpmul_per_s": r4(hw.get("peak_fpmul_per_s")), "hw_floor_frac": r4(hw.get("frac")),
                    "valu_issue_floor_ms": r4(vif.get("floor_ms")), "valu_issue_floor_frac": r4(vif.get("frac")),
                    "pipeline_frac": r4(roofline["compute"]["pipeline_frac"])},
    })
    cpu_out = None
    if cpu:
        cpu_out = {k: r4(cpu.get(k)) for k in ("value", "unit", "cores", "kind", "sample", "sample_tuples",
                                              "sample_seconds", "window_bits", "error") if k in cpu}
        if comp_cpu:
            cpu_out.update({
                "single_core_value": r4(cpu["single_core"]["value"]),
                "oracle_value": r4(cpu["oracle"]["value"]),
                "full_host_extrapolated": r4(cpu["full_host_extrapolated"]["value"]),
                "full_host_threads": cpu["full_host_extrapolated"]["threads"],
                "full_host_note": "EXTRAPOLATION, not measured: single-core tuned rate x the host's hardware threads "
                                  "(linear; this job may use only %s of them)" % cpu.get("cores"),
                "cfg0_n256_ms": r4(cpu.get("cfg0_cpu_n256_ms")),
            })
    sec = {
        "tuples_per_s": r4(value * n),
        "repeats_median_batch_verifies_per_s": r4(statistics.median(rep_values)),
        "single_batch_latency_ms": r4(lat),
        "phase_ms_single_batch": {k: r4(v) for k, v in (phases_single or {}).items() if v},
        "allocs_in_timed_region": allocs_timed,
        "cfg0_n256_gpu_ms": g(cfg0, "gpu_latency_ms"), "cfg0_n256_cpu_ms": g(cfg0, "cpu_ms"),
        "strong_scaling_batch_per_s": g(strong, "batch_verifies_per_s"),
        "trusted_g1_glv_per_s": g(trusted, "batch_verifies_per_s"),
        "fiat_shamir_per_s": g(fsm, "batch_verifies_per_s"),
        "compressed_subgroup_per_s": g(comp, "batch_verifies_per_s"),
        "compressed_convert_ms": g(comp, "phase_ms_single_batch", "convert"),
        "prover_commit_pts_per_s": g(commit, "pts_per_s"),
        "h2d_pinned_per_s": g(h2d, "batch_verifies_per_s_pinned"),
        "h2d_pageable_per_s": g(h2d, "batch_verifies_per_s_pageable"),
        "pcie_h2d_GBps": g(h2d, "pcie_h2d_GBps"),
        "cfg3_msm_2e24_pts_per_s": g(cfg4, "pts_per_s"),
        "cfg3_projected_8gpu_strong_speedup": g(cfg4, "per_rank_share_at_8_gpus", "projected_8gpu_strong_speedup"),
        "shard_2e17_rccl_world1_per_s": g(shard17, "batch_verifies_per_s_sharded_rccl_world1"),
        "shard_2e17_projected_8gpu_strong_speedup": g(shard17, "projected_8gpu_strong_speedup"),
        "cfg4_bn254_2e19_per_s": g(bn, "n2e19_per_gpu_shard", "batch_verifies_per_s"),
        "cfg4_bn254_2e22_per_s": g(bn, "n2e22_whole", "batch_verifies_per_s"),
        "cfg4_bn254_hw_floor_frac": g(bn, "n2e22_whole", "hw_floor_frac"),
        "cfg4_bn254_2e19_hw_floor_frac": g(bn, "n2e19_per_gpu_shard", "hw_floor_frac"),
        "gpu_vs_cpu": r4(value / cpu["value"]) if comp_cpu else None,
        "gpu_vs_cpu_full_host_extrapolated": r4(value / cpu["full_host_extrapolated"]["value"]) if comp_cpu else None,
        "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
        "default_hw_queues_batch_verifies_per_s": g(dq, "batch_verifies_per_s"),
        "default_hw_queues_frac": g(dq, "frac_of_value"),
        "detail_file": os.path.relpath(detail_path, ROOT) if detail_path else None,
    }
    out.update({
        "roofline": roof_out,
        "cpu_baseline": cpu_out,
        "secondary": sec,
        # last, so the driver's stdout tail always holds it: the second half of the metric
        # (BASELINE.json:2, configs[1]) and the binding roofline
        "headline": {
            "batch_verifies_per_s": r4(value),
            "msm_pts_per_s_2e20": r4(msm_rate),
            "msm_pts_per_s_2e20_glv": r4(msm_rate_t),
            "msm_single_latency_ms": r4(msm_latency_ms),
            "repeats_median_batch_verifies_per_s": r4(statistics.median(rep_values)),
            "single_batch_latency_ms": r4(lat),
            "roofline_hbm_frac": r4(roofline["frac"]),
            "roofline_hw_floor_frac": r4(hw.get("frac")),
            "gpu_vs_cpu": sec["gpu_vs_cpu"],
            "gpu_vs_cpu_full_host_extrapolated": sec["gpu_vs_cpu_full_host_extrapolated"],
        },
    })
    print(json.dumps(out), flush=True)
    if sharded:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
