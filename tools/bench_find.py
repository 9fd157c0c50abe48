"""Timing of the search for a rejected batch's invalid tuples (csrc/host_find.hip) and of its parts.

  * the search on BLS12-381 at n = 2^20 with 1 and with 16 invalid tuples and at n = 2^12 with 1, each
    beside one batch_verify of the same device-resident inputs, measured in the same process, and beside
    what n single-tuple verifies would take (one is timed, times n);
  * the batched pairing check at G = 1, 16, 256, 512 record pairs;
  * the crossover between the two paths of a level: `fanout` parts of length L as one grouped launch
    (batch_range_partials) against the same parts as bucket partial jobs one after another
    (batch_partial), for L around the shipped FindTuning::group_terms.

The search and the calls it is compared with are synchronous and include their host round trips, so
every time is wall-clock around the call with the device idle before it; medians over --reps warmed
calls.  Inputs are made on the device (gen_tuples); a tuple is made invalid by changing its y.

    python tools/bench_find.py [--reps 5] [--big 20] [--out-dir profiles/find]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kzg-batch-verification-scheme_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CURVE = "bls12_381"
TAU = 0x5EA2C4F00D15EA5E
SEED = hashlib.sha256(b"bench-find").digest()


def wall(torch, fn, reps, warmup):
    out = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big", type=int, default=20, help="log2 of the large batch")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "find"))
    a = ap.parse_args()
    import torch
    import kzgmi
    import findprobe
    from oracle import oracle as O
    from oracle.pyspec import curves as pc
    from oracle.pyspec import kzg as pk

    ctx = kzgmi.Context(0, 1)
    C = pc.CURVES[CURVE]
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(CURVE, g2, O.g2_mul(CURVE, g2, TAU))
    tune = findprobe.tuning()
    pb = ctx.partial_bytes(CURVE)
    res = {"device": torch.cuda.get_device_name(0), "tuning": tune, "reps": a.reps, "search": [], "pairing": [],
           "crossover": []}

    def gen(n):
        t = [torch.empty(n * s, dtype=torch.uint8, device="cuda") for s in (96, 32, 32, 96)]
        ctx.gen_tuples(CURVE, TAU, SEED, n, *t)
        return t

    # ---- the search
    for logn, nbad in ((a.big, 1), (a.big, 16), (12, 1)):
        n = 1 << logn
        t = gen(n)
        bad = sorted({(n // 3 + k * (n // 16 + 1)) % n for k in range(nbad)})
        for i in bad:
            t[2][32 * i + 31] += 1
        got = ctx.batch_find_invalid(srs, *t, seed=SEED, n=n, max_bad=64)
        assert got == (bad, False), got
        st = ctx.find_invalid_stats()
        ms, lo = wall(torch, lambda: ctx.batch_find_invalid(srs, *t, seed=SEED, n=n, max_bad=64), a.reps, a.warmup)
        vms, _ = wall(torch, lambda: ctx.batch_verify(srs, *t, seed=SEED, n=n), a.reps, a.warmup)
        one = [x[:s].clone() for x, s in zip(t, (96, 32, 32, 96))]
        sms, _ = wall(torch, lambda: ctx.batch_verify(srs, *one, seed=SEED, n=1), a.reps, a.warmup)
        row = {"n": n, "invalid": nbad, "search_ms": ms, "search_min_ms": lo, "verify_ms": vms, "single_verify_ms": sms,
               "n_single_verifies_ms": sms * n, "stats": st}
        res["search"].append(row)
        print(json.dumps(row), flush=True)
        del t

    # ---- the batched pairing
    t = gen(16)
    rec = torch.empty(2 * pb, dtype=torch.uint8, device="cuda")
    ctx.batch_partial(srs, *t, 16, 0, SEED, rec)
    for G in (1, 16, 256, 512):
        recs = rec.repeat(G)
        assert ctx.batch_check_partials(srs, recs, G) == [True] * G
        ms, lo = wall(torch, lambda: ctx.batch_check_partials(srs, recs, G), a.reps, a.warmup)
        row = {"G": G, "ms": ms, "min_ms": lo}
        res["pairing"].append(row)
        print(json.dumps(row), flush=True)

    # ---- the crossover: `fanout` parts of length L, grouped launch against bucket jobs
    F = tune["fanout"]
    shipped = (tune["group_terms"] - 1) // 3
    for L in sorted({shipped // 16, shipped // 4, shipped, 4 * shipped, 16 * shipped}):
        if L < 1:
            continue
        n = F * L
        t = gen(n)
        out = torch.empty(2 * F * pb, dtype=torch.uint8, device="cuda")
        ranges = [(j * L, (j + 1) * L) for j in range(F)]
        row = {"L": L, "parts": F, "wave_terms": F * (3 * L + 1)}
        plan, _ = findprobe.group_plan(ranges)
        row["group_bytes"] = plan["bytes"]
        if plan["bytes"] <= tune["group_bytes"]:
            row["grouped_ms"], row["grouped_min_ms"] = wall(
                torch, lambda: ctx.batch_range_partials(srs, *t, n, 0, SEED, ranges, out), a.reps, a.warmup)

        def buckets():
            for j in range(F):
                ctx.batch_partial(srs, t[0][96 * j * L:96 * (j + 1) * L], t[1][32 * j * L:32 * (j + 1) * L],
                                  t[2][32 * j * L:32 * (j + 1) * L], t[3][96 * j * L:96 * (j + 1) * L], L, j * L, SEED,
                                  out[2 * j * pb:2 * (j + 1) * pb])
        row["bucket_jobs_ms"], row["bucket_jobs_min_ms"] = wall(torch, buckets, a.reps, a.warmup)
        res["crossover"].append(row)
        print(json.dumps(row), flush=True)
        del t

    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_find.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["Milliseconds, wall-clock medians of %d warmed synchronous calls (%s); fanout %d (bucket levels %d), "
             "group_terms %d." % (a.reps, res["device"], tune["fanout"], tune["bucket_fanout"], tune["group_terms"]), "",
             "| n | invalid | search | one batch_verify | search / verify | n single verifies | levels | bucket jobs | wave-terms | pairings |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["search"]:
        s = r["stats"]
        lines.append("| %d | %d | %.2f | %.2f | %.1f | %.0f | %d | %d | %d | %d |"
                     % (r["n"], r["invalid"], r["search_ms"], r["verify_ms"], r["search_ms"] / r["verify_ms"],
                        r["n_single_verifies_ms"], s["levels"], s["bucket_jobs"], s["wave_terms"], s["pairings"]))
    lines += ["", "| pairing groups G | ms |", "|---|---|"]
    lines += ["| %d | %.3f |" % (r["G"], r["ms"]) for r in res["pairing"]]
    lines += ["", "| part length L (x %d parts) | wave-terms | grouped launch | bucket jobs |" % F, "|---|---|---|---|"]
    for r in res["crossover"]:
        lines.append("| %d | %d | %s | %.2f |" % (r["L"], r["wave_terms"],
                                                  "%.2f" % r["grouped_ms"] if "grouped_ms" in r else "past the bound",
                                                  r["bucket_jobs_ms"]))
    with open(os.path.join(a.out_dir, "bench_find.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
