"""Timing of KZG openings over a commit key (csrc/open.hpp, host_open.hip): kzgmi_open_device at
m = 2^20 coefficients for k = 1 and k = 8 points on BLS12-381 and k = 1 on BN254; in the same
process and loop, kzgmi_commit_device of m - 1 coefficients on the same key (the cost of one
quotient's MSM alone), and the scan alone through the diagnostic entry kzgmi_open_quotient_device.

Every figure is a host clock around one synchronous device-form call, which ends in the slot's
wait: the median over --steps calls after --warmup calls of every timed form, the forms
alternating within a step.  The warm-up grows every buffer; kzgmi_alloc_count must not move during
the timed steps.  The key is a stand-in (2^20 independent G1 points from the library's generator
kernel: the loader takes any G1 points), the coefficients and points are random.  The MSM skips
zero digits (one in 2^16 of a random scalar's); every other kernel's work is data-independent.

    python tools/bench_open.py [--log-m 20] [--steps 20] [--warmup 3] [--out-dir profiles/open]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kzg-batch-verification-scheme_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODULI = {
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    "bn254": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
}
CASES = [("bls12_381", (1, 8)), ("bn254", (1,))]


def random_fr(np, rng, n):
    """n x 32 B big-endian values below 2^253 (< r on both curves)"""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 0] &= 0x1F
    return a.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-write", action="store_true", help="print only (runs under a profiler)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "open"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kzgmi

    assert torch.cuda.is_available(), "bench_open.py measures on the GPU only"
    m = 1 << a.log_m
    rng = np.random.default_rng(7594)
    rows = []
    for curve, ks in CASES:
        g1b = 2 * kzgmi.FP_BYTES[curve]
        ctx = kzgmi.Context(0, 1)
        pts = torch.empty(m * g1b, dtype=torch.uint8, device="cuda")
        ctx.gen_g1(curve, torch.from_numpy(random_fr(np, rng, m)).cuda(), m, pts)
        ck = ctx.load_commit_key(curve, pts.cpu().numpy().tobytes(), m)
        del pts
        coeffs = torch.from_numpy(random_fr(np, rng, m)).cuda()
        kmax = max(ks)
        zs = torch.from_numpy(random_fr(np, rng, kmax)).cuda()
        ys = torch.empty(32 * kmax, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(g1b * kmax, dtype=torch.uint8, device="cuda")
        q = torch.empty(32 * kmax * (m - 1), dtype=torch.uint8, device="cuda")
        forms = {"commit": lambda: ctx.commit(ck, coeffs, m - 1)}
        for k in ks:
            forms["open_k%d" % k] = lambda k=k: ctx.open(ck, coeffs, zs, m=m, k=k, ys_out=ys, out=proofs)
            forms["scan_k%d" % k] = lambda k=k: ctx.open_quotient(curve, coeffs, m, zs, k, ys_out=ys, out=q)
        # the opening is what the commit of its quotient gives
        d_p, _ = ctx.open(ck, coeffs, zs, m=m, k=1)
        _, d_q = ctx.open_quotient(curve, coeffs, m, zs, 1)
        assert bytes(d_p.cpu().numpy()) == ctx.commit(ck, d_q, m - 1), "open differs from commit(quotient)"
        for _ in range(a.warmup):
            for f in forms.values():
                f()
        torch.cuda.synchronize()
        allocs = kzgmi.alloc_count()
        times = {name: [] for name in forms}
        for _ in range(a.steps):
            for name, f in forms.items():
                t0 = time.perf_counter()
                f()
                times[name].append((time.perf_counter() - t0) * 1e3)
        assert kzgmi.alloc_count() == allocs, "a timed call allocated"
        row = {"curve": curve, "m": m, "steps": a.steps, "device": torch.cuda.get_device_name(0)}
        for name, t in times.items():
            row[name + "_ms"] = statistics.median(t)
            row[name + "_min_ms"] = min(t)
            row[name + "_max_ms"] = max(t)
        row["open_k1_over_commit"] = row["open_k1_ms"] / row["commit_ms"]
        row["scan_k1_over_commit"] = row["scan_k1_ms"] / row["commit_ms"]
        if 8 in ks:
            row["open_ms_per_extra_point"] = (row["open_k8_ms"] - row["open_k1_ms"]) / 7
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ck, coeffs, q
        ctx.close()
        torch.cuda.empty_cache()
    if a.no_write:
        return
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_open.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out_dir, "bench_open.md"), "w") as f:
        f.write("# kzgmi_open_device, m = 2^%d coefficients (tools/bench_open.py, %s)\n\n" % (a.log_m, rows[0]["device"]))
        f.write("Median wall ms per synchronous device-form call over %d steps (min .. max).\n\n" % a.steps)
        f.write("| curve | form | ms | min .. max |\n|---|---|---|---|\n")
        for r in rows:
            for name in sorted(k[:-7] for k in r if k.endswith("_min_ms")):
                f.write("| %s | %s | %.3f | %.3f .. %.3f |\n" % (r["curve"], name, r[name + "_ms"], r[name + "_min_ms"],
                                                               r[name + "_max_ms"]))
        f.write("\n")
        for r in rows:
            f.write("- %s: open(k = 1) / commit = %.3f, scan(k = 1) / commit = %.3f" %
                    (r["curve"], r["open_k1_over_commit"], r["scan_k1_over_commit"]))
            if "open_ms_per_extra_point" in r:
                f.write(", each further point of k = 8: %.3f ms" % r["open_ms_per_extra_point"])
            f.write("\n")


if __name__ == "__main__":
    main()
