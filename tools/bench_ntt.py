"""Timing of the power-of-two transforms over Fr (csrc/ntt.hpp, host_ntt.hip): kzgmi_fr_ntt_device,
forward and inverse, per curve at logn = 12 (count 1 and 256), 16 (count 16), 20, 24 and 26 (count 1),
for each tile size of --tile-bits (KZGMI_NTT_TILE_BITS, one context each), beside three comparators
taken in the same loop: a device-to-device copy of the same bytes (passes x that copy is the memory
floor of the plan), kzgmi_compute_cells_device on 128 blobs (256 of the shipped 4096-point transforms,
beside logn = 12, count = 256; BLS12-381), and kzgmi_open_device against kzgmi_open_evals_device at
2^20 values, k = 1 (the difference is the inverse transform's share of an opening).

Every figure is a host clock around one synchronous device-form call, which ends in the slot's wait
(the copy: in a stream synchronise): the median over --steps calls after --warmup calls of every timed
form, the forms alternating within a step.  The warm-up grows every buffer; kzgmi_alloc_count must not
move during the timed steps.  Inputs are random values below 2^253; the key is a stand-in (independent
G1 points from the library's generator kernel).

    python tools/bench_ntt.py [--steps 20] [--warmup 3] [--tile-bits 10,11,12] [--out-dir profiles/ntt]
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

CASES = [(12, 1), (12, 256), (16, 16), (20, 1), (24, 1), (26, 1)]
CURVES = ["bls12_381", "bn254"]
OPEN_LOGN = 20


def random_fr(torch, n):
    """n x 32 B big-endian values below 2^253 (< r on both curves), on the device"""
    a = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda")
    a[:, 0] &= 0x1F
    return a.reshape(-1)


def passes(logn, tile_bits):
    return max(1, -(-logn // (tile_bits - 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tile-bits", default="10,11,12")
    ap.add_argument("--max-logn", type=int, default=26)
    ap.add_argument("--no-open", action="store_true", help="skip the opening comparator (it loads a 2^20-point key)")
    ap.add_argument("--no-write", action="store_true", help="print only (runs under a profiler)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ntt"))
    a = ap.parse_args()
    import torch
    import kzgmi

    assert torch.cuda.is_available(), "bench_ntt.py measures on the GPU only"
    torch.manual_seed(7594)
    tiles = [int(x) for x in a.tile_bits.split(",")]
    ctxs = {}
    for tb in tiles:  # the tile size is read when a context is created
        os.environ["KZGMI_NTT_TILE_BITS"] = str(tb)
        ctxs[tb] = kzgmi.Context(0, 1)
    del os.environ["KZGMI_NTT_TILE_BITS"]
    base = kzgmi.Context(0, 1)  # the shipped defaults: the comparators
    device = torch.cuda.get_device_name(0)
    rows = []

    def measure(forms):
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
        return {name: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}

    for curve in CURVES:
        for logn, count in CASES:
            if logn > a.max_logn:
                continue
            total = count << logn
            src = random_fr(torch, total)
            dst = torch.empty_like(src)
            forms = {}

            def copy():
                dst.copy_(src)
                torch.cuda.synchronize()
            forms["copy"] = copy
            for tb, c in ctxs.items():
                forms["fwd_t%d" % tb] = lambda c=c: c.fr_ntt(curve, src, logn, count=count, out=dst)
                forms["inv_t%d" % tb] = lambda c=c: c.fr_ntt(curve, src, logn, count=count, inverse=True, out=dst)
            if curve == "bls12_381" and (logn, count) == (12, 256):
                cells = torch.empty(128 * kzgmi.EXT_BLOB_BYTES, dtype=torch.uint8, device="cuda")
                forms["compute_cells_128"] = lambda: base.compute_cells(src, 128, out=cells)
            # every tile size computes the same
            ref = ctxs[tiles[0]].fr_ntt(curve, src, logn, count=count).clone()
            for tb in tiles[1:]:
                assert torch.equal(ctxs[tb].fr_ntt(curve, src, logn, count=count), ref), "tile sizes disagree"
            del ref
            row = {"curve": curve, "logn": logn, "count": count, "bytes": 32 * total, "steps": a.steps, "device": device,
                   "passes": {str(tb): passes(logn, tb) for tb in tiles}, "forms": measure(forms)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del src, dst, forms
            torch.cuda.empty_cache()
        if a.no_open:
            continue
        m = 1 << OPEN_LOGN
        g1b = 2 * kzgmi.FP_BYTES[curve]
        pts = torch.empty(m * g1b, dtype=torch.uint8, device="cuda")
        base.gen_g1(curve, random_fr(torch, m), m, pts)
        ck = base.load_commit_key(curve, pts.cpu().numpy().tobytes(), m)
        del pts
        evals, zs = random_fr(torch, m), random_fr(torch, 1)
        coeffs = base.fr_ntt(curve, evals, OPEN_LOGN, inverse=True)
        ys = torch.empty(32, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(g1b, dtype=torch.uint8, device="cuda")
        p1, y1 = base.open(ck, coeffs, zs, m=m, k=1)
        p2, y2 = base.open_evals(ck, evals, zs, logn=OPEN_LOGN, k=1)
        assert torch.equal(p1, p2) and torch.equal(y1, y2), "open_evals differs from open on the coefficients"
        forms = {"open": lambda: base.open(ck, coeffs, zs, m=m, k=1, ys_out=ys, out=proofs),
                 "open_evals": lambda: base.open_evals(ck, evals, zs, logn=OPEN_LOGN, k=1, ys_out=ys, out=proofs),
                 "inv": lambda: base.fr_ntt(curve, evals, OPEN_LOGN, inverse=True, out=coeffs)}
        row = {"curve": curve, "logn": OPEN_LOGN, "opening": True, "steps": a.steps, "device": device, "forms": measure(forms)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ck, evals, coeffs
        torch.cuda.empty_cache()
    for c in list(ctxs.values()) + [base]:
        c.close()
    if a.no_write:
        return
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_ntt.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out_dir, "bench_ntt.md"), "w") as f:
        f.write("# kzgmi_fr_ntt_device (tools/bench_ntt.py, %s)\n\n" % device)
        f.write("Median wall ms per synchronous device-form call over %d steps (min .. max).  t10 / t11 / t12: tiles of\n"
                "2^10 / 2^11 / 2^12 elements (passes of at most 8 / 9 / 10 bits).\n\n" % a.steps)
        f.write("| curve | logn | count | MiB | form | passes | ms | min .. max | GB/s moved |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if r.get("opening"):
                continue
            for name, t in r["forms"].items():
                np_ = r["passes"].get(name[5:], "") if name[:3] in ("fwd", "inv") else (1 if name == "copy" else "")
                moved = 2 * r["bytes"] * np_ / (t["ms"] * 1e6) if np_ else 0
                f.write("| %s | %d | %d | %.1f | %s | %s | %.3f | %.3f .. %.3f | %s |\n" % (
                    r["curve"], r["logn"], r["count"], r["bytes"] / 2**20, name, np_, t["ms"], t["min_ms"], t["max_ms"],
                    "%.0f" % moved if moved else ""))
        f.write("\n| curve | form at 2^%d values, k = 1 | ms | min .. max |\n|---|---|---|---|\n" % OPEN_LOGN)
        for r in rows:
            if r.get("opening"):
                for name, t in r["forms"].items():
                    f.write("| %s | %s | %.3f | %.3f .. %.3f |\n" % (r["curve"], name, t["ms"], t["min_ms"], t["max_ms"]))


if __name__ == "__main__":
    main()
