"""Timing of the openings on every coset of a domain (csrc/cosets.hpp, host_g1ntt.hip: kzgmi_open_cosets*).

Parts:
  accept  per curve, kzgmi_open_cosets_device at (logN, logl, logk) = (12, 6, 7), count = 1, beside
          kzgmi_open_all_device at logn = 12 on the same coefficients in the same loop.  On BLS12-381 this is
          the acceptance comparison: open_cosets' median must not exceed open_all's, or the tool exits with
          an error after writing its results.
  cells   BLS12-381, the same shape in bit-reversed order beside kzgmi_compute_cells_and_proofs_device for 1
          blob and for 72 (count = 72), with the two keys' sizes.  A record.
  large   BLS12-381, (16, 6, 11) and (16, 0, 16) beside open_all at logn = 16.  A record.
  forms   per curve, the whole call at (logN, 6, logN - 6), logN = 10 .. 15 -- 2^11 .. 2^16 terms -- under
          KZGMI_G1NTT_FORM=thread and =wave, alternating.  The product kernels alone come from one run of
          this part under a kernel trace, with no counters in that run,
              rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \
                  python tools/bench_open_cosets.py --parts forms --steps 5 --warmup 1 --no-write
          summarised by --trace-csv <dir>/.../*_kernel_trace.csv (one row per kernel and grid size).

Every figure is a host clock around one synchronous device-form call, which ends in the slot's wait: the
median over --steps calls after --warmup calls of every timed form, the forms alternating within a step.
The warm-up grows every buffer; kzgmi_alloc_count must not move during the timed steps.  Inputs are random
values below 2^253; the commit key is a stand-in (independent G1 points from the library's generator kernel),
which costs the same as powers of a tau.

    python tools/bench_open_cosets.py [--steps 20] [--warmup 3] [--parts accept,cells,large,forms] [--out-dir profiles/open_cosets]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kzg-batch-verification-scheme_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CURVES = ["bls12_381", "bn254"]
EIP = (12, 6, 7)
LARGE = [(16, 6, 11), (16, 0, 16)]
FORM_LOGN = range(10, 16)
FORM_LOGL = 6
CELL_BLOBS = [1, 72]


def random_fr(torch, n):
    """n x 32 B big-endian values below 2^253 (< r on both curves), on the device"""
    a = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda")
    a[:, 0] &= 0x1F
    return a.reshape(-1)


def summarise_trace(path, out):
    """one row per kernel and grid size (workgroups) of a rocprofv3 kernel trace in csv form"""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            wg = int(row["Grid_Size_X"]) // max(1, int(row["Workgroup_Size_X"]))
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            groups.setdefault((row["Kernel_Name"].split("(")[0].replace("void ", ""), wg), []).append(us)
    out.write("| kernel | workgroups | launches | median us | min us | max us |\n|---|---|---|---|---|---|\n")
    for (name, wg), t in sorted(groups.items()):
        if "cosets" in name or "g1ntt" in name:
            out.write("| `%s` | %d | %d | %.1f | %.1f | %.1f |\n" % (name, wg, len(t), statistics.median(t), min(t), max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="accept,cells,large,forms")
    ap.add_argument("--no-write", action="store_true", help="print only (runs under a profiler)")
    ap.add_argument("--trace-csv", help="summarise this kernel trace and exit (needs no GPU)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "open_cosets"))
    a = ap.parse_args()
    if a.trace_csv:
        summarise_trace(a.trace_csv, sys.stdout)
        return
    import torch
    import kzgmi

    assert torch.cuda.is_available(), "bench_open_cosets.py measures on the GPU only"
    torch.manual_seed(21)
    device = torch.cuda.get_device_name(0)
    parts = a.parts.split(",")
    rows = []

    def context(form=None):
        if form:
            os.environ["KZGMI_G1NTT_FORM"] = form
        try:
            return kzgmi.Context(0, 1)
        finally:
            os.environ.pop("KZGMI_G1NTT_FORM", None)

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

    def emit(row):
        row.update(steps=a.steps, device=device)
        print(json.dumps(row), flush=True)
        rows.append(row)

    def commit_key(ctx, curve, n):
        pts = torch.empty(n * 2 * kzgmi.FP_BYTES[curve], dtype=torch.uint8, device="cuda")
        ctx.gen_g1(curve, random_fr(torch, n), n, pts)
        return ctx.load_commit_key(curve, pts.cpu().numpy().tobytes(), n)

    def cosets_form(ctx, key, coeffs, shape, count=1, bitrev=False):
        """a timed open_cosets call into buffers of its own, and the buffers"""
        logN, logl, logk = shape
        gb = 2 * kzgmi.FP_BYTES[key.curve]
        ys = torch.empty((32 * count) << (logk + logl), dtype=torch.uint8, device="cuda")
        proofs = torch.empty((gb * count) << logk, dtype=torch.uint8, device="cuda")
        return (lambda: ctx.open_cosets(key, coeffs, logk, m=1 << logN, count=count, bitrev=bitrev, ys_out=ys, out=proofs)), ys, proofs

    def open_all_form(ctx, key, coeffs):
        n, gb = 1 << key.logn, 2 * kzgmi.FP_BYTES[key.curve]
        ys = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(n * gb, dtype=torch.uint8, device="cuda")
        return (lambda: ctx.open_all(key, coeffs, m=n, ys_out=ys, out=proofs)), ys, proofs

    def against_open_all(ctx, curve, ck, shapes, part):
        logN = shapes[0][0]
        coeffs = random_fr(torch, 1 << logN)
        oa_key = ctx.load_open_all_key(ck, logN)
        oa, oa_ys, oa_proofs = open_all_form(ctx, oa_key, coeffs)
        for shape in shapes:
            key = ctx.load_open_cosets_key(ck, shape[0], shape[1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            key = ctx.load_open_cosets_key(ck, shape[0], shape[1])  # the derivation alone: the first load grew the workspace
            load_ms = (time.perf_counter() - t0) * 1e3
            oc, oc_ys, oc_proofs = cosets_form(ctx, key, coeffs, shape)
            oc()
            oa()
            if shape[1] == 0:
                assert torch.equal(oc_proofs, oa_proofs) and torch.equal(oc_ys, oa_ys), "open_cosets at l = 1 differs from open_all"
            t = measure({"open_cosets": oc, "open_all": oa})
            emit({"part": part, "curve": curve, "shape": shape, "key_load_ms": load_ms, "key_bytes": key.device_bytes,
                  "open_all_key_bytes": oa_key.device_bytes, "forms": t,
                  "open_all_over_open_cosets": t["open_all"]["ms"] / t["open_cosets"]["ms"],
                  "not_slower": t["open_cosets"]["ms"] <= t["open_all"]["ms"]})
            del key, oc
            torch.cuda.empty_cache()

    if "accept" in parts:
        ctx = context()
        for curve in CURVES:
            against_open_all(ctx, curve, commit_key(ctx, curve, 1 << EIP[0]), [EIP], "accept")
        ctx.close()

    if "cells" in parts:
        curve = "bls12_381"
        ctx = context()
        srs = torch.empty(4096 * 96, dtype=torch.uint8, device="cuda")
        ctx.gen_g1(curve, random_fr(torch, 4096), 4096, srs)
        srs = srs.cpu().numpy().tobytes()
        key = ctx.load_open_cosets_key(ctx.load_commit_key(curve, srs, 4096), EIP[0], EIP[1])
        pkey = ctx.load_cell_proof_key(srs)
        for nb in CELL_BLOBS:
            data = random_fr(torch, nb * 4096)  # coefficients to one, a blob's evaluations to the other: the same cost
            oc, _, _ = cosets_form(ctx, key, data, EIP, count=nb, bitrev=True)
            cells = torch.empty(nb * 128 * 2048, dtype=torch.uint8, device="cuda")
            proofs = torch.empty(nb * 128 * 48, dtype=torch.uint8, device="cuda")
            t = measure({"open_cosets": oc, "compute_cells_and_proofs": lambda: ctx.compute_cells_and_proofs(
                pkey, data, nb, out=cells, proofs_out=proofs)})
            emit({"part": "cells", "curve": curve, "shape": EIP, "blobs": nb, "key_bytes": key.device_bytes,
                  "cell_proof_key_bytes": pkey.device_bytes, "forms": t})
        del key, pkey
        ctx.close()

    if "large" in parts:
        ctx = context()
        against_open_all(ctx, "bls12_381", commit_key(ctx, "bls12_381", 1 << LARGE[0][0]), LARGE, "large")
        ctx.close()

    if "forms" in parts:
        ctxs = {form: context(form) for form in ("thread", "wave")}
        for curve in CURVES:
            cks = {form: commit_key(c, curve, 1 << max(FORM_LOGN)) for form, c in ctxs.items()}
            for logN in FORM_LOGN:
                shape = (logN, FORM_LOGL, logN - FORM_LOGL)
                coeffs = random_fr(torch, 1 << logN)
                keys = {form: c.load_open_cosets_key(cks[form], logN, FORM_LOGL) for form, c in ctxs.items()}
                forms = {form: cosets_form(c, keys[form], coeffs, shape)[0] for form, c in ctxs.items()}
                emit({"part": "forms", "curve": curve, "shape": shape, "terms": 2 << logN, "forms": measure(forms)})
                del keys, forms
            del cks
            torch.cuda.empty_cache()
        for c in ctxs.values():
            c.close()

    if not a.no_write:
        write(a, rows, device)
    # the acceptance bound (BLS12-381 only: BN254's row is a record); the results are written first
    missed = [r for r in rows if r["part"] == "accept" and r["curve"] == "bls12_381" and not r["not_slower"]]
    if missed:
        t = missed[0]["forms"]
        sys.exit("acceptance missed: open_cosets %.3f ms > open_all %.3f ms at %s" % (
            t["open_cosets"]["ms"], t["open_all"]["ms"], tuple(missed[0]["shape"])))


def write(a, rows, device):
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_open_cosets.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out_dir, "bench_open_cosets.md"), "w") as f:
        f.write("# kzgmi_open_cosets_device (tools/bench_open_cosets.py, %s)\n\n" % device)
        f.write("Median wall ms per synchronous device-form call over %d steps (min .. max).\n\n" % a.steps)
        f.write("| part | curve | (logN, logl, logk) | form | ms | min .. max | note |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            for name, t in r["forms"].items():
                note = ""
                if name == "open_cosets" and "key_load_ms" in r:
                    note = "key: %.1f ms to load, %.2f MiB; open_all / open_cosets = %.2f, not slower: %s" % (
                        r["key_load_ms"], r["key_bytes"] / 2**20, r["open_all_over_open_cosets"], r["not_slower"])
                elif name == "open_all":
                    note = "key: %.2f MiB" % (r["open_all_key_bytes"] / 2**20)
                elif r["part"] == "cells":
                    note = "%d blob(s); key: %.2f MiB" % (
                        r["blobs"], (r["key_bytes"] if name == "open_cosets" else r["cell_proof_key_bytes"]) / 2**20)
                elif r["part"] == "forms":
                    note = "%d terms" % r["terms"]
                f.write("| %s | %s | %s | %s | %.3f | %.3f .. %.3f | %s |\n" % (
                    r["part"], r["curve"], tuple(r["shape"]), name, t["ms"], t["min_ms"], t["max_ms"], note))


if __name__ == "__main__":
    main()
