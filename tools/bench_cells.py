"""Timing of the EIP-7594 cell front end (csrc/cell.hpp) and of the whole verify_cell_batch.

For n = 128, 768 (6 blobs x 128 columns) and 2688 (21 x 128) cells: the device transcript hash
(cell_batch_challenge), fold + inverse NTT (cell_interp), the whole device-resident verification
with the challenge derived on the device and with a caller-supplied one (async form, so the events
bracket device work only), and as yardstick batch_verify in its powers + compressed +
subgroup-check mode at the same n -- what the library did before the cell front end existed, so
the difference is the front end's cost.  Times are torch events on the current stream, ordered
around the library's slot stream by its stream_wait / slot_signal; medians over --reps warmed
calls; the library's own phase marks (set_profiling) split the two hash-free forms.  Beside them
single-thread hashlib.sha256 (OpenSSL) over the same transcript: what a caller holding the bytes
on the host pays to supply r itself.

The inputs are random in-range cells on cosets k mod 128 with arbitrary valid G1 points as
commitments and proofs: every kernel's work is data-independent, the verdict (reject) is not what
is measured.

    python tools/bench_cells.py [--sizes 128,768,2688] [--reps 5] [--out-dir profiles/cells]
"""
import argparse
import hashlib
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kzg-batch-verification-scheme_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(torch, ctx, slot, fn):
    """Milliseconds between two events around fn's work on `slot`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    ctx.signal(slot)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,768,2688")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "cells"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kzgmi
    import cellref as K

    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = kzgmi.Context(0, 2)
    g1m, g2, t64 = K.toy_cell_srs(0x7594)
    csrs = ctx.load_cell_srs(g1m, g2, t64)
    srs = ctx.load_srs(K.CURVE, g2, t64)
    rng = np.random.default_rng(7594)
    rows = []
    for n in sizes:
        m = max(1, n // K.NUM_CELLS)
        host = rng.integers(0, 256, size=(n * K.CELL_N, 32), dtype=np.uint8)
        host[:, 0] &= 0x3F  # < 2^254 < r
        cells = torch.from_numpy(host.reshape(-1)).cuda()
        sc = torch.from_numpy(rng.integers(0, 256, size=(m + n) * 32, dtype=np.uint8)).cuda()
        sc[::32] &= 0x3F
        pts = torch.empty((m + n) * 96, dtype=torch.uint8, device="cuda")
        cp = torch.empty((m + n) * 48, dtype=torch.uint8, device="cuda")
        ctx.gen_g1(K.CURVE, sc, m + n, pts)
        ctx.g1_compress(K.CURVE, pts, m + n, cp)
        cm, pf = cp[:48 * m].clone(), cp[48 * m:].clone()
        cidx_h = [k // K.NUM_CELLS % m for k in range(n)]
        cell_h = [k % K.NUM_CELLS for k in range(n)]
        cidx = torch.frombuffer(bytearray(struct.pack("<%dQ" % n, *cidx_h)), dtype=torch.uint8).cuda()
        cell = torch.frombuffer(bytearray(struct.pack("<%dQ" % n, *cell_h)), dtype=torch.uint8).cuda()
        # the yardstick's inputs: n gathered commitments, z and y as any canonical scalars
        cmh = cm.cpu().numpy().tobytes()
        gath = torch.frombuffer(bytearray(b"".join(cmh[48 * i:48 * i + 48] for i in cidx_h)), dtype=torch.uint8).cuda()
        zs = sc[:32 * n].clone()
        ys = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        # CPU: the transcript, then its hash (single thread)
        pfh = pf.cpu().numpy().tobytes()
        flat = host.reshape(-1).tobytes()
        msg = K.transcript([cmh[48 * i:48 * i + 48] for i in range(m)], cidx_h, cell_h,
                           [flat[K.CELL_BYTES * k:K.CELL_BYTES * (k + 1)] for k in range(n)],
                           [pfh[48 * k:48 * k + 48] for k in range(n)])
        cpu = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dig = hashlib.sha256(msg).digest()
            cpu.append((time.perf_counter() - t0) * 1e3)
        r = int.from_bytes(dig, "big") % K.R
        assert ctx.cell_batch_challenge(cm, cidx, cell, cells, pf, m, n) == r, "device transcript hash differs"
        coef = ctx.cell_interp(cell, cells, n, r)
        t = {k: [] for k in ("challenge", "interp", "verify_derived", "verify_supplied", "batch_verify_powers")}
        for rep in range(a.warmup + a.reps):
            keep = rep >= a.warmup
            runs = {
                "challenge": (0, lambda: ctx.cell_batch_challenge(cm, cidx, cell, cells, pf, m, n)),
                "interp": (0, lambda: ctx.cell_interp(cell, cells, n, r, out=coef)),
                "verify_derived": (1, lambda: ctx.verify_cell_batch_async(csrs, 1, cm, cidx, cell, cells, pf, m, n)),
                "verify_supplied": (1, lambda: ctx.verify_cell_batch_async(csrs, 1, cm, cidx, cell, cells, pf, m, n, r=r)),
                "batch_verify_powers": (1, lambda: ctx.batch_verify_async(srs, 1, gath, zs, ys, pf, n, compressed=True,
                                                                          subgroup_check=True, challenge=r)),
            }
            for key, (slot, fn) in runs.items():
                ms = timed(torch, ctx, slot, fn)
                if slot == 1:
                    ctx.wait(1)
                if keep:
                    t[key].append(ms)
        # the library's own phase marks (events on the slot's stream) for the two forms without the hash
        phases = {}
        for key in ("verify_supplied", "batch_verify_powers"):
            ctx.set_profiling(True)
            for _ in range(a.reps):
                runs[key][1]()
                ctx.wait(1)
            phases[key] = {k: round(v, 4) for k, v in ctx.phase_ms().items() if v}
            ctx.set_profiling(False)
        row = {"n": n, "m": m, "reps": a.reps, "transcript_bytes": len(msg), "phase_ms": phases}
        row.update({key + "_ms": statistics.median(v) for key, v in t.items()})
        row.update({key + "_min_ms": min(v) for key, v in t.items()})
        row["cpu_sha256_ms"] = statistics.median(cpu)
        row["front_end_supplied_ms"] = row["verify_supplied_ms"] - row["batch_verify_powers_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del cells, host
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_cells.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    cols = ["challenge", "interp", "verify_derived", "verify_supplied", "batch_verify_powers"]
    lines = ["| n | m | " + " | ".join(cols) + " | CPU sha256 |", "|" + "---|" * (len(cols) + 3)]
    for r_ in rows:
        lines.append("| %d | %d | " % (r_["n"], r_["m"]) + " | ".join("%.3f" % r_[c + "_ms"] for c in cols)
                     + " | %.3f |" % r_["cpu_sha256_ms"])
    with open(os.path.join(a.out_dir, "bench_cells.md"), "w") as f:
        f.write("Milliseconds, medians of %d warmed calls (%s).  batch_verify_powers: the powers + compressed +\n"
                "subgroup-check batch check at the same n (the library without the cell front end).  CPU sha256:\n"
                "single-thread hashlib over the same transcript.\n\n" % (a.reps, torch.cuda.get_device_name(0)))
        f.write("\n".join(lines) + "\n")
        f.write("\nPhase marks of the library (ms per call), verify with r supplied / batch_verify_powers:\n\n")
        names = [k for k in kzgmi.PHASES if any(k in r_["phase_ms"]["verify_supplied"] for r_ in rows)]
        f.write("| n | " + " | ".join(names) + " |\n|" + "---|" * (len(names) + 1) + "\n")
        for r_ in rows:
            ph = r_["phase_ms"]
            f.write("| %d | " % r_["n"] + " | ".join("%.3f / %.3f" % (ph["verify_supplied"].get(k, 0), ph["batch_verify_powers"].get(k, 0))
                                                    for k in names) + " |\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
