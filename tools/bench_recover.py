"""Timing of EIP-7594 cell extension and recovery (csrc/recover.hpp): compute_cells and
recover_cells for nb = 1, 6 and 72 blobs, recovery from k = 64 cells (the even ones).

Device time: torch events on the current stream around the async device form on slot 1, ordered
around the library's slot stream by its stream_wait / slot_signal, so they bracket device work
only; the median over --steps warmed calls.  Wall time: a host clock around --steps synchronous
device-form calls (each ends in the slot's wait), per call -- what a caller that blocks pays.
Buffers are grown by the warm-up calls (Context.reserve sizes the verification workspace, which
these calls do not use).

HBM traffic is counted from the shapes: compute_cells reads nb x 128 KiB and writes nb x 256 KiB;
recover_cells reads its nb x k x 2 KiB twice (the load, and the compare as the output is written),
parks two 128 KiB vectors per blob in the output's second half (written and read back once each)
and writes nb x 256 KiB.  The 768 KiB transform table is shared by every workgroup and stays in
L2.  The implied bandwidth is that traffic over the device time, beside the 6.29 TB/s a float4
copy reaches on this chip: one workgroup per blob, so nb = 1 and 6 are latency-bound on a handful
of the 256 CUs and the ratio there is no utilisation figure.

The inputs are random in-range elements: every kernel's work is data-independent.  With k = 64 any
input is consistent, so recovery succeeds on them.

    python tools/bench_recover.py [--sizes 1,6,72] [--steps 200] [--warmup 20] [--out-dir profiles/recover]
"""
import argparse
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

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the chip
BLOB_BYTES, CELL_BYTES, EXT_BYTES = 4096 * 32, 2048, 8192 * 32


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
    ap.add_argument("--sizes", default="1,6,72")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "recover"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kzgmi

    assert torch.cuda.is_available(), "bench_recover.py measures on the GPU only"
    sizes = [int(x) for x in a.sizes.split(",")]
    k = a.k
    idx_h = list(range(0, 128, 2)) + list(range(1, 2 * (k - 64), 2))
    assert len(idx_h) == k
    ctx = kzgmi.Context(0, 2)
    rng = np.random.default_rng(7594)
    idx = torch.frombuffer(bytearray(struct.pack("<%dQ" % k, *idx_h)), dtype=torch.uint8).cuda()
    rows = []
    for nb in sizes:
        def rand(nbytes):
            host = rng.integers(0, 256, size=(nbytes // 32, 32), dtype=np.uint8)
            host[:, 0] &= 0x3F  # < 2^254 < r
            return torch.from_numpy(host.reshape(-1)).cuda()
        blobs, cells = rand(nb * BLOB_BYTES), rand(nb * k * CELL_BYTES)
        out = torch.empty(nb * EXT_BYTES, dtype=torch.uint8, device="cuda")
        runs = {
            "compute": (lambda: ctx.compute_cells_async(1, blobs, nb, out), lambda: ctx.compute_cells(blobs, nb, out=out)),
            "recover": (lambda: ctx.recover_cells_async(1, idx, cells, nb, out),
                        lambda: ctx.recover_cells(idx, cells, nb, out=out)),
        }
        traffic = {"compute": nb * (BLOB_BYTES + EXT_BYTES),
                   "recover": nb * (2 * k * CELL_BYTES + 4 * BLOB_BYTES + EXT_BYTES)}
        row = {"nb": nb, "k": k, "steps": a.steps}
        for key, (enqueue, sync_call) in runs.items():
            dev = []
            for step in range(a.warmup + a.steps):
                ms = timed(torch, ctx, 1, enqueue)
                ctx.wait(1)
                if step >= a.warmup:
                    dev.append(ms)
            for _ in range(a.warmup):
                sync_call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                sync_call()
            wall = (time.perf_counter() - t0) * 1e3 / a.steps
            med = statistics.median(dev)
            row.update({key + "_ms": med, key + "_min_ms": min(dev), key + "_p90_ms": sorted(dev)[int(0.9 * len(dev))],
                        key + "_wall_ms": wall, key + "_hbm_bytes": traffic[key],
                        key + "_implied_tbs": traffic[key] / (med * 1e-3) / 1e12,
                        key + "_ratio_of_copy_rate": traffic[key] / (med * 1e-3) / 1e12 / HBM_COPY_TBS})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del blobs, cells, out
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_recover.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": HBM_COPY_TBS, "rows": rows}, f, indent=1)
    lines = ["| nb | op | device ms (median) | min | p90 | wall ms per sync call | HBM bytes | implied TB/s | / %.2f TB/s |"
             % HBM_COPY_TBS, "|" + "---|" * 9]
    for r_ in rows:
        for key in ("compute", "recover"):
            lines.append("| %d | %s | %.4f | %.4f | %.4f | %.4f | %d | %.3f | %.3f |" % (
                r_["nb"], key if key == "compute" else "recover k=%d" % r_["k"], r_[key + "_ms"], r_[key + "_min_ms"],
                r_[key + "_p90_ms"], r_[key + "_wall_ms"], r_[key + "_hbm_bytes"], r_[key + "_implied_tbs"],
                r_[key + "_ratio_of_copy_rate"]))
    with open(os.path.join(a.out_dir, "bench_recover.md"), "w") as f:
        f.write("Cell extension and recovery, %d warmed calls per row (%s).  Device ms: events around the async\n"
                "device form; wall ms: a host clock around synchronous device-form calls.  HBM bytes: counted from\n"
                "the shapes (tools/bench_recover.py); the last column is the implied rate over the chip's measured\n"
                "copy rate, no utilisation figure at nb = 1 and 6 (one workgroup per blob).\n\n"
                % (a.steps, torch.cuda.get_device_name(0)))
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
