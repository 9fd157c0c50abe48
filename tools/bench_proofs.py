"""Timing of EIP-7594 cell proof generation (csrc/fk20.hpp): compute_cells_and_proofs for nb = 1, 6
and 72 blobs, the proof key's load time and its device memory.

Device time: torch events on the current stream around the async device form on slot 1, ordered
around the library's slot stream by its stream_wait / slot_signal, so they bracket device work
only; the median over --steps warmed calls.  Wall time: a host clock around --steps synchronous
device-form calls (each ends in the slot's wait), per call.  Buffers are grown by the warm-up calls.

The SRS is a toy one ([tau^m]_1 from the library's generator kernel); the blobs are random in-range
elements.  The work of every kernel but the MSM is data-independent; the MSM skips zero digits
(one in sixteen of a random scalar's).

Per-kernel times come from a separate run under a kernel trace, e.g.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_proofs.py --sizes 6 --steps 20 --warmup 5 --no-write

    python tools/bench_proofs.py [--sizes 1,6,72] [--steps 100] [--warmup 10] [--out-dir profiles/proofs]
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

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU = 0x7594_0000_1234_5678_9ABC_DEF1
BLOB_BYTES, EXT_BYTES, PROOFS_BYTES = 4096 * 32, 8192 * 32, 128 * 48


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--key-loads", type=int, default=3)
    ap.add_argument("--no-write", action="store_true", help="print only (runs under a profiler)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "proofs"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kzgmi

    assert torch.cuda.is_available(), "bench_proofs.py measures on the GPU only"
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = kzgmi.Context(0, 2)
    scal, x = bytearray(), 1
    for _ in range(4096):
        scal += x.to_bytes(32, "big")
        x = x * TAU % R
    pts = torch.empty(4096 * 96, dtype=torch.uint8, device="cuda")
    ctx.gen_g1("bls12_381", torch.frombuffer(scal, dtype=torch.uint8).cuda(), 4096, pts)
    srs = pts.cpu().numpy().tobytes()
    loads = []
    key = None
    for _ in range(a.key_loads):  # the first load also builds the context's transform table
        del key
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        key = ctx.load_cell_proof_key(srs)
        loads.append((time.perf_counter() - t0) * 1e3)
    head = {"device": torch.cuda.get_device_name(0), "key_load_ms": loads, "key_device_bytes": key.device_bytes}
    print(json.dumps(head), flush=True)
    rng = np.random.default_rng(7594)
    rows = []
    for nb in sizes:
        host = rng.integers(0, 256, size=(nb * 4096, 32), dtype=np.uint8)
        host[:, 0] &= 0x3F  # < 2^254 < r
        blobs = torch.from_numpy(host.reshape(-1)).cuda()
        cells = torch.empty(nb * EXT_BYTES, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(nb * PROOFS_BYTES, dtype=torch.uint8, device="cuda")
        runs = {
            "cells_and_proofs": (lambda: ctx.compute_cells_and_proofs_async(key, 1, blobs, nb, cells, proofs),
                                 lambda: ctx.compute_cells_and_proofs(key, blobs, nb, out=cells, proofs_out=proofs)),
            "proofs_only": (lambda: ctx.compute_cells_and_proofs_async(key, 1, blobs, nb, None, proofs),
                            lambda: ctx.compute_cells_and_proofs(key, blobs, nb, cells=False, proofs_out=proofs)),
        }
        row = {"nb": nb, "steps": a.steps}
        for name, (enqueue, sync_call) in runs.items():
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
            row.update({name + "_ms": med, name + "_min_ms": min(dev), name + "_p90_ms": sorted(dev)[int(0.9 * len(dev))],
                        name + "_wall_ms": wall, name + "_ms_per_blob": med / nb})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del blobs, cells, proofs
    lines = ["| nb | form | device ms (median) | min | p90 | per blob | wall ms per sync call |", "|" + "---|" * 7]
    for r_ in rows:
        for name in ("cells_and_proofs", "proofs_only"):
            lines.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
                r_["nb"], name, r_[name + "_ms"], r_[name + "_min_ms"], r_[name + "_p90_ms"], r_[name + "_ms_per_blob"],
                r_[name + "_wall_ms"]))
    print("\n".join(lines))
    if not a.no_write:
        os.makedirs(a.out_dir, exist_ok=True)
        head["rows"] = rows
        with open(os.path.join(a.out_dir, "bench_proofs.json"), "w") as f:
            json.dump(head, f, indent=1)
        with open(os.path.join(a.out_dir, "bench_proofs.md"), "w") as f:
            f.write("Cell proof generation (compute_cells_and_proofs), %d warmed calls per row (%s).  Device ms: events\n"
                    "around the async device form; wall ms: a host clock around synchronous device-form calls\n"
                    "(tools/bench_proofs.py).\n\nProof key: load %s ms (the first load also builds the context's transform\n"
                    "table), %d bytes on the device.\n\n"
                    % (a.steps, head["device"], ", ".join("%.1f" % v for v in loads), head["key_device_bytes"]))
            f.write("\n".join(lines) + "\n")
    del key
    ctx.close()


if __name__ == "__main__":
    main()
