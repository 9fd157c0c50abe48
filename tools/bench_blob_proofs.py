"""Timing of the EIP-4844 producer calls (csrc/blobproof.hpp): blob_commit, compute_kzg_proofs and
compute_blob_proofs for nb = 1, 6 and 72 blobs, the blob proof key's load time and its device memory,
and the baseline for commitments: nb sequential kzgmi_commit_device calls (the bucket MSM) over a
commit key of the same 4096 points, timed in the same run, alternating with blob_commit.

Device time: torch events on the current stream around the async device form on slot 1, ordered
around the library's slot stream by its stream_wait / slot_signal, so they bracket device work
only; the median over --steps warmed calls.  Wall time: a host clock around --steps synchronous
device-form calls (each ends in the slot's wait), per call.  The baseline has no async form that
leaves its result on the device, so its events bracket the nb synchronous calls on slot 0, host
round trips included; its wall time is the same host clock around the nb calls.  Buffers are grown
by the warm-up calls.

The key is a toy one (4096 points [tau^j]_1 from the library's generator kernel: the loader takes
any 4096 G1 points); the blobs are random in-range elements.  The MSM skips zero digits (one in
sixteen of a random scalar's); every other kernel's work is data-independent.

Per-kernel times come from a separate run under a kernel trace, one size at a time, e.g.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_blob_proofs.py --sizes 6 --steps 20 --warmup 5 --no-write

    python tools/bench_blob_proofs.py [--sizes 1,6,72] [--steps 100] [--warmup 10] [--out-dir profiles/blobproof]
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
TAU = 0x4844_0000_1234_5678_9ABC_DEF1
BLOB_BYTES = 4096 * 32
CALLS = ("blob_commit", "compute_kzg_proofs", "compute_blob_proofs")


def timed(torch, ctx, slot, fn):
    """Milliseconds between two events around fn's work on `slot`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    ctx.signal(slot)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(name, dev, wall, nb):
    med = statistics.median(dev)
    return {name + "_ms": med, name + "_min_ms": min(dev), name + "_p90_ms": sorted(dev)[int(0.9 * len(dev))],
            name + "_wall_ms": wall, name + "_ms_per_blob": med / nb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,6,72")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--key-loads", type=int, default=3)
    ap.add_argument("--no-write", action="store_true", help="print only (runs under a profiler)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "blobproof"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kzgmi

    assert torch.cuda.is_available(), "bench_blob_proofs.py measures on the GPU only"
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = kzgmi.Context(0, 2)
    scal, x = bytearray(), 1
    for _ in range(4096):
        scal += x.to_bytes(32, "big")
        x = x * TAU % R
    pts = torch.empty(4096 * 96, dtype=torch.uint8, device="cuda")
    ctx.gen_g1("bls12_381", torch.frombuffer(scal, dtype=torch.uint8).cuda(), 4096, pts)
    points = pts.cpu().numpy().tobytes()
    loads = []
    key = None
    for _ in range(a.key_loads):
        del key
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        key = ctx.load_blob_proof_key(points)
        loads.append((time.perf_counter() - t0) * 1e3)
    ck = ctx.load_commit_key("bls12_381", points, 4096)
    head = {"device": torch.cuda.get_device_name(0), "key_load_ms": loads, "key_device_bytes": key.device_bytes}
    print(json.dumps(head), flush=True)
    rng = np.random.default_rng(4844)
    rows = []
    for nb in sizes:
        host = rng.integers(0, 256, size=(nb * 4096, 32), dtype=np.uint8)
        host[:, 0] &= 0x3F  # < 2^254 < r
        blobs = torch.from_numpy(host.reshape(-1)).cuda()
        each = [blobs[i * BLOB_BYTES:(i + 1) * BLOB_BYTES] for i in range(nb)]
        zs = blobs[:32 * nb].clone()  # any in-range elements
        out = torch.empty(48 * nb, dtype=torch.uint8, device="cuda")
        ys = torch.empty(32 * nb, dtype=torch.uint8, device="cuda")
        cs = ctx.blob_commit(key, blobs, nb)
        one = torch.empty(48, dtype=torch.uint8, device="cuda")  # the two commit routes agree
        ctx.g1_compress("bls12_381", torch.frombuffer(bytearray(ctx.commit(ck, each[0], 4096)), dtype=torch.uint8).cuda(), 1, one)
        assert bytes(one.cpu().numpy()) == bytes(cs[:48].cpu().numpy()), "blob_commit differs from kzgmi_commit"
        runs = {
            "blob_commit": (lambda: ctx.blob_commit_async(key, 1, blobs, nb, out),
                            lambda: ctx.blob_commit(key, blobs, nb, out=out)),
            "compute_kzg_proofs": (lambda: ctx.compute_kzg_proofs_async(key, 1, blobs, zs, nb, out, ys),
                                   lambda: ctx.compute_kzg_proofs(key, blobs, zs, nb, out=out, ys_out=ys)),
            "compute_blob_proofs": (lambda: ctx.compute_blob_proofs_async(key, 1, blobs, cs, nb, out),
                                    lambda: ctx.compute_blob_proofs(key, blobs, cs, nb, out=out)),
        }

        def baseline():
            for b in each:
                ctx.commit(ck, b, 4096)

        row = {"nb": nb, "steps": a.steps}
        for name, (enqueue, sync_call) in runs.items():
            dev, base = [], []
            for step in range(a.warmup + a.steps):
                ms = timed(torch, ctx, 1, enqueue)
                ctx.wait(1)
                if step >= a.warmup:
                    dev.append(ms)
                if name == "blob_commit":  # the baseline alternates with the call it is compared with
                    ms = timed(torch, ctx, 0, baseline)
                    if step >= a.warmup:
                        base.append(ms)
            for _ in range(a.warmup):
                sync_call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                sync_call()
            wall = (time.perf_counter() - t0) * 1e3 / a.steps
            row.update(stats(name, dev, wall, nb))
            if base:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    baseline()
                row.update(stats("commit_baseline", base, (time.perf_counter() - t0) * 1e3 / a.steps, nb))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del blobs, each, zs, out, ys, cs
    lines = ["| nb | call | device ms (median) | min | p90 | per blob | wall ms per sync call |", "|" + "---|" * 7]
    for r_ in rows:
        for name in CALLS + ("commit_baseline",):
            label = name if name != "commit_baseline" else "nb x kzgmi_commit_device (baseline)"
            lines.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
                r_["nb"], label, r_[name + "_ms"], r_[name + "_min_ms"], r_[name + "_p90_ms"], r_[name + "_ms_per_blob"],
                r_[name + "_wall_ms"]))
    print("\n".join(lines))
    if not a.no_write:
        os.makedirs(a.out_dir, exist_ok=True)
        head["rows"] = rows
        with open(os.path.join(a.out_dir, "bench_blob_proofs.json"), "w") as f:
            json.dump(head, f, indent=1)
        with open(os.path.join(a.out_dir, "bench_blob_proofs.md"), "w") as f:
            f.write("EIP-4844 commitments and proofs, %d warmed calls per row (%s).  Device ms: events around the async\n"
                    "device form; wall ms: a host clock around synchronous device-form calls (tools/bench_blob_proofs.py).\n"
                    "The baseline is nb sequential kzgmi_commit_device calls over a commit key of the same points, in the\n"
                    "same run, alternating with blob_commit; its events bracket the synchronous calls, host round trips\n"
                    "included.\n\nBlob proof key: load %s ms, %d bytes on the device.\n\n"
                    % (a.steps, head["device"], ", ".join("%.1f" % v for v in loads), head["key_device_bytes"]))
            f.write("\n".join(lines) + "\n")
    del key, ck
    ctx.close()


if __name__ == "__main__":
    main()
