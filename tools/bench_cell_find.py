"""Timing of the search for a rejected EIP-7594 cell batch's invalid cells (csrc/host_find.hip) and of
its parts.

  * the search at n = 9 216 cells (128 columns x 72 blobs) and at n = 65 536, the most one call takes,
    with 1 and with 16 scattered invalid cells, each beside one verify_cell_batch of the same
    device-resident inputs, measured in the same process (with r derived on the device, which is one
    sequential hash over the batch, and with r given by the caller), and beside what n single-cell verifies would
    take: ONE single-cell verify is timed and multiplied by n, an extrapolation, not a measurement;
  * the coefficient stage alone (Context.cell_coeffs: k_cell_z, k_cell_coeffs and its big-endian
    output, with the call's host round trip) at both sizes;
  * level 0 alone at both sizes (Context.cell_range_partials over the level's `fanout` parts: the cell
    front end, k_cell_range_fold and the tail-64 grouped kernel, no pairing).

Every call is synchronous and includes its host round trips, so every time is wall-clock around the
call with the device idle before it; medians over --reps warmed calls.  --once N runs one warmed search
of N cells with one invalid cell and nothing else: the run to put under a kernel trace for per-kernel
times.

The cells are valid openings made on the CPU from the toy secret (tests/cellref.py): 8 polynomials of
degree 4095 on all 128 cosets, cell k = (polynomial (k // 128) % 8, coset k % 128), so m = 8 unique
commitments; a cell is made invalid by adding 1 to one of its elements.

    python tools/bench_cell_find.py [--reps 5] [--sizes 9216,65536] [--out-dir profiles/find]
"""
import argparse
import hashlib
import json
import os
import random
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kzg-batch-verification-scheme_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAU = 0x7594BE7C00001234
SEED = hashlib.sha256(b"bench-cell-find").digest()
R_GIVEN = int.from_bytes(hashlib.sha256(b"bench-cell-find-r").digest(), "big") >> 2  # a caller-supplied challenge < r
POLYS = 8


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
    ap.add_argument("--sizes", default="9216,65536")
    ap.add_argument("--once", type=int, default=0, help="one warmed search of this many cells, nothing else")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "find"))
    a = ap.parse_args()
    import torch
    import kzgmi
    import cellref as K
    import findprobe

    ctx = kzgmi.Context(0, 1)
    srs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
    tune = findprobe.tuning()
    pb = ctx.partial_bytes(K.CURVE)
    rng = random.Random(7594)
    polys = [[rng.randrange(K.R) for _ in range(K.BLOB_N)] for _ in range(POLYS)]
    commitments = b"".join(K.commit(p, TAU) for p in polys)
    opened = [[K.open_cell(p, i, TAU) for i in range(K.NUM_CELLS)] for p in polys]

    def dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    def gen(n, bad):
        cidx = [(k // K.NUM_CELLS) % POLYS for k in range(n)]
        cell = [k % K.NUM_CELLS for k in range(n)]
        cells = bytearray(b"".join(opened[c][i][0] for c, i in zip(cidx, cell)))
        for k in bad:  # element 41 + 1 (mod r)
            o = k * K.CELL_BYTES + 32 * 41
            cells[o:o + 32] = ((int.from_bytes(cells[o:o + 32], "big") + 1) % K.R).to_bytes(32, "big")
        proofs = b"".join(opened[c][i][1] for c, i in zip(cidx, cell))
        u64 = lambda xs: struct.pack("<%dQ" % len(xs), *xs)  # noqa: E731
        return dev(commitments), dev(u64(cidx)), dev(u64(cell)), dev(bytes(cells)), dev(proofs)

    if a.once:
        n = a.once
        bad = [n // 3]
        d = gen(n, bad)
        for _ in range(2):
            assert ctx.cell_batch_find_invalid(srs, *d, m=POLYS, n=n, seed=SEED) == (bad, False)
        print(json.dumps({"n": n, "stats": ctx.find_invalid_stats()}))
        ctx.close()
        return

    res = {"device": torch.cuda.get_device_name(0), "tuning": tune, "reps": a.reps, "search": [], "stages": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        for nbad in (1, 16):
            bad = sorted({(n // 3 + k * (n // 16 + 1)) % n for k in range(nbad)})
            d = gen(n, bad)
            find = lambda: ctx.cell_batch_find_invalid(srs, *d, m=POLYS, n=n, seed=SEED, max_bad=64)  # noqa: E731
            got = find()
            assert got == (bad, False), got
            st = ctx.find_invalid_stats()
            ms, lo = wall(torch, find, a.reps, a.warmup)
            assert ctx.verify_cell_batch(srs, *d, m=POLYS, n=n) is False
            # r derived on the device: one sequential SHA-256 over the batch, 33 compressions per cell
            vms, _ = wall(torch, lambda: ctx.verify_cell_batch(srs, *d, m=POLYS, n=n), a.reps, a.warmup)
            # r supplied by the caller: the verification without the transcript hash
            assert ctx.verify_cell_batch(srs, *d, m=POLYS, n=n, r=R_GIVEN) is False
            rms, _ = wall(torch, lambda: ctx.verify_cell_batch(srs, *d, m=POLYS, n=n, r=R_GIVEN), a.reps, a.warmup)
            one = (d[0], d[1][:8], d[2][:8], d[3][:K.CELL_BYTES], d[4][:48])
            sms, _ = wall(torch, lambda: ctx.verify_cell_batch(srs, *one, m=POLYS, n=1), a.reps, a.warmup)
            row = {"n": n, "invalid": nbad, "search_ms": ms, "search_min_ms": lo, "verify_ms": vms, "verify_given_r_ms": rms,
                   "single_verify_ms": sms, "n_single_verifies_ms_extrapolated": sms * n, "stats": st}
            res["search"].append(row)
            print(json.dumps(row), flush=True)
        # ---- the stages alone, on the last batch of this size
        out = torch.empty(n * K.CELL_BYTES, dtype=torch.uint8, device="cuda")
        cms, _ = wall(torch, lambda: ctx.cell_coeffs(d[2], d[3], n, out=out), a.reps, a.warmup)
        parts = findprobe.split(0, n, tune["fanout"])
        rec = torch.empty(2 * len(parts) * pb, dtype=torch.uint8, device="cuda")
        lms, _ = wall(torch, lambda: ctx.cell_range_partials(srs, *d, POLYS, n, 0, SEED, parts, rec), a.reps, a.warmup)
        row = {"n": n, "cell_coeffs_ms": cms, "level0_parts": len(parts),
               "level0_wave_terms": sum(3 * (hi - lo) + 64 for lo, hi in parts), "level0_partials_ms": lms}
        res["stages"].append(row)
        print(json.dumps(row), flush=True)
        del d, out, rec

    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "bench_cell_find.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = ["Milliseconds, wall-clock medians of %d warmed synchronous calls (%s); every level grouped at fanout %d. "
             "\"n single verifies\" is ONE timed single-cell verify_cell_batch times n: an extrapolation."
             % (a.reps, res["device"], tune["fanout"]), "",
             "| n cells | invalid | search | one verify_cell_batch, r derived | one verify_cell_batch, r given "
             "| search / verify (r given) | n single verifies (extrapolated) | levels | wave-terms | pairings |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["search"]:
        s = r["stats"]
        lines.append("| %d | %d | %.2f | %.2f | %.2f | %.1f | %.0f | %d | %d | %d |"
                     % (r["n"], r["invalid"], r["search_ms"], r["verify_ms"], r["verify_given_r_ms"],
                        r["search_ms"] / r["verify_given_r_ms"], r["n_single_verifies_ms_extrapolated"], s["levels"],
                        s["wave_terms"], s["pairings"]))
    lines += ["", "| n cells | cell_coeffs call (k_cell_z + k_cell_coeffs, host round trip included) | level 0: parts "
              "| wave-terms | cell_range_partials call (front end + fold + tail-64 kernel) | us per wave-term |",
              "|---|---|---|---|---|---|"]
    for r in res["stages"]:
        lines.append("| %d | %.3f | %d | %d | %.2f | %.3f |"
                     % (r["n"], r["cell_coeffs_ms"], r["level0_parts"], r["level0_wave_terms"], r["level0_partials_ms"],
                        1e3 * r["level0_partials_ms"] / r["level0_wave_terms"]))
    with open(os.path.join(a.out_dir, "bench_cell_find.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
