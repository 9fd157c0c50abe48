"""Child process of tests/test_gpu_env_forms.py for the knobs that are process-wide statics: the
staging copy's pool (KZGMI_COPY_THREADS, fixed at the first staged copy) and the queue-sharing
warning (KZGMI_QUIET, printed once per process).  The parent sets the environment.  Reports
through its exit status and one JSON line on stdout.

  gpu_env_worker.py copy    43691 compressed BLS12-381 tuples verified from pageable host memory
  gpu_env_worker.py quiet   6-slot contexts with KZGMI_QUIET set, then without it
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kzg-batch-verification-scheme_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import kzgmi  # noqa: E402

CURVE = "bls12_381"
MARK = "--- gpu_env_worker: KZGMI_QUIET unset from here ---"


def _threads():
    return len(os.listdir("/proc/self/task"))


def copy():
    n, tau = 43691, 0xC0B1
    ctx = kzgmi.Context(0, 1)
    Cm = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    P = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    z = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    y = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    ctx.gen_tuples(CURVE, tau, hashlib.sha256(b"copy-threads").digest(), n, Cm, z, y, P)
    C48 = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    P48 = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    ctx.g1_compress(CURVE, Cm, n, C48)
    ctx.g1_compress(CURVE, P, n, P48)
    srs = ctx.load_srs(CURVE, *ctx.toy_srs(CURVE, tau))
    seed = hashlib.sha256(b"copy-threads-verify").digest()
    out = {"n": n, "staged_bytes": C48.numel()}
    out["device_accepted"] = ctx.batch_verify(srs, C48, z, y, P48, seed=seed, n=n, compressed=True)
    want = ctx.last_combination(CURVE)
    # pageable host copies (numpy arrays over torch's ordinary CPU allocations)
    hC, hz, hy, hP = (t.cpu().numpy().copy() for t in (C48, z, y, P48))
    before = _threads()
    out["host_accepted"] = ctx.batch_verify(srs, hC, hz, hy, hP, seed=seed, n=n, compressed=True)
    out["new_threads"] = _threads() - before
    out["same_combination"] = ctx.last_combination(CURVE) == want
    hy[32 * (n - 1) + 31] ^= 1  # the last tuple's y
    out["flipped_rejected"] = ctx.batch_verify(srs, hC, hz, hy, hP, seed=seed, n=n, compressed=True) is False
    del srs
    ctx.close()
    ok = (out["device_accepted"] is True and out["host_accepted"] is True and out["same_combination"]
          and out["flipped_rejected"])
    return out, ok


def quiet():
    os.environ["KZGMI_QUIET"] = "1"
    kzgmi.Context(0, 6).close()
    kzgmi.Context(0, 6).close()
    sys.stderr.flush()
    sys.stderr.write(MARK + "\n")
    sys.stderr.flush()
    del os.environ["KZGMI_QUIET"]
    for _ in range(3):
        kzgmi.Context(0, 6).close()
    return {"mark": MARK}, True


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("copy", "quiet"):
        print(json.dumps({"error": "usage: gpu_env_worker.py copy|quiet"}))
        return 2
    try:
        out, ok = copy() if mode == "copy" else quiet()
    except Exception as e:  # reported to the parent, which fails on it
        print(json.dumps({"error": "%s: %s" % (type(e).__name__, e)}))
        return 1
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
