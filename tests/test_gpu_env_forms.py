"""Every form of the library that only an environment variable selects, run once on the GPU.

csrc/api.hip reads its KZGMI_* variables when a context is created (KZGMI_COPY_THREADS at the first
staged copy of the process).  The kernel layers are pinned op by op elsewhere; these tests pin that
each variable reaches the code it names and that the form it selects computes what the default form
computes: the wave-per-blob hash (KZGMI_BLOB_HASH=wave, a second SHA-256 round function), both
window widths at sizes where they are not the default (KZGMI_WBITS), the reduction on 2 and on 4
threads per segment (KZGMI_SEG4_WAVES), the split accumulation's side stream at both issue
priorities (KZGMI_SPLIT_LOWPRIO), slot streams with and without spread priorities
(KZGMI_STREAM_PRIO), and, in child processes of their own because they are process-wide, the staging
copy on 32 threads (KZGMI_COPY_THREADS) and the queue-sharing warning (KZGMI_QUIET).

Every comparison is exact: integers, encodings and verdicts against tests/blobref.py and the oracle.
"""
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import blobref as B  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_env_worker.py")
CURVES = ["bls12_381", "bn254"]
TAU = 0xE57F0435
ERR_SCALAR = -4


def _context_with_env(slots=2, **env):
    """A kzgmi.Context created with the given environment overrides (read at creation)."""
    import kzgmi
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzgmi.Context(0, slots)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(len(b) // 32)]


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


class _Inputs:
    """Generated inputs and the oracle's answers for them, each computed once per module."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._batch = {}
        self._msm = {}

    def srs_bytes(self, curve):
        C = pc.CURVES[curve]
        g2 = pk.g2_to_bytes(C.g2, C)
        return g2, O.g2_mul(curve, g2, TAU)

    def batch(self, curve, n):
        """n valid tuples on the device, the same with one y altered, the verification seed, and the
        oracle's (verdict, A, B) for both."""
        if (curve, n) not in self._batch:
            import torch
            g1b = 2 * pc.CURVES[curve].fp_bytes
            Cm = torch.empty(n * g1b, dtype=torch.uint8, device="cuda")
            P = torch.empty(n * g1b, dtype=torch.uint8, device="cuda")
            z = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            y = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            self.ctx.gen_tuples(curve, TAU, hashlib.sha256(b"env-forms%d" % n).digest(), n, Cm, z, y, P)
            ybad = y.clone()
            ybad[32 * (n // 2) + 31] ^= 1
            seed = hashlib.sha256(b"env-forms-verify%d" % n).digest()
            g2, tg2 = self.srs_bytes(curve)
            hb = [_host(t) for t in (Cm, z, y, P)]
            good = O.batch_verify(curve, hb[0], hb[1], hb[2], hb[3], n, g2, tg2, seed, want_ab=True)
            bad = O.batch_verify(curve, hb[0], hb[1], _host(ybad), hb[3], n, g2, tg2, seed, want_ab=True)
            assert good[0] is True and bad[0] is False
            self._batch[curve, n] = {"C": Cm, "z": z, "y": y, "P": P, "ybad": ybad, "seed": seed, "n": n,
                                     "good": good, "bad": bad}
        return self._batch[curve, n]

    def msm(self, curve, n):
        """n points k_i G1 and n uniform scalars on the device, and the oracle's sum."""
        if (curve, n) not in self._msm:
            import torch
            C = pc.CURVES[curve]
            rng = random.Random(1000 + n)
            ks = b"".join(pk.fr_to_bytes(rng.randrange(1, C.r)) for _ in range(n))
            sc = b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n))
            pts = torch.empty(n * 2 * C.fp_bytes, dtype=torch.uint8, device="cuda")
            self.ctx.gen_g1(curve, _dev(ks), n, pts)
            self._msm[curve, n] = (pts, _dev(sc), O.msm_g1(curve, _host(pts), sc, n))
        return self._msm[curve, n]


@pytest.fixture(scope="module")
def inputs(ctx):
    return _Inputs(ctx)


def _check_batch(c, srs, curve, b):
    """The valid batch is accepted and the altered one rejected, A and B the oracle's both times."""
    assert c.batch_verify(srs, b["C"], b["z"], b["y"], b["P"], seed=b["seed"], n=b["n"]) is True
    assert c.last_combination(curve) == (b["good"][1], b["good"][2])
    assert c.batch_verify(srs, b["C"], b["z"], b["ybad"], b["P"], seed=b["seed"], n=b["n"]) is False
    assert c.last_combination(curve) == (b["bad"][1], b["bad"][2])


# ------------------------------------------------------------------------------ KZGMI_BLOB_HASH
@pytest.fixture(scope="module")
def wave_ctx():
    c = _context_with_env(KZGMI_BLOB_HASH="wave")
    yield c
    c.close()


@pytest.fixture(scope="module")
def blob_kinds():
    rng = random.Random(0x3A7E)
    return [B.blob_from_ints([rng.randrange(B.R) for _ in range(B.N)]) for _ in range(3)] + \
        [B.blob_from_ints([0] * B.N), B.blob_from_ints([B.R - 1] * B.N)]


@pytest.mark.parametrize("n", [1, 3, 65])
def test_blob_hash_wave_challenges(ctx, wave_ctx, blob_kinds, n):
    """k_blob_challenge<true> (one wave per blob, blob_compress_uniform): random, all-zero and
    all-(r-1) blobs under distinct commitments give blobref's challenges and the lane form's bytes;
    an element equal to r anywhere is KZGMI_ERR_SCALAR."""
    import kzgmi
    rng = random.Random(n)
    # blob_kinds: 0-2 random, 3 all-zero, 4 all-(r-1); n = 1 takes one call per kind
    variants = {1: [[0], [3], [4]], 3: [[0, 3, 4]]}.get(n, [[i % 5 for i in range(n)]])
    r_be = _dev(B.R.to_bytes(32, "big"))
    for order in variants:
        blobs = [blob_kinds[k] for k in order]
        cs = [B.g1_of(rng.randrange(1, B.R)) for _ in range(n)]
        assert len(set(cs)) == n
        db, dc = _dev(b"".join(blobs)), _dev(b"".join(cs))
        got = _host(wave_ctx.blob_challenges(db, dc, n))
        assert _ints(got) == [B.blob_challenge(b, c) for b, c in zip(blobs, cs)], order
        assert got == _host(ctx.blob_challenges(db, dc, n)), order
        for blob, elem in [(0, 0), (n - 1, 4095), (n // 2, 2049)]:
            bad = db.clone()
            o = blob * B.BLOB_BYTES + 32 * elem
            bad[o:o + 32] = r_be
            with pytest.raises(kzgmi.KzgmiError) as e:
                wave_ctx.blob_challenges(bad, dc, n)
            assert e.value.code == ERR_SCALAR, (order, blob, elem)
        assert _host(wave_ctx.blob_challenges(db, dc, n)) == got  # the context still works


def test_blob_hash_wave_verify_batch(wave_ctx):
    """verify_blob_batch at n = 5 through the wave form: the valid batch is accepted; one blob
    element altered (its z and y change) and one proof replaced are rejected."""
    n, tau = 5, 0x4844_0000_0000_1235
    rng = random.Random(0xB10C)
    kinds = [[rng.randrange(B.R) for _ in range(B.N)] for _ in range(2)] + [[B.R - 1] * B.N]
    opened = [B.open_blob(v, tau) for v in kinds]
    rows = [opened[i % len(opened)] for i in range(n)]
    blobs, cs, ps = (b"".join(r[k] for r in rows) for k in (0, 1, 4))
    C = pc.CURVES[B.CURVE]
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = wave_ctx.load_srs(B.CURVE, g2, O.g2_mul(B.CURVE, g2, tau))
    db, dc, dp = _dev(blobs), _dev(cs), _dev(ps)
    assert _ints(_host(wave_ctx.blob_challenges(db, dc, n))) == [r[2] for r in rows]
    assert wave_ctx.verify_blob_batch(srs, db, dc, dp, n) is True
    bad = bytearray(blobs)
    o = 3 * B.BLOB_BYTES + 32 * 2049
    bad[o:o + 32] = ((int.from_bytes(bad[o:o + 32], "big") + 1) % B.R).to_bytes(32, "big")
    assert wave_ctx.verify_blob_batch(srs, _dev(bytes(bad)), dc, dp, n) is False
    assert wave_ctx.verify_blob_batch(srs, db, dc, _dev(ps[:48 * (n - 1)] + B.g1_of(0xC0FFEE)), n) is False
    assert wave_ctx.verify_blob_batch(srs, blobs, cs, ps, n) is True  # the host entry, same form


# ------------------------------------------------------------------------------ KZGMI_WBITS
@pytest.mark.parametrize("wbits", ["13", "16"])
@pytest.mark.parametrize("curve", CURVES)
def test_forced_window_width(inputs, curve, wbits):
    """Both window widths at sizes where the plan picks the other one (16 at n = 3000 and 3001, 13
    at a 70000-point MSM and a 40000-tuple batch), through the buckets at the small sizes too
    (KZGMI_SMALL_TERMS=0): MSMs and the batches' A, B bit-exact against the oracle."""
    c = _context_with_env(1, KZGMI_WBITS=wbits, KZGMI_SMALL_TERMS="0")
    try:
        for n in (3000, 70000):
            pts, sc, want = inputs.msm(curve, n)
            assert c.msm_g1(curve, pts, sc, n) == want, n
        srs = c.load_srs(curve, *inputs.srs_bytes(curve))
        for n in (3001, 40000):
            _check_batch(c, srs, curve, inputs.batch(curve, n))
        del srs
    finally:
        c.close()


# ------------------------------------------------------------------------------ KZGMI_SEG4_WAVES
@pytest.mark.parametrize("waves", ["0", "64"])
@pytest.mark.parametrize("curve", CURVES)
def test_reduction_threads_per_segment(inputs, curve, waves):
    """Launch::reduce on 2 threads per segment at every size (KZGMI_SEG4_WAVES=0) and on 4 up to 64
    waves per SIMD (the default 1 keeps 4 for few bucket sets only): the variable reaches the
    launcher and both give the oracle's MSM and A, B."""
    c = _context_with_env(1, KZGMI_SEG4_WAVES=waves, KZGMI_SMALL_TERMS="0")
    try:
        pts, sc, want = inputs.msm(curve, 3000)
        assert c.msm_g1(curve, pts, sc, 3000) == want
        srs = c.load_srs(curve, *inputs.srs_bytes(curve))
        _check_batch(c, srs, curve, inputs.batch(curve, 3001))
        del srs
    finally:
        c.close()


# ------------------------------------------------------------------------------ KZGMI_SPLIT_LOWPRIO
@pytest.mark.parametrize("lowprio", ["0", "1"])
@pytest.mark.parametrize("curve", CURVES)
def test_split_side_stream_issue_priority(inputs, curve, lowprio):
    """The split accumulation forced on (KZGMI_SPLIT_ACC=1) at 2^17 tuples, its side stream's
    reduction and combination kernels with (0) and without (1, the default) the tail's raised issue
    priority: A, B and both verdicts are the oracle's."""
    c = _context_with_env(1, KZGMI_SPLIT_ACC="1", KZGMI_SPLIT_LOWPRIO=lowprio)
    try:
        srs = c.load_srs(curve, *inputs.srs_bytes(curve))
        _check_batch(c, srs, curve, inputs.batch(curve, 1 << 17))
        del srs
    finally:
        c.close()


# ------------------------------------------------------------------------------ KZGMI_STREAM_PRIO
@pytest.mark.parametrize("prio", ["0", "1"])
def test_slot_stream_priorities(inputs, prio):
    """Six slots with their streams at one priority (0: they share hardware queues where those are
    fewer than seven; KZGMI_QUIET keeps the warning about it out of the log) and spread over the
    device's priority levels (1): 18 asynchronous batches of 3000 and 20000 tuples round the
    slots, every fifth one altered, each verdict as submitted and the last ones collected out of
    submission order; one shard partial mid-stream carries the oracle's A and B."""
    import torch
    curve = "bls12_381"
    c = _context_with_env(6, KZGMI_STREAM_PRIO=prio, KZGMI_QUIET="1")
    try:
        srs = c.load_srs(curve, *inputs.srs_bytes(curve))
        batches = [inputs.batch(curve, 3000), inputs.batch(curve, 20000)]
        part = torch.empty(2 * c.partial_bytes(curve), dtype=torch.uint8, device="cuda")
        pending = {}
        part_of = None

        def collect(s):
            exp = pending.pop(s)
            assert c.wait(s) is (True if exp == "partial" else exp), s

        for k in range(18):
            s = (5 * k) % 6
            if s in pending:
                collect(s)
            b = batches[k % 2]
            if k == 10:
                part_of = b
                c.batch_partial_async(srs, s, b["C"], b["z"], b["y"], b["P"], b["n"], 0, b["seed"], part)
                pending[s] = "partial"
                continue
            bad = k % 5 == 4
            c.batch_verify_async(srs, s, b["C"], b["z"], b["ybad"] if bad else b["y"], b["P"], b["n"], seed=b["seed"])
            pending[s] = not bad
        for s in sorted(pending, reverse=True):
            collect(s)
        assert c.partial_encode(curve, part, 2) == [part_of["good"][1], part_of["good"][2]]
        del srs
    finally:
        c.close()


# ------------------------------------------------------------------------------ process-wide knobs
def _run_worker(mode, **env):
    """tests/gpu_env_worker.py in a fresh process (the copy pool and the warning are process-wide
    statics): its exit status, the JSON line it printed last, its stderr."""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, WORKER, mode], env=e, capture_output=True, text=True, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.returncode, json.loads(lines[-1]), r.stderr


def test_copy_threads_32_stages_whole_arrays():
    """KZGMI_COPY_THREADS=32: 43691 compressed BLS12-381 tuples from pageable host memory.  The
    commitments and proofs are 2097168 bytes each, which 32 parts of a 64-byte multiple do not
    divide: the earlier part arithmetic left the last 16 bytes of both arrays uncopied.  Accepted,
    with the device-buffer run's combination; one flipped y rejected."""
    rc, out, err = _run_worker("copy", KZGMI_COPY_THREADS="32")
    assert out.get("error") is None, (out, err[-2000:])
    assert out["n"] == 43691 and out["staged_bytes"] == 2097168
    assert out["device_accepted"] is True
    assert out["host_accepted"] is True
    assert out["same_combination"] is True
    assert out["flipped_rejected"] is True
    assert out["new_threads"] >= 31, out  # the pool's workers: the variable reached it
    assert rc == 0


def test_quiet_silences_the_queue_sharing_warning():
    """Six slots at one stream priority on four hardware queues share queues: with KZGMI_QUIET set
    nothing is printed, without it the warning appears exactly once however many contexts follow."""
    rc, out, err = _run_worker("quiet", GPU_MAX_HW_QUEUES="4", KZGMI_STREAM_PRIO="0")
    assert out.get("error") is None, (out, err[-2000:])
    quiet, _, loud = err.partition(out["mark"])
    assert out["mark"] in err
    warning = "slots sharing a queue run one after another"
    assert quiet.count(warning) == 0, quiet[-2000:]
    assert loud.count(warning) == 1, loud[-2000:]
    assert rc == 0
