"""The accumulation with its subtractions folded into the Montgomery products (csrc/msm.hpp
acc_loop29 and x29_add on field29.hpp's mulsub29 / sqrsub3_29), end to end: whole batch
verifications on the bucket path against the C oracle, byte for byte in A, B and the verdict.

Shapes: n = 2048 tuples (the bucket path needs more than 4096 terms; small calls take
k_small_msm) and a ragged n = 1500, both curves.  Half of every batch repeats two tuples and
their negatives -- (-C, z, -y, -pi) opens the negated polynomial, so it is as valid as (C, z, y,
pi) -- so that buckets hold the same point twice (the doubling branch) and a point with its
negative (the running sum returns to infinity) right after a fused P and R.  One corrupted tuple
must be rejected.  Each batch runs through the default context and through one whose work queue
cuts the sorted entries into 4-entry chunks (KZGMI_ACC_QUEUE_MIN), so that most buckets of two
or more entries are cut into pieces and k_fixup joins them with x29_add."""
import hashlib
import os

import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
SIZES = [2048, 1500]
SMALL_CHUNKS = dict(KZGMI_ACC_THREADS="256", KZGMI_ACC_QUEUE="128", KZGMI_ACC_QUEUE_FROM="0", KZGMI_ACC_QUEUE_MIN="4")


def _context(env):
    import kzgmi
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzgmi.Context(0, 1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def contexts():
    cs = {"default": _context({}), "small_chunks": _context(SMALL_CHUNKS)}
    yield cs
    for c in cs.values():
        c.close()


_batches = {}


def _batch(ctx, curve, n):
    """(C, z, y, pi, g2, tau g2, seed, oracle's (ok, A, B), ys with one tuple corrupted), made once."""
    if (curve, n) in _batches:
        return _batches[curve, n]
    import torch
    C = pc.CURVES[curve]
    g1b, tau = 2 * C.fp_bytes, 777 + n
    seed = hashlib.sha256(b"fused accumulate %d" % n).digest()
    bufs = [torch.empty(n * w, dtype=torch.uint8, device="cuda") for w in (g1b, 32, 32, g1b)]
    ctx.gen_tuples(curve, tau, seed, n, *bufs)
    Cm, z, y, Pi = (bytearray(t.cpu().numpy().tobytes()) for t in bufs)

    def neg_pt(b):
        return pk.g1_to_bytes(pc.g1_neg(pk.g1_from_bytes(bytes(b), C), C), C)

    def neg_fr(b):
        return pk.fr_to_bytes((C.r - pk.fr_from_bytes(bytes(b), C)) % C.r)

    # the second half: tuples 0 and 1 and their negatives, in turn
    var = []
    for j in (0, 1):
        t = (Cm[j * g1b:(j + 1) * g1b], z[j * 32:(j + 1) * 32], y[j * 32:(j + 1) * 32], Pi[j * g1b:(j + 1) * g1b])
        var += [t, (neg_pt(t[0]), t[1], neg_fr(t[2]), neg_pt(t[3]))]
    for i in range(n // 2, n):
        c, zz, yy, p = var[(i * 7 + i // 5) % 4]
        Cm[i * g1b:(i + 1) * g1b], z[i * 32:(i + 1) * 32] = c, zz
        y[i * 32:(i + 1) * 32], Pi[i * g1b:(i + 1) * g1b] = yy, p
    Cm, z, y, Pi = bytes(Cm), bytes(z), bytes(y), bytes(Pi)
    g2 = pk.g2_to_bytes(C.g2, C)
    tg2 = O.g2_mul(curve, g2, tau)
    want = O.batch_verify(curve, Cm, z, y, Pi, n, g2, tg2, seed, want_ab=True)
    k = n // 2 + 3  # one of the repeated tuples, its y off by one
    ybad = bytearray(y)
    ybad[k * 32:(k + 1) * 32] = pk.fr_to_bytes((pk.fr_from_bytes(y[k * 32:(k + 1) * 32], C) + 1) % C.r)
    ybad = bytes(ybad)
    want_bad = O.batch_verify(curve, Cm, z, ybad, Pi, n, g2, tg2, seed, want_ab=True)
    _batches[curve, n] = (Cm, z, y, Pi, g2, tg2, seed, want, ybad, want_bad)
    return _batches[curve, n]


@pytest.mark.parametrize("path", ["default", "small_chunks"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_batch_matches_oracle(contexts, curve, n, path):
    Cm, z, y, Pi, g2, tg2, seed, want, ybad, want_bad = _batch(contexts["default"], curve, n)
    assert want[0] is True and want_bad[0] is False
    c = contexts[path]
    srs = c.load_srs(curve, g2, tg2)
    ok = c.batch_verify(srs, Cm, z, y, Pi, seed=seed, n=n)
    assert (ok,) + tuple(c.last_combination(curve)) == tuple(want)
    bad = c.batch_verify(srs, Cm, z, ybad, Pi, seed=seed, n=n)
    assert (bad,) + tuple(c.last_combination(curve)) == tuple(want_bad)
