"""EIP-4844 blob batch verification on the GPU (csrc/blob.hpp) vs the pure-Python transcript of
tests/blobref.py and the C oracle's powers mode.

The evaluation kernel gives blob element j to thread j % 512 (pass j // 512, 8 passes) of a
512-thread workgroup: the in-domain points below sit on its thread, wave and pass boundaries.
The lane-per-blob hash puts blob i on lane i % 64 of wave i // 64: n = 65 spans two waves.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

import blobref as B  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402
from pointcases import non_subgroup_points  # noqa: E402

CURVE = B.CURVE
TAU = 0x4844_0000_1234_5678_9ABC_DEF1
NMAX = 65
E2E_SIZES = [1, 2, 7, 65]
# k_blob_eval's boundaries: first/last thread of a pass, wave boundaries, pass boundaries
EVAL_DOMAIN_POINTS = [0, 1, 63, 64, 511, 512, 513, 3583, 3584, 4032, 4095]


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs(ctx):
    C = pc.CURVES[CURVE]
    g2 = pk.g2_to_bytes(C.g2, C)
    return ctx.load_srs(CURVE, g2, O.g2_mul(CURVE, g2, TAU)), g2, O.g2_mul(CURVE, g2, TAU)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(len(b) // 32)]


@pytest.fixture(scope="module")
def batch():
    """NMAX valid openings (every prefix is a valid batch), computed once: three distinct random
    blobs and an all-(r-1) one, cycled.  Lists blobs, C, z, y, pi."""
    rng = random.Random(0xB10B)
    kinds = [[rng.randrange(B.R) for _ in range(B.N)] for _ in range(3)] + [[B.R - 1] * B.N]
    opened = [B.open_blob(v, TAU) for v in kinds]
    cols = [[o[k] for o in (opened[i % len(opened)] for i in range(NMAX))] for k in range(5)]
    return {"blobs": cols[0], "C": cols[1], "z": cols[2], "y": cols[3], "pi": cols[4]}


def _arrays(batch, n):
    return b"".join(batch["blobs"][:n]), b"".join(batch["C"][:n]), b"".join(batch["pi"][:n])


def test_challenges_small(ctx):
    rng = random.Random(3)
    blobs = [B.blob_from_ints([rng.randrange(B.R) for _ in range(B.N)]) for _ in range(3)]
    cs = [B.g1_of(rng.randrange(B.R)) for _ in range(3)]
    z = ctx.blob_challenges(_dev(b"".join(blobs)), _dev(b"".join(cs)), 3)
    assert _ints(_host(z)) == [B.blob_challenge(b, c) for b, c in zip(blobs, cs)]


def test_challenges_two_waves(ctx, batch):
    """65 blobs sharing content (4 distinct ones) under 65 distinct commitments."""
    rng = random.Random(4)
    cs = [B.g1_of(rng.randrange(B.R)) for _ in range(NMAX)]
    assert len(set(cs)) == NMAX
    z = ctx.blob_challenges(_dev(b"".join(batch["blobs"])), _dev(b"".join(cs)), NMAX)
    assert _ints(_host(z)) == [B.blob_challenge(b, c) for b, c in zip(batch["blobs"], cs)]


def test_eval(ctx):
    """random / all-zero / constant / all-(r-1) blobs at random z, 0, and domain points."""
    rng = random.Random(5)
    c = rng.randrange(1, B.R)
    kinds = {"random": [rng.randrange(B.R) for _ in range(B.N)], "zero": [0] * B.N, "const": [c] * B.N,
             "max": [B.R - 1] * B.N}
    points = [rng.randrange(B.R), rng.randrange(B.R), 0, B.R - 2] + [B.DOM[j] for j in EVAL_DOMAIN_POINTS]
    assert B.DOM[0] == 1 and B.DOM[1] == B.R - 1
    cases = [(k, z) for k in kinds for z in points]
    blobs = {k: B.blob_from_ints(v) for k, v in kinds.items()}
    want = [B.evaluate(kinds[k], z) for k, z in cases]
    for (k, z), y in zip(cases, want):  # the constant blob pins the (z^N - 1)/N factor
        if k == "const":
            assert y == c
        if k == "zero":
            assert y == 0
    db = _dev(b"".join(blobs[k] for k, _ in cases))
    dz = _dev(b"".join(z.to_bytes(32, "big") for _, z in cases))
    got = _ints(_host(ctx.blob_eval(db, dz, len(cases))))
    assert got == want


def test_eval_rejects_z_out_of_range(ctx):
    import kzgmi
    blob = B.blob_from_ints([1] * B.N)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.blob_eval(_dev(blob), _dev(B.R.to_bytes(32, "big")), 1)
    assert e.value.code == -4


@pytest.mark.parametrize("which,index", [(0, 0), (0, 4095), (2, 0), (2, 4095)])
def test_range_check(ctx, srs, batch, which, index):
    """An element equal to r: KZGMI_ERR_SCALAR from every entry point that reads blobs."""
    import kzgmi
    n = 3
    blobs, cs, ps = _arrays(batch, n)
    bad = bytearray(blobs)
    o = which * B.BLOB_BYTES + 32 * index
    bad[o:o + 32] = B.R.to_bytes(32, "big")
    bad = bytes(bad)
    db, dc, dp = _dev(bad), _dev(cs), _dev(ps)
    dz = _dev(b"".join(z.to_bytes(32, "big") for z in batch["z"][:n]))
    calls = [lambda: ctx.blob_challenges(db, dc, n),
             lambda: ctx.blob_eval(db, dz, n),
             lambda: ctx.verify_blob_batch(srs[0], db, dc, dp, n),
             lambda: ctx.verify_blob_batch(srs[0], bad, cs, ps, n),
             lambda: (ctx.verify_blob_batch_async(srs[0], 1, db, dc, dp, n), ctx.wait(1))]
    for call in calls:
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == -4
    assert ctx.verify_blob_batch(srs[0], _dev(blobs), dc, dp, n) is True  # the context still works


@pytest.mark.parametrize("n", [1, 2, 5])
def test_batch_challenge(ctx, batch, n):
    """32 + 160 n bytes: odd n fills its last block (a padding-only block follows), even n leaves 32 bytes."""
    cs, zs, ys, ps = batch["C"][:n], batch["z"][:n], batch["y"][:n], batch["pi"][:n]
    got = ctx.blob_batch_challenge(_dev(b"".join(cs)), _dev(b"".join(z.to_bytes(32, "big") for z in zs)),
                                   _dev(b"".join(y.to_bytes(32, "big") for y in ys)), _dev(b"".join(ps)), n)
    assert got == B.batch_challenge(cs, zs, ys, ps)


@pytest.mark.parametrize("n", E2E_SIZES)
def test_verify_device(ctx, srs, batch, n):
    s, g2, tg2 = srs
    blobs, cs, ps = _arrays(batch, n)
    db, dc, dp = _dev(blobs), _dev(cs), _dev(ps)
    zs, ys = batch["z"][:n], batch["y"][:n]
    assert _ints(_host(ctx.blob_challenges(db, dc, n))) == zs
    r = B.batch_challenge(batch["C"][:n], zs, ys, batch["pi"][:n])
    ok, A, Bc = O.batch_verify_powers(CURVE, B.decompress(batch["C"][:n]), b"".join(z.to_bytes(32, "big") for z in zs),
                                      b"".join(y.to_bytes(32, "big") for y in ys), B.decompress(batch["pi"][:n]), n,
                                      g2, tg2, r)
    assert ok is True
    assert ctx.verify_blob_batch(s, db, dc, dp, n) is True
    assert ctx.last_combination(CURVE) == (A, Bc)
    # one blob element changed to another in-range value
    bad = bytearray(blobs)
    o = (n - 1) * B.BLOB_BYTES + 32 * 2049
    bad[o:o + 32] = ((int.from_bytes(bad[o:o + 32], "big") + 1) % B.R).to_bytes(32, "big")
    assert ctx.verify_blob_batch(s, _dev(bytes(bad)), dc, dp, n) is False
    # one proof replaced by another valid G1 point
    other = B.g1_of(0xC0FFEE)
    assert ctx.verify_blob_batch(s, db, dc, _dev(ps[:48 * (n - 1)] + other), n) is False
    # two commitments swapped (of different blobs)
    if n >= 2:
        assert batch["C"][0] != batch["C"][1]
        assert ctx.verify_blob_batch(s, db, _dev(cs[48:96] + cs[:48] + cs[96:]), dp, n) is False
    assert ctx.verify_blob_batch(s, db, dc, dp, n) is True


def test_verify_point_errors_and_empty(ctx, srs, batch):
    import kzgmi
    s = srs[0]
    n = 2
    blobs, cs, ps = _arrays(batch, n)
    db, dc = _dev(blobs), _dev(cs)
    noflag = bytearray(ps)
    noflag[48] &= 0x7F  # compression bit missing
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.verify_blob_batch(s, db, dc, _dev(bytes(noflag)), n)
    assert e.value.code == -2
    off = pk.g1_to_bytes_compressed(non_subgroup_points(1)[0], pc.BLS12_381)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.verify_blob_batch(s, db, dc, _dev(ps[:48] + off), n)
    assert e.value.code == -7
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.verify_blob_batch(s, db, _dev(off + cs[48:]), _dev(ps), n)
    assert e.value.code == -7
    assert ctx.verify_blob_batch(s, db[:0], dc[:0], dc[:0], 0) is True
    assert ctx.verify_blob_batch(s, b"", b"", b"", 0) is True


def test_bn254_srs_is_rejected(ctx, batch):
    import kzgmi
    C = pc.CURVES["bn254"]
    g2 = pk.g2_to_bytes(C.g2, C)
    s = ctx.load_srs("bn254", g2, O.g2_mul("bn254", g2, 5))
    blobs, cs, ps = _arrays(batch, 1)
    for args in ((_dev(blobs), _dev(cs), _dev(ps)), (blobs, cs, ps)):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.verify_blob_batch(s, *args, 1)
        assert e.value.code == -1


def test_verify_host(ctx, srs, batch):
    """The host form equals the device form at n = 7, from pageable and from pinned buffers."""
    import numpy as np
    import kzgmi
    s = srs[0]
    n = 7
    blobs, cs, ps = _arrays(batch, n)
    assert ctx.verify_blob_batch(s, _dev(blobs), _dev(cs), _dev(ps), n) is True
    want = ctx.last_combination(CURVE)
    assert ctx.verify_blob_batch(s, blobs, cs, ps) is True
    assert ctx.last_combination(CURVE) == want
    assert kzgmi.verify_blob_batch(blobs, cs, ps, s) is True
    hb = kzgmi.HostBuffer(len(blobs) + 2 * 48 * n)
    try:
        hb.array[:] = np.frombuffer(blobs + cs + ps, dtype=np.uint8)
        views = (hb.view(0, len(blobs)), hb.view(len(blobs), 48 * n), hb.view(len(blobs) + 48 * n, 48 * n))
        assert ctx.verify_blob_batch(s, *views, n) is True
        assert ctx.last_combination(CURVE) == want
        hb.array[32 * 5 + 31] ^= 1  # blob 0, element 5 (r - 1 would wrap: the low bit keeps it in range)
        assert ctx.verify_blob_batch(s, *views, n) is False
        del views
    finally:
        hb.free()
    bad = bytearray(blobs)
    bad[32 * 5 + 31] ^= 1
    assert ctx.verify_blob_batch(s, bytes(bad), cs, ps) is False


def test_verify_async_two_slots(ctx, srs, batch):
    s = srs[0]
    n = 7
    blobs, cs, ps = _arrays(batch, n)
    bad = bytearray(blobs)
    bad[2 * B.BLOB_BYTES + 32 * 100 + 31] ^= 1  # blob 2: a random one (an in-range change)
    db, dbad, dc, dp = _dev(blobs), _dev(bytes(bad)), _dev(cs), _dev(ps)
    ctx.verify_blob_batch_async(s, 0, db, dc, dp, n)
    ctx.verify_blob_batch_async(s, 1, dbad, dc, dp, n)
    assert ctx.wait(1) is False
    assert ctx.wait(0) is True
    ctx.verify_blob_batch_async(s, 0, dbad, dc, dp, n)
    ctx.verify_blob_batch_async(s, 1, db, dc, dp, n)
    assert ctx.wait(0) is False
    assert ctx.wait(1) is True
