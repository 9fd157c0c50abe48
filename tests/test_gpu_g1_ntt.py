"""Power-of-two transforms over G1 (kzgmi_g1_ntt*) against the oracle: inputs are k_i G from the oracle's
g1_mul_gen, the expectation is g1_mul_gen of the model's transform of the k_i (tests/g1nttref.py),
byte-exact.  Every case runs under the shipped choice of stage form and under each form forced
(KZGMI_G1NTT_FORM=thread|wave, read when the context is created).

Named boundaries of csrc/g1ntt.hpp crossed here: G1NTT_THREADS = 64 butterflies per workgroup of a stage
(63, 64, 65 butterflies), the 256 threads per workgroup of the gathers (254, 256, 258 points), and the
bounds G1NTT_MAX_LOGN = 20 and count * n <= 2^20 (one above each, as errors), and G1NTT_WAVE_MAX_BFLY = 2^14
butterflies per stage, up to which the shipped choice is the wave form (2^14 - 1, 2^14, 2^14 + 1).
"""
import functools
import os
import random

import pytest

pytestmark = pytest.mark.gpu

import g1nttref as G  # noqa: E402
import nttref as N  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
INV, REV = G.INVERSE, G.BITREV
ALL_FLAGS = [0, INV, REV, INV | REV]
POOL = 4096
ERR_ARG, ERR_ENCODING, ERR_NOT_ON_CURVE = -1, -2, -3


def _context(form):
    import kzgmi
    if form:
        os.environ["KZGMI_G1NTT_FORM"] = form
    try:
        return kzgmi.Context(0, 2)
    finally:
        os.environ.pop("KZGMI_G1NTT_FORM", None)


@pytest.fixture(scope="module", params=[None, "thread", "wave"], ids=["auto", "thread", "wave"])
def ctx(request):
    c = _context(request.param)
    yield c
    c.close()


_POOL = {}


def _pool(curve):
    """(scalars, encodings) of POOL random points, computed once"""
    if curve not in _POOL:
        r = pc.CURVES[curve].r
        rng = random.Random(500 + len(curve))
        ks = [rng.randrange(1, r) for _ in range(POOL)]
        _POOL[curve] = (ks, _gen(curve, ks))
    return _POOL[curve]


def _gb(curve):
    return 2 * pc.CURVES[curve].fp_bytes


@functools.lru_cache(maxsize=None)
def _gen_cached(curve, ks):
    return O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), len(ks)) if ks else b""


def _gen(curve, ks):
    """k G for every k, computed once per list (the three contexts ask for the same expectations)"""
    return _gen_cached(curve, tuple(ks))


def _points(curve, idx):
    """pool points by index; None: the point at infinity"""
    ks, enc = _pool(curve)
    gb = _gb(curve)
    inf = pk.g1_to_bytes(None, pc.CURVES[curve])
    return [0 if i is None else ks[i] for i in idx], b"".join(inf if i is None else enc[i * gb:(i + 1) * gb] for i in idx)


def _model(curve, ks, logn, count, flags):
    C = pc.CURVES[curve]
    n = 1 << logn
    out = []
    for t in range(count):
        out += G.transform_staged(ks[t * n:(t + 1) * n], logn, C.r, N.GENERATOR[curve], flags)
    return out


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _run(ctx, curve, enc, logn, count, flags):
    return ctx.g1_ntt(curve, enc, logn=logn, count=count, inverse=bool(flags & INV), bitrev=bool(flags & REV))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", range(0, 10))
def test_sizes_against_oracle(ctx, curve, logn):
    n = 1 << logn
    ks, enc = _points(curve, range(n))
    for flags in ALL_FLAGS:
        want = _gen(curve, _model(curve, ks, logn, 1, flags))
        assert _run(ctx, curve, enc, logn, 1, flags) == want, (logn, flags)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("flags", [0, INV | REV])
def test_several_workgroups_per_stage(ctx, curve, flags):
    logn = 12
    ks, enc = _points(curve, range(1 << logn))
    got = _host(_run(ctx, curve, _dev(enc), logn, 1, flags))
    assert got == _gen(curve, _model(curve, ks, logn, 1, flags))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("count", [63, 64, 65, 127, 128, 129])
def test_workgroup_boundaries(ctx, curve, count):
    """logn = 1: `count` butterflies in one stage, 2 count points in the gathers"""
    ks, enc = _points(curve, range(2 * count))
    for flags in (0, INV):
        assert _run(ctx, curve, enc, 1, count, flags) == _gen(curve, _model(curve, ks, 1, count, flags)), flags


@pytest.mark.parametrize("curve", CURVES)
def test_form_threshold(curve):
    """one below, at and above the butterflies up to which a stage takes the wave form: the shipped choice
    and both forced forms agree byte for byte (each form is held to the oracle by the other tests).  This
    checks results on both sides of the documented count; it does not pin G1NTT_WAVE_MAX_BFLY to 2^14, and
    would pass as well if the shipped choice switched elsewhere: the forms compute the same."""
    import torch
    gb = _gb(curve)
    top = (1 << 14) + 1
    ctxs = [_context(f) for f in (None, "thread", "wave")]
    try:
        vals = torch.randint(0, 256, (2 * top, 32), dtype=torch.uint8, device="cuda")
        vals[:, 0] &= 0x1F
        pts = torch.empty(2 * top * gb, dtype=torch.uint8, device="cuda")
        ctxs[0].gen_g1(curve, vals.reshape(-1), 2 * top, pts)
        for count in (top - 2, top - 1, top):  # logn = 1: `count` butterflies
            outs = [c.g1_ntt(curve, pts[:2 * count * gb], logn=1, count=count) for c in ctxs]
            assert not torch.equal(outs[0], pts[:2 * count * gb])
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), count
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [3, 6])
def test_exceptional_inputs(ctx, curve, logn):
    n = 1 << logn
    cases = {
        "equal": [7] * n,                                   # first-stage differences infinite, sums doublings
        "infinity": [None] * n,
        "single": [None] * 5 + [9] + [None] * (n - 6),
    }
    for name, idx in cases.items():
        ks, enc = _points(curve, idx)
        for flags in ALL_FLAGS:
            assert _run(ctx, curve, enc, logn, 1, flags) == _gen(curve, _model(curve, ks, logn, 1, flags)), (name, flags)
    # in[i + n/2] = -in[i]: every first-stage sum is infinity
    r = pc.CURVES[curve].r
    ks = _pool(curve)[0][:n // 2]
    ks = ks + [(-k) % r for k in ks]
    enc = _gen(curve, ks)
    for flags in ALL_FLAGS:
        assert _run(ctx, curve, enc, logn, 1, flags) == _gen(curve, _model(curve, ks, logn, 1, flags)), flags


@pytest.mark.parametrize("curve", CURVES)
def test_batches_forms_and_slots(ctx, curve):
    """count > 1 with n below a workgroup's 64 butterflies; in place; host = device = async; two jobs in flight"""
    logn, count = 3, 5
    gb, total = _gb(curve), 5 << 3
    ks, enc = _points(curve, range(100, 100 + total))
    for flags in ALL_FLAGS:
        want = _gen(curve, _model(curve, ks, logn, count, flags))
        assert _run(ctx, curve, enc, logn, count, flags) == want
        assert _host(_run(ctx, curve, _dev(enc), logn, count, flags)) == want
        d = _dev(enc)
        out = ctx.g1_ntt(curve, d, logn=logn, count=count, inverse=bool(flags & INV), bitrev=bool(flags & REV), out=d)
        assert out is d and _host(d) == want  # in place
    ks2, enc2 = _points(curve, range(300, 300 + total))
    a, b = _dev(enc), _dev(enc2)
    oa = ctx.g1_ntt_async(0, curve, a, logn, count)
    ob = ctx.g1_ntt_async(1, curve, b, logn, count, inverse=True, out=_dev(bytes(total * gb)))
    assert ctx.wait(1) and ctx.wait(0)
    assert _host(oa) == _gen(curve, _model(curve, ks, logn, count, 0))
    assert _host(ob) == _gen(curve, _model(curve, ks2, logn, count, INV))
    assert ctx.g1_ntt(curve, b"", logn=4, count=0) == b""


@pytest.mark.parametrize("curve", CURVES)
def test_inverse_of_forward(ctx, curve):
    logn, count = 5, 3
    _, enc = _points(curve, range(count << logn))
    for rev in (False, True):
        f = ctx.g1_ntt(curve, enc, logn=logn, count=count, bitrev=rev)
        assert f != enc
        assert ctx.g1_ntt(curve, f, logn=logn, count=count, inverse=True, bitrev=rev) == enc


@pytest.mark.parametrize("inverse", [False, True])
def test_equals_the_cell_transform(ctx, inverse):
    _, enc = _points("bls12_381", range(2 * 128))
    d = _dev(enc)
    want = _host(ctx.g1_fft128(d, 2, inverse=inverse))
    assert _host(ctx.g1_ntt("bls12_381", d, logn=7, count=2, inverse=inverse)) == want


@pytest.mark.parametrize("curve", CURVES)
def test_logn_16(ctx, curve):
    """a single non-infinite input at index 1 (out[j] = [w^j] P), and random input made by the library's
    generator: 64 sampled outputs against the oracle, and the round trip"""
    import torch
    C = pc.CURVES[curve]
    logn, n, gb = 16, 1 << 16, _gb(curve)
    rng = random.Random(16)
    sample = [0, 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(60)]
    w = N.root(C.r, N.GENERATOR[curve], logn)
    ks, enc = _pool(curve)
    inf = pk.g1_to_bytes(None, C)
    single = inf + enc[:gb] + inf * (n - 2)
    got = _host(ctx.g1_ntt(curve, _dev(single), logn=logn))
    want = _gen(curve, [ks[0] * pow(w, j, C.r) % C.r for j in sample])
    assert b"".join(got[j * gb:(j + 1) * gb] for j in sample) == want
    vals = [rng.randrange(C.r) for _ in range(n)]
    pts = torch.empty(n * gb, dtype=torch.uint8, device="cuda")
    ctx.gen_g1(curve, _dev(b"".join(pk.fr_to_bytes(v) for v in vals)), n, pts)
    f = ctx.g1_ntt(curve, pts, logn=logn, bitrev=True)
    model = G.transform(vals, logn, C.r, N.GENERATOR[curve], REV)
    got = _host(f)
    assert b"".join(got[j * gb:(j + 1) * gb] for j in sample) == _gen(curve, [model[j] for j in sample])
    back = ctx.g1_ntt(curve, f, logn=logn, inverse=True, bitrev=True)
    assert torch.equal(back, pts)


@pytest.mark.parametrize("curve", CURVES)
def test_errors_leave_outputs_and_slot(ctx, curve):
    import kzgmi
    import torch
    C = pc.CURVES[curve]
    gb, logn, n = _gb(curve), 3, 8
    ks, enc = _points(curve, range(n))
    fill = bytes([0xA5]) * (n * gb)

    def expect(code, pts, **kw):
        out = _dev(fill)
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.g1_ntt(curve, pts, out=out, **kw)
        assert e.value.code == code, kw
        assert _host(out) == fill

    bad = bytearray(enc)
    bad[3 * gb:3 * gb + C.fp_bytes] = b"\xff" * C.fp_bytes  # x >= p
    expect(ERR_ENCODING, _dev(bytes(bad)), logn=logn)
    off = bytearray(enc)
    off[5 * gb - 1] ^= 1  # y changed: off the curve
    expect(ERR_NOT_ON_CURVE, _dev(bytes(off)), logn=logn)
    d = _dev(enc)
    # (the bounds are checked before any array is read: the raw entry point on the small arrays)
    for lg, count, flags in ((21, 1, 0), (10, 1025, 0), (20, 2, 0), (logn, 1, 4), (logn, 1, 0x80000000)):
        out = _dev(fill)
        rc = kzgmi.lib().kzgmi_g1_ntt_device(ctx.handle, kzgmi.CURVES[curve], d.data_ptr(), lg, count, flags, out.data_ptr())
        assert rc == ERR_ARG and _host(out) == fill, (lg, count, flags)
    big = torch.zeros(2 * n * gb, dtype=torch.uint8, device="cuda")
    big[:n * gb] = d
    with pytest.raises(kzgmi.KzgmiError) as e:  # partial overlap
        ctx.g1_ntt(curve, big[:n * gb], logn=logn, out=big[16:16 + n * gb])
    assert e.value.code == ERR_ARG
    # an async job that fails on the device reports at the wait, writes nothing, and leaves the slot usable
    out = _dev(fill)
    ctx.g1_ntt_async(1, curve, _dev(bytes(off)), logn, out=out)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.wait(1)
    assert e.value.code == ERR_NOT_ON_CURVE and _host(out) == fill
    ctx.g1_ntt_async(1, curve, d, logn, out=out)
    assert ctx.wait(1)
    assert _host(out) == _gen(curve, _model(curve, ks, logn, 1, 0))
    before = kzgmi.alloc_count()
    ctx.g1_ntt_async(1, curve, d, logn, out=out)
    assert ctx.wait(1) and kzgmi.alloc_count() == before
