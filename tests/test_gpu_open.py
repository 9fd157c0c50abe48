"""KZG opening proofs over a commit key (kzgmi_open*) against the oracle: for a key of 300 powers of
a toy tau, proofs equal the oracle's MSM of the model's quotient (tests/openref.py) over the powers
and [q(tau)]_1, evaluations equal p(z); host, device and async forms agree; the GPU batch verifier
accepts the openings; errors leave the outputs untouched and the slot usable.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

import openref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988  # the toy tau of test_gpu_commit.py
N = 300


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


_POWERS = {}


def _powers(curve):
    if curve not in _POWERS:
        C = pc.CURVES[curve]
        sc, x = [], 1
        for _ in range(N):
            sc.append(pk.fr_to_bytes(x))
            x = x * TAU % C.r
        _POWERS[curve] = O.g1_mul_gen(curve, b"".join(sc), N)
    return _POWERS[curve]


@pytest.fixture(scope="module")
def keys(ctx):
    return {curve: ctx.load_commit_key(curve, _powers(curve)) for curve in CURVES}


def _fr(vals):
    return b"".join(pk.fr_to_bytes(v) for v in vals)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b or bytes(32)), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _want(curve, coeffs, zs):
    """(proofs, ys) from the model's quotients: the oracle's MSM over the powers"""
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    proofs, ys = [], []
    for z in zs:
        y, q = R.divide(coeffs, z, C.r)
        ys.append(y)
        proofs.append(O.msm_g1(curve, _powers(curve)[:len(q) * g1b], _fr(q), len(q)) if q else pk.g1_to_bytes(None, C))
    return b"".join(proofs), _fr(ys)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [0, 1, 2, 17, 299, 300])
def test_open_matches_oracle(ctx, keys, curve, m):
    C = pc.CURVES[curve]
    rng = random.Random(40 + m)
    coeffs = [rng.randrange(C.r) for _ in range(m)]
    zs = [rng.randrange(C.r) for _ in range(4)]
    want_p, want_y = _want(curve, coeffs, zs)
    # host form
    proofs, ys = ctx.open(keys[curve], _fr(coeffs), _fr(zs), m=m, k=4)
    assert ys == want_y == _fr([R.evaluate(coeffs, z, C.r) for z in zs])
    assert proofs == want_p
    # [q_j(tau)]_1
    for j, z in enumerate(zs):
        q_tau = R.evaluate(R.divide(coeffs, z, C.r)[1], TAU, C.r)
        g1b = 2 * C.fp_bytes
        assert proofs[j * g1b:(j + 1) * g1b] == O.g1_mul_gen(curve, pk.fr_to_bytes(q_tau), 1), (m, j)
    # device form
    d_p, d_y = ctx.open(keys[curve], _dev(_fr(coeffs)), _dev(_fr(zs)), m=m, k=4)
    assert _host(d_p) == proofs and _host(d_y) == ys


@pytest.mark.parametrize("curve", CURVES)
def test_open_repeated_points(ctx, keys, curve):
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    rng = random.Random(41)
    coeffs = [rng.randrange(C.r) for _ in range(64)]
    a, b = rng.randrange(C.r), rng.randrange(C.r)
    proofs, ys = ctx.open(keys[curve], _fr(coeffs), _fr([a, b, a, a]))
    cut = lambda x, w: [x[i:i + w] for i in range(0, len(x), w)]  # noqa: E731
    p, y = cut(proofs, g1b), cut(ys, 32)
    assert p[0] == p[2] == p[3] != p[1] and y[0] == y[2] == y[3] != y[1]
    assert (proofs, ys) == _want(curve, coeffs, [a, b, a, a])


@pytest.mark.parametrize("curve", CURVES)
def test_open_round_trip_with_the_verifier(ctx, keys, curve):
    """commit p, open it at 8 points, and the GPU batch verifier accepts the 8 tuples"""
    C = pc.CURVES[curve]
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(curve, g2, O.g2_mul(curve, g2, TAU))
    rng = random.Random(42)
    coeffs = [rng.randrange(C.r) for _ in range(128)]
    zs = [rng.randrange(C.r) for _ in range(8)]
    cm = ctx.commit(keys[curve], _fr(coeffs))
    proofs, ys = ctx.open(keys[curve], _fr(coeffs), _fr(zs))
    assert ctx.batch_verify(srs, cm * 8, _fr(zs), ys, proofs, seed=bytes(32)) is True
    y3 = (int.from_bytes(ys[96:128], "big") + 1) % C.r
    bad = ys[:96] + pk.fr_to_bytes(y3) + ys[128:]
    assert ctx.batch_verify(srs, cm * 8, _fr(zs), bad, proofs, seed=bytes(32)) is False


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("first", [0, 1])
def test_open_async_slots(ctx, keys, curve, first):
    """two opens in flight on slots 0 and 1, waited for in either order"""
    import torch
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    rng = random.Random(43)
    jobs = []
    for slot, (m, k) in enumerate([(300, 3), (37, 5)]):
        coeffs = [rng.randrange(C.r) for _ in range(m)]
        zs = [rng.randrange(C.r) for _ in range(k)]
        outs = (torch.zeros(32 * k, dtype=torch.uint8, device="cuda"), torch.zeros(g1b * k, dtype=torch.uint8, device="cuda"))
        jobs.append((_dev(_fr(coeffs)), _dev(_fr(zs)), m, k, outs, _want(curve, coeffs, zs)))
    for slot, (dc, dz, m, k, (ys, out), _) in enumerate(jobs):
        ctx.open_async(keys[curve], slot, dc, dz, m, k, ys, out)
    for slot in (first, 1 - first):
        assert ctx.wait(slot) is True
        _, _, _, _, (ys, out), (want_p, want_y) = jobs[slot]
        assert _host(out) == want_p and _host(ys) == want_y


@pytest.mark.parametrize("curve", CURVES)
def test_open_in_several_groups(curve, monkeypatch):
    """KZGMI_OPEN_GROUP = 700 scalars: 299-coefficient quotients go two per group, 5 points in 3 groups"""
    import kzgmi
    for name, value in {"KZGMI_OPEN_GROUP": "700"}.items():  # read when the context is created
        monkeypatch.setenv(name, value)
    c = kzgmi.Context(0, 1)
    try:
        C = pc.CURVES[curve]
        ck = c.load_commit_key(curve, _powers(curve))
        rng = random.Random(44)
        coeffs = [rng.randrange(C.r) for _ in range(300)]
        zs = [rng.randrange(C.r) for _ in range(5)]
        assert c.open(ck, _fr(coeffs), _fr(zs)) == _want(curve, coeffs, zs)
        d_p, d_y = c.open(ck, _dev(_fr(coeffs)), _dev(_fr(zs)))
        assert (_host(d_p), _host(d_y)) == _want(curve, coeffs, zs)
        # the diagnostic entry takes the same groups
        ys, q = c.open_quotient(curve, _dev(_fr(coeffs)), 300, _dev(_fr(zs)), 5)
        res = [R.divide(coeffs, z, C.r) for z in zs]
        assert _host(ys) == _fr([y for y, _ in res]) and _host(q) == b"".join(_fr(qq) for _, qq in res)
        del ck
    finally:
        c.close()


@pytest.mark.parametrize("curve", CURVES)
def test_open_errors(ctx, keys, curve):
    import torch
    import kzgmi
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    ck = keys[curve]
    rng = random.Random(45)
    coeffs = [rng.randrange(C.r) for _ in range(50)]
    zs = [rng.randrange(C.r) for _ in range(4)]
    want = _want(curve, coeffs, zs)
    d_c, d_z = _dev(_fr(coeffs)), _dev(_fr(zs))
    ys = torch.full((32 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((g1b * 4,), 0xA5, dtype=torch.uint8, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return _host(ys) == b"\xa5" * 128 and _host(out) == b"\xa5" * (4 * g1b)

    def refused(code, call):
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == code
        assert untouched()
        # a following open on the same slot is correct
        p2, y2 = ctx.open(ck, d_c, d_z)
        assert (_host(p2), _host(y2)) == want

    big = _dev(_fr([1] * (N + 1)))
    refused(-1, lambda: ctx.open(ck, big, d_z, m=N + 1, k=4, ys_out=ys, out=out))  # m > n
    many = torch.zeros(32 * 4097, dtype=torch.uint8, device="cuda")
    refused(-1, lambda: ctx.open(ck, d_c, many, m=50, k=4097, ys_out=torch.zeros(32 * 4097, dtype=torch.uint8, device="cuda"),
                                 out=torch.zeros(g1b * 4097, dtype=torch.uint8, device="cuda")))
    other = kzgmi.Context(0, 1)
    try:
        refused(-1, lambda: other.open(ck, d_c, d_z, ys_out=ys, out=out))  # a key of another context
    finally:
        other.close()
    bad_c = _dev(_fr(coeffs[:30]) + C.r.to_bytes(32, "big") + _fr(coeffs[31:]))
    refused(-4, lambda: ctx.open(ck, bad_c, d_z, ys_out=ys, out=out))
    bad_z = _dev(_fr(zs[:3]) + C.r.to_bytes(32, "big"))
    refused(-4, lambda: ctx.open(ck, d_c, bad_z, ys_out=ys, out=out))
    # the async form reports a device-side error at the wait
    ctx.open_async(ck, 1, bad_c, d_z, 50, 4, ys, out)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.wait(1)
    assert e.value.code == -4 and untouched()
    ctx.open_async(ck, 1, d_c, d_z, 50, 4, ys, out)
    assert ctx.wait(1) is True
    assert (_host(out), _host(ys)) == want
    # host form: a bad scalar
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.open(ck, _fr(coeffs), _fr(zs[:3]) + C.r.to_bytes(32, "big"))
    assert e.value.code == -4
    assert ctx.open(ck, _fr(coeffs), _fr(zs)) == want
