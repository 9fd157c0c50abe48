"""The opening scan on the GPU (csrc/open.hpp) through the diagnostic entry kzgmi_open_quotient_device,
bit-exact against the big-integer model (tests/openref.py): y = p(z) and every coefficient of
(p - y) / (X - z), for both curves, at every size around the kernel's boundaries.

Boundaries (open.hpp): runs of 16 coefficients per thread, tiles of 4096 per workgroup -- powers of
two, so m in {2^j - 1, 2^j, 2^j + 1}, j = 4..16, crosses each with a ragged and a full last run and
tile, one and several tiles -- and 256 tile aggregates (2^20 coefficients) per step of the
second-level scan, crossed by the one case at 2^20 + 1.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

import openref as R  # noqa: E402
from oracle.pyspec import curves as pc  # noqa: E402

CURVES = ["bls12_381", "bn254"]
SIZES = list(range(10)) + [(1 << j) + d for j in range(4, 17) for d in (-1, 0, 1)]
SPAN_COEFFS = 256 * 4096  # OPEN_SPAN x OPEN_TILE


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 1)
    yield c
    c.close()


def _be(vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b or bytes(32)), dtype=torch.uint8).cuda()


def _run(ctx, curve, coeffs, zs):
    """(ys, q) bytes from the device"""
    ys, q = ctx.open_quotient(curve, _dev(_be(coeffs)), len(coeffs), _dev(_be(zs)), len(zs))
    return ys.cpu().numpy().tobytes(), q.cpu().numpy().tobytes()


def _want(coeffs, zs, r):
    res = [R.divide(coeffs, z, r) for z in zs]
    return _be([y for y, _ in res]), b"".join(_be(q) for _, q in res)


def _check(ctx, curve, coeffs, zs):
    r = pc.CURVES[curve].r
    got = _run(ctx, curve, coeffs, zs)
    want = _want(coeffs, zs, r)
    assert got[0] == want[0], "ys differ (m = %d)" % len(coeffs)
    assert got[1] == want[1], "quotients differ (m = %d)" % len(coeffs)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", SIZES)
def test_quotient_sizes(ctx, curve, m):
    r = pc.CURVES[curve].r
    rng = random.Random(1000 + m)
    coeffs = [rng.randrange(r) for _ in range(m)]
    _check(ctx, curve, coeffs, [rng.randrange(r), 0, r - 1])


def test_quotient_across_the_second_level_span(ctx):
    """257 tiles: the second-level workgroup takes two steps, the upper one with a single tile"""
    curve = "bls12_381"
    r = pc.CURVES[curve].r
    rng = random.Random(77)
    m = SPAN_COEFFS + 1
    coeffs = [rng.getrandbits(255) % r for _ in range(m)]
    _check(ctx, curve, coeffs, [rng.randrange(r), 0, r - 1])


@pytest.mark.parametrize("curve", CURVES)
def test_quotient_edge_values(ctx, curve):
    r = pc.CURVES[curve].r
    rng = random.Random(5)
    zs = [rng.randrange(r), 0, r - 1]
    m = 4099  # two tiles, a ragged last one
    _check(ctx, curve, [0] * m, zs)
    _check(ctx, curve, [r - 1] * m, zs)
    _check(ctx, curve, [0] * (m - 1) + [7], zs)
    # z a root of p = (X - a) s(X)
    a = rng.randrange(r)
    s = [rng.randrange(r) for _ in range(40)]
    p = [0] * 41
    for i, c in enumerate(s):
        p[i] = (p[i] - a * c) % r
        p[i + 1] = (p[i + 1] + c) % r
    assert R.divide(p, a, r) == (0, s)
    _check(ctx, curve, p, [a, a, rng.randrange(r)])


@pytest.mark.parametrize("curve", CURVES)
def test_quotient_errors_and_empty(ctx, curve):
    import torch
    import kzgmi
    r = pc.CURVES[curve].r
    rng = random.Random(6)
    coeffs = [rng.randrange(r) for _ in range(33)]
    zs = [rng.randrange(r) for _ in range(3)]
    for bad_c, bad_z in [(coeffs[:20] + [r] + coeffs[21:], zs), (coeffs, [zs[0], r, zs[2]]),
                         (coeffs, zs[:2] + [(1 << 256) - 1])]:
        with pytest.raises(kzgmi.KzgmiError) as e:
            _run(ctx, curve, bad_c, bad_z)
        assert e.value.code == -4
    # the slot is usable afterwards
    _check(ctx, curve, coeffs, zs)
    # k = 0 succeeds and writes nothing
    ys = torch.full((32,), 0xA5, dtype=torch.uint8, device="cuda")
    q = torch.full((32 * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.open_quotient(curve, _dev(_be(coeffs)), 33, _dev(b""), 0, ys_out=ys, out=q)
    torch.cuda.synchronize()
    assert bytes(ys.cpu().numpy()) == b"\xa5" * 32 and bytes(q.cpu().numpy()) == b"\xa5" * 1024
