"""The opening scan's model (tests/openref.py) against plain synthetic division, for both scalar
moduli: the tiled three-pass form of csrc/open.hpp equals Horner's rule at every size around its
boundaries, and the quotient satisfies the opening identity."""
import random

import pytest

import openref as R
from oracle.pyspec import curves as pc

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988
# (run, block, span): small tile choices, every boundary within reach of m <= 70
TILINGS = [(2, 4, 2), (4, 2, 4), (1, 8, 2), (2, 2, 8)]


def _boundary_sizes(run, block, span):
    tile = run * block
    ms = set(range(0, 71))
    for b in (run, tile, tile * span, 2 * tile * span):
        ms.update(x for x in (b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1) if x >= 0)
    return sorted(ms)


def _points(r, rng):
    return [0, 1, r - 1, rng.randrange(r)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("tiling", TILINGS)
def test_tiled_scan_equals_synthetic_division(curve, tiling):
    r = pc.CURVES[curve].r
    rng = random.Random(hash(tiling) & 0xFFFF)
    for m in _boundary_sizes(*tiling):
        coeffs = [rng.randrange(r) for _ in range(m)]
        for z in _points(r, rng):
            assert R.divide_tiled(coeffs, z, r, *tiling) == R.divide(coeffs, z, r), (m, z)


@pytest.mark.parametrize("curve", CURVES)
def test_tiled_scan_at_the_kernels_parameters(curve):
    r = pc.CURVES[curve].r
    rng = random.Random(3)
    for m in [0, 1, 2, 15, 16, 17, 4095, 4096, 4097]:
        coeffs = [rng.randrange(r) for _ in range(m)]
        z = rng.randrange(r)
        assert R.divide_tiled(coeffs, z, r) == R.divide(coeffs, z, r), m


@pytest.mark.parametrize("curve", CURVES)
def test_division_edges(curve):
    r = pc.CURVES[curve].r
    assert R.divide([], 5, r) == (0, [])
    assert R.divide([7], 5, r) == (7, [])
    assert R.divide([0] * 9, r - 1, r) == (0, [0] * 8)
    # z a root of p = (X - 3)(X + 2) = X^2 - X - 6
    assert R.divide([r - 6, r - 1, 1], 3, r) == (0, [2, 1])
    # a single nonzero top coefficient: q = sum z^(m-2-i) X^i
    y, q = R.divide([0, 0, 0, 1], 2, r)
    assert (y, q) == (8, [4, 2, 1])


@pytest.mark.parametrize("curve", CURVES)
def test_opening_identity(curve):
    """p(tau) - y = q(tau) (tau - z) under a toy tau."""
    r = pc.CURVES[curve].r
    rng = random.Random(11)
    for m in [1, 2, 3, 17, 70]:
        coeffs = [rng.randrange(r) for _ in range(m)]
        for z in _points(r, rng) + [TAU]:
            y, q = R.divide_tiled(coeffs, z, r, 2, 4, 2)
            assert y == R.evaluate(coeffs, z, r)
            assert (R.evaluate(coeffs, TAU, r) - y) % r == R.evaluate(q, TAU, r) * (TAU - z) % r
