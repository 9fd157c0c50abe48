"""The models of the G1 transforms (g1nttref.py) and of open_all (openallref.py) held to the definitions:
nttref's transforms and openref's synthetic division.  No GPU.
"""
import random

import pytest

import g1nttref as G
import nttref as N
import openallref as A
import openref as R

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988


def _rg(curve):
    return N.MODULUS[curve], N.GENERATOR[curve]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("flags", [0, G.INVERSE, G.BITREV, G.INVERSE | G.BITREV])
def test_staged_transform_is_the_definition(curve, flags):
    r, g = _rg(curve)
    rng = random.Random(7 + flags)
    for logn in range(0, 8):
        vals = [rng.randrange(r) for _ in range(1 << logn)]
        want = N.dft_naive(vals, logn, r, g, inverse=bool(flags & G.INVERSE), bitrev=bool(flags & G.BITREV))
        assert G.transform(vals, logn, r, g, flags) == want
        assert G.transform_staged(vals, logn, r, g, flags) == want, logn


@pytest.mark.parametrize("curve", CURVES)
def test_staged_round_trip_and_exceptional_inputs(curve):
    r, g = _rg(curve)
    rng = random.Random(8)
    for logn in (3, 6):
        n = 1 << logn
        k = rng.randrange(1, r)
        half = [rng.randrange(r) for _ in range(n // 2)]
        for vals in ([k] * n, [0] * n, half + [(-v) % r for v in half], [0] * 5 + [k] + [0] * (n - 6)):
            for flags in (0, G.BITREV):
                f = G.transform_staged(vals, logn, r, g, flags)
                assert f == N.dft_naive(vals, logn, r, g, bitrev=bool(flags))
                assert G.transform_staged(f, logn, r, g, flags | G.INVERSE) == vals
        # all inputs equal: every first-stage difference is infinity, so that stage multiplies nothing
        data = [k] * n
        assert G.stages(data, logn, r, g, False) == 0
        assert data == [k * n % r] + [0] * (n - 1)


def test_multiplication_count_of_a_random_transform():
    """(n / 2) logn butterflies, of which those with k = 0 -- n - 1 of them -- multiply nothing"""
    r, g = _rg("bls12_381")
    rng = random.Random(9)
    for logn in (1, 4, 7):
        n = 1 << logn
        data = [rng.randrange(1, r) for _ in range(n)]
        assert G.stages(data, logn, r, g, False) == (n // 2) * logn - (n - 1)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("tau_in_domain", [False, True])
def test_open_all_is_n_openings(curve, tau_in_domain):
    """for n = 1 .. 64 and m in {0, 1, n - 1, n}: proof_e = q_e(tau), q_e = (p - p(w^e)) / (X - w^e)"""
    r, g = _rg(curve)
    rng = random.Random(10)
    for logn in range(0, 7):
        n = 1 << logn
        w = N.root(r, g, logn)
        tau = w if tau_in_domain else TAU
        xhat = A.key(logn, tau, r, g)
        for m in sorted({0, 1, n - 1, n}):
            coeffs = [rng.randrange(r) for _ in range(m)]
            for flags in (0, A.BITREV):
                proofs, ys = A.open_all(coeffs, logn, tau, r, g, flags, xhat)
                for e in range(n):
                    z = pow(w, e, r)
                    y, q = R.divide(coeffs, z, r)
                    at = N.rev(e, logn) if flags else e
                    assert ys[at] == y == R.evaluate(coeffs, z, r)
                    assert proofs[at] == R.evaluate(q, tau, r), (logn, m, e)


@pytest.mark.parametrize("curve", CURVES)
def test_open_all_special_polynomials(curve):
    r, g = _rg(curve)
    logn, n = 4, 16
    proofs, ys = A.open_all([5], logn, TAU, r, g)
    assert proofs == [0] * n and ys == [5] * n  # a constant: every quotient is zero
    proofs, _ = A.open_all([0] * (n - 1) + [1], logn, TAU, r, g)  # X^(n-1)
    w = N.root(r, g, logn)
    for e in range(n):
        z = pow(w, e, r)
        assert proofs[e] == sum(pow(z, n - 2 - j, r) * pow(TAU, j, r) for j in range(n - 1)) % r
    # X^n - 1 truncated to m = n is the constant -1
    proofs, ys = A.open_all([r - 1] + [0] * (n - 1), logn, TAU, r, g)
    assert proofs == [0] * n and ys == [r - 1] * n
