"""The model of open_cosets (opencosetsref.py) held to the definition: synthetic division by X^l - z_e for the
quotient and the remainder, direct evaluation for ys.  No GPU.
"""
import os
import random
import re

import pytest

import nttref as N
import openallref as A
import opencosetsref as C
import openref as R

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["kzgmi_open_cosets_key_load", "kzgmi_open_cosets_key_free", "kzgmi_open_cosets_key_device_bytes",
               "kzgmi_open_cosets", "kzgmi_open_cosets_device", "kzgmi_open_cosets_device_async"]


def _rg(curve):
    return N.MODULUS[curve], N.GENERATOR[curve]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("tau_in_domain", [False, True])
@pytest.mark.parametrize("logN", range(0, 6))
def test_open_cosets_is_the_definition(curve, tau_in_domain, logN):
    """every logl <= logN, logk - (logN - logl) in {0, 1, 2}, m in {0, 1, N - 1, N}, both orders:
    proof_e = q_e(tau) with p = q_e (X^l - z_e) + I_e, and ys = p = I_e on coset e"""
    r, g = _rg(curve)
    rng = random.Random(100 + logN)
    n_cap = 1 << logN
    for logl in range(0, logN + 1):
        l = 1 << logl
        for logk in range(logN - logl, logN - logl + 3):
            K, logn = 1 << logk, logk + logl
            w = N.root(r, g, logn)
            tau = w if tau_in_domain else TAU
            xhat = C.key(logN, logl, tau, r, g)
            for m in sorted({0, 1, n_cap - 1, n_cap}):
                coeffs = [rng.randrange(r) for _ in range(m)]
                for flags in (0, C.BITREV):
                    proofs, ys = C.open_cosets(coeffs, logN, logl, logk, tau, r, g, flags, xhat)
                    assert len(proofs) == K and len(ys) == K * l
                    for e in range(K):
                        z = pow(w, e * l, r)
                        q, rem = C.divide_coset(coeffs, l, z, r)
                        assert proofs[N.rev(e, logk) if flags else e] == R.evaluate(q, tau, r), (logl, logk, m, e)
                        for j in range(l):
                            x = pow(w, e + K * j, r)
                            at = N.rev(e + K * j, logn) if flags else e * l + j
                            assert ys[at] == R.evaluate(coeffs, x, r) == R.evaluate(rem, x, r), (logl, logk, m, e, j)


@pytest.mark.parametrize("curve", CURVES)
def test_division_identity(curve):
    """divide_coset itself: p = q (X^l - z) + I with deg I < l"""
    r, _ = _rg(curve)
    rng = random.Random(101)
    for l, m in ((1, 5), (4, 16), (4, 3), (8, 8), (2, 7)):
        coeffs = [rng.randrange(r) for _ in range(m)]
        z, x = rng.randrange(r), rng.randrange(r)
        q, rem = C.divide_coset(coeffs, l, z, r)
        assert len(rem) <= l
        assert (R.evaluate(q, x, r) * (pow(x, l, r) - z) + R.evaluate(rem, x, r)) % r == R.evaluate(coeffs, x, r)


@pytest.mark.parametrize("curve", CURVES)
def test_coset_size_one_is_open_all(curve):
    r, g = _rg(curve)
    rng = random.Random(102)
    for logn in range(0, 6):
        n = 1 << logn
        for m in sorted({0, 1, n - 1, n}):
            coeffs = [rng.randrange(r) for _ in range(m)]
            for flags in (0, C.BITREV):
                assert C.open_cosets(coeffs, logn, 0, logn, TAU, r, g, flags) == A.open_all(coeffs, logn, TAU, r, g, flags)


@pytest.mark.parametrize("curve", CURVES)
def test_whole_domain_coset_has_no_quotient(curve):
    """l = N (R = 1): every proof is the point at infinity"""
    r, g = _rg(curve)
    rng = random.Random(103)
    coeffs = [rng.randrange(r) for _ in range(8)]
    for logk in (0, 2):
        proofs, _ = C.open_cosets(coeffs, 3, 3, logk, TAU, r, g)
        assert proofs == [0] * (1 << logk)


def test_new_symbols_in_header_library_and_binding():
    import kzgmi
    with open(os.path.join(ROOT, "include", "kzgmi.h")) as f:
        header = set(re.findall(r"\b(kzgmi_[a-z0-9_]+)\s*\(", f.read()))
    lib = kzgmi.lib()
    for s in NEW_SYMBOLS:
        assert s in header and s in kzgmi.exported_symbols() and hasattr(lib, s), s
    for name in ("OpenCosetsKey", "open_cosets"):
        assert hasattr(kzgmi, name)
    for name in ("load_open_cosets_key", "open_cosets", "open_cosets_async"):
        assert hasattr(kzgmi.Context, name)
