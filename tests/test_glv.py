"""GLV decomposition on the CPU.

1. The spec (oracle/pyspec/glv.py): phi(P) = [lam] P, k = k0 + k1 lam (mod r) and
   |k0|, |k1| < 2^127 -- the bound that lets a half scalar use 8 signed 16-bit windows.
2. The product constants (csrc/params_gen.hpp, from tools/gen_params.py) equal the spec's.
3. `device_split` restates csrc/glv.hpp step by step (Barrett rounding division, mod-2^128
   arithmetic, sign-magnitude halves) and must equal the spec's exact Babai rounding on
   edge and random scalars.  The device code itself is held to the spec word for word by
   tests/test_gpu_points_ops.py (glv.round_div_*, glv.split and the glv_split launcher), whose
   cases tests/pointref.py picks with `device_round_div`'s count of Barrett corrections.
"""
import os
import random
import re

import pytest

from oracle.pyspec import curves as pc
from oracle.pyspec import glv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "kzg-batch-verification-scheme_amd", "csrc", "params_gen.hpp")
CURVES = {"bls12_381": "Bls12_381", "bn254": "Bn254"}


def product_consts(curve):
    src = open(PARAMS).read()
    body = src[src.index("struct %sConsts" % CURVES[curve]):]
    body = body[:body.index("\n};")]
    out = {}
    for m in re.finditer(r"static constexpr uint32_t (GLV_\w+)\[\d+\] = \{([^}]*)\}", body):
        words = [int(w.strip().rstrip("u"), 16) for w in m.group(2).split(",")]
        out[m.group(1)] = sum(w << (32 * i) for i, w in enumerate(words))
    return out


def device_round_div(curve, k, g, K=None):
    """Mirror of glv.hpp glv_round_div: (round(k g / r), Barrett corrections taken)."""
    r = pc.CURVES[curve].r
    K = K or product_consts(curve)
    N = k * g + K["GLV_HALF_R"]
    q = ((N >> 224) * K["GLV_MU"]) >> 288
    rem = (N - q * r) % (1 << 288)
    steps = 0
    for _ in range(2):
        if rem >= r:
            rem -= r
            q += 1
            steps += 1
    assert rem < r, "Barrett needs more than two corrections"
    assert q < 1 << 128
    return q, steps


def device_split(curve, k):
    """Mirror of glv.hpp glv_split: returns the two 128-bit sign-magnitude words."""
    K = product_consts(curve)
    m128 = (1 << 128) - 1

    def round_div(g):
        return device_round_div(curve, k, g, K)[0]

    c1, c2 = round_div(K["GLV_G1"]), round_div(K["GLV_G2"])
    h0 = (k - c1 * K["GLV_A1"] - c2 * K["GLV_A2"]) & m128
    h1 = (-c1 * K["GLV_B1"] - c2 * K["GLV_B2"]) & m128

    def sm(v):
        if v >> 127:
            v = ((1 << 128) - v) | (1 << 127)
        return v
    return sm(h0), sm(h1)


def signed(w):
    return -(w & ((1 << 127) - 1)) if w >> 127 else w


@pytest.mark.parametrize("curve", list(CURVES))
def test_spec_decomposition(curve):
    C = pc.CURVES[curve]
    beta, lam, v1, v2 = glv.params(curve)
    assert pow(beta, 3, C.p) == 1 and beta != 1
    assert (lam * lam + lam + 1) % C.r == 0
    for v in (v1, v2):
        assert (v[0] + v[1] * lam) % C.r == 0
    rng = random.Random(3)
    for _ in range(3):
        P = pc.g1_mul(C.g1, rng.randrange(1, C.r), C)
        assert glv.phi(curve, P) == pc.g1_mul(P, lam, C)
    for k in glv.edge_scalars(curve, 64) + [rng.randrange(C.r) for _ in range(2000)]:
        k0, k1 = glv.decompose(curve, k)
        assert (k0 + k1 * lam - k) % C.r == 0
        assert abs(k0) < 1 << 127 and abs(k1) < 1 << 127


@pytest.mark.parametrize("curve", list(CURVES))
def test_product_constants_match_spec(curve):
    C = pc.CURVES[curve]
    K = product_consts(curve)
    beta, lam, v1, v2 = glv.params(curve)
    nbits = 32 * (12 if curve == "bls12_381" else 8)
    assert K["GLV_BETA_M"] == beta * (1 << nbits) % C.p
    assert K["GLV_LAMBDA"] == lam
    m128 = (1 << 128) - 1
    assert (K["GLV_A1"], K["GLV_B1"], K["GLV_A2"], K["GLV_B2"]) == \
        (v1[0] & m128, v1[1] & m128, v2[0] & m128, v2[1] & m128)
    assert K["GLV_G1"] == v2[1] and K["GLV_G2"] == -v1[1]
    assert K["GLV_HALF_R"] == (C.r - 1) // 2 and K["GLV_MU"] == (1 << 512) // C.r


@pytest.mark.parametrize("curve", list(CURVES))
def test_device_algorithm_equals_spec(curve):
    C = pc.CURVES[curve]
    rng = random.Random(11)
    for k in glv.edge_scalars(curve, 128) + [rng.randrange(C.r) for _ in range(20000)]:
        h0, h1 = device_split(curve, k)
        assert (signed(h0), signed(h1)) == glv.decompose(curve, k), hex(k)
