"""KZG openings at every point of a domain (kzgmi_open_all*) against the oracle and against kzgmi_open: for a
commit key of 2^10 powers of a toy tau, the proofs equal the oracle's g1_mul_gen of the model's exponents
(tests/openallref.py) and, byte for byte, ctx.open of the same coefficients at the n domain points; the
evaluations equal both.  Forms, orders, special polynomials, a degenerate SRS, the verifier round trip, keys
and errors.  Every case runs under the shipped choice of stage form and under each form forced
(KZGMI_G1NTT_FORM=thread|wave, read when the context is created): at these sizes the shipped choice is the
wave form, so the forced thread form is what takes the FK20 job through k_g1ntt_stage.
"""
import functools
import os
import random

import pytest

pytestmark = pytest.mark.gpu

import nttref as N  # noqa: E402
import openallref as A  # noqa: E402
import openref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988  # the toy tau of test_gpu_commit.py
NPOW = 1 << 10
ERR_ARG, ERR_SCALAR = -1, -4


@pytest.fixture(scope="module", params=[None, "thread", "wave"], ids=["auto", "thread", "wave"])
def ctx(request):
    import kzgmi
    if request.param:
        os.environ["KZGMI_G1NTT_FORM"] = request.param
    try:
        c = kzgmi.Context(0, 2)
    finally:
        os.environ.pop("KZGMI_G1NTT_FORM", None)
    yield c
    _KEYS.clear()  # the keys belong to this context
    c.close()


def _fr(vals):
    return b"".join(pk.fr_to_bytes(v) for v in vals)


@functools.lru_cache(maxsize=None)
def _gen_cached(curve, ks):
    return O.g1_mul_gen(curve, _fr(ks), len(ks))


def _gen(curve, ks):
    """k G for every k, computed once per list (the three contexts ask for the same expectations)"""
    return _gen_cached(curve, tuple(ks))


def _powers(curve, tau, n):
    r = pc.CURVES[curve].r
    sc, x = [], 1
    for _ in range(n):
        sc.append(x)
        x = x * tau % r
    return _gen(curve, sc)


@pytest.fixture(scope="module")
def cks(ctx):
    return {curve: ctx.load_commit_key(curve, _powers(curve, TAU, NPOW)) for curve in CURVES}


_KEYS = {}


def _key(ctx, cks, curve, logn):
    if (curve, logn) not in _KEYS:
        _KEYS[curve, logn] = ctx.load_open_all_key(cks[curve], logn)
    return _KEYS[curve, logn]


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b or bytes(32)), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _domain(curve, logn):
    C = pc.CURVES[curve]
    w = N.root(C.r, N.GENERATOR[curve], logn)
    return [pow(w, e, C.r) for e in range(1 << logn)]


def _rg(curve):
    return pc.CURVES[curve].r, N.GENERATOR[curve]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [0, 1, 2, 5, 8])
def test_against_oracle_and_open(ctx, cks, curve, logn):
    r, g = _rg(curve)
    n = 1 << logn
    key = _key(ctx, cks, curve, logn)
    zs = _domain(curve, logn)
    rng = random.Random(60 + logn)
    xhat = A.key(logn, TAU, r, g)
    for m in sorted({0, 1, n - 1, n}):
        coeffs = [rng.randrange(r) for _ in range(m)]
        ex, ys = A.open_all(coeffs, logn, TAU, r, g, 0, xhat)
        proofs, got_ys = ctx.open_all(key, _fr(coeffs), m=m)
        assert got_ys == _fr(ys) == _fr([R.evaluate(coeffs, z, r) for z in zs]), m
        assert proofs == _gen(curve, ex), m
        o_p, o_y = ctx.open(cks[curve], _fr(coeffs), _fr(zs), m=m, k=n)
        assert proofs == o_p and got_ys == o_y, m


@pytest.mark.parametrize("curve", CURVES)
def test_logn_10(ctx, cks, curve):
    r, g = _rg(curve)
    logn, n = 10, 1 << 10
    gb = 2 * pc.CURVES[curve].fp_bytes
    rng = random.Random(70)
    coeffs = [rng.randrange(r) for _ in range(n)]
    d_p, d_y = ctx.open_all(_key(ctx, cks, curve, logn), _dev(_fr(coeffs)))
    o_p, o_y = ctx.open(cks[curve], _dev(_fr(coeffs)), _dev(_fr(_domain(curve, logn))))
    assert _host(d_p) == _host(o_p) and _host(d_y) == _host(o_y)
    ex, _ = A.open_all(coeffs, logn, TAU, r, g)
    sample = [0, 1, n - 1] + [rng.randrange(n) for _ in range(61)]
    got = _host(d_p)
    assert b"".join(got[e * gb:(e + 1) * gb] for e in sample) == _gen(curve, [ex[e] for e in sample])


@pytest.mark.parametrize("curve", CURVES)
def test_order_and_forms(ctx, cks, curve):
    import torch
    r, g = _rg(curve)
    logn, n = 5, 32
    gb = 2 * pc.CURVES[curve].fp_bytes
    key = _key(ctx, cks, curve, logn)
    rng = random.Random(71)
    c1 = [rng.randrange(r) for _ in range(n)]
    c2 = [rng.randrange(r) for _ in range(n - 3)]
    want = {}
    for name, c in (("c1", c1), ("c2", c2)):
        for flags in (0, A.BITREV):
            ex, ys = A.open_all(c, logn, TAU, r, g, flags)
            want[name, flags] = (_gen(curve, ex), _fr(ys))
    for flags in (0, A.BITREV):
        rev = bool(flags)
        assert ctx.open_all(key, _fr(c1), bitrev=rev) == want["c1", flags]                       # host
        d_p, d_y = ctx.open_all(key, _dev(_fr(c1)), bitrev=rev)                                  # device
        assert (_host(d_p), _host(d_y)) == want["c1", flags]
        assert ctx.open_all(key, _fr(c1), bitrev=rev, want_ys=False) == (want["c1", flags][0], None)  # ys_out = NULL
        d_p, d_y = ctx.open_all(key, _dev(_fr(c1)), bitrev=rev, want_ys=False)
        assert d_y is None and _host(d_p) == want["c1", flags][0]
    # two jobs in flight on two slots
    outs = [(torch.empty(n * 32, dtype=torch.uint8, device="cuda"), torch.empty(n * gb, dtype=torch.uint8, device="cuda"))
            for _ in range(2)]
    ctx.open_all_async(key, 0, _dev(_fr(c1)), n, outs[0][0], outs[0][1])
    ctx.open_all_async(key, 1, _dev(_fr(c2)), n - 3, outs[1][0], outs[1][1], bitrev=True)
    assert ctx.wait(1) and ctx.wait(0)
    assert (_host(outs[0][1]), _host(outs[0][0])) == want["c1", 0]
    assert (_host(outs[1][1]), _host(outs[1][0])) == want["c2", A.BITREV]


@pytest.mark.parametrize("curve", CURVES)
def test_special_polynomials(ctx, cks, curve):
    C = pc.CURVES[curve]
    r, g = _rg(curve)
    logn, n = 5, 32
    key = _key(ctx, cks, curve, logn)
    zs = _fr(_domain(curve, logn))
    inf = pk.g1_to_bytes(None, C)
    proofs, ys = ctx.open_all(key, _fr([5]))
    assert proofs == inf * n and ys == _fr([5] * n)                       # a constant
    for coeffs in ([0] * (n - 1) + [1], [r - 1] + [0] * (n - 1), [0] * n):  # X^(n-1); X^n - 1 cut to m = n; zero
        proofs, ys = ctx.open_all(key, _fr(coeffs))
        ex, my = A.open_all(coeffs, logn, TAU, r, g)
        assert (proofs, ys) == (_gen(curve, ex), _fr(my))
        assert (proofs, ys) == ctx.open(cks[curve], _fr(coeffs), zs)


@pytest.mark.parametrize("curve", CURVES)
def test_degenerate_srs(ctx, curve):
    """tau = w_16: the proofs are still ctx.open's and the model's"""
    r, g = _rg(curve)
    logn, n = 4, 16
    tau = N.root(r, g, logn)
    ck = ctx.load_commit_key(curve, _powers(curve, tau, n))
    key = ctx.load_open_all_key(ck, logn)
    rng = random.Random(72)
    for m in (n - 1, n):
        coeffs = [rng.randrange(r) for _ in range(m)]
        proofs, ys = ctx.open_all(key, _fr(coeffs))
        assert (proofs, ys) == ctx.open(ck, _fr(coeffs), _fr(_domain(curve, logn)))
        ex, my = A.open_all(coeffs, logn, tau, r, g)
        assert (proofs, ys) == (_gen(curve, ex), _fr(my))


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip_with_the_verifier(ctx, cks, curve):
    C = pc.CURVES[curve]
    logn, n = 6, 64
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(curve, g2, O.g2_mul(curve, g2, TAU))
    rng = random.Random(73)
    coeffs = [rng.randrange(C.r) for _ in range(n)]
    cm = ctx.commit(cks[curve], _fr(coeffs))
    proofs, ys = ctx.open_all(_key(ctx, cks, curve, logn), _fr(coeffs))
    zs = _fr(_domain(curve, logn))
    seed = bytes(range(32))
    assert ctx.batch_verify(srs, _dev(cm * n), _dev(zs), _dev(ys), _dev(proofs), seed=seed, n=n) is True
    bad = bytearray(ys)
    bad[32 * 17 + 31] ^= 1
    assert ctx.batch_verify(srs, _dev(cm * n), _dev(zs), _dev(bytes(bad)), _dev(proofs), seed=seed, n=n) is False


@pytest.mark.parametrize("curve", CURVES)
def test_keys_and_errors(ctx, cks, curve):
    import kzgmi
    C = pc.CURVES[curve]
    r, g = _rg(curve)
    gb = 2 * C.fp_bytes
    k3, k5 = _key(ctx, cks, curve, 3), _key(ctx, cks, curve, 5)
    assert k5.device_bytes >= 2 * 32 * 2 * gb
    rng = random.Random(74)
    for key in (k3, k5, k3, k5):  # keys of two sizes from one commit key, used alternately
        coeffs = [rng.randrange(r) for _ in range(1 << key.logn)]
        ex, ys = A.open_all(coeffs, key.logn, TAU, r, g)
        assert ctx.open_all(key, _fr(coeffs)) == (_gen(curve, ex), _fr(ys))
    small = ctx.load_commit_key(curve, _powers(curve, TAU, 6))
    assert ctx.load_open_all_key(small, 2).logn == 2  # n - 1 = 3 <= 6
    for logn in (3, 20):  # n - 1 = 7 > 6 powers; logn out of range
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.load_open_all_key(small if logn == 3 else cks[curve], logn)
        assert e.value.code == ERR_ARG
    n = 8
    coeffs = _fr([rng.randrange(r) for _ in range(n)])
    fill_p, fill_y = bytes([0xA5]) * (n * gb), bytes([0x5A]) * (n * 32)

    def expect(code, context, key, cf, m, flags=0):
        p, y = _dev(fill_p), _dev(fill_y)
        rc = kzgmi.lib().kzgmi_open_all_device(context.handle, key.handle, _dev(cf).data_ptr(), m, flags, y.data_ptr(),
                                               p.data_ptr())
        assert rc == code, (rc, m, flags)
        assert _host(p) == fill_p and _host(y) == fill_y

    other = kzgmi.Context(0, 1)
    try:
        expect(ERR_ARG, other, k3, coeffs, n)                       # a key of another context
    finally:
        other.close()
    expect(ERR_ARG, ctx, k3, coeffs + bytes(32), n + 1)             # m > n
    expect(ERR_ARG, ctx, k3, coeffs, n, flags=1)                    # KZGMI_NTT_INVERSE is not accepted
    expect(ERR_SCALAR, ctx, k3, coeffs[:96] + r.to_bytes(32, "big") + coeffs[128:], n)  # a coefficient = r
    # the slot is usable afterwards, and a repeat call of the same shape allocates nothing
    want = ctx.open_all(k3, coeffs)
    before = kzgmi.alloc_count()
    assert ctx.open_all(k3, coeffs) == want and kzgmi.alloc_count() == before
