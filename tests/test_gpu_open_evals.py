"""KZG openings of a polynomial given by its evaluations (kzgmi_open_evals*): for a key of 256 powers of
a toy tau, evaluations and proofs equal kzgmi_open on the model's coefficients (tests/nttref.py) and
[q(tau)]_1 from tests/openref.py and the oracle; a point of the domain returns the given evaluation;
the GPU batch verifier accepts the openings; the three forms agree; errors write nothing.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

import nttref as N  # noqa: E402
import openref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988  # the toy tau of test_gpu_open.py
KEY_N = 256


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
        for _ in range(KEY_N):
            sc.append(pk.fr_to_bytes(x))
            x = x * TAU % C.r
        _POWERS[curve] = O.g1_mul_gen(curve, b"".join(sc), KEY_N)
    return _POWERS[curve]


@pytest.fixture(scope="module")
def keys(ctx):
    return {curve: ctx.load_commit_key(curve, _powers(curve)) for curve in CURVES}


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _case(curve, logn, bitrev, seed, k=4):
    """(evals as given to the call, the coefficients, k points: the first of the domain)"""
    r, g = N.MODULUS[curve], N.GENERATOR[curve]
    rng = random.Random(seed)
    n = 1 << logn
    evals = [rng.randrange(r) for _ in range(n)]
    coeffs = N.dft(evals, logn, r, g, inverse=True, bitrev=bitrev)
    at = rng.randrange(n)  # index `at` of the given array holds the point w^at, or w^rev(at)
    zs = [pow(N.root(r, g, logn), N.rev(at, logn) if bitrev else at, r)] + [rng.randrange(r) for _ in range(k - 1)]
    return evals, coeffs, zs, at


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("logn", [0, 1, 4, 8])
def test_open_evals_matches_open_and_the_oracle(ctx, keys, curve, logn, bitrev):
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    evals, coeffs, zs, at = _case(curve, logn, bitrev, 50 + logn)
    proofs, ys = ctx.open_evals(keys[curve], N.to_bytes(evals), N.to_bytes(zs), logn=logn, bitrev=bitrev)
    assert (proofs, ys) == ctx.open(keys[curve], N.to_bytes(coeffs), N.to_bytes(zs))
    assert ys == N.to_bytes([R.evaluate(coeffs, z, C.r) for z in zs])
    assert ys[:32] == evals[at].to_bytes(32, "big")  # a point of the domain: the given evaluation
    for j, z in enumerate(zs):
        q_tau = R.evaluate(R.divide(coeffs, z, C.r)[1], TAU, C.r)
        assert proofs[j * g1b:(j + 1) * g1b] == O.g1_mul_gen(curve, pk.fr_to_bytes(q_tau), 1), (logn, j)
    # device and async forms
    import torch
    d_e, d_z = _dev(N.to_bytes(evals)), _dev(N.to_bytes(zs))
    d_p, d_y = ctx.open_evals(keys[curve], d_e, d_z, logn=logn, bitrev=bitrev)
    assert (_host(d_p), _host(d_y)) == (proofs, ys)
    a_y = torch.zeros(32 * len(zs), dtype=torch.uint8, device="cuda")
    a_p = torch.zeros(g1b * len(zs), dtype=torch.uint8, device="cuda")
    ctx.open_evals_async(keys[curve], 1, d_e, d_z, logn, len(zs), a_y, a_p, bitrev=bitrev)
    assert ctx.wait(1) is True
    assert (_host(a_p), _host(a_y)) == (proofs, ys)


@pytest.mark.parametrize("curve", CURVES)
def test_open_evals_round_trip_with_the_verifier(ctx, keys, curve):
    """commit the polynomial, open it from its evaluations at 8 points, and the GPU batch verifier accepts"""
    C = pc.CURVES[curve]
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(curve, g2, O.g2_mul(curve, g2, TAU))
    evals, coeffs, zs, _ = _case(curve, 7, True, 60, k=8)
    cm = ctx.commit(keys[curve], N.to_bytes(coeffs))
    proofs, ys = ctx.open_evals(keys[curve], N.to_bytes(evals), N.to_bytes(zs), bitrev=True)
    assert ctx.batch_verify(srs, cm * 8, N.to_bytes(zs), ys, proofs, seed=bytes(32)) is True
    y3 = (int.from_bytes(ys[96:128], "big") + 1) % C.r
    bad = ys[:96] + pk.fr_to_bytes(y3) + ys[128:]
    assert ctx.batch_verify(srs, cm * 8, N.to_bytes(zs), bad, proofs, seed=bytes(32)) is False


@pytest.mark.parametrize("curve", CURVES)
def test_open_evals_errors(ctx, keys, curve):
    import torch
    import kzgmi
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    ck = keys[curve]
    logn = 5
    evals, coeffs, zs, _ = _case(curve, logn, False, 70)
    want = ctx.open(ck, N.to_bytes(coeffs), N.to_bytes(zs))
    d_e, d_z = _dev(N.to_bytes(evals)), _dev(N.to_bytes(zs))
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
        p2, y2 = ctx.open_evals(ck, d_e, d_z, logn=logn)  # the slot is usable afterwards
        assert (_host(p2), _host(y2)) == want

    big = torch.zeros(32 * 2 * KEY_N, dtype=torch.uint8, device="cuda")
    refused(-1, lambda: ctx.open_evals(ck, big, d_z, logn=9, ys_out=ys, out=out))  # n > the key's n
    import ctypes  # a flag other than KZGMI_NTT_BITREV
    rc = kzgmi.lib().kzgmi_open_evals_device(ctx.handle, ck.handle, d_e.data_ptr(), logn, kzgmi.NTT_INVERSE, d_z.data_ptr(),
                                             ctypes.c_size_t(4), ys.data_ptr(), out.data_ptr())
    assert rc == -1 and untouched()
    for at, bad in ((0, C.r), (17, (1 << 256) - 1), (31, C.r)):
        w = list(evals)
        w[at] = bad
        d_bad = _dev(N.to_bytes(w))
        refused(-4, lambda: ctx.open_evals(ck, d_bad, d_z, logn=logn, ys_out=ys, out=out))
    bad_z = _dev(N.to_bytes(zs[:3]) + C.r.to_bytes(32, "big"))
    refused(-4, lambda: ctx.open_evals(ck, d_e, bad_z, logn=logn, ys_out=ys, out=out))
    ctx.open_evals_async(ck, 1, d_bad, d_z, logn, 4, ys, out)
    with pytest.raises(kzgmi.KzgmiError) as e:  # the async form reports it at the wait
        ctx.wait(1)
    assert e.value.code == -4 and untouched()
    ctx.open_evals_async(ck, 1, d_e, d_z, logn, 4, ys, out)
    assert ctx.wait(1) is True
    assert (_host(out), _host(ys)) == want
    with pytest.raises(kzgmi.KzgmiError) as e:  # host form
        ctx.open_evals(ck, N.to_bytes(w), N.to_bytes(zs), logn=logn)
    assert e.value.code == -4
    assert ctx.open_evals(ck, N.to_bytes(evals), N.to_bytes(zs), logn=logn) == want
