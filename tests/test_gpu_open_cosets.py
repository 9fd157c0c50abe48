"""FK20 multi-proofs on every coset of a domain (kzgmi_open_cosets*) against the oracle: for a commit key of
2^10 powers of a toy tau, the proofs equal the oracle's g1_mul_gen of the model's exponents
(tests/opencosetsref.py), the evaluations equal the model and direct evaluation.  Shapes (logN, logl, logk),
orders, forms, the EIP-7594 shape against compute_cells_and_proofs and verify_cell_batch, a pairing round
trip off that shape, a degenerate SRS, keys and errors.  Every case runs under the shipped choice of the
products' and stages' form and under each form forced (KZGMI_G1NTT_FORM=thread|wave, read when the context is
created): at these sizes the shipped choice is the wave form, so the forced thread form is what takes the job
through k_cosets_mul and its segmented sums.
"""
import functools
import os
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

import nttref as N  # noqa: E402
import opencosetsref as C  # noqa: E402
import openref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
TAU = 0x1F2E3D4C5B6A7988  # the toy tau of test_gpu_commit.py
NPOW = 1 << 10
ERR_ARG, ERR_SCALAR = -1, -4

# (logN, logl, logk): the smallest shapes at which each part can go wrong
SHAPES = [
    (0, 0, 0),  # smallest shape
    (3, 3, 0),  # R = 1: no H, all proofs at infinity
    (3, 2, 1),  # R = 2: one H entry
    (3, 1, 2),  # with count = 3 a partly filled wave: 48 terms
    (4, 2, 4),  # K = 4R: padding
    (6, 3, 3),  # l < 64: segmented reduction
    (8, 6, 3),  # l = 64: one full wave per position
    (8, 7, 1),  # l = 128: two partial sums per position
    (5, 0, 5),  # l = 1: also byte for byte ctx.open_all at logn = 5
]


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


def _key(ctx, cks, curve, logN, logl):
    if (curve, logN, logl) not in _KEYS:
        _KEYS[curve, logN, logl] = ctx.load_open_cosets_key(cks[curve], logN, logl)
    return _KEYS[curve, logN, logl]


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b or bytes(32)), dtype=torch.uint8).cuda()


def _host(t):
    return t.cpu().numpy().tobytes()


def _rg(curve):
    return pc.CURVES[curve].r, N.GENERATOR[curve]


@functools.lru_cache(maxsize=None)
def _xhat(curve, logN, logl, tau):
    r, g = _rg(curve)
    return C.key(logN, logl, tau, r, g)


@functools.lru_cache(maxsize=None)
def _model(curve, shape, tau, flags, polys):
    """(proof encodings, ys bytes) of the polynomials `polys` (a tuple of coefficient tuples), one after the other"""
    r, g = _rg(curve)
    logN, logl, logk = shape
    ex, ys = [], []
    for coeffs in polys:
        e, y = C.open_cosets(list(coeffs), logN, logl, logk, tau, r, g, flags, _xhat(curve, logN, logl, tau))
        ex += e
        ys += y
    return _gen(curve, ex), _fr(ys)


def _polys(rng, r, count, m):
    return tuple(tuple(rng.randrange(r) for _ in range(m)) for _ in range(count))


def _flat(polys):
    return _fr([c for p in polys for c in p])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_against_oracle(ctx, cks, curve, shape):
    r, g = _rg(curve)
    logN, logl, logk = shape
    n_cap, l, K = 1 << logN, 1 << logl, 1 << logk
    key = _key(ctx, cks, curve, logN, logl)
    assert key.device_bytes >= 2 * n_cap * 4 * pc.CURVES[curve].fp_bytes
    w = N.root(r, g, logk + logl)
    rng = random.Random(1000 + 100 * logN + 10 * logl + logk)
    for count in (1, 3):
        for m in sorted({0, 1, n_cap - 1, n_cap}):
            polys = _polys(rng, r, count, m)
            want_p, want_y = _model(curve, shape, TAU, 0, polys)
            proofs, ys = ctx.open_cosets(key, _flat(polys), logk, m=m, count=count)
            assert ys == want_y, (count, m)
            assert proofs == want_p, (count, m)
            direct = [R.evaluate(polys[-1], pow(w, e + K * j, r), r) for e in range(K) for j in range(l)]
            assert ys[-32 * K * l:] == _fr(direct), (count, m)
            if logl == 0:  # coset size 1: open_all, byte for byte
                if (curve, "open_all", logN) not in _KEYS:
                    _KEYS[curve, "open_all", logN] = ctx.load_open_all_key(cks[curve], logN)
                pb = len(proofs) // count
                for t, p in enumerate(polys):
                    assert ctx.open_all(_KEYS[curve, "open_all", logN], _fr(p), m=m) == (
                        proofs[t * pb:(t + 1) * pb], ys[t * 32 * K:(t + 1) * 32 * K])


@pytest.mark.parametrize("curve", CURVES)
def test_orders_and_forms(ctx, cks, curve):
    import torch
    r, _ = _rg(curve)
    shape = (4, 2, 3)
    logN, logl, logk = shape
    gb = 2 * pc.CURVES[curve].fp_bytes
    key = _key(ctx, cks, curve, logN, logl)
    rng = random.Random(171)
    p2 = _polys(rng, r, 2, 16)
    p1 = _polys(rng, r, 1, 13)
    for flags in (0, C.BITREV):
        rev = bool(flags)
        want = _model(curve, shape, TAU, flags, p2)
        assert ctx.open_cosets(key, _flat(p2), logk, count=2, bitrev=rev) == want                              # host
        d_p, d_y = ctx.open_cosets(key, _dev(_flat(p2)), logk, count=2, bitrev=rev)                            # device
        assert (_host(d_p), _host(d_y)) == want
        assert ctx.open_cosets(key, _flat(p2), logk, count=2, bitrev=rev, want_ys=False) == (want[0], None)   # ys_out = NULL
        d_p, d_y = ctx.open_cosets(key, _dev(_flat(p2)), logk, count=2, bitrev=rev, want_ys=False)
        assert d_y is None and _host(d_p) == want[0]
    import kzgmi
    assert kzgmi.open_cosets(key, _flat(p2), logk, count=2) == _model(curve, shape, TAU, 0, p2)
    # two jobs in flight on two slots
    sizes = [(2 << logk) * gb, (2 << (logk + logl)) * 32, (1 << logk) * gb, (1 << (logk + logl)) * 32]
    o = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in sizes]
    ctx.open_cosets_async(key, 0, _dev(_flat(p2)), 16, logk, o[1], o[0], count=2)
    ctx.open_cosets_async(key, 1, _dev(_flat(p1)), 13, logk, o[3], o[2], bitrev=True)
    assert ctx.wait(1) and ctx.wait(0)
    assert (_host(o[0]), _host(o[1])) == _model(curve, shape, TAU, 0, p2)
    assert (_host(o[2]), _host(o[3])) == _model(curve, shape, TAU, C.BITREV, p1)


_EIP = {}


def _eip_expected(ctx):
    """one blob's polynomial, the commit key's powers, and compute_cells_and_proofs' cells and proofs"""
    if not _EIP:
        import cellref as K
        import fk20ref as F
        import recoverref as RR
        rng = random.Random(0x7594)
        coeffs = [rng.randrange(K.R) for _ in range(K.BLOB_N)]
        srs = _gen(K.CURVE, F.srs_scalars(TAU))
        blob = RR.cells_to_bytes(RR.coeffs_to_cells(coeffs)[:64])
        pkey = ctx.load_cell_proof_key(srs)
        cells, proofs = ctx.compute_cells_and_proofs(pkey, _dev(blob), 1)
        _EIP.update(coeffs=coeffs, srs=srs, cells=_host(cells), proofs=_host(proofs))
        del pkey
    return _EIP


def test_eip_7594_shape(ctx):
    """BLS12-381 at (12, 6, 7), bit-reversed: the cells and proofs of compute_cells_and_proofs, accepted by
    verify_cell_batch"""
    import cellref as K
    want = _eip_expected(ctx)
    ck = ctx.load_commit_key(K.CURVE, want["srs"])
    key = ctx.load_open_cosets_key(ck, 12, 6)
    assert key.device_bytes == 2 * 4096 * 192  # 1.5 MiB
    proofs, ys = ctx.open_cosets(key, _fr(want["coeffs"]), 7, bitrev=True)
    assert ys == want["cells"]
    comp = O.g1_compress(K.CURVE, proofs, 128)
    assert comp == want["proofs"]
    idx = [0, 1, 5, 63, 64, 77, 126, 127]
    cells = [ys[2048 * i:2048 * (i + 1)] for i in idx]
    pf = [comp[48 * i:48 * (i + 1)] for i in idx]
    cm = K.commit(want["coeffs"], TAU)
    srs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
    args = (_dev(cm), _dev(struct.pack("<8Q", *([0] * 8))), _dev(struct.pack("<8Q", *idx)))
    r = K.challenge([cm], [0] * 8, idx, cells, pf)
    assert ctx.verify_cell_batch(srs, *args, _dev(b"".join(cells)), _dev(b"".join(pf)), m=1, n=8, r=r) is True
    bad = [cells[0][:-1] + bytes([cells[0][-1] ^ 1])] + cells[1:]
    r = K.challenge([cm], [0] * 8, idx, bad, pf)
    assert ctx.verify_cell_batch(srs, *args, _dev(b"".join(bad)), _dev(b"".join(pf)), m=1, n=8, r=r) is False


def test_round_trip_with_a_pairing_off_the_eip_shape(ctx, cks):
    """BN254 at (4, 2, 3): e(proof_e, [tau^l]_2) = e(C + z_e proof_e - [I_e(tau)]_1, [1]_2), I_e interpolated from ys"""
    curve = "bn254"
    Cv = pc.CURVES[curve]
    r, g = _rg(curve)
    logN, logl, logk = 4, 2, 3
    l, K = 1 << logl, 1 << logk
    gb = 2 * Cv.fp_bytes
    g2 = pk.g2_to_bytes(Cv.g2, Cv)
    tau_l_g2 = O.g2_mul(curve, g2, pow(TAU, l, r))
    rng = random.Random(173)
    coeffs = [rng.randrange(r) for _ in range(1 << logN)]
    cm = ctx.commit(cks[curve], _fr(coeffs))
    proofs, ys = ctx.open_cosets(_key(ctx, cks, curve, logN, logl), _fr(coeffs), logk)
    w = N.root(r, g, logk + logl)

    def check(e, ys):
        h, z = pow(w, e, r), pow(w, e * l, r)
        vals = [int.from_bytes(ys[32 * (e * l + j):32 * (e * l + j + 1)], "big") for j in range(l)]
        ci = N.dft(vals, logl, r, g, inverse=True)  # c_i h^i
        i_tau = sum(c * pow(h, -i, r) * pow(TAU, i, r) for i, c in enumerate(ci)) % r
        proof = proofs[e * gb:(e + 1) * gb]
        b = O.msm_g1(curve, cm + proof + _gen(curve, [(-i_tau) % r]), _fr([1, z, 1]), 3)
        return O.pairing_check(curve, proof, b, g2, tau_l_g2)

    for e in (1, 6):
        assert check(e, ys) is True
        bad = bytearray(ys)
        bad[32 * (e * l + 2) + 31] ^= 1
        assert check(e, bytes(bad)) is False


@pytest.mark.parametrize("curve", CURVES)
def test_degenerate_srs(ctx, curve):
    """tau a primitive cube root of unity: the powers take three values, so equal points, opposite sums and
    infinities meet all through the key's transforms, the sums of the products and the stages"""
    r, g = _rg(curve)
    shape = (6, 2, 4)
    tau = pow(g, (r - 1) // 3, r)
    assert tau != 1 and pow(tau, 3, r) == 1
    ck = ctx.load_commit_key(curve, _powers(curve, tau, 64))
    key = ctx.load_open_cosets_key(ck, 6, 2)
    rng = random.Random(172)
    for m in (63, 64):
        polys = _polys(rng, r, 1, m)
        for flags in (0, C.BITREV):
            assert ctx.open_cosets(key, _flat(polys), 4, bitrev=bool(flags)) == _model(curve, shape, tau, flags, polys)
    # all coefficients equal: the terms of a position are multiples of three points by scalars that repeat
    polys = (tuple([5] * 64),)
    assert ctx.open_cosets(key, _flat(polys), 4) == _model(curve, shape, tau, 0, polys)


@pytest.mark.parametrize("curve", CURVES)
def test_keys_and_errors(ctx, cks, curve):
    import kzgmi
    Cv = pc.CURVES[curve]
    r, _ = _rg(curve)
    gb = 2 * Cv.fp_bytes
    small = ctx.load_commit_key(curve, _powers(curve, TAU, 6))
    k31 = ctx.load_open_cosets_key(small, 3, 1)  # N - l = 6: exactly the commit key's powers
    assert (k31.logN, k31.logl) == (3, 1)
    five = ctx.load_commit_key(curve, _powers(curve, TAU, 5))
    for ck, logN, logl in ((five, 3, 1), (cks[curve], 2, 3), (cks[curve], 20, 10)):  # one power short; l > N; N > 2^19
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.load_open_cosets_key(ck, logN, logl)
        assert e.value.code == ERR_ARG
    shape = (3, 1, 2)
    logN, logl, logk = shape
    n, K, l = 8, 4, 2
    rng = random.Random(174)
    polys = _polys(rng, r, 1, n)
    coeffs = _flat(polys)
    want = _model(curve, shape, TAU, 0, polys)
    assert ctx.open_cosets(k31, coeffs, logk) == want  # the key of the smaller commit key computes the same
    fill_p, fill_y = bytes([0xA5]) * (4 * K * gb), bytes([0x5A]) * (4 * K * l * 32)

    def expect(code, context, key, cf, m, count=1, logk=logk, flags=0, off_c=0, off_y=0, off_p=0, y_in_p=False, c_in=None):
        p, y, c = _dev(fill_p), _dev(fill_y), _dev(cf + bytes(32))
        cp = {None: c.data_ptr() + off_c, "ys": y.data_ptr() + 16, "proofs": p.data_ptr() + 16}[c_in]
        rc = kzgmi.lib().kzgmi_open_cosets_device(context.handle, key.handle, cp, m, count, logk, flags,
                                                 (p.data_ptr() + 16 if y_in_p else y.data_ptr() + off_y), p.data_ptr() + off_p)
        assert rc == code, (rc, m, count, logk, flags)
        assert _host(p) == fill_p and _host(y) == fill_y

    other = kzgmi.Context(0, 1)
    try:
        expect(ERR_ARG, other, k31, coeffs, n)                       # a key of another context
    finally:
        other.close()
    expect(ERR_ARG, ctx, k31, coeffs + bytes(32), n + 1)             # m > N
    expect(ERR_ARG, ctx, k31, coeffs, n, flags=1)                    # KZGMI_NTT_INVERSE is not accepted
    expect(ERR_ARG, ctx, k31, coeffs, n, flags=4)                    # an unknown flag
    expect(ERR_ARG, ctx, k31, coeffs, n, logk=1)                     # K l < N
    expect(ERR_ARG, ctx, k31, coeffs, n, logk=20)                    # K l > 2^20
    expect(ERR_ARG, ctx, k31, coeffs, n, count=(1 << 16) + 1)        # count N > 2^19
    expect(ERR_ARG, ctx, k31, coeffs, n, count=3, logk=18)           # count K l > 2^20
    expect(ERR_ARG, ctx, k31, coeffs, n, off_c=8)                    # misaligned arrays
    expect(ERR_ARG, ctx, k31, coeffs, n, off_y=8)
    expect(ERR_ARG, ctx, k31, coeffs, n, off_p=8)
    expect(ERR_ARG, ctx, k31, coeffs, n, y_in_p=True)                # ys inside the proofs
    expect(ERR_ARG, ctx, k31, coeffs, n, c_in="ys")                  # the coefficients inside ys
    expect(ERR_ARG, ctx, k31, coeffs, n, c_in="proofs")              # the coefficients inside the proofs
    expect(ERR_SCALAR, ctx, k31, coeffs[:96] + r.to_bytes(32, "big") + coeffs[128:], n)  # a coefficient = r
    # count == 0 succeeds and writes nothing, in every form
    expect(0, ctx, k31, coeffs, n, count=0)
    assert ctx.open_cosets(k31, b"", logk, m=n, count=0) == (b"", b"")
    # the slot is usable afterwards, and a repeat call of the same shape allocates nothing
    assert ctx.open_cosets(k31, coeffs, logk) == want
    before = kzgmi.alloc_count()
    assert ctx.open_cosets(k31, coeffs, logk) == want and kzgmi.alloc_count() == before
    d = _dev(coeffs)
    got = ctx.open_cosets(k31, d, logk)
    before = kzgmi.alloc_count()
    again = ctx.open_cosets(k31, d, logk)
    assert (_host(again[0]), _host(again[1])) == (_host(got[0]), _host(got[1])) == want and kzgmi.alloc_count() == before
