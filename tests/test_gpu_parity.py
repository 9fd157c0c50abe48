"""HIP path vs the oracle (C restatement + golden fixtures from the Python spec).

Bar: bit-exact for every integer/point/Fp12 output (task rule 3).  Parity against the
reference itself is unpinned (the reference has no code or vectors).
"""
import hashlib
import os
import random

import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
SIZES = {"bls12_381": [4, 16, 256], "bn254": [4, 16, 64]}


def h(x):
    return bytes.fromhex(x)


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


def _context_with_env(slots=2, **env):
    """A kzgmi.Context created with the given environment overrides (read at creation)."""
    import kzgmi
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzgmi.Context(0, slots)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def bctx():
    """BLS12-381 calls of up to KZGMI_SMALL_TERMS terms take the one-wave-per-term path
    (csrc/msm_small.hpp); this context never does, so the bucket method's small-size corner cases
    stay covered."""
    c = _context_with_env(KZGMI_SMALL_TERMS="0")
    yield c
    c.close()


@pytest.fixture
def pctx(request, ctx, bctx):
    return ctx if request.param == "default" else bctx


PATHS = pytest.mark.parametrize("pctx", ["default", "buckets"], indirect=True)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_native_library_is_hip(ctx):
    import kzgmi
    assert b"gfx950" in kzgmi.lib().kzgmi_version()


def fp12_cube(curve, e: bytes) -> bytes:
    """e^3 of a tower-ordered big-endian Fp12 (kzgmi_pairing layout), via the pyspec's flat Fp12
    (inverting oracle/pyspec/pairing.py flat_to_tower: w^k coefficient (x, y) -> f[k] = x - beta y,
    f[k + 6] = y)."""
    from oracle.pyspec.pairing import f12_mul, flat_to_tower
    C = pc.CURVES[curve]
    fb = C.fp_bytes
    t = [int.from_bytes(e[i * fb:(i + 1) * fb], "big") for i in range(12)]
    f = [0] * 12
    for j, k in enumerate([0, 2, 4, 1, 3, 5]):
        x, y = t[2 * j], t[2 * j + 1]
        f[k + 6] = y
        f[k] = (x - C.beta * y) % C.p
    assert flat_to_tower(f, C) == t
    c = f12_mul(f12_mul(f, f, C), f, C)
    return b"".join(v.to_bytes(fb, "big") for v in flat_to_tower(c, C))


@pytest.mark.parametrize("curve", CURVES)
def test_pairing_golden(ctx, curve, golden):
    """kzgmi_pairing is the standard e(P, Q).  The golden values (pyspec) and the oracle give
    e^3 on BLS12-381 (the hard part of their final exponentiation is the x-chain of 3 (p^4 - p^2 +
    1) / r), so there the GPU value is checked as e(P, Q) = e([3^-1 mod r] P, Q)^3 against the
    oracle, and cubed against the golden e^3 (a cube in the order-r group G_T)."""
    g = golden("%s_pairing.json" % curve)
    for P, Q, key in ((g["g1"], g["g2"], "e_g1_g2"), (g["aP"], g["bQ"], "e_aP_bQ")):
        e = ctx.pairing(curve, h(P), h(Q))
        if curve == "bn254":
            assert e.hex() == g[key]
            continue
        inv3 = pow(3, -1, pc.CURVES[curve].r).to_bytes(32, "big")
        P3 = O.msm_g1(curve, h(P), inv3, 1)
        assert e == O.pairing(curve, P3, h(Q)), key
        assert fp12_cube(curve, e) == h(g[key]), key


@PATHS
@pytest.mark.parametrize("curve", CURVES)
def test_msm_golden(pctx, curve, golden):
    g = golden("%s_msm.json" % curve)
    for case in g["cases"]:
        got = pctx.msm_g1(curve, h(case["points"]), h(case["scalars"]))
        assert got.hex() == case["expected"], case["name"]


@PATHS
@pytest.mark.parametrize("curve", CURVES)
def test_batch_golden(pctx, curve, golden):
    for n in SIZES[curve]:
        g = golden("%s_batch_n%d.json" % (curve, n))
        srs = pctx.load_srs(curve, h(g["g2"]), h(g["tau_g2"]))
        for key in ["valid", "neg_flip_y", "neg_swap_proofs"]:
            src = g if key == "valid" else g[key]
            exp = g[key]
            ok = pctx.batch_verify(srs, h(src["commitments"]), h(src["zs"]), h(src["ys"]), h(src["proofs"]),
                                  seed=h(g["seed"]))
            A, B = pctx.last_combination(curve)
            assert A.hex() == exp["A"], (n, key)
            assert B.hex() == exp["B"], (n, key)
            assert ok == exp["ok"], (n, key)


@pytest.mark.parametrize("curve", CURVES)
def test_genuine_kzg(ctx, curve, golden):
    g = golden("%s_genuine_kzg.json" % curve)
    srs = ctx.load_srs(curve, h(g["g2"]), h(g["tau_g2"]))
    assert ctx.batch_verify(srs, h(g["commitments"]), h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
    assert ctx.batch_verify(srs, h(g["commitments"]), h(g["zs"]), h(g["ys"]), h(g["proofs"]))  # OS seed


@pytest.mark.parametrize("curve", CURVES)
def test_errors_and_empty(ctx, curve, golden):
    import kzgmi
    C = pc.CURVES[curve]
    g = golden("%s_batch_n4.json" % curve)
    srs = ctx.load_srs(curve, h(g["g2"]), h(g["tau_g2"]))
    assert ctx.batch_verify(srs, b"", b"", b"", b"", seed=h(g["seed"])) is True
    zs = bytearray(h(g["zs"]))
    zs[32:64] = C.r.to_bytes(32, "big")
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.batch_verify(srs, h(g["commitments"]), bytes(zs), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
    assert e.value.code == -4
    cm = bytearray(h(g["commitments"]))
    cm[2 * C.fp_bytes - 1] ^= 1
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.batch_verify(srs, bytes(cm), h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
    assert e.value.code == -3
    # the context keeps working after an error
    assert ctx.batch_verify(srs, h(g["commitments"]), h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))


@pytest.mark.parametrize("curve", CURVES)
def test_uncompressed_point_validation(ctx, curve, golden):
    """Every uncompressed-point rule through the batch conversion (radix-29 store for
    BLS12-381) and the MSM conversion, against the oracle's MSM on the valid cases."""
    import kzgmi
    C = pc.CURVES[curve]
    g = golden("%s_batch_n4.json" % curve)
    srs = ctx.load_srs(curve, h(g["g2"]), h(g["tau_g2"]))
    g1b = 2 * C.fp_bytes
    cm = h(g["commitments"])
    rng = random.Random(41)
    pts = b"".join(pk.g1_to_bytes(pc.g1_mul(C.g1, rng.randrange(1, C.r), C), C) for _ in range(5))
    sc = b"".join(rng.randrange(C.r).to_bytes(32, "big") for _ in range(5))
    from pointcases import invalid_uncompressed
    for enc, err in invalid_uncompressed(C, rng):
        bad = cm[:g1b] + enc + cm[2 * g1b:]
        bad_pts = pts[:2 * g1b] + enc + pts[3 * g1b:]
        if err is None:  # the identity: a valid input that breaks the batch equation
            assert ctx.batch_verify(srs, bad, h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"])) is False
            assert ctx.msm_g1(curve, bad_pts, sc) == O.msm_g1(curve, bad_pts, sc, 5)
            continue
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.batch_verify(srs, bad, h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
        assert e.value.code == err, enc.hex()
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.msm_g1(curve, bad_pts, sc)
        assert e.value.code == err, enc.hex()
    assert ctx.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, 5)


@PATHS
@pytest.mark.parametrize("curve", CURVES)
def test_msm_random_vs_oracle(pctx, curve):
    C = pc.CURVES[curve]
    rng = random.Random(17)
    for n in [1, 2, 31, 33, 1000, 5000]:
        ks = [rng.randrange(C.r) for _ in range(n)]
        pts = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), n)
        sc = b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n))
        assert pctx.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, n), n


@PATHS
@pytest.mark.parametrize("curve", CURVES)
def test_msm_infinity_and_zero_terms(pctx, curve):
    """Points at infinity, zero scalars, a point with its negation and repeated points among the
    terms (the one-wave-per-term path's tree adds O + P, P + P and P + (-P) leaves), sizes around
    the small path's term limit and a one-term MSM."""
    C = pc.CURVES[curve]
    rng = random.Random(97)
    g1b = 2 * C.fp_bytes
    inf_pt = (b"\x40" + b"\x00" * (g1b - 1)) if curve == "bls12_381" else b"\x00" * g1b
    ks = [rng.randrange(1, C.r) for _ in range(8)]
    base = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks + [C.r - ks[0]]), 9)
    pt = lambda j: base[j * g1b:(j + 1) * g1b]  # noqa: E731
    for n in [1, 2, 3, 7, 64, 513]:
        terms, scal = [], []
        for i in range(n):
            kind = rng.randrange(6)
            terms.append(inf_pt if kind == 0 else pt(8) if kind == 1 else pt(i % 8))
            scal.append(0 if kind == 2 else rng.randrange(C.r))
        pb = b"".join(terms)
        sb = b"".join(pk.fr_to_bytes(x) for x in scal)
        assert pctx.msm_g1(curve, pb, sb) == O.msm_g1(curve, pb, sb, n), n
    # P and -P with equal scalars: the sum is O
    pb = pt(0) + pt(8)
    sb = pk.fr_to_bytes(12345) * 2
    assert pctx.msm_g1(curve, pb, sb) == O.msm_g1(curve, pb, sb, 2)


@PATHS
@pytest.mark.parametrize("curve", CURVES)
def test_msm_reduction_special_cases(pctx, curve):
    """Adjacent buckets whose sums cancel or coincide, so that the bucket-sum reduction's running
    sums hit P + (-P) = O and P + P (the doubling branch of its general addition):
    digits 8, 7, 6, 5 on P, -P, P, P (buckets 7..4 of the first segment half) = 12 P, plus the
    same pattern repeated in a high window and a lone top-bucket digit (acc + run = 2 run), and
    digits in the upper halves of segments (the V records)."""
    C = pc.CURVES[curve]
    rng = random.Random(83)
    k = rng.randrange(1, C.r)
    base = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(x) for x in [k, C.r - k]), 2)
    g1b = 2 * C.fp_bytes
    P, nP = base[:g1b], base[g1b:]
    cases = [
        ([P, nP, P, P], [8, 7, 6, 5]),
        ([P, nP, P, P], [8 << 48, 7 << 48, 6 << 48, 5 << 48]),
        ([P], [8]),
        ([P, P], [8, 7]),
        ([P, nP], [16, 15]),
        # upper segment halves (buckets 8..15): their sums leave k_reduce_segments as V records,
        # scaled by 8 once per set in k_reduce_bits_finish
        ([P], [9]),
        ([P, P], [9, 1]),
        ([P, P, nP, P], [16, 12, 11, 9]),
        ([P, nP, P, P, P], [24, 23, 9, 17, 32]),
        ([P, P, P], [16 << 16, 9 << 16, 8 << 16]),
    ]
    for pts, sc in cases:
        pb = b"".join(pts)
        sb = b"".join(pk.fr_to_bytes(x) for x in sc)
        assert pctx.msm_g1(curve, pb, sb) == O.msm_g1(curve, pb, sb, len(pts)), sc


@pytest.mark.parametrize("curve", CURVES)
def test_msm_skewed_buckets(ctx, curve):
    """Adversarial digit distribution: one huge bucket (all scalars equal) + duplicates."""
    C = pc.CURVES[curve]
    rng = random.Random(5)
    n = 3000
    ks = [rng.randrange(C.r) for _ in range(50)]
    base = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), 50)
    g1b = 2 * C.fp_bytes
    pts = b"".join(base[(i % 50) * g1b:(i % 50 + 1) * g1b] for i in range(n))
    for sc in [b"".join(pk.fr_to_bytes(7) for _ in range(n)),
               b"".join(pk.fr_to_bytes(C.r - 1) for _ in range(n)),
               b"".join(pk.fr_to_bytes(rng.choice([1, 2, 3, 65535, 65536])) for _ in range(n))]:
        assert ctx.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, n)


@pytest.mark.parametrize("curve", CURVES)
def test_msm_skewed_large_bins(ctx, curve):
    """Coarse bins above the fine sort's 8192-entry staging array (k_fine_sort's chunked path):
    one bucket per window holding every term (it spans several 4096-entry chunks, so its
    first-of-bucket flag and running cursor cross chunk boundaries), and a few heavy buckets
    sharing one coarse bin (digits 1..5)."""
    C = pc.CURVES[curve]
    rng = random.Random(41)
    n = 20000
    ks = [rng.randrange(C.r) for _ in range(64)]
    base = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), 64)
    g1b = 2 * C.fp_bytes
    pts = b"".join(base[(i % 64) * g1b:(i % 64 + 1) * g1b] for i in range(n))
    for sc in [b"".join(pk.fr_to_bytes(0x1234567) for _ in range(n)),
               b"".join(pk.fr_to_bytes(rng.choice([1, 2, 3, 4, 5])) for _ in range(n))]:
        assert ctx.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, n)


@pytest.mark.parametrize("curve", CURVES)
def test_split_sort_entries(curve, golden):
    """The sort's split coarse-pass entries (4-B value + 1-B fine index, used from 2^24 points
    on) at small sizes: a context made with KZGMI_SORT_SPLIT=1 uses them for every call.  Golden
    batches (A, B, verdict) and the large-bin skewed MSMs against the oracle."""
    import kzgmi
    old = os.environ.get("KZGMI_SORT_SPLIT")
    os.environ["KZGMI_SORT_SPLIT"] = "1"
    try:
        c = kzgmi.Context(0, 1)
    finally:
        if old is None:
            del os.environ["KZGMI_SORT_SPLIT"]
        else:
            os.environ["KZGMI_SORT_SPLIT"] = old
    try:
        for n in SIZES[curve]:
            g = golden("%s_batch_n%d.json" % (curve, n))
            srs = c.load_srs(curve, h(g["g2"]), h(g["tau_g2"]))
            ok = c.batch_verify(srs, h(g["commitments"]), h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
            A, B = c.last_combination(curve)
            assert (A.hex(), B.hex(), ok) == (g["valid"]["A"], g["valid"]["B"], g["valid"]["ok"]), n
        C = pc.CURVES[curve]
        g1b = 2 * C.fp_bytes
        base = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in range(3, 67)), 64)
        n = 20000
        pts = b"".join(base[(i % 64) * g1b:(i % 64 + 1) * g1b] for i in range(n))
        rng = random.Random(43)
        for sc in [b"".join(pk.fr_to_bytes(0x1234567) for _ in range(n)),
                   b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n))]:
            assert c.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, n)
    finally:
        c.close()


@pytest.mark.parametrize("curve", CURVES)
def test_accumulation_work_queue(curve, golden):
    """k_accumulate's work-queue form (calls whose grid reaches the cap): a context whose cap is
    256 threads (KZGMI_ACC_THREADS) with 8 chunks per thread (KZGMI_ACC_QUEUE), and the queue
    enabled at every size (KZGMI_ACC_QUEUE_FROM=0; by default only calls of >= 2^26 entries use it),
    makes every wave take several 64-chunk groups from the counter.  Random and skewed MSMs (one bucket cut into
    many chunk pieces: the two-level join) against the oracle, and the largest golden batch
    (below the queue's 32-entry minimum chunk: the static grid) through the same context."""
    import kzgmi
    saved = {k: os.environ.get(k) for k in ("KZGMI_ACC_THREADS", "KZGMI_ACC_QUEUE", "KZGMI_ACC_QUEUE_FROM")}
    os.environ.update(KZGMI_ACC_THREADS="256", KZGMI_ACC_QUEUE="8", KZGMI_ACC_QUEUE_FROM="0")
    try:
        c = kzgmi.Context(0, 1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        C = pc.CURVES[curve]
        rng = random.Random(59)
        n = 5000
        ks = [rng.randrange(C.r) for _ in range(n)]
        pts = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), n)
        for sc in [b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n)),
                   b"".join(pk.fr_to_bytes(0x1234567) for _ in range(n)),
                   b"".join(pk.fr_to_bytes(rng.choice([1, 2, 3, 65535])) for _ in range(n))]:
            assert c.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, n)
        g = golden("%s_batch_n%d.json" % (curve, SIZES[curve][-1]))
        srs = c.load_srs(curve, h(g["g2"]), h(g["tau_g2"]))
        ok = c.batch_verify(srs, h(g["commitments"]), h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
        A, B = c.last_combination(curve)
        assert (A.hex(), B.hex(), ok) == (g["valid"]["A"], g["valid"]["B"], g["valid"]["ok"])
    finally:
        c.close()


@PATHS
@pytest.mark.parametrize("curve", CURVES)
def test_msm_cancelling_buckets(pctx, curve):
    """Buckets whose running sum returns to infinity mid-chunk (P + (-P)), then keeps adding
    (the accumulation's infinity flag, csrc/msm.hpp acc_loop29), doubling (P + P),
    pieces that cancel across chunk boundaries (k_fixup), and an all-cancelling MSM (result
    infinity).  Equal scalars put every term of a window into one bucket."""
    C = pc.CURVES[curve]
    rng = random.Random(29)
    ks = [rng.randrange(1, C.r) for _ in range(6)]
    allk = ks + [C.r - k for k in ks]  # P_j, then -P_j
    base = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in allk), len(allk))
    g1b = 2 * C.fp_bytes
    pt = lambda j: base[j * g1b:(j + 1) * g1b]  # noqa: E731
    cases = [
        [pt(0), pt(6)] * 1500 + [pt(1), pt(2)],                      # +-P0 pairs, then two survivors
        [pt(0), pt(0), pt(6), pt(6), pt(1)] * 700,                   # P0 + P0 doublings, -P0 cancels
        [pt(j % 6) for j in range(2000)] + [pt(6 + j % 6) for j in range(2000)],  # all cancel: O
        [pt(3), pt(9)] * 40 + [pt(4)],                               # short: single chunk
    ]
    try:
        for trusted in (False, True):  # True: points declared G1 members -> GLV split path
            pctx.set_trusted_g1(trusted)
            for terms in cases:
                n = len(terms)
                pts = b"".join(terms)
                for s in [5, C.r - 3, 0x10000]:
                    sc = b"".join(pk.fr_to_bytes(s) for _ in range(n))
                    assert pctx.msm_g1(curve, pts, sc) == O.msm_g1(curve, pts, sc, n), (trusted, n, s)
    finally:
        pctx.set_trusted_g1(False)


@pytest.mark.parametrize("curve", CURVES)
def test_gen_g1_vs_oracle(ctx, curve, torch_dev):
    torch = torch_dev
    C = pc.CURVES[curve]
    rng = random.Random(23)
    n = 777
    sc = b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n))
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
    out = torch.empty(n * 2 * C.fp_bytes, dtype=torch.uint8, device="cuda")
    ctx.gen_g1(curve, d_sc, n, out)
    assert out.cpu().numpy().tobytes() == O.g1_mul_gen(curve, sc, n)


def _gen_batch(ctx, torch, curve, n, tau, seed):
    C = pc.CURVES[curve]
    g1b = 2 * C.fp_bytes
    Cm = torch.empty(n * g1b, dtype=torch.uint8, device="cuda")
    P = torch.empty(n * g1b, dtype=torch.uint8, device="cuda")
    z = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    y = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    ctx.gen_tuples(curve, tau, seed, n, Cm, z, y, P)
    return Cm, z, y, P


@pytest.mark.parametrize("curve", CURVES)
def test_generated_batch_vs_oracle(ctx, curve, torch_dev):
    torch = torch_dev
    C = pc.CURVES[curve]
    n, tau = 2000, 0x1234567890ABCDEF1234567890
    seed = hashlib.sha256(b"gen").digest()
    Cm, z, y, P = _gen_batch(ctx, torch, curve, n, tau, seed)
    # host-side restatement of the generator for a few tuples
    import kzgmi
    for i in [0, 1, n - 1]:
        c = kzgmi.tuple_scalars_host(seed, i, "c")
        zi = kzgmi.tuple_scalars_host(seed, i, "z")
        assert z[32 * i:32 * i + 32].cpu().numpy().tobytes() == zi.to_bytes(32, "big")
        assert Cm[i * 2 * C.fp_bytes:(i + 1) * 2 * C.fp_bytes].cpu().numpy().tobytes() == \
            O.g1_mul_gen(curve, pk.fr_to_bytes(c), 1)
    g2 = pk.g2_to_bytes(C.g2, C)
    tg2 = O.g2_mul(curve, g2, tau)
    srs = ctx.load_srs(curve, g2, tg2)
    vseed = hashlib.sha256(b"verify").digest()
    assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=n) is True
    A, B = ctx.last_combination(curve)
    hb = [t.cpu().numpy().tobytes() for t in (Cm, z, y, P)]
    ok, Ao, Bo = O.batch_verify(curve, hb[0], hb[1], hb[2], hb[3], n, g2, tg2, vseed, want_ab=True)
    assert ok and A == Ao and B == Bo
    # corrupt one evaluation
    y2 = y.clone()
    y2[32 * 1234 + 31] ^= 1
    assert ctx.batch_verify(srs, Cm, z, y2, P, seed=vseed, n=n) is False


@pytest.mark.parametrize("curve", CURVES)
def test_evaluation_point_at_tau(ctx, curve, torch_dev):
    """SURVEY.md 4.4's last negative case: one tuple opened at z_i = tau (the trapdoor itself) with
    its proof left as generated.  The check must reject, and A, B match the oracle bit for bit (the
    point is a regular scalar to both: nothing special-cases z = tau)."""
    torch = torch_dev
    C = pc.CURVES[curve]
    n, tau = 300, 0x1234567890ABCDEF1234567890
    Cm, z, y, P = _gen_batch(ctx, torch, curve, n, tau, hashlib.sha256(b"z-at-tau").digest())
    g2 = pk.g2_to_bytes(C.g2, C)
    tg2 = O.g2_mul(curve, g2, tau)
    srs = ctx.load_srs(curve, g2, tg2)
    vseed = hashlib.sha256(b"verify-tau").digest()
    assert ctx.batch_verify(srs, Cm, z, y, P, seed=vseed, n=n) is True
    z2 = z.clone()
    z2[32 * 77:32 * 78] = torch.frombuffer(bytearray(tau.to_bytes(32, "big")), dtype=torch.uint8).cuda()
    assert ctx.batch_verify(srs, Cm, z2, y, P, seed=vseed, n=n) is False
    A, B = ctx.last_combination(curve)
    hb = [t.cpu().numpy().tobytes() for t in (Cm, z2, y, P)]
    ok, Ao, Bo = O.batch_verify(curve, hb[0], hb[1], hb[2], hb[3], n, g2, tg2, vseed, want_ab=True)
    assert ok is False and A == Ao and B == Bo


@pytest.mark.parametrize("curve", CURVES)
def test_async_slots(ctx, curve, torch_dev):
    torch = torch_dev
    C = pc.CURVES[curve]
    n, tau = 3000, 987654321
    seed = hashlib.sha256(b"async").digest()
    Cm, z, y, P = _gen_batch(ctx, torch, curve, n, tau, seed)
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(curve, g2, O.g2_mul(curve, g2, tau))
    y_bad = y.clone()
    y_bad[5] ^= 1
    ctx.batch_verify_async(srs, 0, Cm, z, y, P, n, seed=seed)
    ctx.batch_verify_async(srs, 1, Cm, z, y_bad, P, n, seed=seed)
    assert ctx.wait(0) is True
    assert ctx.wait(1) is False


def test_async_accumulation_order(torch_dev):
    """The accumulation order across slots (host.hpp kzgmi_ctx::acc_order, forced on here although 8
    slots may share hardware queues): 20 batches of four sizes (both order depths: 2^18 is above
    ACC_ORDER_WIDE) and pipelined MSMs on 8 slots, verdicts and MSM results as submitted, the
    last slots collected out of submission order."""
    torch = torch_dev
    curve = "bls12_381"
    C = pc.CURVES[curve]
    c8 = _context_with_env(8, KZGMI_ACC_ORDER="2", KZGMI_ACC_ORDER_SMALL="3")
    try:
        tau = 0x5EED
        g2 = pk.g2_to_bytes(C.g2, C)
        srs = c8.load_srs(curve, g2, O.g2_mul(curve, g2, tau))
        seed = hashlib.sha256(b"order").digest()
        batches = {}
        sizes = (3000, 20000, 1 << 17, 1 << 18)  # 2^18: 10.5 M window entries, the large-call order depth
        for n in sizes:
            Cm, z, y, P = _gen_batch(c8, torch, curve, n, tau, seed)
            y_bad = y.clone()
            y_bad[32 * (n // 2) + 31] ^= 1
            batches[n] = (Cm, z, y, P, y_bad)
        rng = random.Random(5)
        m = 2048
        pts = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(m)), m)
        sc = b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(m))
        dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
        ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
        want_msm = O.msm_g1(curve, pts, sc, m)
        pending = {}  # slot -> expected outcome ("msm" or a verdict)

        def collect(s):
            exp = pending.pop(s)
            if exp == "msm":
                assert c8.msm_wait(s) == want_msm, s
            else:
                assert c8.wait(s) is exp, s

        for k in range(20):
            s = (5 * k) % 8
            if s in pending:
                collect(s)
            if k % 7 == 3:
                c8.msm_g1_async(curve, s, dp, ds, m)
                pending[s] = "msm"
                continue
            n = sizes[k % 4]
            Cm, z, y, P, y_bad = batches[n]
            bad = k % 5 == 1
            c8.batch_verify_async(srs, s, Cm, z, y_bad if bad else y, P, n, seed=seed)
            pending[s] = not bad
        for s in sorted(pending, reverse=True):  # newest-first is not submission order
            collect(s)
    finally:
        c8.close()


@pytest.mark.slow
def test_bench_shape_pipeline_vs_oracle(torch_dev):
    """The headline's exact shape (bench.py: 16 slots x 2^20 BLS12-381 tuples, accumulation order
    D = 2, forced here since this process may share hardware queues): 40 submissions round the
    slots with two corrupted batches in flight among valid ones -- every verdict as submitted --
    and one slot's job mid-pipeline a shard partial whose A, B are bit-exact vs the oracle."""
    torch = torch_dev
    curve = "bls12_381"
    C = pc.CURVES[curve]
    n, tau = 1 << 20, 0xBE9C4
    c16 = _context_with_env(16, KZGMI_ACC_ORDER="2", KZGMI_ACC_ORDER_SMALL="4")
    try:
        g2 = pk.g2_to_bytes(C.g2, C)
        tg2 = O.g2_mul(curve, g2, tau)
        srs = c16.load_srs(curve, g2, tg2)
        seed = hashlib.sha256(b"bench-shape").digest()
        Cm, z, y, P = _gen_batch(c16, torch, curve, n, tau, hashlib.sha256(b"bench-shape-tuples").digest())
        y_bad = y.clone()
        y_bad[32 * (n // 2) + 31] ^= 1
        part = torch.empty(2 * c16.partial_bytes(curve), dtype=torch.uint8, device="cuda")
        pending = {}
        for k in range(40):
            s = k % 16
            if s in pending:
                exp = pending.pop(s)
                assert c16.wait(s) is (True if exp == "partial" else exp), (k, s)
            if k == 20:
                c16.batch_partial_async(srs, s, Cm, z, y, P, n, 0, seed, part)
                pending[s] = "partial"
                continue
            bad = k in (7, 23)
            c16.batch_verify_async(srs, s, Cm, z, y_bad if bad else y, P, n, seed=seed)
            pending[s] = not bad
        for s in sorted(pending):
            exp = pending.pop(s)
            assert c16.wait(s) is (True if exp == "partial" else exp), s
        hb = [t.cpu().numpy().tobytes() for t in (Cm, z, y, P)]
        ok, Ao, Bo = O.batch_verify(curve, hb[0], hb[1], hb[2], hb[3], n, g2, tg2, seed, want_ab=True)
        assert ok is True
        assert c16.partial_encode(curve, part, 2) == [Ao, Bo]
        del srs
    finally:
        c16.close()


@pytest.mark.parametrize("curve", CURVES)
def test_async_msm_slots(ctx, curve, torch_dev):
    """Pipelined MSM: two different MSMs in flight on slots 0/1, each bit-exact vs the oracle;
    the empty MSM and a slot reused after wait; misuse errors."""
    import kzgmi
    torch = torch_dev
    C = pc.CURVES[curve]
    rng = random.Random(71)
    n = 1500
    pts = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n)), n)
    sc0 = b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n))
    sc1 = b"".join(pk.fr_to_bytes(rng.randrange(1 << 64)) for _ in range(n))
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    dp, d0, d1 = dev(pts), dev(sc0), dev(sc1)
    ctx.msm_g1_async(curve, 0, dp, d0, n)
    ctx.msm_g1_async(curve, 1, dp, d1, n - 7)
    with pytest.raises(kzgmi.KzgmiError):
        ctx.msm_g1_async(curve, 0, dp, d0, n)  # slot busy
    assert ctx.msm_wait(1) == O.msm_g1(curve, pts[:(n - 7) * 2 * C.fp_bytes], sc1[:(n - 7) * 32], n - 7)
    assert ctx.msm_wait(0) == O.msm_g1(curve, pts, sc0, n)
    with pytest.raises(kzgmi.KzgmiError):
        ctx.msm_wait(0)  # nothing pending
    ctx.msm_g1_async(curve, 0, dp, d0, 0)
    assert ctx.msm_wait(0) == O.msm_g1(curve, b"", b"", 0)


@pytest.mark.gpu
def test_sharded_pipeline_rccl_world1(ctx, torch_dev):
    """kzgmi.distributed.ShardedPipeline on the device over a world-1 RCCL group: async shard
    partials, all-gather, async combine on the combine slot; verdicts in submission order."""
    import socket
    import torch.distributed as dist
    from kzgmi.distributed import ShardedPipeline
    torch = torch_dev
    curve = "bls12_381"
    C = pc.CURVES[curve]
    n, tau = 700, 99
    seed = hashlib.sha256(b"pipe").digest()
    Cm, z, y, P = _gen_batch(ctx, torch, curve, n, tau, seed)
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(curve, g2, O.g2_mul(curve, g2, tau))
    ybad = y.clone()
    ybad[31] ^= 1
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    created = not dist.is_initialized()
    if created:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pipe = ShardedPipeline(ctx, srs, slots=1, lanes=1)  # ctx has 2 slots: 1 shard slot + 1 combine lane
        out = []
        for b in range(5):
            out += pipe.submit(Cm, z, ybad if b in (1, 4) else y, P, n, 0, seed)
        out += pipe.drain()
        assert out == [True, False, True, True, False]
    finally:
        if created:
            dist.destroy_process_group()


def test_sharded_msm_pipeline_rccl_world1(ctx, torch_dev):
    """kzgmi.distributed.ShardedMsmPipeline over a world-1 RCCL group: async shard partials,
    all-gather, async combine; results in submission order, bit-exact vs the oracle."""
    import socket
    import torch.distributed as dist
    from kzgmi.distributed import ShardedMsmPipeline
    torch = torch_dev
    curve = "bls12_381"
    C = pc.CURVES[curve]
    rng = random.Random(72)
    n = 900
    pts = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n)), n)
    scs = [b"".join(pk.fr_to_bytes(rng.randrange(C.r)) for _ in range(n)) for _ in range(2)]
    want = [O.msm_g1(curve, pts, sc, n) for sc in scs]
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    dp, dsc = dev(pts), [dev(sc) for sc in scs]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    created = not dist.is_initialized()
    if created:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pipe = ShardedMsmPipeline(ctx, curve, slots=1, lanes=1)
        out = []
        order = [0, 1, 1, 0, 1]
        for b in order:
            out += pipe.submit(dp, dsc[b], n)
        out += pipe.drain()
        assert out == [want[b] for b in order]
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.gpu
def test_srs_outliving_context(torch_dev, golden):
    """An Srs freed after its Context was closed must not touch the destroyed context (it used
    to leave a sticky 'invalid device ordinal' in the HIP runtime)."""
    import gc
    import kzgmi
    torch = torch_dev
    g = golden("bls12_381_batch_n4.json")
    c = kzgmi.Context(0, 1)
    srs = c.load_srs("bls12_381", h(g["g2"]), h(g["tau_g2"]))
    c.close()
    del srs
    gc.collect()
    x = torch.ones(8, device="cuda") * 2
    torch.cuda.synchronize()
    assert x.sum().item() == 16
    c2 = kzgmi.Context(0, 1)
    srs2 = c2.load_srs("bls12_381", h(g["g2"]), h(g["tau_g2"]))
    assert c2.batch_verify(srs2, h(g["commitments"]), h(g["zs"]), h(g["ys"]), h(g["proofs"]), seed=h(g["seed"]))
    c2.close()
