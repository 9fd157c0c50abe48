"""The model of the G1 point layer (tests/pointref.py) without a GPU.

1. Every case's preconditions: operands inside the input contracts, the subgroup verdicts by
   definition ([r]P = O), the chain of the order-3 points really going through infinity and out again
   (no prefix of |x| vanishes mod 11 or a larger cofactor prime, which is asserted too), the edge of
   the compression flag held by no curve point, every half scalar below 2^127, Barrett corrections as
   the case list claims.
2. The model against the C oracle where the oracle has the operation: O.g1_decompress, O.g1_compress,
   O.g1_subgroup_check, O.g1_mul_gen (and against oracle.pyspec's decoders).
3. Every checker on the outputs a correct kernel returns (no report) and on planted faults (a report
   each): the doubling result where infinity is due, y negated, a coordinate one p past its bound,
   ZZ^3 != ZZZ^2, a half scalar moved by one lattice vector (still a valid decomposition), a wrong
   error code, a non-zero slot under a rejected point, an overwritten guard.
"""
import random

import pytest

import fieldref as F
import pointcases
import pointref as R
import test_glv
from oracle import oracle as O
from oracle.pyspec import curves as pc
from oracle.pyspec import glv
from oracle.pyspec import kzg as pk

CURVES = R.CURVES
BLS = pc.BLS12_381


# ---------------------------------------------------------------------------- 1. preconditions
def test_registry_matches_probe_source():
    """Every op and stage id has cases; the ids are what tests/native/points_probe.hip registers."""
    import os
    src = open(os.path.join(R.F.ROOT, "tests", "native", "points_probe.hip")).read()
    for curve, op in R.all_op_ids():
        assert '"%s"' % op in src, op
        assert R.op_of(curve, op).cases
    assert len(set(R.all_stage_ids())) == len(R.all_stage_ids())


@pytest.mark.parametrize("curve", CURVES)
def test_special_points_and_lambdas(curve):
    K = R.curve_of(curve)
    C, p = K.C, K.p
    for P in K.specials():
        assert pc.g1_on_curve(P, C)
    if curve == "bls12_381":
        for T in K.specials():                     # order 3: 2T = -T
            assert pc.g1_add(T, T, C) == pc.g1_neg(T, C) and not pc.g1_in_subgroup(T, C)
    else:
        assert {P[0] for P in K.specials()} == {1, p - 1}
    lams = K.lams(random.Random(1))
    assert lams[:4] == [1, 2, p - 1, (p + 1) // 2] and all(l % p for l in lams)
    # equal points under independent scalings have unequal coordinates
    pairs = R.op_of(curve, "g1.xyzz_add").cases
    assert any(P == Q and l1 != l2 and K.xyzzw(P, l1) != K.xyzzw(Q, l2) for P, l1, Q, l2 in pairs if P is not None)
    kinds = {(P is None, Q is None) for P, _, Q, _ in pairs}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert any(P is not None and Q == pc.g1_neg(P, C) for P, _, Q, _ in pairs)


def test_subgroup_cases_by_definition():
    mem, non = R.subgroup_points()
    assert len(mem) == 67 and len(non) == 64 + 2 * len(R.COFACTOR_PRIMES)
    for P, tag in mem:
        assert pc.g1_on_curve(P, BLS) and pc.g1_in_subgroup(P, BLS), tag
    for P, tag in non:
        assert pc.g1_on_curve(P, BLS) and not pc.g1_in_subgroup(P, BLS), tag
    assert pointcases.COFACTOR == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2
    small = {tag: P for P, tag in non if tag.startswith("order")}
    for ell in R.COFACTOR_PRIMES:
        T = small["order %d" % ell]
        assert pc.g1_mul_unreduced(T, ell, BLS) is None
    walk = R.single_launch_members()
    assert len(walk) == 600 == len(set(walk))
    for P in walk[::37] + [walk[q] for q in R.SINGLE_POSITIONS]:
        assert pc.g1_in_subgroup(P, BLS)
    # members by construction: multiples of the generator
    st = R.stage_of("bls12_381", "subgroup_check", "single256")
    assert [i for i, e in enumerate(st.err_codes) if e] == [256]
    each = R.stage_of("bls12_381", "subgroup_check", "each")
    flagged = [(P, inf) for P, inf, _ in each.cases if inf]
    assert any(not pc.g1_on_curve(P, BLS) for P, _ in flagged)


def test_order3_chain_goes_through_infinity():
    """[|x|]T for T of order 3 by the chain's own steps: the running multiple X >> b vanishes mod 3 at
    a prefix that ends on a set bit (the addition cancels: infinity), doublings of infinity follow,
    and the next set bit leaves infinity through O + q.  So the cancelling branch, dbl(O) and O + q
    all run in mul_by_x_abs29 for the order-3 cases."""
    X, ell = R.X_ABS, 3
    van = R.vanishing_prefixes(ell)
    assert van == [62, 61, 57] + list(range(56, 48, -1))
    b = van[0]
    assert (X >> b) & 1, "the multiple vanishes on an addition (the cancelling branch)"
    assert b - 1 in van, "a doubling of infinity follows"
    lower = [k for k in range(b - 1, -1, -1) if (X >> k) & 1]
    assert lower and (X >> lower[0]) % ell == 1, "the next set bit leaves infinity through O + q"
    for T in R.curve_of("bls12_381").specials() + [pointcases.small_order_point(3)]:
        acc, seen_inf, left_inf = T, False, False
        for k in range(62, -1, -1):
            acc = pc.g1_add(acc, acc, BLS)
            if (X >> k) & 1:
                was = acc is None
                acc = pc.g1_add(acc, T, BLS)
                left_inf |= was and acc is not None
            seen_inf |= acc is None
        assert seen_inf and left_inf and acc == pc.g1_mul_unreduced(T, X, BLS) == pc.g1_neg(T, BLS)


def test_other_small_orders_never_reach_infinity():
    """No prefix of |x| vanishes mod 11, 10177, 859267 or 52437899 (a doubling keeps the prefix, so
    only prefixes matter): points of those orders run the chain's general branches only and are
    rejected by the final comparison, [|x|]T = -T.  Only order 3 drives the chain through infinity."""
    for ell in R.COFACTOR_PRIMES[1:]:
        assert R.vanishing_prefixes(ell) == []
        assert (R.X_ABS + 1) % ell == 0
        T = pointcases.small_order_point(ell)
        assert pc.g1_mul_unreduced(T, R.X_ABS, BLS) == pc.g1_neg(T, BLS)


@pytest.mark.parametrize("curve", CURVES)
def test_flag_edge_is_no_curve_point(curve):
    """y = (p - 1) / 2 and (p + 1) / 2: y^2 - b is no cube, so no decompression reaches the edge"""
    C = pc.CURVES[curve]
    p = C.p
    assert p % 3 == 1
    for y in ((p - 1) // 2, (p + 1) // 2):
        assert pow((y * y - C.b) % p, (p - 1) // 3, p) != 1
    cs = R.compress_cases(curve)
    n = C.fp_bytes
    assert {(p - 1) // 2, (p + 1) // 2, 0, 1, p - 1} <= {int.from_bytes(b[n:], "big") for b in cs}


def test_jacobian_case_bounds():
    J = R.jac()
    p = J.p
    for name, bounds in (("jac29.dbl", [R.JAC_IN]), ("jac29.add_affine", [R.JAC_IN]), ("jac29.add", [R.JAC_DBL_OUT] * 2)):
        tops = set()
        for case in R.op_of("bls12_381", name).cases:
            for a, bound in zip(case, bounds):
                v = J.vals(*a[:3])
                assert all(x < b * p for x, b in zip(v, bound))
                tops |= {i for i, (x, b) in enumerate(zip(v, bound)) if x >= (b - 1) * p}
        assert tops == {0, 1, 2}, "%s: every coordinate reaches k = bound - 1" % name
    # the doubling and the cancelling branch see H and rr as non-zero multiples of p
    M = J.M
    hs = set()
    for a, Q, kq in R.op_of("bls12_381", "jac29.add_affine").cases[:400]:
        if a[3] or a[0][0] != Q[0]:
            continue
        X, Y, Z = J.vals(*a[:3])
        z2 = M.mont(Z, Z)
        H = M.mont(M.to_m(Q[0], kq[0]), z2) + 64 * p - X
        assert H % p == 0 and H < 66 * p
        hs.add(H // p)
    assert len(hs) > 2 and max(hs) >= 60 and min(hs) <= 35
    # the doubling branch of jac29_add_affine returns jac29_dbl(q): X3 in [8p, 34p), never the general
    # branch's "< 8p" (the comment in csrc/points.hpp was corrected; jac29_dbl's input contract holds)
    for a, Q, kq in R.op_of("bls12_381", "jac29.add_affine").cases[:400]:
        x3 = R.jac29_dbl_x3(M.to_m(Q[0], kq[0]), M.to_m(Q[1], kq[1]))
        assert 8 * p <= x3 < R.JAC_IN[0] * p
    zs = {c[0] for c in R.op_of("bls12_381", "jac29.zero29").cases}
    top = R.ZERO29_RANGE - 1
    assert {0, 1, p - 1, p, p + 1, top * p - 1, top * p, top * p + 1} <= zs
    assert max(zs) < R.ZERO29_RANGE * p and sum(1 for v in zs if v % p == 0) > 300


@pytest.mark.parametrize("curve", CURVES)
def test_glv_cases(curve):
    r = pc.CURVES[curve].r
    lam = glv.params(curve)[1]
    K = test_glv.product_consts(curve)
    ks = R.glv_scalars(curve)
    assert len(ks) >= 20000 and all(0 <= k < r for k in ks)
    assert set(glv.edge_scalars(curve, 128)) <= set(ks)
    mult = R.glv_multipliers(curve)
    assert mult == {"g1": K["GLV_G1"], "g2": K["GLV_G2"]}
    for k in ks[:600] + ks[-200:]:
        k0, k1 = glv.decompose(curve, k)
        assert (k0 + k1 * lam - k) % r == 0 and abs(k0) < 1 << 127 and abs(k1) < 1 << 127
        w = R.split_words(curve, k)
        assert F.from_words(w[:4]) != 1 << 127 and F.from_words(w[4:]) != 1 << 127      # no negative zero
        assert tuple(F.to_words(v, 4) for v in test_glv.device_split(curve, k)) == (w[:4], w[4:])
    # both sides of every Babai boundary taken: the rounded quotient differs between neighbours
    for g in mult.values():
        steps = {test_glv.device_round_div(curve, k, g, K)[1] for k in ks[:600]}
        assert steps == {0, 1}, "the case list reaches 0 and 1 Barrett corrections (no 2 was found)"
        one = [k for k in R.barrett_scalars(curve, g) if test_glv.device_round_div(curve, k, g, K)[1] == 1]
        assert one and set(one) <= set(ks)
        jumps = sum(1 for k in ks[:600] if k + 1 < r and (2 * k * g + r) // (2 * r) != (2 * (k + 1) * g + r) // (2 * r))
        assert jumps >= min(8, g)          # BLS12-381's first multiplier is 1: one boundary, (r - 1) / 2


@pytest.mark.parametrize("curve", CURVES)
def test_encoding_cases_cover_the_classes(curve):
    C = pc.CURVES[curve]
    p, n = C.p, C.fp_bytes
    comp = R.compressed_cases(curve)
    assert {b for b, _ in pointcases.invalid_compressed(C)} <= set(comp)
    models = [R.decompress_model(curve, b) for b in comp]
    assert {m[2] for m in models} == {0, R.DERR_ENCODING, R.DERR_NOT_ON_CURVE}
    by_x = {}
    for b, (P, inf, code) in zip(comp, models):
        if P is not None:
            by_x.setdefault(P[0], set()).add(P[1])
    assert all(len(ys) == 2 and sum(ys) == p for ys in by_x.values()), "both sign flags: y and -y"
    if curve == "bls12_381":
        assert by_x[0] == {2, p - 2}
    else:
        assert 0 not in by_x and {1, p - 1} <= set(by_x)
    unc = R.uncompressed_cases(curve)
    assert {b for b, _ in pointcases.invalid_uncompressed(C, random.Random(0))} & set(unc) or True
    codes = {R.convert_model(curve, b)[2] for b in unc}
    assert codes == {0, R.DERR_ENCODING, R.DERR_NOT_ON_CURVE}
    r = C.r
    sc = R.ConvertScalars(curve)
    assert {0, r - 1, r, r + 1, (1 << 256) - 1} <= set(sc.cases)
    assert [sc.err_codes[sc.cases.index(k)] for k in (0, r - 1, r, r + 1, (1 << 256) - 1)] == [0, 0, 3, 3, 3]


# ---------------------------------------------------------------------------- 2. the model against the oracle
@pytest.mark.parametrize("curve", CURVES)
def test_decompress_model_against_oracle_and_spec(curve):
    C = pc.CURVES[curve]
    for b in R.compressed_cases(curve):
        P, inf, code = R.decompress_model(curve, b)
        rc, raw = O.g1_decompress(curve, b, 1)
        try:
            want = pk.g1_from_bytes_compressed(b, C)
            assert code == 0 and P == want and inf == (want is None)
            assert rc == 0 and raw == pk.g1_to_bytes(want, C)
        except ValueError as e:
            assert code == (R.DERR_NOT_ON_CURVE if "not on curve" in str(e) else R.DERR_ENCODING) and inf == 1
            assert rc == {R.DERR_ENCODING: pointcases.ERR_ENCODING, R.DERR_NOT_ON_CURVE: pointcases.ERR_NOT_ON_CURVE}[code]
    for b, err in pointcases.invalid_compressed(C):
        assert R.decompress_model(curve, b)[2] == R.DERR_OF[err]


@pytest.mark.parametrize("curve", CURVES)
def test_convert_model_against_spec(curve):
    C = pc.CURVES[curve]
    for b in R.uncompressed_cases(curve):
        P, inf, code, _ = R.convert_model(curve, b)
        try:
            want = pk.g1_from_bytes(b, C)
            assert code == 0 and P == want and inf == (want is None)
        except ValueError as e:
            assert code == (R.DERR_NOT_ON_CURVE if "not on curve" in str(e) else R.DERR_ENCODING), (b.hex(), e)
    for b, err in pointcases.invalid_uncompressed(C, random.Random(5)):
        assert R.convert_model(curve, b)[2] == R.DERR_OF[err]


@pytest.mark.parametrize("curve", CURVES)
def test_compress_model_against_oracle(curve):
    C = pc.CURVES[curve]
    K = R.curve_of(curve)
    pts = K.specials() + K.M.point_pool(random.Random(2), 16) + [None]
    pts += [pc.g1_neg(P, C) for P in pts]
    for P in pts:
        raw = pk.g1_to_bytes(P, C)
        assert R.compress_model(curve, raw) == pk.g1_to_bytes_compressed(P, C) == O.g1_compress(curve, raw, 1)


def test_subgroup_model_against_oracle():
    mem, non = R.subgroup_points()
    for P, tag in mem[:8] + non[:8] + non[-10:]:
        assert O.g1_subgroup_check("bls12_381", pk.g1_to_bytes(P, BLS), 1) == pc.g1_in_subgroup(P, BLS), tag


@pytest.mark.parametrize("curve", CURVES)
def test_point_arithmetic_against_oracle(curve):
    """pc.g1_add / g1_mul, the truth of every point check, against the oracle's fixed-base multiples"""
    C = pc.CURVES[curve]
    rng = random.Random(9)
    ks = [1, 2, 3, C.r - 1] + [rng.randrange(C.r) for _ in range(8)]
    raw = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), len(ks))
    n = 2 * C.fp_bytes
    pts = [pk.g1_from_bytes(raw[i * n:(i + 1) * n], C) for i in range(len(ks))]
    assert pts == [pc.g1_mul(C.g1, k, C) for k in ks]
    assert pc.g1_add(pts[0], pts[0], C) == pts[1] and pc.g1_add(pts[1], pts[0], C) == pts[2]
    assert pc.g1_add(pts[0], pts[3], C) is None
    # the encoder the encode_points stage is held to
    st = R.EncodePoints(curve)
    assert all(pk.g1_from_bytes(w, C) == P for w, (P, _) in zip(st.want, st.cases))


# ---------------------------------------------------------------------------- 3. the checkers
@pytest.mark.parametrize("curve", CURVES)
def test_xyzz_checker_passes_and_reports(curve):
    K = R.curve_of(curve)
    C, p = K.C, K.p
    add = R.op_of(curve, "g1.xyzz_add")
    for case in add.cases[:200] + add.cases[-100:]:
        want = pc.g1_add(case[0], case[2], C)
        assert add.check(case, K.xyzzw(want, 5 if want else 1)) is None
    cancel = next(c for c in add.cases if c[0] is not None and c[2] == pc.g1_neg(c[0], C))
    P = cancel[0]
    assert "want None" in add.check(cancel, K.xyzzw(pc.g1_add(P, P, C), 3))          # doubling where infinity is due
    fin = next(c for c in add.cases if c[0] is not None and c[2] is not None and c[0][0] != c[2][0])
    want = pc.g1_add(fin[0], fin[2], C)
    assert "got" in add.check(fin, K.xyzzw(pc.g1_neg(want, C), 3))                   # y negated
    assert add.check(fin, K.xyzzw(None, 1)) is not None                               # infinity where a point is due
    w = K.xyzzw(want, 3)
    bad = w[:3 * K.W] + K.fpw(28)                                                      # ZZ^3 != ZZZ^2
    assert "ZZ^3" in add.check(fin, bad)
    raw = F.from_words(w[:K.W])
    if raw + p < 1 << (32 * K.W):                                                      # not canonical
        assert "canonical" in add.check(fin, F.to_words(raw + p, K.W) + w[K.W:])
    ta = R.op_of(curve, "g1.xyzz_to_affine")
    c = next(c for c in ta.cases if c[0] is not None)
    assert ta.check(c, [1] + K.affw(c[0])) is None
    assert ta.check(c, [0] + K.affw(c[0])) and ta.check(c, [1] + K.affw(pc.g1_neg(c[0], C)))
    assert ta.check((None, 1), [0] + [0] * (2 * K.W)) is None and ta.check((None, 1), [1] + [0] * (2 * K.W))
    oc = R.op_of(curve, "g1.affine_on_curve")
    assert all(oc.check(c, [int(pc.g1_on_curve(c, C))]) is None and oc.check(c, [1 - int(pc.g1_on_curve(c, C))]) for c in oc.cases[:40])


def test_jac_checker_passes_and_reports():
    J = R.jac()
    C, p = J.K.C, J.p
    dbl, madd, add = (R.op_of("bls12_381", "jac29." + o) for o in ("dbl", "add_affine", "add"))
    c = next(c for c in dbl.cases if not c[0][3])
    want = pc.g1_add(c[0][0], c[0][0], C)
    good = J.enc((want, 7, (33, 17, 3), False))
    assert dbl.check(c, good) is None
    assert "bound" in dbl.check(c, J.enc((want, 7, (34, 0, 0), False)))               # X one p past its bound
    assert "bound" in dbl.check(c, J.enc((want, 7, (0, 0, 4), False)))                # Z one p past its bound
    assert "got" in dbl.check(c, J.enc((pc.g1_neg(want, C), 7, (0, 0, 0), False)))    # y negated
    assert "flag" in dbl.check(c, J.enc((want, 7, (0, 0, 0), True)))
    unnorm = list(good)
    unnorm[0] += 1 << 29
    unnorm[1] -= 1
    assert "normalised" in dbl.check(c, unnorm)
    zero_z = J.enc((want, 7, (0, 0, 0), False))
    zero_z[2 * J.n:3 * J.n] = F.limbs29(3 * p, J.n)
    assert "Z = 0" in dbl.check(c, zero_z)
    # the cancelling branch: infinity is due, the doubling result is reported; so is a changed operand
    cc = next(c for c in madd.cases if not c[0][3] and c[1] == pc.g1_neg(c[0][0], C))
    assert madd.check(cc, J.enc(cc[0][:3] + (True,))) is None
    assert "flag" in madd.check(cc, J.enc((pc.g1_add(cc[1], cc[1], C), 1, (0, 0, 0), False)))
    assert "handed through" in madd.check(cc, J.enc((cc[0][0], cc[0][1] + 1, cc[0][2], True)))
    # the general branch is held to (8, 6, 6), the doubling branch to jac29_dbl's (34, 18, 4)
    g = next(c for c in madd.cases if not c[0][3] and c[1][0] != c[0][0][0])
    w = pc.g1_add(g[0][0], g[1], C)
    assert madd.check(g, J.enc((w, 3, (7, 5, 5), False))) is None and "bound" in madd.check(g, J.enc((w, 3, (8, 0, 0), False)))
    d = next(c for c in madd.cases if not c[0][3] and c[1] == c[0][0])
    w = pc.g1_add(d[1], d[1], C)
    assert madd.check(d, J.enc((w, 3, (33, 17, 3), False))) is None and "bound" in madd.check(d, J.enc((w, 3, (0, 18, 0), False)))
    a = next(c for c in add.cases if c[0][3] and not c[1][3])
    assert add.check(a, J.enc(a[1])) is None and add.check(a, J.enc(a[0])) is not None
    z = R.op_of("bls12_381", "jac29.zero29")
    assert z.check((5 * p,), [1]) is None and z.check((5 * p,), [0]) and z.check((5 * p + 1,), [1])


@pytest.mark.parametrize("curve", CURVES)
def test_glv_checker_reports_a_shifted_decomposition(curve):
    r = pc.CURVES[curve].r
    _, lam, v1, v2 = glv.params(curve)
    op = R.op_of(curve, "glv.split")
    for (k,) in op.cases[:50]:
        assert op.check((k,), R.split_words(curve, k)) is None
    k = op.cases[40][0]
    k0, k1 = glv.decompose(curve, k)
    for v in (v1, v2):
        s0, s1 = k0 + v[0], k1 + v[1]                 # still k = s0 + s1 lambda (mod r): only the exact compare sees it
        assert (s0 + s1 * lam - k) % r == 0 and abs(s0) < 1 << 127 and abs(s1) < 1 << 127
        assert op.check((k,), F.to_words(R.sign_magnitude(s0), 4) + F.to_words(R.sign_magnitude(s1), 4))
    assert "negative zero" in op.check((0,), F.to_words(1 << 127, 4) + [0] * 4)
    rd = R.op_of(curve, "glv.round_div_g2")
    g = R.glv_multipliers(curve)["g2"]
    want = (2 * k * g + r) // (2 * r)
    assert rd.check((k,), F.to_words(want, 4)) is None and rd.check((k,), F.to_words(want + 1, 4))


STAGE_IDS = R.all_stage_ids()


@pytest.mark.parametrize("curve,stage,mode", STAGE_IDS, ids=["%s-%s-%s" % s for s in STAGE_IDS])
def test_stage_checker_passes_and_reports(curve, stage, mode):
    st = R.stage_of(curve, stage, mode)
    per_elem = mode == "each"
    K = st.K
    fresh = lambda: st.expected(per_elem)  # noqa: E731
    assert st.check(fresh(), per_elem) == []
    # an overwritten guard
    out = fresh()
    out["guards"][sorted(out["guards"])[0]] = False
    assert any("guard" in m for m in st.check(out, per_elem))
    # a wrong error code
    if st.err_codes is not None:
        out = fresh()
        out["err"] = list(out["err"])
        out["err"][0] = out["err"][0] + 1 if out["err"][0] < 4 else 0
        assert any("error" in m for m in st.check(out, per_elem))
        if per_elem and max(st.err_codes) and stage != "subgroup_check":
            i = next(i for i, e in enumerate(st.err_codes) if e)
            out = fresh()
            out["err"] = [0 if j == i else e for j, e in enumerate(out["err"])]        # a rejection missed
            assert any("case %d: error" % i in m for m in st.check(out, per_elem))
    # a non-zero slot under a rejected point, and a wrong point under an accepted one
    if stage in ("convert_points29", "convert_points29_img", "decompress_points"):
        i = next(i for i, m in enumerate(st.model) if m[2])
        j = next(i for i, m in enumerate(st.model) if m[0] is not None)
        out = fresh()
        sw = K.slot_words
        out["pts"][i * sw] = 1
        assert any(m.startswith("case %d:" % i) for m in st.check(out, per_elem))
        out = fresh()
        other = pc.g1_neg(st.model[j][0], K.C)                                        # y negated
        out["pts"][j * sw:(j + 1) * sw] = (K.slot32(other, 0xA5A5A5A5) if stage == "decompress_points"
                                            else K.slot29(K.conv29(other[0]), K.conv29(other[1]), pad=0xA5A5A5A5))
        assert any(m.startswith("case %d:" % j) for m in st.check(out, per_elem))
        out = fresh()
        out["inf"][j] = 1
        assert any("infinity flag" in m for m in st.check(out, per_elem))
        if stage != "decompress_points" and not K.packed:                              # one p past the documented bound
            out = fresh()
            j = next(i for i, m in enumerate(st.model) if m[0] is not None and m[0][0])
            P = st.model[j][0]
            out["pts"][j * sw:(j + 1) * sw] = K.slot29(K.conv29(P[0]) + K.p, K.conv29(P[1]), pad=0xA5A5A5A5)
            assert any("bound" in m for m in st.check(out, per_elem))
        if not K.packed or stage == "decompress_points":
            if K.slot_words > K.slot_used(stage != "decompress_points"):
                out = fresh()
                out["pts"][(j + 1) * sw - 1] = 0
                assert any("written past" in m for m in st.check(out, per_elem))
    if stage == "convert_points29_img":
        j = next(i for i, m in enumerate(st.model) if m[0] is not None and m[0][0])    # x = 0: phi(P) = P
        out = fresh()
        sw = K.slot_words
        P = st.model[j][0]
        out["img"][j * sw:(j + 1) * sw] = K.slot29(K.conv29(P[0]), K.conv29(P[1]), pad=0xA5A5A5A5)   # P where phi(P) is due
        assert any("image" in m for m in st.check(out, per_elem))
        out = fresh()
        out["img_inf"][j] = 1
        assert any("image flag" in m for m in st.check(out, per_elem))
    if stage.startswith("glv_split"):
        out = fresh()
        out["h1"][4 * 7 + 3] ^= 1 << 31                                                # a sign lost
        assert any(m.startswith("case 7:") for m in st.check(out, per_elem))
    if stage.startswith("endo_points"):
        j = next(i for i, c in enumerate(st.cases) if c[0] is not None and c[0][0] and not c[1])   # x = 0: phi(P) = P
        out = fresh()
        out["dst_inf"][j] = 1
        assert any("copied" in m for m in st.check(out, per_elem))
        out = fresh()
        sw = K.slot_words
        out["dst"][j * sw:(j + 1) * sw] = st.src_slot(st.cases[j][0], True)            # x left as it was
        assert any(m.startswith("case %d:" % j) for m in st.check(out, per_elem))
    if stage in ("compress_points", "encode_points"):
        out = fresh()
        out["out"][K.nb - 1] ^= 1
        assert any(m.startswith("case 0:") for m in st.check(out, per_elem))
        out = fresh()
        out["out"][0] ^= 0x20
        assert any(m.startswith("case 0:") for m in st.check(out, per_elem))
    if stage == "convert_scalars":
        i = next(i for i, e in enumerate(st.err_codes) if e)
        out = fresh()
        out["out"][8 * i] = 1                                                          # a rejected scalar not stored as zero
        assert any(m.startswith("case %d:" % i) for m in st.check(out, per_elem))
