"""The row accumulation's hot loop (csrc/msm.hpp acc_row29) negates an entry's y lazily -- ACC_NEG - q.y
limb by limb, no carry pass -- and multiplies that by ZZZ.  In the limb model of tests/rowarithref.py
(tests/fusedref.py's product scan, every column asserted below 2^64) the words of R = q.y' ZZZ - y are
those the normalised operand gives, on both curves (the site is enabled on both: fused into the product
on BLS12-381, with sub29 behind it on BN254), over the operand families the bounds admit; the carry pass
of the restart after P + (-P) returns sub29's words; a fault of one limb in the lazy operand is caught;
and tools/gen_params29.py check_bounds carries the site's assertions.

The peeled first addition of an item (BLS12-381; ZZ = ZZZ = ONE, no products by ONE) gives, word for
word, the generic body's P, R, X3, Y3, ZZ3 and ZZZ3 on random operands and the families; each guard
(q.x, S2 under both signs, PP; PPP on the identity it protects) falls back just below its threshold and
not at it, and at p's two top limbs and past p; P = 0 with R != 0 and P = R = 0 fall back to the
generic body's exits; a one-limb fault in any output is caught; the threshold is check_bounds' own.
The lists of tests/test_gpu_msm_rows_arith.py are held to what they promise, in the model as well."""
import random

import pytest

import fieldref as F
import msmref as MR
import msmrowsarithcases as AC
import rowarithref as RA

NRANDOM = 300


@pytest.mark.parametrize("curve", F.CURVES)
def test_lazy_negation_gives_the_normalised_words(curve):
    md = RA.model(curve)
    p, n = md.p, md.N
    qys, zs, ys = md.families()
    kq, kz, ky = md.bounds()
    low = (1 << (29 * (n - 1))) - 1
    # the families the comparison rests on are really there
    assert 0 in qys and 1 in qys and p - 1 in qys, "q.y = 0 (every limb 0), 1, p - 1"
    assert any(v & low == low for v in qys), "q.y: every lower limb 2^29 - 1"
    assert md.m.below(kz) in zs and any(v & low == low and v >> (29 * (n - 1)) for v in zs), "ZZZ at its bound, all ones"
    assert md.kr * p in ys, "y at ACC_R p (BLS12-381: 16 p)"
    assert md.neg_lazy(0) == md.H["ACC_NEG"] and max(md.neg_lazy(0)[:n - 1]) >= 1 << 29, "the widest lazy limbs"
    cases = [(q, z, y) for q in qys for z in zs for y in ys[:4]] + [(q, zs[0], y) for q in qys for y in ys]
    rng = random.Random("%d row lazy %s" % (F.SEED, curve))
    cases += [(md.m.rand_below(rng, kq), md.m.rand_below(rng, kz), md.m.rand_below(rng, ky)) for _ in range(NRANDOM)]
    for c in cases:
        msg = md.check_site(*c)
        assert msg is None, "%s: %s, case %s" % (curve, msg, F.hexs(c))
    assert md.f.peak < 1 << 64


@pytest.mark.parametrize("curve", F.CURVES)
def test_a_one_limb_fault_in_the_lazy_operand_is_caught(curve):
    md = RA.model(curve)
    qys, zs, ys = md.families()
    n = md.N

    def plant(i, d):
        def fault(l):
            l[i] += d
            return l
        return fault
    for q, z, y in ((qys[1], zs[0], ys[0]), (qys[-1], zs[1], ys[2]), (md.p - 1, zs[0], 0)):
        assert md.check_site(q, z, y) is None
        for i in (0, n // 2, n - 1):
            assert md.check_site(q, z, y, fault=plant(i, 1)) is not None, "limb %d + 1 went through" % i
        assert md.check_site(q, z, y, fault=plant(0, -1)) is not None
    # ZZZ = 0 hides the operand from the product: the restart's carry pass still sees the fault
    assert md.check_site(qys[1], 0, 0, fault=plant(3, 1)) is not None


@pytest.mark.parametrize("curve", F.CURVES)
def test_model_refuses_a_bias_that_lets_a_limb_go_negative(curve):
    """An unbiased multiple of p (plain limbs of ACC_NEG p) is outside neg_lazy29's contract."""
    md = RA.model(curve)
    plain = F.limbs29(md.kneg * md.p, md.N)
    saved = md.H["ACC_NEG"]
    md.H["ACC_NEG"] = plain
    try:
        with pytest.raises(AssertionError):
            for q in md.families()[0]:
                md.neg_lazy(q)
    finally:
        md.H["ACC_NEG"] = saved


# ---------------------------------------------------------------------- the peeled first addition
PEEL_CURVE = "bls12_381"     # csrc/msm.hpp kPeelFirst: BN254 keeps the generic body


def _sqrt(a, p):
    r = pow(a, (p + 1) // 4, p)
    return r if r * r % p == a % p else None


def _first_cases(md, rng, nrandom):
    """(x, y, q.x, q.y, sign): the running sum after the prologue (a point's x, its y or ACC_NEG p - y)
    and the second entry, random and from the operand families."""
    m, p = md.m, md.p
    kq = md.bounds()[0]
    out = []
    for _ in range(nrandom):
        y0 = m.rand_below(rng, 1)
        out.append((m.rand_below(rng, 1), rng.choice((y0, md.kneg * p - y0)), m.rand_below(rng, 1),
                    m.rand_below(rng, 1), rng.randrange(2)))
    fam = F.dedupe(m.family(kq) + [(1 << (29 * (md.N - 1))) - 1])
    for i, a in enumerate(fam):
        for j, b in enumerate(fam):
            out.append((fam[(i + 2 * j) % len(fam)], fam[(3 * i + j) % len(fam)] if j % 2 else md.kneg * p - b, a, b, (i + j) & 1))
    return out


def test_peeled_first_addition_is_the_generic_body():
    md = RA.model(PEEL_CURVE)
    assert md.PEEL[PEEL_CURVE] and not md.PEEL["bn254"] and "PEEL_LO" not in RA.model("bn254").H
    rng = random.Random("%d row peel" % F.SEED)
    outcomes = {}
    for c in _first_cases(md, rng, NRANDOM):
        msg, q = md.check_first(*c)
        assert msg is None, "%s, case %s" % (msg, F.hexs(c))
        outcomes[q[:2] if q[0] == "fallback" else q[0]] = outcomes.get(q[:2] if q[0] == "fallback" else q[0], 0) + 1
    assert outcomes["sum"] >= NRANDOM and outcomes.get(("fallback", "q.x")) and outcomes.get(("fallback", "S2"))
    assert md.f.peak < 1 << 64


def test_every_guard_falls_back_exactly_at_its_threshold():
    """q.x, S2 under both signs and PP forced just below and at the lower threshold, and at the upper
    one (p's two top limbs, and past p where a negation wraps): the peel falls back below and not at
    or above, and agrees with the generic body there.  PPP's guard is forced on the identity it
    protects (a whole addition with a chosen PPP needs a cube root mod p, p = 1 mod 9)."""
    md = RA.model(PEEL_CURVE)
    p, n = md.p, md.N
    lo, hi = md.threshold()
    rng = random.Random("%d row peel guards" % F.SEED)
    x, y, other = (md.m.rand_below(rng, 1) for _ in range(3))
    # q.x
    for qx, o in ((lo - 1, ("fallback", "q.x")), (0, ("fallback", "q.x")), (lo, "sum"), (hi - 1, "sum"),
                  (hi, ("fallback", "q.x")), (p - 1, ("fallback", "q.x")), (p, ("fallback", "q.x")), (p + 1, ("fallback", "q.x"))):
        got = md.check_first(x, y, qx, other, 0)
        assert got[0] is None and (got[1][0] if o == "sum" else got[1][:2]) == o, (hex(qx), got)
    # S2 = q.y (sign 0) and p - q.y (sign 1)
    for s2, o in ((lo - 1, "fb"), (lo, "sum"), (hi - 1, "sum"), (hi, "fb"), (p - 1, "fb")):
        for sign, qy in ((0, s2), (1, p - s2)):
            got = md.check_first(x, y, other, qy, sign)
            assert got[0] is None and got[1][:2] == (("fallback", "S2") if o == "fb" else got[1][:2]) and \
                (got[1][0] == "sum") == (o == "sum"), (hex(s2), sign, got)
    for sign, qy in ((0, p), (0, p + 1), (1, p), (1, p + 1)):             # q.y >= p: S2 = 0, or wrapped below 0
        got = md.check_first(x, y, other, qy, sign)
        assert got == (None, ("fallback", "S2")), (hex(qy), sign, got)
    # PP: P = q.x - x with P^2 / R29 = t, t scanned from the threshold for a square
    R29 = md.m.R
    seen = set()
    for start, step, o in ((lo - 1, -1, "fb"), (lo, 1, "sum")):
        t = start
        while _sqrt(t * R29 % p, p) is None:
            t += step
        assert abs(t - start) < 64
        s = _sqrt(t * R29 % p, p)
        got = md.check_first(x, y, (x + s) % p, other, 0)
        assert got[0] is None and (got[1][:2] == ("fallback", "PP") if o == "fb" else got[1][0] == "sum"), (hex(t), got)
        if o == "sum":
            assert F.value29(got[1][3]) == t, "ZZ3 is the residue itself"
        seen.add(o)
    assert seen == {"fb", "sum"}
    # the identity under every guard, PPP's included: mont(ONE, v) = canon(v) wherever peel_ok says so,
    # for v and v + p around both thresholds; below the lower one it is refused
    one = md.H["ONE"]
    for v in (lo, lo + 1, hi - 1, lo + p, hi - 1 + p, p - hi + lo + p) + tuple(rng.randrange(lo, hi) for _ in range(64)):
        c = md.canon(md.f.L(v))
        assert md.peel_ok(c) and md.f.scan(one, md.f.L(v)) == c, hex(v)
    for v in (0, 1, lo - 1, lo - 1 + p, p, hi, p - 1, hi + p):
        if v < 2 * p:
            assert not md.peel_ok(md.canon(md.f.L(v))), hex(v)
    # and the threshold is what makes it hold: a residue small enough fails the identity itself
    a = (md.kneg - 1) * p + 1                                              # a negated q.y = p - 1: residue 1
    assert md.f.scan(md.f.L(a), one) == md.f.L(p + 1) != md.f.L(a % p)


def test_first_addition_that_doubles_or_cancels_takes_the_generic_exits():
    md = RA.model(PEEL_CURVE)
    p = md.p
    rng = random.Random("%d row peel degenerate" % F.SEED)
    for _ in range(8):
        x, y = md.m.rand_below(rng, 1), md.m.rand_below(rng, 1)
        x, y = max(x, md.threshold()[0]), max(y, md.threshold()[0])
        for ysum, qy, sign, g in ((y, y, 0, "dbl"), (y, y, 1, "inf"), (md.kneg * p - y, y, 1, "dbl"),
                                  (md.kneg * p - y, y, 0, "inf")):
            assert md.first_generic(x, ysum, x, qy, sign) == (g,)
            assert md.check_first(x, ysum, x, qy, sign) == (None, ("fallback", "P = 0"))


def test_a_one_limb_fault_in_the_peel_is_caught():
    md = RA.model(PEEL_CURVE)
    rng = random.Random("%d row peel fault" % F.SEED)
    c = tuple(md.m.rand_below(rng, 1) for _ in range(4)) + (1,)
    assert md.check_first(*c) == (None, md.first_peeled(*c)) and md.first_peeled(*c)[0] == "sum"

    def plant(part, limb):
        def fault(q):
            q = [q[0]] + [list(w) for w in q[1:]]
            q[part][limb] ^= 1
            return tuple([q[0]] + [w for w in q[1:]])
        return fault
    for part in (1, 2, 3, 4):                                   # x3, y3, zz, zzz
        for limb in (0, md.N - 1):
            assert md.check_first(*c, fault=plant(part, limb))[0] is not None, (part, limb)


def test_check_bounds_carries_the_peel_threshold():
    g = F.gen29
    name, p, n, r32, b, nkp, roles = g.CURVES[0]
    assert name in g.PEEL_FIRST and g.CURVES[1][0] not in g.PEEL_FIRST
    lo = g.check_bounds(p, n, nkp, roles, peel=True)["PEEL_LO"]
    md = RA.model(PEEL_CURVE)
    assert lo == md.H["PEEL_LO"]
    # the threshold from its derivation: the least two-top-limb value at or above ACC_NEG p ONE / R29
    T = -(-md.kneg * p * F.value29(md.H["ONE"]) // md.m.R)
    s = 29 * (n - 2)
    assert (lo << s) >= T > ((lo - 1) << s)
    # BN254 has no such headroom: the same derivation refuses it
    name, p, n, r32, b, nkp, roles = g.CURVES[1]
    with pytest.raises(AssertionError):
        g.check_bounds(p, n, nkp, roles, peel=True)


@pytest.mark.parametrize("pattern", AC.PATTERNS)
@pytest.mark.parametrize("curve", F.CURVES)
def test_the_gpu_lists_hold_what_they_promise(curve, pattern):
    """The lists of tests/test_gpu_msm_rows_arith.py: size, signs, bucket lengths 1, 2, 3 by the row,
    one bucket over L, and in the mixed list the degenerate buckets and the tiny-x points."""
    b = AC.arith_list(curve, pattern)
    assert 2500 <= len(b) <= 6000 and AC.signs_hold(b, pattern)
    off, cnt = MR.off_cnt(b.skey, MR.Win(AC.WBITS).nbuckets)
    assert all(sum(1 for c in cnt if c == n) >= 64 for n in (1, 2, 3)) and sum(1 for c in cnt if c > AC.L) == 1
    if pattern != "mixed":
        return
    tiny = b.points[-2:]
    assert all(AC.limb_top_is_tiny(curve, P) for P in tiny) and tiny[0] != tiny[1]
    ents = {}
    for v, k in zip(b.sval, b.skey):
        ents.setdefault(k, []).append(v & ~MR.SV_FIRST)
    two = [vs[:2] for vs in ents.values() if len(vs) >= 2]
    assert any(u == v for u, v in two) and any(u == v ^ 1 for u, v in two), "(P, P) and (P, -P) as first two entries"
    ti = {b.index[P] for P in tiny}
    assert {(u & 1, v & 1) for u, v in two if v >> 1 in ti and u >> 1 not in ti} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(u >> 1 in ti for u, _ in two)
    # in the peel's model: the tiny-x points as second entry fall back on q.x, the small-PP pair on PP
    if curve != PEEL_CURVE:
        assert AC.small_pp_point(curve, b.points[0]) is None
        return
    md, M = RA.model(curve), MR.layers(curve)[0]
    mont = lambda P: (P[0] * M.R % M.p, P[1] * M.R % M.p)  # noqa: E731
    fell = {}
    for u, v in two:
        (x, y), (qx, qy) = mont(b.points[u >> 1]), mont(b.points[v >> 1])
        q = md.first_peeled(x, md.kneg * M.p - y if u & 1 else y, qx, qy, v & 1)
        if q[0] == "fallback":
            fell[q[1]] = fell.get(q[1], 0) + 1
    assert fell.get("q.x", 0) >= 8 and fell.get("PP", 0) >= 8 and fell.get("P = 0", 0) >= 6, fell


@pytest.mark.parametrize("idx", [0, 1])
def test_check_bounds_covers_the_lazy_site(idx):
    g = F.gen29
    name, p, n, r32, b, nkp, roles = g.CURVES[idx]
    g.check_bounds(p, n, nkp, roles)
    src = open(g.__file__).read()
    assert "lazy_operand(biased(roles[\"ACC_NEG\"]" in src
    # a bias below the point's y (fp_to29 returns up to (p / R29 + 1) p): refused
    with pytest.raises(AssertionError):
        g.check_bounds(p, n, nkp, dict(roles, ACC_NEG=1))
