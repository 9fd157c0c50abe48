"""Generates csrc/params29_gen.hpp: the Fp constants of the radix-2^29 accumulation arithmetic
(csrc/field29.hpp) for both curves -- BLS12-381 in 14 x 29-bit limbs (R29 = 2^406) and BN254 in
9 x 29-bit limbs (R29 = 2^261): p, -p^-1 mod 2^32, the Montgomery conversions to/from the
32-bit-limb domain (R = 2^384 / 2^256), biased multiples of p for carry-free subtraction, the
small multiples of p for the exact zero test, and the ROLE constants -- which biased multiple
each subtraction of the accumulation loop and its doubling uses.

The roles differ per curve because the headroom differs: R29 / p is 2^25 for BLS12-381 but only
~169 for BN254, so a Montgomery product of inputs below a p and b p returns below
(a b p / R29 + 1) p, and on BN254 that is only < 2p while a b < 169.  check_bounds() below runs
the value bounds of every step (in units of p) through the loop until they are stable and
asserts each precondition: a bias k p is at least the subtrahend's bound, the zero-tested values
stay below NKP p, and every product's output stays within the bounds its consumers assume.

python3 kzg-batch-verification-scheme_amd/tools/gen_params29.py > kzg-batch-verification-scheme_amd/csrc/params29_gen.hpp
"""
from fractions import Fraction

W = 29
MASK = (1 << W) - 1

CURVES = [
    # name, p, limbs, 32-bit-limb Montgomery exponent, curve b, NKP, roles (multiples of p)
    ("Bls12_381Fp29",
     0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
     14, 384, 4, 20,
     dict(ACC_NEG=8, ACC_P=16, ACC_R=16, ACC_X3=8, ACC_QX=16, ACC_PPP=8, DBL_X=8, DBL_QX=16, DBL_Y=8)),
    ("Bn254Fp29",
     0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
     9, 256, 3, 12,
     dict(ACC_NEG=2, ACC_P=8, ACC_R=4, ACC_X3=4, ACC_QX=8, ACC_PPP=2, DBL_X=4, DBL_QX=8, DBL_Y=2)),
]
# bucket records (x29_add / x29_dbl inputs and outputs, both curves): x < 10p, y < 16p, zz, zzz < 2p
REC = dict(x=10, y=16, z=2)


def limbs(x, n):
    out = []
    for _ in range(n - 1):
        out.append(x & MASK)
        x >>= W
    out.append(x)
    return out


def biased(k, p, n):
    """k p with limbs 0..n-2 moved into [2^29, 2^30) (borrowing from the next limb)."""
    b = limbs(k * p, n)
    b[0] += 1 << W
    for i in range(1, n - 1):
        b[i] += (1 << W) - 1
    b[n - 1] -= 1
    assert sum(v << (W * i) for i, v in enumerate(b)) == k * p
    assert all((1 << W) <= v < (1 << (W + 1)) for v in b[:n - 1]) and b[n - 1] >= 0
    return b


def biased3(k, p, n):
    """k p with limbs 0..n-2 in [3 (2^29 - 1), 2^31): the bias of sub3_29 (a + B - s - 2t in one
    carry pass, s and t normalised, so every limb's s + 2t <= 3 (2^29 - 1) <= B_i)."""
    b = limbs(k * p, n)
    b[0] += 3 << W
    for i in range(1, n - 1):
        b[i] += (3 << W) - 3
    b[n - 1] -= 3
    assert sum(v << (W * i) for i, v in enumerate(b)) == k * p
    assert all(3 * ((1 << W) - 1) <= v < (1 << 31) for v in b[:n - 1]) and b[n - 1] >= 0
    return b


PEEL_FIRST = {"Bls12_381Fp29"}  # curves whose row loop peels an item's first addition (msm.hpp kPeelFirst)


def check_bounds(p, n, nkp, roles, peel=False):
    """Value bounds (units of p) of the accumulation loop (msm.hpp acc_loop29, acc_row29), its doubling
    (dbl_affine29), the record addition/doubling (x29_add, x29_dbl) and the on-curve test; with
    `peel` also the guard threshold of acc_row29's peeled first addition (peel_threshold)."""
    R = 1 << (W * n)
    lim = Fraction(R, p)  # values must stay representable: < 2^(29 n)
    def mont(a, b):       # (a p)(b p)/R + p, in units of p
        assert a < lim and b < lim
        return Fraction(a) * b * p / R + 1
    def mont2(a, b, c, d):
        assert max(a, b, c, d) < lim
        return (Fraction(a) * b + Fraction(c) * d) * p / R + 1
    def fused(bias, k, sub):
        # A subtraction fused into its product (field29.hpp mulsub29 / sqrsub3_29): high column K
        # also adds the limb bias[K - n] - (the subtrahend's limbs).  The bias k p covers the
        # subtrahend's bound `sub`; the addend is at most the bias limb (< 2^30, sub3_29's form
        # < 2^31) and not negative (biased()/biased3() put every limb at or above what normalised
        # subtrahend limbs reach); the column -- at most n limb products a_i b_j (or the square's
        # pre-doubled off-diagonal ones) and n of m_i p_j, each below 2^58, the carry of the column
        # before it (< 2^35) and the addend -- stays below 2^64.
        assert k >= sub
        addend = max(bias[:n - 1])
        assert addend < 1 << 31
        assert 2 * n * MASK * MASK + (1 << 35) + addend < 1 << 64, "fused column overflows"
    def lazy_operand(bias, k, sub, addend):
        # A product operand negated limb by limb, bias - b with no carry pass (field29.hpp
        # neg_lazy29): b normalised and below sub p <= k p.  Limbs 0..n-2 land in (0, 2^30) because
        # the bias limbs lie in [2^29, 2^30); the top limb must not go negative (unsigned limbs:
        # only the top limb of a biased multiple can be smaller than the subtrahend's).  The column
        # -- n limb products of a lazy limb (at most the largest bias limb) and a normalised one,
        # n of m_i p_j, the carry (< 2^35) and the addend of a fused subtraction -- stays below 2^64.
        assert k >= sub
        assert bias[n - 1] >= (int(sub * p) >> (W * (n - 1))) + 1, "lazy top limb goes negative"
        lazy = max(bias)
        assert lazy < 1 << 30
        assert n * lazy * MASK + n * MASK * MASK + (1 << 35) + addend < 1 << 64, "lazy column overflows"
    ro = {k: Fraction(v) for k, v in roles.items()}
    # points come out of a Montgomery product with canonical inputs (fp_to29, k_convert_points
    # <To29>): below (p / R29 + 1) p, NOT below p -- on BN254 that is 1.006 p, so negating q.y
    # needs a bias of 2p (a bias of 1p goes negative for ~0.3 % of the points)
    qin = mont(1, 1)
    assert ro["ACC_NEG"] >= qin
    # dbl_affine29: the running sum := 2q (q.x < qin p, q.y < ACC_NEG p)
    qx, qy = qin, ro["ACC_NEG"]
    U = 2 * qy
    V = mont(U, U); Wd = mont(U, V); S = mont(qx, V); M = 3 * mont(qx, qx)
    assert ro["DBL_X"] >= 2 * S
    dx = mont(M, M) + ro["DBL_X"]
    assert ro["DBL_QX"] >= dx
    t = mont(M, S + ro["DBL_QX"]); w = mont(Wd, qy)
    assert ro["DBL_Y"] >= w
    dy = t + ro["DBL_Y"]
    # the loop from a bucket start (x = q.x, y = q.y, zz = zzz = ONE < p) to a fixed point
    X, Y, Z = max(qx, dx), max(qy, dy), max(Fraction(1), V, Wd)
    for _ in range(50):
        U2, S2 = mont(qx, Z), mont(qy, Z)
        assert ro["ACC_P"] >= X and ro["ACC_R"] >= Y
        fused(biased(roles["ACC_P"], p, n), ro["ACC_P"], X)   # P = mulsub29(q.x, zz, x)
        fused(biased(roles["ACC_R"], p, n), ro["ACC_R"], Y)   # R = mulsub29(q.y, zzz, y)
        # acc_row29's hot loop: a negated q.y enters that product as ACC_NEG - q.y limb by limb (the
        # point's y < qin p), beside ZZZ < Z p normalised and, where the subtraction is fused, its
        # ACC_R limb; the same integer as sub29's form, so the bounds of R above hold as they are
        assert Z < lim
        lazy_operand(biased(roles["ACC_NEG"], p, n), ro["ACC_NEG"], qin, max(biased(roles["ACC_R"], p, n)[:n - 1]))
        P, Rr = U2 + ro["ACC_P"], S2 + ro["ACC_R"]
        assert P < nkp and Rr < nkp, "zero test range"
        PP = mont(P, P); PPP = mont(P, PP); Q2 = mont(X, PP)
        assert ro["ACC_X3"] >= PPP + 2 * Q2
        fused(biased3(roles["ACC_X3"], p, n), ro["ACC_X3"], PPP + 2 * Q2)  # X3 = sqrsub3_29(R, PPP, Q2)
        X3 = mont(Rr, Rr) + ro["ACC_X3"]
        assert ro["ACC_QX"] >= X3 and ro["ACC_PPP"] >= PPP
        # neg_lazy29 (ACC_PPP - PPP limb by limb, no carries): the top limb must not go negative
        assert limbs(roles["ACC_PPP"] * p, n)[n - 1] - 1 >= (int(PPP * p) >> (W * (n - 1))) + 1
        Y3 = mont2(Rr, Q2 + ro["ACC_QX"], Y, ro["ACC_PPP"])
        Zn = max(Z, mont(Z, PP), mont(Z, PPP))
        Xn, Yn = max(X, X3), max(Y, Y3)
        if (Xn, Yn, Zn) == (X, Y, Z):
            break
        X, Y, Z = Xn, Yn, Zn
    else:
        raise AssertionError("loop bounds do not settle")
    assert X < REC["x"] and Y < REC["y"] and Z < REC["z"], "flushed records within the record bounds"
    # x29_add on records (B2, B8, B16) and x29_dbl (B4, B8, B16)
    x, y, z = (Fraction(REC[k]) for k in "xyz")
    U1, S1 = mont(x, z), mont(y, z)
    P, Rr = U1 + 2, S1 + 2
    assert 2 >= U1 and 2 >= S1 and P < nkp and Rr < nkp
    PP = mont(P, P); PPP = mont(P, PP); Q2 = mont(U1, PP)
    assert 8 >= PPP + 2 * Q2
    fused(biased(2, p, n), 2, max(U1, S1))          # x29_add's P and R (mulsub29, B2)
    fused(biased3(8, p, n), 8, PPP + 2 * Q2)        # x29_add's X3 (sqrsub3_29, C8)
    X3 = mont(Rr, Rr) + 8
    assert 16 >= X3 and 8 >= PPP
    Y3 = mont2(Rr, Q2 + 16, S1, 8)
    ZZ = mont(mont(z, z), PP); ZZZ = mont(mont(z, z), PPP)
    assert X3 < REC["x"] and Y3 < REC["y"] and ZZ < REC["z"] and ZZZ < REC["z"]
    U = 2 * y
    V = mont(U, U); Wd = mont(U, V); S = mont(x, V); M = 3 * mont(x, x)
    assert 4 >= 2 * S
    X3 = mont(M, M) + 4
    assert 8 >= X3 and 16 >= y
    Y3 = mont2(M, S + 8, Wd, 16)
    assert X3 < REC["x"] and Y3 < REC["y"] and mont(V, z) < REC["z"] and mont(Wd, z) < REC["z"]
    # to32: canon29 needs mont(record, TO32 < p) < 2p
    assert mont(max(REC.values()), 1) < 2
    # k_convert_points<To29>: y^2 - (x^3 + b) with B4, zero-tested
    rhs = mont(mont(1, 1), 1) + 1
    assert 4 >= rhs and mont(1, 1) + 4 < nkp
    out = dict(X=float(X), Y=float(Y), Z=float(Z))
    if peel:
        out["PEEL_LO"] = peel_threshold(p, n, roles, qin, mont)
    return out


def peel_threshold(p, n, roles, qin, mont):
    """acc_row29's peeled first addition (ZZ = ZZZ = ONE): the four products by ONE = R29 mod p are
    replaced by the value itself.  For a < k p, mont(a, ONE) = (a ONE + m p) / R29 with m < R29 is
    congruent to a and below a ONE / R29 + p, so it is a's canonical residue c unless c < a ONE /
    R29: c >= T = ceil(k p ONE / R29) is enough.  The four values: q.x (< qin p; U2 = q.x needs q.x
    < p too), q.y or its negation (< ACC_NEG p; S2 = q.y or p - q.y needs q.y < p), PP and PPP (<
    2 p, canon29's range) -- k = ACC_NEG covers all four.  The kernel tests the two top limbs t =
    v >> 29 (n - 2): t >= PEEL_LO makes v >= T, t < p >> 29 (n - 2) makes v < p (a q.y >= p under
    a negation wraps p - q.y to a top limb of 2^32 - 1, which fails it).  -> PEEL_LO."""
    R = 1 << (W * n)
    ro = {k: Fraction(v) for k, v in roles.items()}
    x, y = qin, ro["ACC_NEG"]                    # the prologue's copy: the first point, y negated or not
    assert ro["ACC_P"] >= x and ro["ACC_R"] >= y  # P = sub29(q.x, x, ACC_P), R = sub29(S2, y, ACC_R)
    # (S2 = sub29(0, q.y, B1) needs q.y <= p: the guard's own condition, tested on the result)
    P = qin + ro["ACC_P"]
    PP = mont(P, P); PPP = mont(P, PP)
    assert PP < 2 and PPP < 2, "canon29's range"
    k = ro["ACC_NEG"]
    assert k >= max(qin, PP, PPP)
    T = -(-int(k) * p * (R % p) // R)
    shift = W * (n - 2)
    lo = -(-T // (1 << shift))
    assert lo << shift >= T and lo < 1 << W, "the threshold has to sit in limb n - 2"
    # a wave of 64 lanes x 4 values falls back when one of them lies below the threshold or shares
    # p's two top limbs: rarer than once in 2^10 waves
    assert 256 * ((lo + 1) << shift) * (1 << 10) < p
    return lo


def arr(v):
    return "{" + ", ".join("0x%xu" % x for x in v) + "}"


def emit(name, p, n, r32, b, nkp, roles):
    R29 = 1 << (W * n)
    assert p < R29 and (n - 1) * W < p.bit_length()
    bounds = check_bounds(p, n, nkp, roles, peel=name in PEEL_FIRST)
    inv = (-pow(p, -1, 1 << 32)) % (1 << 32)
    print("struct %s {  // R29 = 2^%d; loop bounds x < %.2fp, y < %.2fp, zz, zzz < %.2fp"
          % (name, W * n, bounds["X"], bounds["Y"], bounds["Z"]))
    print("  static constexpr int N = %d;" % n)
    print("  static constexpr uint32_t MOD[N] = %s;" % arr(limbs(p, n)))
    print("  static constexpr uint32_t INV = 0x%xu;  // -p^-1 mod 2^32 (used mod 2^29)" % inv)
    print("  static constexpr uint32_t ONE[N] = %s;  // R29 mod p" % arr(limbs(R29 % p, n)))
    e29 = 2 * W * n - r32
    print("  static constexpr uint32_t TO29[N] = %s;  // 2^%d mod p: mont29(x 2^%d, TO29) = x R29"
          % (arr(limbs((1 << e29) % p, n)), e29, r32))
    print("  static constexpr uint32_t TO32[N] = %s;  // 2^%d mod p: mont29(x R29, TO32) = x 2^%d"
          % (arr(limbs((1 << r32) % p, n)), r32, r32))
    print("  static constexpr uint32_t R2[N] = %s;  // R29^2 mod p: mont29(x, R2) = x R29" % arr(limbs(R29 * R29 % p, n)))
    print("  static constexpr uint32_t BCURVE[N] = %s;  // %d R29 mod p (y^2 = x^3 + %d)" % (arr(limbs(b * R29 % p, n)), b, b))
    for k in (1, 2, 4, 8, 16, 32, 64):
        print("  static constexpr uint32_t B%d[N] = %s;  // %d p, biased limbs" % (k, arr(biased(k, p, n)), k))
    for k in (4, 8):
        print("  static constexpr uint32_t C%d[N] = %s;  // %d p, limbs in [3 (2^29 - 1), 2^31) (sub3_29)"
              % (k, arr(biased3(k, p, n)), k))
    print("  // roles (tools/gen_params29.py check_bounds): the bias of each subtraction in acc_loop29 / dbl_affine29")
    for role, k in roles.items():
        kind = "C" if role == "ACC_X3" else "B"
        print("  static constexpr const uint32_t (&%s)[N] = %s%d;" % (role, kind, k))
    print("  static constexpr const uint32_t (&ACC_X3_B)[N] = B%d;  // ACC_X3 for two carry passes (A/B build)"
          % roles["ACC_X3"])
    if "PEEL_LO" in bounds:
        print("  static constexpr uint32_t PEEL_LO = %d;  // acc_row29's peeled first addition: a value whose top two"
              % bounds["PEEL_LO"])
        print("  // limbs v >> %d lie in [PEEL_LO, p >> %d) is its own product by ONE (check_bounds peel_threshold)"
              % (W * (n - 2), W * (n - 2)))
    print("  static constexpr int NKP = %d;" % nkp)
    print("  static constexpr uint32_t KP_LO[NKP] = %s;  // low limb of k p" % arr([(k * p) & MASK for k in range(nkp)]))
    print("  static constexpr uint32_t KP[NKP][N] = {%s};  // k p" % ", ".join(arr(limbs(k * p, n)) for k in range(nkp)))
    print("};\n")


def main():
    print("// GENERATED by tools/gen_params29.py -- do not edit.  Fp in radix 2^29: BLS12-381 (14 limbs,")
    print("// R29 = 2^406) and BN254 (9 limbs, R29 = 2^261).")
    print("#pragma once")
    print("#include <cstdint>\n")
    print("namespace kzgmi {\n")
    for c in CURVES:
        emit(*c)
    print("}  // namespace kzgmi")


if __name__ == "__main__":
    main()
