"""Plain big-integer model of the G1 point layer and the cases its probe tests run
(tests/test_gpu_points_ops.py on the GPU, tests/test_pointref_cpu.py without).

  csrc/g1.hpp      32-bit XYZZ formulas: from_affine, dbl, dbl_affine, add_affine, add, neg, to_affine,
                   affine_on_curve
  csrc/points.hpp  the radix-2^29 Jacobian chain of the BLS12-381 subgroup check (jac29_dbl,
                   jac29_add_affine, jac29_add, mul_by_x_abs29, zero29), fp_pow_sqrt29, fp_raw_gt,
                   compress_encoding
  csrc/glv.hpp     glv_round_div, glv_split
  csrc/launch_io.hip  convert_points (three forms), decompress_points, compress_points,
                   subgroup_check, glv_split, endo_points (two forms), convert_scalars, encode_points

Points are affine (x, y) tuples or None (oracle.pyspec.curves); the decomposition is
oracle.pyspec.glv's; word, limb and record encodings are those of tests/fieldref.py and
tests/msmref.py.  Device functions are `fieldref.Op`s (cases, encode, check); launchers are `Stage`s
(cases with their expected outputs, `run` = the probe call, `check` = every output against the model,
`expected` = the outputs a correct kernel returns, which the planted-fault tests damage).  Every
generator asserts its cases' preconditions; nothing is filtered on the GPU side.

How outputs are judged.  A projective result stands for an affine point, and that point is compared;
infinity is what the code's own test says (Xyzz: zz == 0, Jac29: the flag).  A finite XYZZ result must
have canonical coordinates and ZZ^3 = ZZZ^2.  A radix-29 coordinate must have normalised limbs and lie
below its bound.  Bytes, flags, error words and GLV half scalars are exact.

Bounds of the Jacobian chain (units of p; R29 = 2^406, p / R29 < 2^-25, so a product of inputs below
a p and b p is below (a b 2^-25 + 1) p, i.e. below 2 p for every pair here).
  jac29_dbl        X < 34, Y < 18, Z < 8  ->  X3 < 34, Y3 < 18, Z3 < 4: as documented.  D = 2 (D0 + 2p -
                   A + 2p - C) < 12, X3 = E^2 + 32p - 2D < 34, Y3 = E (..) + 16p - 8C < 18, Z3 = 2 Y Z < 4.
  jac29_add_affine documented "X3, Y3, Z3 < 8p".  That is the general branch alone (X3 < 8, Y3 < 6,
                   Z3 < 6).  The doubling branch (H = rr = 0) returns jac29_dbl(q): X3 = E^2 + 32p - 2D
                   with D < 12 is only below 34 (Y3 < 18, Z3 < 4), and the cancelling branch returns p's
                   own coordinates (X < 34, Y < 18, Z < 8) under the infinity flag.  All of them are
                   inside jac29_dbl's input contract, and the chain (mul_by_x_abs29) only ever hands an
                   addition's result to jac29_dbl, so the comment was corrected, not the code.
  jac29_add        documented "X3 < 8p, Y3 < 6p, Z3 < 2p": again the general branch; the doubling branch
                   returns jac29_dbl(p) (34, 18, 4), the cancelling branch p under the flag, an infinite
                   operand the other one.  Its consumers are jac29_dbl and fp_from29 (< 2^12 p).
  H, rr            jac29_add_affine: H < 66, rr < 68, tested by zero29 (any v < 2^12 p);
                   jac29_add: H < 4, rr < 8, tested by is_zero29 (v < NKP p = 20 p).
check_jac holds each result to the bound of the branch the model says it took.

Barrett corrections of glv_round_div.  The estimate q3 = ((N >> 224) mu) >> 288 is the true quotient
for every one of 10^6 seeded random scalars per curve and multiplier (search run while writing this
model: 0 corrections 10^6 times, 1 and 2 never).  One correction needs N = k g + (r - 1) / 2 within
about 2^-30 r above a multiple of r; `barrett_scalars` solves k g + (r - 1) / 2 = rem (mod r) for
small rem, which gives 1-correction cases for every multiplier.  No 2-correction case was found,
neither by the random search nor in that family."""
import random

import fieldref as F
import msmref
import pointcases
import test_glv
from oracle.pyspec import curves as pc
from oracle.pyspec import glv
from oracle.pyspec import kzg as pk

SEED = 20261020
NRANDOM = 2048
CURVES = F.CURVES
DERR_ENCODING, DERR_NOT_ON_CURVE, DERR_SCALAR, DERR_NOT_IN_SUBGROUP = 1, 2, 3, 4
DERR_OF = {pointcases.ERR_ENCODING: DERR_ENCODING, pointcases.ERR_NOT_ON_CURVE: DERR_NOT_ON_CURVE,
           pointcases.ERR_NOT_IN_SUBGROUP: DERR_NOT_IN_SUBGROUP, None: 0}
X_ABS = pointcases.X_ABS
COFACTOR_PRIMES = [3, 11, 10177, 859267, 52437899]
N_SINGLE = 300          # cases of a single-launch call: more than one block of 256
N_EACH_MAX = 320        # cases of a per-element call (one launch each)
Op = F.Op
hexs = F.hexs


def _rng(tag):
    return random.Random("%d %s" % (SEED, tag))


class Curve:
    """Encoders and decoders of one curve's point forms."""

    def __init__(self, curve):
        self.curve, self.C = curve, pc.CURVES[curve]
        self.M, self.L = msmref.layers(curve)          # radix-29 and 32-bit layers of fieldref
        self.p, self.r = self.C.p, self.C.r
        self.W, self.R32, self.n29 = self.L.W, self.L.R32, self.M.N
        self.nb = self.C.fp_bytes
        assert 4 * self.W == self.nb
        self.slot_words = 32 if 2 * self.W == 24 else 2 * self.W       # g1.hpp kAffineAlign
        self.packed = 4 * self.slot_words < 2 * self.n29 * 4           # msm.hpp kPackPts
        self.beta = glv.params(curve)[0]
        self.half = (self.p - 1) // 2
        # the documented bound of a converted coordinate, (p / R29 + 1) p
        self.qin = self.M.bounds["qin"]

    # ---- 32-bit Montgomery words (field.hpp)
    def fpw(self, v):
        return F.to_words(v * self.R32 % self.p, self.W)

    def fp_of(self, words):
        """(field element, raw integer) of Montgomery words"""
        raw = F.from_words(words)
        return raw * pow(self.R32, -1, self.p) % self.p, raw

    def affw(self, P):
        return self.fpw(P[0]) + self.fpw(P[1])

    def xyzzw(self, P, lam):
        """(P, lam): ZZ = lam^2, ZZZ = lam^3.  P = None: Xyzz::inf() for lam = 1, else zz = zzz = 0
        under coordinates that are no point's (what xyzz_dbl makes of an infinite operand)."""
        if P is None and lam != 1:
            return self.fpw(7 * lam) + self.fpw(11 * lam) + [0] * (2 * self.W)
        return self.L.xyzz(P, lam)

    def xyzz_decode(self, words):
        """(point or None, None) or (None, what is wrong)"""
        p, W = self.p, self.W
        v = [self.fp_of(words[i * W:(i + 1) * W]) for i in range(4)]
        for nm, (_, raw) in zip(("x", "y", "zz", "zzz"), v):
            if raw >= p:
                return None, "%s not canonical: %#x" % (nm, raw)
        X, Y, ZZ, ZZZ = (e for e, _ in v)
        if ZZ == 0:                                    # Xyzz::is_inf
            return None, None
        if pow(ZZ, 3, p) != pow(ZZZ, 2, p):
            return None, "not a point: ZZ^3 != ZZZ^2"
        return (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p), None

    def slot32(self, P, pad=0):
        """An Affine slot in 32-bit form (O: zeros, flagged apart); pad fills the slot's unused words."""
        w = [0] * (2 * self.W) if P is None else self.affw(P)
        return w + [pad] * (self.slot_words - 2 * self.W)

    # ---- point slots in the accumulation's radix-29 form (msm.hpp store_pt29 / load_pt29)
    def slot29(self, vx, vy, pad=0):
        """vx, vy: the integers x R29, y R29 (mod p, below 2^256 when packed)"""
        if self.packed:
            return F.to_words(vx, self.W) + F.to_words(vy, self.W)
        return F.limbs29(vx, self.n29) + F.limbs29(vy, self.n29) + [pad] * (self.slot_words - 2 * self.n29)

    def slot29_decode(self, words):
        """((vx, vy), None) or (None, what is wrong)"""
        if self.packed:
            return (F.from_words(words[:self.W]), F.from_words(words[self.W:2 * self.W])), None
        n = self.n29
        for i in range(2 * n):
            if (i + 1) % n and words[i] > F.M29:
                return None, "limb %d not normalised: %#x" % (i, words[i])
        return (F.value29(words[:n]), F.value29(words[n:2 * n])), None

    def slot_used(self, form29):
        return 2 * self.W if not form29 or self.packed else 2 * self.n29

    def conv29(self, v):
        """What k_convert_points<To29> makes of a canonical coordinate: mont29(v, R29^2)."""
        return self.M.mont(v, F.value29(self.M.H["R2"]))

    def check_slot29(self, words, want, bound, what):
        """A radix-29 slot against the point it must hold (None: zeros) and the bound of its
        coordinates (units of p)."""
        got, msg = self.slot29_decode(words)
        if msg:
            return "%s: %s" % (what, msg)
        if want is None:
            return None if got == (0, 0) else "%s: rejected or infinite point's slot not zero: %s" % (what, hexs(got))
        aff = (self.M.from_m(got[0]), self.M.from_m(got[1]))
        if aff != want:
            return "%s: holds %s, want %s" % (what, hexs(aff), hexs(want))
        for nm, v in zip("xy", got):
            if not v < bound * self.p:
                return "%s: %s = %.6f p, documented bound %.6f p" % (what, nm, v / self.p, float(bound))
        return None

    # ---- encodings
    def enc_words(self, data):
        """bytes as the kernels load them: little-endian words"""
        assert len(data) % 4 == 0
        return [int.from_bytes(data[i:i + 4], "little") for i in range(0, len(data), 4)]

    def words_bytes(self, words):
        return b"".join(int(w).to_bytes(4, "little") for w in words)

    def raw(self, x, y):
        return x.to_bytes(self.nb, "big") + y.to_bytes(self.nb, "big")

    # ---- points
    def random_curve_point(self, rng):
        return pointcases._random_curve_point(self.C, rng)

    def specials(self):
        """BLS12-381: the order-3 points (0, +-2), 2T = -T; BN254: the points with x = 1 and x = p - 1."""
        p, b = self.p, self.C.b
        if self.curve == "bls12_381":
            out = [(0, 2), (0, p - 2)]
        else:
            out = []
            for x in (1, p - 1):
                y = pow((x ** 3 + b) % p, (p + 1) // 4, p)
                assert y * y % p == (x ** 3 + b) % p
                out += [(x, y), (x, p - y)]
        assert all(pc.g1_on_curve(P, self.C) for P in out)
        return out

    def lams(self, rng):
        p = self.p
        return [1, 2, p - 1, (p + 1) // 2, rng.randrange(3, p - 1)]


_curves = {}


def curve_of(curve):
    if curve not in _curves:
        _curves[curve] = Curve(curve)
    return _curves[curve]


# ====================================================================== g1.hpp: 32-bit XYZZ
def pair_matrix(K, rng, finite_q=False):
    """(P, lam1, Q, lam2): P + Q, P + P, P + (-P), O + Q, P + O, O + O over the lambda set squared
    (chosen independently, so equal points have unequal coordinates), the curve's special points
    among the P, then NRANDOM seeded cases.  finite_q: Q is an affine operand, never O."""
    C = K.C
    pool = K.M.point_pool(rng, 64)
    lams = K.lams(rng)
    cases = []
    for i, P in enumerate(K.specials() + pool[:3]):
        Q = pool[8 + i]
        for l1 in lams:
            for l2 in lams:
                cases += [(P, l1, Q, l2), (P, l1, P, l2), (P, l1, pc.g1_neg(P, C), l2), (None, l1, Q, l2)]
                if not finite_q:
                    cases += [(P, l1, None, l2), (None, l1, None, l2)]
    lam = lambda: rng.randrange(1, K.p)  # noqa: E731
    for _ in range(NRANDOM):
        P, Q = rng.choice(pool), rng.choice(pool)
        kind = rng.randrange(16)
        Q = P if kind == 0 else pc.g1_neg(P, C) if kind == 1 else Q
        if kind == 2:
            P = None
        elif kind == 3 and not finite_q:
            Q = None
        cases.append((P, lam(), Q, lam()))
    assert all(c[1] % K.p and c[3] % K.p for c in cases)
    assert all(X is None or pc.g1_on_curve(X, C) for c in cases for X in (c[0], c[2]))
    assert not finite_q or all(c[2] is not None for c in cases)
    return cases


def g1_ops(curve):
    K = curve_of(curve)
    C, p, W = K.C, K.p, K.W
    rng = _rng(curve + " g1")
    pairs = pair_matrix(K, rng)
    pairs_aff = pair_matrix(K, rng, finite_q=True)
    singles = F.dedupe([(None, 1), (None, 2)] + [(P, l) for P, l, _, _ in pairs if P is not None][:600]
                       + [(P, l) for P, l, _, _ in pairs[-NRANDOM:] if P is not None])
    affs = F.dedupe([(P,) for P, _ in singles if P is not None])

    def point_out(want):
        def check(case, out):
            got, msg = K.xyzz_decode(out)
            if msg:
                return msg
            w = want(case)
            return None if got == w else "got %s, want %s" % (got and hexs(got), w and hexs(w))
        return check

    def chk_to_affine(case, out):
        P = case[0]
        if P is None:
            return None if out[0] == 0 else "flag %d for infinity" % out[0]
        if out[0] != 1:
            return "flag %d for a finite point" % out[0]
        return None if out[1:] == K.affw(P) else "got %s, want %s" % (
            hexs([K.fp_of(out[1:1 + W])[0], K.fp_of(out[1 + W:])[0]]), hexs(P))

    # on-curve: points, their neighbours, the origin, (x, -y)
    oc = []
    for P in K.specials() + [a[0] for a in affs[:256]]:
        oc += [P, (P[0], (P[1] + 1) % p), ((P[0] + 1) % p, P[1]), (P[0], p - P[1]), (P[1] % p, P[0])]
    oc += [(0, 0), (0, 1), (1, 0), (p - 1, p - 1)]
    oc = F.dedupe(oc)
    assert any(pc.g1_on_curve(P, C) for P in oc) and not all(pc.g1_on_curve(P, C) for P in oc)

    def chk_on_curve(case, out):
        want = int(pc.g1_on_curve(case, C))
        return None if out == [want] else "got %r, want %d" % (out, want)

    dbl = lambda P: pc.g1_add(P, P, C)  # noqa: E731
    ops = [
        Op("g1.xyzz_from_affine", affs, lambda c: K.affw(c[0]), point_out(lambda c: c[0])),
        Op("g1.xyzz_dbl", singles, lambda c: K.xyzzw(*c), point_out(lambda c: dbl(c[0]))),
        Op("g1.xyzz_dbl_affine", affs, lambda c: K.affw(c[0]), point_out(lambda c: dbl(c[0]))),
        Op("g1.xyzz_add_affine", pairs_aff, lambda c: K.xyzzw(c[0], c[1]) + K.affw(c[2]),
           point_out(lambda c: pc.g1_add(c[0], c[2], C))),
        Op("g1.xyzz_add", pairs, lambda c: K.xyzzw(c[0], c[1]) + K.xyzzw(c[2], c[3]),
           point_out(lambda c: pc.g1_add(c[0], c[2], C))),
        Op("g1.xyzz_neg", singles, lambda c: K.xyzzw(*c), point_out(lambda c: pc.g1_neg(c[0], C))),
        Op("g1.xyzz_to_affine", singles, lambda c: K.xyzzw(*c), chk_to_affine),
        Op("g1.affine_on_curve", oc, lambda c: K.affw(c), chk_on_curve),
    ]
    return ops


# ====================================================================== points.hpp: encoding helpers
def compress_model(curve, data):
    """compress_encoding / k_compress_points: no validation; the infinity test is the encoding's own
    (BLS12-381: bit 0x40 of byte 0, BN254: all zeros)."""
    K = curve_of(curve)
    n = K.nb
    assert len(data) == 2 * n
    larger = int.from_bytes(data[n:], "big") > K.half
    if curve == "bls12_381":
        if data[0] & 0x40:
            return bytes([0xC0]) + bytes(n - 1)
        return bytes([data[0] | 0x80 | (0x20 if larger else 0)]) + data[1:n]
    if not any(data):
        return bytes([0x40]) + bytes(n - 1)
    return bytes([data[0] | (0xC0 if larger else 0x80)]) + data[1:n]


def compress_cases(curve):
    """y free (the kernel does not validate): (p - 1) / 2 and (p + 1) / 2, the exact edge of the
    'larger' flag, which no curve point has (tests/test_pointref_cpu.py); 0, 1, p - 1; curve points
    with both signs; both infinity forms; x with every bit below the flags set."""
    K = curve_of(curve)
    p, n, rng = K.p, K.nb, _rng(curve + " compress")
    xs = [0, 1, p - 1, rng.randrange(p), (1 << (p.bit_length() - 1)) - 1]
    ys = [K.half, K.half + 1, K.half - 1, K.half + 2, 0, 1, p - 1]
    out = [K.raw(x, y) for x in xs for y in ys if x or y]
    for P in K.specials() + K.M.point_pool(rng, 16):
        out += [K.raw(*P), K.raw(P[0], p - P[1])]
    out.append(pk.g1_to_bytes(None, K.C))
    if curve == "bls12_381":
        out.append(bytes([0x40]) + K.raw(3, 5)[1:])        # flagged infinite over junk: still infinity
    else:
        out.append(K.raw(0, 1))                            # not all zero: a finite encoding
    out += [K.raw(rng.randrange(p), rng.randrange(p)) for _ in range(64)]
    assert all(len(b) == 2 * n for b in out)
    return out


def point_helper_ops(curve):
    K = curve_of(curve)
    p, W, rng = K.p, K.W, _rng(curve + " helpers")
    top = (1 << (32 * W)) - 1
    vals = [0, 1, K.half - 1, K.half, K.half + 1, p - 1, p, top]
    for i in range(W):                                      # HALF with one word moved either way
        for d in (-1, 1):
            v = K.half + d * (1 << (32 * i))
            vals += [v, v ^ (1 << (32 * i + 31))]
    vals = F.dedupe([v for v in vals if 0 <= v <= top]) + [rng.randrange(top + 1) for _ in range(NRANDOM)]

    def chk_gt(case, out):
        want = int(case[0] > K.half)
        return None if out == [want] else "got %r, want %d" % (out, want)

    def chk_comp(case, out):
        want = K.enc_words(compress_model(curve, case[0]))
        return None if out == want else "got %s, want %s" % (K.words_bytes(out).hex(), K.words_bytes(want).hex())
    return [Op("pt.fp_raw_gt_half", [(v,) for v in vals], lambda c: F.to_words(c[0], W), chk_gt),
            Op("pt.compress_encoding", [(b,) for b in compress_cases(curve)], lambda c: K.enc_words(c[0]), chk_comp)]


# ====================================================================== points.hpp: the Jacobian chain
JAC_IN = (34, 18, 8)            # jac29_dbl's and jac29_add_affine's input contract, units of p
JAC_DBL_OUT = (34, 18, 4)       # jac29_dbl's outputs = jac29_add's input contract
JAC_MADD_OUT = (8, 6, 6)        # jac29_add_affine, general branch
JAC_ADD_OUT = (8, 6, 2)         # jac29_add, general branch
ZERO29_RANGE = 1 << 12          # zero29: any v < 2^12 p


class Jac:
    """(P, lam, shifts, inf): X = x lam^2, Y = y lam^3, Z = lam in radix-29 Montgomery form, each plus
    shifts[i] p.  inf: the flag; the coordinates (those of P) are then ignored by the model."""

    def __init__(self):
        self.K = curve_of("bls12_381")
        self.M, self.p, self.n = self.K.M, self.K.p, self.K.n29
        self.one = F.value29(self.M.H["ONE"])

    def vals(self, P, lam, sh):
        p, M = self.p, self.M
        return (M.to_m(P[0] * lam * lam % p, sh[0]), M.to_m(P[1] * pow(lam, 3, p) % p, sh[1]), M.to_m(lam % p, sh[2]))

    def enc(self, op):
        P, lam, sh, inf = op
        return [w for v in self.vals(P, lam, sh) for w in F.limbs29(v, self.n)] + [int(inf)]

    def enc29(self, v):
        return F.limbs29(v, self.n)

    def point(self, op):
        return None if op[3] else op[0]

    def decode(self, out):
        """((X, Y, Z), inf flag, None) or (.., .., what is wrong)"""
        n = self.n
        for i in range(3 * n):
            if (i + 1) % n and out[i] > F.M29:
                return None, None, "limb %d not normalised: %#x" % (i, out[i])
        if out[3 * n] > 1:
            return None, None, "infinity flag %#x" % out[3 * n]
        return tuple(F.value29(out[i * n:(i + 1) * n]) for i in range(3)), bool(out[3 * n]), None

    def check(self, out, want, bound, exact=None):
        """want: the affine point or None; bound: (X, Y, Z) in units of p, held for infinite results
        too (jac29_dbl computes on them); exact: the (X, Y, Z) a branch must hand through."""
        v, inf, msg = self.decode(out)
        if msg:
            return msg
        p, M = self.p, self.M
        if inf != (want is None):
            return "infinity flag %d, want %s" % (inf, want and hexs(want))
        if exact is not None and v != tuple(exact):
            return "operand not handed through: got %s" % hexs(v)
        for nm, x, b in zip("XYZ", v, bound):
            if not x < b * p:
                return "%s = %.4f p, bound %d p" % (nm, x / p, b)
        if want is None:
            return None
        z = M.from_m(v[2])
        if z == 0:
            return "Z = 0 mod p on a result not flagged infinite"
        zi = pow(z, -1, p)
        got = (M.from_m(v[0]) * zi * zi % p, M.from_m(v[1]) * pow(zi, 3, p) % p)
        return None if got == want else "got %s, want %s" % (hexs(got), hexs(want))


def jac29_dbl_x3(X, Y):
    """jac29_dbl's X3 as the integer the code computes: E^2 / R29 + 32 p - 2 D, D = 2 (D0 + 2p - A + 2p - C).
    With D < 12 p it is at least 8 p for every input: the doubling branch of an addition cannot keep
    the general branch's X3 < 8p."""
    M = curve_of("bls12_381").M
    p = M.p
    A, B = M.mont(X, X), M.mont(Y, Y)
    Cc = M.mont(B, B)
    D = 2 * (M.mont(X + B, X + B) + 2 * p - A + 2 * p - Cc)
    E = 3 * A
    return M.mont(E, E) + 32 * p - 2 * D


_jac = []


def jac():
    if not _jac:
        _jac.append(Jac())
    return _jac[0]


def jac_operands(rng, bound, pool, specials):
    """Operands over the point set at k = 0 and k = bound - 1 per coordinate (all low, all high, and
    the two mixed patterns), over the lambda set."""
    K = curve_of("bls12_381")
    top = tuple(b - 1 for b in bound)
    shifts = [(0, 0, 0), top, (top[0], 0, top[2]), (0, top[1], 0)]
    out = []
    for P in specials + pool:
        for lam in K.lams(rng):
            for sh in shifts:
                out.append((P, lam, sh))
    return out, shifts


def jac_ops():
    J = jac()
    K, C, p, M = J.K, J.K.C, J.p, J.M
    rng = _rng("jac29")
    pool = M.point_pool(rng, 64)
    pts = K.specials() + pool[:3]
    rs = lambda bound: tuple(rng.randrange(b) for b in bound)  # noqa: E731
    lam = lambda: rng.randrange(1, p)  # noqa: E731
    dbl = lambda P: pc.g1_add(P, P, C)  # noqa: E731
    ops = []

    def in_bound(op, bound):
        return all(v < b * p for v, b in zip(J.vals(*op[:3]), bound))

    # -- jac29_dbl
    base, shifts = jac_operands(rng, JAC_IN, pool[:3], K.specials())
    dc = [(o + (False,),) for o in base] + [(base[i] + (True,),) for i in range(0, len(base), 7)]
    dc += [((rng.choice(pool), lam(), rs(JAC_IN), rng.randrange(16) == 0),) for _ in range(NRANDOM)]
    assert all(in_bound(c[0], JAC_IN) for c in dc)
    ops.append(Op("jac29.dbl", dc, lambda c: J.enc(c[0]),
                  lambda c, out: J.check(out, dbl(J.point(c[0])), JAC_DBL_OUT)))

    # -- jac29_add_affine: q affine below 2 p
    def q_vals(Q, kq):
        return (M.to_m(Q[0], kq[0]), M.to_m(Q[1], kq[1]))
    ac = []
    for i, P in enumerate(pts):
        Q = pool[8 + i]
        for l1 in K.lams(rng):
            for sh in shifts:
                for kq in ((0, 0), (1, 1)):
                    ac += [((P, l1, sh, False), Q, kq), ((P, l1, sh, False), P, kq),
                           ((P, l1, sh, False), pc.g1_neg(P, C), kq), ((P, l1, sh, True), Q, kq)]
    for _ in range(NRANDOM):
        P, Q = rng.choice(pool), rng.choice(pool)
        kind = rng.randrange(16)
        Q = P if kind == 0 else pc.g1_neg(P, C) if kind == 1 else Q
        ac.append(((P, lam(), rs(JAC_IN), kind == 2), Q, (rng.randrange(2), rng.randrange(2))))
    assert all(in_bound(a, JAC_IN) and all(v < 2 * p for v in q_vals(Q, kq)) for a, Q, kq in ac)

    def chk_madd(case, out):
        a, Q, kq = case
        P = J.point(a)
        want = pc.g1_add(P, Q, C)
        if P is None:
            return J.check(out, Q, (2, 2, 1), exact=q_vals(Q, kq) + (J.one,))
        if want is None:                       # cancelling branch: p itself under the flag
            return J.check(out, None, JAC_IN, exact=J.vals(*a[:3]))
        return J.check(out, want, JAC_DBL_OUT if P == Q else JAC_MADD_OUT)
    ops.append(Op("jac29.add_affine", ac, lambda c: J.enc(c[0]) + J.enc29(q_vals(c[1], c[2])[0]) + J.enc29(q_vals(c[1], c[2])[1]),
                  chk_madd))

    # -- jac29_add: both operands as jac29_dbl's outputs
    base2, shifts2 = jac_operands(rng, JAC_DBL_OUT, [], [])
    jc = []
    for i, P in enumerate(pts):
        Q = pool[8 + i]
        for l1, l2 in zip(K.lams(rng), reversed(K.lams(rng))):
            for sh in shifts2:
                for sh2 in shifts2:
                    a = (P, l1, sh, False)
                    jc += [(a, (Q, l2, sh2, False)), (a, (P, l2, sh2, False)), (a, (pc.g1_neg(P, C), l2, sh2, False)),
                           ((P, l1, sh, True), (Q, l2, sh2, False)), (a, (Q, l2, sh2, True)),
                           ((P, l1, sh, True), (Q, l2, sh2, True))]
    for _ in range(NRANDOM):
        P, Q = rng.choice(pool), rng.choice(pool)
        kind = rng.randrange(16)
        Q = P if kind == 0 else pc.g1_neg(P, C) if kind == 1 else Q
        jc.append(((P, lam(), rs(JAC_DBL_OUT), kind == 2), (Q, lam(), rs(JAC_DBL_OUT), kind == 3)))
    assert all(in_bound(a, JAC_DBL_OUT) and in_bound(b, JAC_DBL_OUT) for a, b in jc)

    def chk_add(case, out):
        a, b = case
        P, Q = J.point(a), J.point(b)
        if P is None or Q is None:             # the other operand, flag and all
            o = b if P is None else a
            return J.check(out, J.point(o), JAC_DBL_OUT, exact=J.vals(*o[:3]))
        want = pc.g1_add(P, Q, C)
        if want is None:
            return J.check(out, None, JAC_DBL_OUT, exact=J.vals(*a[:3]))
        return J.check(out, want, JAC_DBL_OUT if P == Q else JAC_ADD_OUT)
    ops.append(Op("jac29.add", jc, lambda c: J.enc(c[0]) + J.enc(c[1]), chk_add))

    # -- mul_by_x_abs29: [|x|] q.  <true>: q = (qx, qy, 1), as k_subgroup_check calls it, converted
    # coordinates below 2 p; <false>: q a result of the first chain (jac29_dbl's outputs) or infinity
    mem, non = subgroup_points()
    mp = [P for P, _ in mem[:12] + non[:12] + non[-10:]]
    mc = [((P, 1, (0, 0, 0), False), kq) for P in mp for kq in ((0, 0), (1, 1))]
    ops.append(Op("jac29.mul_by_x_affine", mc,
                  lambda c: J.enc(c[0]) + J.enc29(q_vals(c[0][0], c[1])[0]) + J.enc29(q_vals(c[0][0], c[1])[1]),
                  lambda c, out: J.check(out, pc.g1_mul_unreduced(c[0][0], X_ABS, C), JAC_DBL_OUT)))
    top = tuple(b - 1 for b in JAC_DBL_OUT)
    xc = [((P, l, sh, False), (0, 0)) for P in mp for l, sh in ((1, (0, 0, 0)), (lam(), top))]
    xc += [((mp[0], 5, top, True), (0, 0))]
    assert all(in_bound(c[0], JAC_DBL_OUT) for c in xc)
    ops.append(Op("jac29.mul_by_x_jac", xc,
                  lambda c: J.enc(c[0]) + J.enc29(q_vals(c[0][0], c[1])[0]) + J.enc29(q_vals(c[0][0], c[1])[1]),
                  lambda c, out: J.check(out, pc.g1_mul_unreduced(J.point(c[0]), X_ABS, C), JAC_DBL_OUT)))

    # -- zero29: k p and k p +- 1 for k up to 2^12 - 1 in steps, both ends exactly
    ks = sorted(set([0, 1, 2, 19, 20, 21, ZERO29_RANGE - 2, ZERO29_RANGE - 1] + list(range(0, ZERO29_RANGE, 37))))
    zv = [k * p + e for k in ks for e in (-1, 0, 1) if 0 <= k * p + e]
    zv += [rng.randrange(ZERO29_RANGE * p) for _ in range(NRANDOM)] + [rng.randrange(ZERO29_RANGE) * p for _ in range(256)]
    assert all(0 <= v < ZERO29_RANGE * p for v in zv) and {0, (ZERO29_RANGE - 1) * p, (ZERO29_RANGE - 1) * p + 1} <= set(zv)

    def chk_zero(case, out):
        want = int(case[0] % p == 0)
        return None if out == [want] else "got %r, want %d" % (out, want)
    ops.append(Op("jac29.zero29", [(v,) for v in zv], lambda c: J.enc29(c[0]), chk_zero))

    # -- fp_pow_sqrt29: a^((p + 1) / 4) on canonical 32-bit Montgomery words, canonical out
    m32 = F.layer("fp", "bls12_381")
    R, rinv = m32.R, pow(m32.R, -1, p)
    sq = [(a,) for a in m32.canonical_edges()] + [(rng.randrange(p),) for _ in range(NRANDOM)]
    sq += [(y * y % p * R % p,) for y in (2, p - 2, rng.randrange(p))]
    ops.append(Op("jac29.fp_pow_sqrt29", sq, lambda c: F.to_words(c[0], m32.N),
                  lambda c, out: None if F.from_words(out) == pow(c[0] * rinv % p, (p + 1) // 4, p) * R % p
                  else "got %#x" % F.from_words(out)))
    return ops


# ====================================================================== subgroup membership
_sub = {}


def subgroup_points():
    """([(member, tag)], [(non-member, tag)]) of BLS12-381.  Truth is [r]P = O by definition
    (pc.g1_in_subgroup), asserted in tests/test_pointref_cpu.py."""
    if "pts" not in _sub:
        C, rng = pc.BLS12_381, _rng("subgroup")
        G = C.g1
        mem = [(G, "G"), (pc.g1_neg(G, C), "-G"), (pc.g1_mul(G, C.r - 1, C), "[r-1]G")]
        mem += [(pc.g1_mul(G, rng.randrange(1, C.r), C), "G1 %d" % i) for i in range(64)]
        non = [(P, "random %d" % i) for i, P in enumerate(pointcases.non_subgroup_points(64, seed=SEED))]
        small = [(pointcases.small_order_point(ell), "order %d" % ell) for ell in COFACTOR_PRIMES]
        shifted = [(pc.g1_add(mem[3 + i][0], T, C), "G1 + %s" % tag) for i, (T, tag) in enumerate(small)]
        _sub["pts"] = (mem, non + small + shifted)
    return _sub["pts"]


def vanishing_prefixes(ell):
    """The bit positions b at which the chain's running multiple X_ABS >> b vanishes mod ell: a point
    of order ell goes through infinity there, and leaves it at the next set bit."""
    return [b for b in range(63, -1, -1) if (X_ABS >> b) % ell == 0]


def single_launch_members():
    """600 members for the single-launch mode: a walk P, P + S, ... inside G1."""
    if "walk" not in _sub:
        C, rng = pc.BLS12_381, _rng("walk")
        P = pc.g1_mul(C.g1, rng.randrange(1, C.r), C)
        S = pc.g1_mul(C.g1, rng.randrange(1, C.r), C)
        out = []
        for _ in range(600):
            out.append(P)
            P = pc.g1_add(P, S, C)
        _sub["walk"] = out
    return _sub["walk"]


SINGLE_POSITIONS = [0, 255, 256, 599]


# ====================================================================== glv.hpp
def sign_magnitude(v):
    assert abs(v) < 1 << 127, "half scalar reaches the sign bit"
    return abs(v) | ((1 << 127) if v < 0 else 0)


def glv_multipliers(curve):
    _, _, v1, v2 = glv.params(curve)
    return {"g1": v2[1], "g2": -v1[1]}


def barrett_scalars(curve, g):
    """Scalars with k g + (r - 1) / 2 = rem (mod r) for small rem: the quotient estimate is one short."""
    r = pc.CURVES[curve].r
    half = (r - 1) // 2
    return [(rem - half) * pow(g, -1, r) % r for rem in range(6)]


def glv_scalars(curve, nrandom=20000):
    """edge_scalars, the scalars next to each multiplier's Babai rounding boundary
    k = floor((m + 1/2) r / g) and its neighbours for m over an edge set, the Barrett family, random."""
    r = pc.CURVES[curve].r
    rng = _rng(curve + " glv")
    out = list(glv.edge_scalars(curve, 128))
    for g in glv_multipliers(curve).values():
        ms = F.dedupe([0, 1, 2, g // 2, g - 2, g - 1] + [rng.randrange(g) for _ in range(32)])
        for m in ms:
            if not 0 <= m < g:
                continue
            k = ((2 * m + 1) * r) // (2 * g)
            out += [k - 1, k, k + 1]
        out += barrett_scalars(curve, g)
    out = F.dedupe([k for k in out if 0 <= k < r])
    out += [rng.randrange(r) for _ in range(nrandom)]
    return out


def split_words(curve, k):
    """The two sign-magnitude half scalars glv_split must return for k, as 4 + 4 words."""
    k0, k1 = glv.decompose(curve, k)
    return F.to_words(sign_magnitude(k0), 4) + F.to_words(sign_magnitude(k1), 4)


def check_split(curve, k, out):
    want = split_words(curve, k)
    if out == want:
        return None
    for h, nm in ((out[:4], "h0"), (out[4:], "h1")):
        if F.from_words(h) == 1 << 127:
            return "%s is a negative zero" % nm
    return "got (%#x, %#x), want (%#x, %#x)" % (F.from_words(out[:4]), F.from_words(out[4:]),
                                                  F.from_words(want[:4]), F.from_words(want[4:]))


def glv_ops(curve):
    r = pc.CURVES[curve].r
    ks = glv_scalars(curve)
    enc = lambda c: F.to_words(c[0], 8)  # noqa: E731
    ops = []
    for nm, g in glv_multipliers(curve).items():
        assert 0 < g < 1 << 128
        ops.append(Op("glv.round_div_" + nm, [(k,) for k in ks], enc,
                      lambda c, out, g=g: None if F.from_words(out) == (2 * c[0] * g + r) // (2 * r)
                      else "got %#x, want %#x" % (F.from_words(out), (2 * c[0] * g + r) // (2 * r))))
    ops.append(Op("glv.split", [(k,) for k in ks], enc, lambda c, out: check_split(curve, c[0], out)))
    return ops


# ====================================================================== registry of device-function ops
OP_NAMES = {"g1": ["xyzz_from_affine", "xyzz_dbl", "xyzz_dbl_affine", "xyzz_add_affine", "xyzz_add", "xyzz_neg",
                   "xyzz_to_affine", "affine_on_curve"],
            "pt": ["fp_raw_gt_half", "compress_encoding"],
            "glv": ["round_div_g1", "round_div_g2", "split"],
            "jac29": ["dbl", "add_affine", "add", "mul_by_x_affine", "mul_by_x_jac", "zero29", "fp_pow_sqrt29"]}


def all_op_ids():
    ids = []
    for c in CURVES:
        for grp in ("g1", "pt", "glv") + (("jac29",) if c == "bls12_381" else ()):
            ids += [(c, "%s.%s" % (grp, o)) for o in OP_NAMES[grp]]
    return ids


_cache = {}


def ops_of(curve, group):
    key = (curve, group)
    if key not in _cache:
        mk = {"g1": lambda: g1_ops(curve), "pt": lambda: point_helper_ops(curve), "glv": lambda: glv_ops(curve),
              "jac29": jac_ops}[group]
        _cache[key] = {o.name: o for o in mk()}
        assert list(_cache[key]) == ["%s.%s" % (group, o) for o in OP_NAMES[group]]
    return _cache[key]


def op_of(curve, name):
    return ops_of(curve, name.split(".")[0])[name]


# ====================================================================== launch_io.hip: the stages
def convert_model(curve, data):
    """k_convert_points on one uncompressed encoding: (point or None, infinity flag, error code,
    zeroed) -- `zeroed`: the code stores zero coordinates (always in the radix-29 forms; in the 32-bit
    form only where the flags decide, a coordinate out of range or off the curve is stored as
    converted)."""
    K = curve_of(curve)
    n, p = K.nb, K.p
    if curve == "bls12_381":
        f = data[0] & 0xE0
        if f & 0x80:
            return None, 1, DERR_ENCODING, True
        if f & 0x40:
            bad = data[0] != 0x40 or any(data[1:])
            return None, 1, DERR_ENCODING if bad else 0, True
        if f & 0x20:
            return None, 1, DERR_ENCODING, True
    elif not any(data):
        return None, 1, 0, True
    x, y = int.from_bytes(data[:n], "big"), int.from_bytes(data[n:], "big")
    if x >= p or y >= p:
        return None, 1, DERR_ENCODING, False
    if not pc.g1_on_curve((x, y), K.C):
        return None, 1, DERR_NOT_ON_CURVE, False
    return (x, y), 0, 0, False


def decompress_model(curve, data):
    """k_decompress_points on one compressed encoding: (point or None, infinity flag, error code)."""
    K = curve_of(curve)
    p, b0 = K.p, data[0]
    if curve == "bls12_381":
        if not b0 & 0x80:
            return None, 1, DERR_ENCODING
        if b0 & 0x40:
            return None, 1, DERR_ENCODING if b0 != 0xC0 or any(data[1:]) else 0
        larger, x = bool(b0 & 0x20), int.from_bytes(bytes([b0 & 0x1F]) + data[1:], "big")
    else:
        m = b0 & 0xC0
        if m == 0x40:
            return None, 1, DERR_ENCODING if b0 != 0x40 or any(data[1:]) else 0
        if m == 0:
            return None, 1, DERR_ENCODING
        larger, x = m == 0xC0, int.from_bytes(bytes([b0 & 0x3F]) + data[1:], "big")
    if x >= p:
        return None, 1, DERR_ENCODING
    rhs = (x ** 3 + K.C.b) % p
    y = pow(rhs, (p + 1) // 4, p)
    if y * y % p != rhs:
        return None, 1, DERR_NOT_ON_CURVE
    if y == 0 and larger:
        return None, 1, DERR_ENCODING
    if (y > K.half) != larger:
        y = p - y
    return (x, y), 0, 0


def uncompressed_cases(curve):
    """pointcases.invalid_uncompressed plus the valid classes: random points, the curve's special
    points, x or y with a zero top byte, both infinity forms where the format has two."""
    K = curve_of(curve)
    rng = _rng(curve + " uncompressed")
    out = [b for b, _ in pointcases.invalid_uncompressed(K.C, rng)]
    out += [K.raw(*P) for P in K.specials() + K.M.point_pool(rng, 24)]
    out += [K.raw(K.p - 1, 1), K.raw((1 << (8 * K.nb - 3)) - 1, 2) if curve == "bls12_381" else K.raw((1 << 256) - 1, 2)]
    out.append(pk.g1_to_bytes(None, K.C))
    return out


def compressed_cases(curve):
    """For every valid class x with both sign flags; x = 0; x = 1 and p - 1 on BN254; x = p, p + 1 and
    every x bit set; a non-residue right-hand side; pointcases.invalid_compressed; both infinity forms
    (the canonical one, and infinity with a sign or junk, which is an error)."""
    K = curve_of(curve)
    C, p, n = K.C, K.p, K.nb
    rng = _rng(curve + " compressed")
    small, large = (0x80, 0xA0) if curve == "bls12_381" else (0x80, 0xC0)

    def enc(x, flag):
        b = bytearray(x.to_bytes(n, "big"))
        assert b[0] & (0xE0 if curve == "bls12_381" else 0xC0) == 0
        b[0] |= flag
        return bytes(b)
    xs = [P[0] for P in K.specials() + K.M.point_pool(rng, 24)] + [0, 1, p - 1, p, p + 1,
                                                                    (1 << (8 * n - (3 if curve == "bls12_381" else 2))) - 1]
    while True:                                           # right-hand side a non-residue
        x = rng.randrange(p)
        if pow((x ** 3 + C.b) % p, (p - 1) // 2, p) == p - 1:
            xs.append(x)
            break
    out = [enc(x, f) for x in F.dedupe(xs) for f in (small, large)]
    out += [b for b, _ in pointcases.invalid_compressed(C)]
    out.append(pk.g1_to_bytes_compressed(None, C))
    out.append(bytes(n))                                  # no flag at all
    return out


def cycle(cases, n):
    """cases repeated up to n of them (a single launch crosses a block boundary)"""
    return [cases[i % len(cases)] for i in range(max(n, len(cases)))]


class Stage:
    """One launcher of csrc/launch_io.hip on a list of cases.  Sub-classes give `inputs` (what the
    probe call takes), `call(probe, per_elem)` and `verdicts(out)` -> [(case index, message)]."""
    err_codes = None             # per case, where the stage has an error word
    slots = ()                   # (output name, radix-29 form) of the Affine slot arrays, for the padding check

    def __init__(self, curve, cases):
        self.curve, self.K, self.cases, self.n = curve, curve_of(curve), cases, len(cases)

    def check(self, out, per_elem, poison=0xA5):
        """Every output against the model: a list of messages, empty when all is right."""
        bad = ["guard behind %s overwritten" % nm for nm, ok in sorted(out["guards"].items()) if not ok]
        if self.err_codes is not None:
            err = [int(e) for e in out["err"]]
            if per_elem:
                bad += ["case %d: error %d, want %d" % (i, e, w) for i, (e, w) in enumerate(zip(err, self.err_codes)) if e != w]
                if len(err) != self.n:
                    bad.append("%d error words for %d cases" % (len(err), self.n))
            elif err != [max(self.err_codes)]:
                bad.append("error word %r, want %d" % (err, max(self.err_codes)))
        pw = poison * 0x01010101
        for nm, form29 in self.slots:                      # a kernel writes its own words of a slot only
            sw, used = self.K.slot_words, self.K.slot_used(form29)
            arr = out[nm]
            for i in range(self.n):
                if any(int(w) != pw for w in arr[i * sw + used:(i + 1) * sw]):
                    bad.append("case %d: %s slot written past its %d words" % (i, nm, used))
        bad += ["case %d: %s" % (i, m) for i, m in self.verdicts(out)]
        return bad

    def slot(self, arr, i):
        sw = self.K.slot_words
        return [int(w) for w in arr[i * sw:(i + 1) * sw]]


class ConvertPoints(Stage):
    def __init__(self, curve, form, cases=None):
        super().__init__(curve, cases or uncompressed_cases(curve))
        self.form = form
        self.model = [convert_model(curve, b) for b in self.cases]
        self.err_codes = [m[2] for m in self.model]
        self.slots = (("pts", form >= 1),) + ((("img", True),) if form == 2 else ())

    def call(self, probe, per_elem):
        return probe.convert_points(self.curve, self.form, b"".join(self.cases), self.n, per_elem)

    def verdicts(self, out):
        K, bad = self.K, []
        for i, (P, inf, _, zeroed) in enumerate(self.model):
            if int(out["inf"][i]) != inf:
                bad.append((i, "infinity flag %d, want %d" % (out["inf"][i], inf)))
            w = self.slot(out["pts"], i)
            if self.form == 0:
                want = K.slot32(P)[:2 * K.W]
                if (P is not None or zeroed) and w[:2 * K.W] != want:
                    bad.append((i, "slot holds %s, want %s" % (hexs(w[:2 * K.W]), hexs(want))))
                continue
            msg = K.check_slot29(w, P, K.qin, "slot")
            if msg:
                bad.append((i, msg))
            if self.form == 2:
                if int(out["img_inf"][i]) != inf:
                    bad.append((i, "image flag %d, want %d" % (out["img_inf"][i], inf)))
                msg = K.check_slot29(self.slot(out["img"], i), glv.phi(self.curve, P), K.qin, "image")
                if msg:
                    bad.append((i, msg))
        return bad

    def expected(self, per_elem, poison=0xA5):
        K, pw = self.K, poison * 0x01010101
        pts, img = [], []
        for P, inf, _, _ in self.model:
            if self.form == 0:
                pts += K.slot32(P, pw)
            else:
                pts += K.slot29(*(K.conv29(v) for v in (P or (0, 0))), pad=pw)
                Q = glv.phi(self.curve, P) or (0, 0)
                img += K.slot29(K.conv29(Q[0]), K.conv29(Q[1]), pad=pw)
        o = dict(pts=pts, inf=[m[1] for m in self.model], err=self.err_codes if per_elem else [max(self.err_codes)],
                 guards={"in": True, "pts": True, "inf": True, "err": True})
        if self.form == 2:
            o.update(img=img, img_inf=list(o["inf"]))
        return o


class DecompressPoints(Stage):
    slots = (("pts", False),)

    def __init__(self, curve, cases=None):
        super().__init__(curve, cases or compressed_cases(curve))
        self.model = [decompress_model(curve, b) for b in self.cases]
        self.err_codes = [m[2] for m in self.model]

    def call(self, probe, per_elem):
        return probe.decompress_points(self.curve, b"".join(self.cases), self.n, per_elem)

    def verdicts(self, out):
        K, bad = self.K, []
        for i, (P, inf, _) in enumerate(self.model):
            if int(out["inf"][i]) != inf:
                bad.append((i, "infinity flag %d, want %d" % (out["inf"][i], inf)))
            w, want = self.slot(out["pts"], i)[:2 * K.W], K.slot32(P)[:2 * K.W]
            if w != want:                                  # a rejected point's coordinates are zeroed
                bad.append((i, "slot holds %s, want %s" % (hexs(w), hexs(want))))
        return bad

    def expected(self, per_elem, poison=0xA5):
        pw = poison * 0x01010101
        return dict(pts=[w for P, _, _ in self.model for w in self.K.slot32(P, pw)], inf=[m[1] for m in self.model],
                    err=self.err_codes if per_elem else [max(self.err_codes)],
                    guards={"in": True, "pts": True, "inf": True, "err": True})


class CompressPoints(Stage):
    def __init__(self, curve, cases=None):
        super().__init__(curve, cases or compress_cases(curve))
        self.want = [compress_model(curve, b) for b in self.cases]

    def call(self, probe, per_elem):
        return probe.compress_points(self.curve, b"".join(self.cases), self.n, per_elem)

    def verdicts(self, out):
        n, got = self.K.nb, bytes(bytearray(int(b) for b in out["out"]))
        return [(i, "got %s, want %s" % (got[i * n:(i + 1) * n].hex(), w.hex()))
                for i, w in enumerate(self.want) if got[i * n:(i + 1) * n] != w]

    def expected(self, per_elem, poison=0xA5):
        return dict(out=list(b"".join(self.want)), guards={"in": True, "out": True})


class SubgroupCheck(Stage):
    """cases: (point, infinity flag, member).  A flagged entry is skipped whatever its coordinates."""

    def __init__(self, curve, cases):
        super().__init__(curve, cases)
        bls = curve == "bls12_381"        # BN254: cofactor 1, the launcher does nothing
        self.err_codes = [0 if (inf or member or not bls) else DERR_NOT_IN_SUBGROUP for _, inf, member in cases]

    def call(self, probe, per_elem):
        pts = [w for P, _, _ in self.cases for w in self.K.slot32(P)]
        return probe.subgroup_check(self.curve, pts, bytes(inf for _, inf, _ in self.cases), per_elem)

    def verdicts(self, out):
        return []

    def expected(self, per_elem, poison=0xA5):
        return dict(err=self.err_codes if per_elem else [max(self.err_codes)], guards={"pts": True, "inf": True, "err": True})


def subgroup_stage(curve, position=None):
    """position None: the per-element list (members, non-members, a flagged entry over coordinates
    that are no curve point's); else 600 members with one non-member at `position`."""
    mem, non = subgroup_points()
    if curve != "bls12_381":              # every curve point is a member; the stage must leave err alone
        K = curve_of(curve)
        return SubgroupCheck(curve, [(P, 0, True) for P in K.specials() + K.M.point_pool(_rng("bn sub"), 4)])
    if position is None:
        cases = [(P, 0, True) for P, _ in mem] + [(P, 0, False) for P, _ in non]
        cases += [((5, 7), 1, False), (non[0][0], 1, False)]
        return SubgroupCheck(curve, cases)
    cases = [(P, 0, True) for P in single_launch_members()]
    cases[position] = (non[position % len(non)][0], 0, False)
    return SubgroupCheck(curve, cases)


class GlvSplit(Stage):
    def __init__(self, curve, stride, cases):
        super().__init__(curve, cases)
        self.stride = stride
        self.want = [split_words(curve, k) for k in cases]

    def call(self, probe, per_elem):
        scal = []
        for i, k in enumerate(self.cases):                 # the words between scalars are not the kernel's to read
            scal += F.to_words(k, 8) + [0xDEAD0000 + (i & 0xFFFF)] * (self.stride - 8)
        return probe.glv_split(self.curve, scal, self.stride, self.n, per_elem)

    def verdicts(self, out):
        bad = []
        for i, k in enumerate(self.cases):
            got = [int(w) for w in out["h0"][4 * i:4 * i + 4]] + [int(w) for w in out["h1"][4 * i:4 * i + 4]]
            msg = check_split(self.curve, k, got)
            if msg:
                bad.append((i, "k = %#x: %s" % (k, msg)))
        return bad

    def expected(self, per_elem, poison=0xA5):
        return dict(h0=[w for s in self.want for w in s[:4]], h1=[w for s in self.want for w in s[4:]],
                    guards={"in": True, "h0": True, "h1": True})


class EndoPoints(Stage):
    """cases: (point or None, infinity flag, conv): phi(P) = (beta x, y), flags copied.  conv (radix-29
    form): the slot holds mont29(v, R29^2), as k_convert_points leaves it, or the canonical v R29 mod p."""

    def __init__(self, curve, in29, cases):
        super().__init__(curve, cases)
        self.in29 = in29
        # the 32-bit form copies whole slots, padding and all; store_pt29 writes its own words only
        self.slots = (("dst", True),) if in29 else ()

    def src_slot(self, P, conv):
        K = self.K
        if not self.in29:
            return K.slot32(P)
        x, y = P or (0, 0)
        return K.slot29(*((K.conv29(x), K.conv29(y)) if conv else (K.M.to_m(x), K.M.to_m(y))))

    def call(self, probe, per_elem):
        src = [w for P, _, conv in self.cases for w in self.src_slot(P, conv)]
        return probe.endo_points(self.curve, self.in29, src, bytes(inf for _, inf, _ in self.cases), per_elem)

    def verdicts(self, out):
        K, bad = self.K, []
        for i, (P, inf, _) in enumerate(self.cases):
            if int(out["dst_inf"][i]) != inf:
                bad.append((i, "flag %d, want %d (copied)" % (out["dst_inf"][i], inf)))
            w, Q = self.slot(out["dst"], i), glv.phi(self.curve, P)
            if self.in29:
                msg = K.check_slot29(w, Q, K.qin, "image")
            else:
                msg = None if w[:2 * K.W] == K.slot32(Q)[:2 * K.W] else "holds %s, want %s" % (hexs(w[:2 * K.W]), Q and hexs(Q))
            if msg:
                bad.append((i, msg))
        return bad

    def expected(self, per_elem, poison=0xA5):
        K, pw, dst = self.K, poison * 0x01010101, []
        for P, _, _ in self.cases:
            Q = glv.phi(self.curve, P)
            dst += K.slot29(*(K.conv29(v) for v in (Q or (0, 0))), pad=pw) if self.in29 else K.slot32(Q, pw)
        return dict(dst=dst, dst_inf=[inf for _, inf, _ in self.cases],
                    guards={"in": True, "in_inf": True, "pts": True, "inf": True})


def endo_stage(curve, in29):
    K, rng = curve_of(curve), _rng(curve + " endo")
    pts = K.specials() + K.M.point_pool(rng, 24)
    cases = [(P, 0, c) for P in pts for c in (True, False)][:(2 * len(pts) if in29 else len(pts))]
    cases += [(None, 1, True), (pts[0], 1, True)]            # zeros under the flag; a flagged finite slot
    assert all(P is None or pc.g1_on_curve(glv.phi(curve, P), K.C) for P, _, _ in cases)
    return EndoPoints(curve, in29, cases)


class ConvertScalars(Stage):
    def __init__(self, curve, cases=None):
        r = pc.CURVES[curve].r
        rng = _rng(curve + " scalars")
        super().__init__(curve, cases or [0, 1, r - 1, r, r + 1, (1 << 256) - 1, 1 << 255, (1 << 255) - 1, r - 2,
                                          (1 << 32) - 1, 1 << 224] + [rng.randrange(r) for _ in range(16)]
                         + [rng.randrange(r, 1 << 256) for _ in range(4)])
        self.err_codes = [DERR_SCALAR if k >= r else 0 for k in self.cases]
        self.want = [F.to_words(k if k < r else 0, 8) for k in self.cases]    # a rejected scalar is stored as zero

    def call(self, probe, per_elem):
        return probe.convert_scalars(self.curve, b"".join(pk.fr_to_bytes(k) for k in self.cases), self.n, per_elem)

    def verdicts(self, out):
        return [(i, "k = %#x: stored %s, want %s" % (self.cases[i], hexs([int(x) for x in out["out"][8 * i:8 * i + 8]]), hexs(w)))
                for i, w in enumerate(self.want) if [int(x) for x in out["out"][8 * i:8 * i + 8]] != w]

    def expected(self, per_elem, poison=0xA5):
        return dict(out=[w for s in self.want for w in s], err=self.err_codes if per_elem else [max(self.err_codes)],
                    guards={"in": True, "out": True, "err": True})


class EncodePoints(Stage):
    """cases: (point or None, lam): lambda-scaled XYZZ records against pk.g1_to_bytes."""

    def __init__(self, curve, cases=None):
        K, rng = curve_of(curve), _rng(curve + " encode")
        if cases is None:
            cases = [(None, 1), (None, 3)]
            cases += [(P, l) for P in K.specials() + K.M.point_pool(rng, 6) for l in K.lams(rng)]
        super().__init__(curve, cases)
        self.want = [pk.g1_to_bytes(P, K.C) for P, _ in cases]

    def call(self, probe, per_elem):
        return probe.encode_points(self.curve, [w for c in self.cases for w in self.K.xyzzw(*c)], self.n, per_elem)

    def verdicts(self, out):
        n, got = 2 * self.K.nb, bytes(bytearray(int(b) for b in out["out"]))
        return [(i, "got %s, want %s" % (got[i * n:(i + 1) * n].hex(), w.hex()))
                for i, w in enumerate(self.want) if got[i * n:(i + 1) * n] != w]

    def expected(self, per_elem, poison=0xA5):
        return dict(out=list(b"".join(self.want)), guards={"in": True, "out": True})


# (stage id, per_elem) -> Stage.  "each": one launch per case with its own error word; "single": one
# launch over at least N_SINGLE cases (the per-element list repeated), which tests the indexing
STAGE_NAMES = (["convert_points32", "convert_points29", "convert_points29_img", "decompress_points", "compress_points",
                "glv_split8", "glv_split12", "endo_points32", "endo_points29", "convert_scalars", "encode_points"])


def all_stage_ids():
    ids = []
    for c in CURVES:
        for s in STAGE_NAMES:
            ids += [(c, s, "each"), (c, s, "single")]
        ids.append((c, "subgroup_check", "each"))
        ids += [(c, "subgroup_check", "single%d" % q) for q in SINGLE_POSITIONS] if c == "bls12_381" else []
    return ids


def _build_stage(curve, name, mode):
    each = mode == "each"
    rep = (lambda cs: cs) if each else (lambda cs: cycle(cs, N_SINGLE))
    if name.startswith("convert_points"):
        form = {"convert_points32": 0, "convert_points29": 1, "convert_points29_img": 2}[name]
        return ConvertPoints(curve, form, rep(uncompressed_cases(curve)))
    if name == "decompress_points":
        return DecompressPoints(curve, rep(compressed_cases(curve)))
    if name == "compress_points":
        return CompressPoints(curve, rep(compress_cases(curve)))
    if name == "subgroup_check":
        return subgroup_stage(curve, None if each else int(mode[6:]))
    if name.startswith("glv_split"):
        ks = glv_scalars(curve)
        return GlvSplit(curve, int(name[9:]), ks[:N_EACH_MAX] if each else ks)
    if name.startswith("endo_points"):
        st = endo_stage(curve, int(name == "endo_points29"))
        return st if each else EndoPoints(curve, st.in29, cycle(st.cases, N_SINGLE))
    if name == "convert_scalars":
        return ConvertScalars(curve) if each else ConvertScalars(curve, cycle(ConvertScalars(curve).cases, N_SINGLE))
    if name == "encode_points":
        return EncodePoints(curve) if each else EncodePoints(curve, cycle(EncodePoints(curve).cases, N_SINGLE))
    raise KeyError(name)


def stage_of(curve, name, mode):
    key = (curve, name, mode)
    if key not in _cache:
        st = _build_stage(curve, name, mode)
        assert mode != "each" or st.n <= N_EACH_MAX, (name, st.n)
        assert mode == "each" or st.n >= N_SINGLE
        _cache[key] = st
    return _cache[key]
