"""Limb-level model of what the row accumulation's hot loop (csrc/msm.hpp acc_row29) does to a
negated entry's y, for tests/test_row_arith_cpu.py: q.y enters R = q.y ZZZ - y as ACC_NEG - q.y
limb by limb with no carry pass (field29.hpp neg_lazy29), where the chunk loop and the row loop's
prologue hand the product sub29's normalised form.  The product scan is tests/fusedref.py's (every
column asserted below 2^64); the subtraction is fused into it where the curve fuses it
(csrc/msm.hpp kFusedSub: BLS12-381) and a sub29 pass behind it where not (BN254).

And of an item's first addition in both forms: the loop's generic body on ZZ = ZZZ = ONE, and the peel
in front of the loop (csrc/msm.hpp kPeelFirst: BLS12-381) with its guards (field29.hpp peel_ok29)."""
from fractions import Fraction

import fieldref as F
import fusedref as FR

M29 = F.M29
FUSED_SUB = {"bls12_381": True, "bn254": False}   # csrc/msm.hpp kFusedSub


class RowArith:
    def __init__(self, curve):
        self.curve = curve
        self.f = FR.model(curve)
        self.m = self.f.m
        self.p, self.N, self.H = self.m.p, self.m.N, self.m.H
        self.kneg, self.kr = self.m.bias("ACC_NEG"), self.m.bias("ACC_R")

    # ------------------------------------------------------------------ the forms of -q.y
    def neg_normalised(self, qy):
        """sub29(zero, q.y, ACC_NEG): the limbs of ACC_NEG p - q.y"""
        return self.f.sub29([0] * self.N, self.f.L(qy), self.H["ACC_NEG"])

    def neg_lazy(self, qy):
        """neg_lazy29(q.y, ACC_NEG): limb by limb, nothing may go negative"""
        out = [b - l for b, l in zip(self.H["ACC_NEG"], self.f.L(qy))]
        assert all(0 <= v < 1 << 30 for v in out), "a lazy limb left [0, 2^30)"
        return out

    def norm(self, limbs):
        """norm29: the carry pass on its own"""
        r, c = [], 0
        for i, v in enumerate(limbs):
            x = v + c
            assert x < 1 << 32
            r.append(x & M29 if i < self.N - 1 else x)
            c = x >> 29
        return r

    # ------------------------------------------------------------------ R = q.y' ZZZ - y
    def r_of(self, qy_limbs, zzz, y):
        """The words of R from an operand given as limbs (normalised or lazy)."""
        B, yl, n = self.H["ACC_R"], self.f.L(y), self.N
        if FUSED_SUB[self.curve]:
            return self.f.scan(qy_limbs, self.f.L(zzz), addend=lambda i: B[i] - yl[i], top=B[n - 1] - yl[n - 1])
        return self.f.sub29(self.f.scan(qy_limbs, self.f.L(zzz)), yl, B)

    def check_site(self, qy, zzz, y, fault=None):
        """None, or what differs: the lazy operand's R against the normalised operand's and against
        the integer mont((ACC_NEG p - q.y), ZZZ) + ACC_R p - y in its normal form; the restart's
        norm29 of the lazy form against sub29's words.  fault(limbs) plants an error in the lazy
        operand."""
        lazy, want_op = self.neg_lazy(qy), self.neg_normalised(qy)
        if fault:
            lazy = fault(list(lazy))
        if self.norm(lazy) != want_op:
            return "norm29 of the lazy form is not sub29's form"
        got, want = self.r_of(lazy, zzz, y), self.r_of(want_op, zzz, y)
        if got != want:
            return "lazy operand gives %s, normalised %s" % (got, want)
        integer = self.m.mont(self.kneg * self.p - qy, zzz) + self.kr * self.p - y
        if integer < 0 or got != F.limbs29(integer, self.N):
            return "not the normal form of the integer"
        return None

    # ------------------------------------------------------------------ operands
    def bounds(self):
        """(q.y, ZZZ, y) bounds in units of p: a point's y out of fp_to29, the loop's ZZZ, and the
        running sum's y up to its bias (sub29's precondition is y <= ACC_R p)."""
        B = self.m.bounds
        return B["qin"], B["Z"], Fraction(self.kr)

    def families(self):
        m, p, n = self.m, self.p, self.N
        kq, kz, ky = self.bounds()
        low = (1 << (29 * (n - 1))) - 1

        def ones(k):   # every lower limb 2^29 - 1 under the largest top limb the bound admits
            top = m.below(k)
            v = ((top >> (29 * (n - 1))) << (29 * (n - 1))) | low
            return v if v <= top else v - (1 << (29 * (n - 1)))
        qys = F.dedupe([0, 1, p - 1, low, ones(kq), m.below(kq)] + m.family(kq))
        zs = F.dedupe([m.below(kz), ones(kz), low, 0, 1] + m.family(kz))
        ys = F.dedupe([self.kr * p, self.kr * p - 1, 0, low, ones(ky)] + m.family(ky))
        assert all(v < kq * p for v in qys) and all(v < kz * p for v in zs) and all(v <= ky * p for v in ys)
        return qys, zs, ys


    # ------------------------------------------------------------------ the item's first addition
    # Running sum (x, y, ZZ = ZZZ = ONE) + the second entry (q.x, q.y, sign), as limb lists.  The two
    # forms differ in P, R, ZZ3 and ZZZ3, which are modelled limb by limb; Q2, X3 and Y3 are the same
    # code on those in both, taken here from the integers (fieldref's mont) in their normal form.
    PEEL = {"bls12_381": True, "bn254": False}    # csrc/msm.hpp kPeelFirst

    def _tail(self, x, y, P, R, PP, PPP):
        m, p, n = self.m, self.p, self.N
        v = F.value29
        Q2 = m.mont(v(x), v(PP))
        X3 = m.mont(v(R), v(R)) + m.bias("ACC_X3") * p - v(PPP) - 2 * Q2
        D = Q2 + m.bias("ACC_QX") * p - X3
        assert X3 >= 0 and D >= 0 and m.bias("ACC_PPP") * p >= v(PPP)
        Y3 = m.mont(v(R), D, v(y), m.bias("ACC_PPP") * p - v(PPP))
        return F.limbs29(X3, n), F.limbs29(Y3, n)

    def zero29(self, a):
        return F.value29(a) % self.p == 0

    def first_generic(self, x, y, qx, qy, sign):
        """The loop body (acc_row29's hot loop) on ZZ = ZZZ = ONE -> ("sum", x3, y3, zz, zzz, P, R), ("inf",)
        or ("dbl",)."""
        f, H, n = self.f, self.H, self.N
        one, L = H["ONE"], f.L
        xl, yl = L(x), L(y)
        qyl = self.neg_lazy(qy) if sign else L(qy)
        BP = H["ACC_P"]
        if FUSED_SUB[self.curve]:
            P = f.scan(L(qx), one, addend=lambda i: BP[i] - xl[i], top=BP[n - 1] - xl[n - 1])
        else:
            P = f.sub29(f.scan(L(qx), one), xl, BP)
        R = self.r_of(qyl, F.value29(one), y)
        if self.zero29(P):
            return ("dbl",) if self.zero29(R) else ("inf",)
        PP = f.scan(P, None, square=True)
        PPP = f.scan(P, PP)
        zz, zzz = f.scan(one, PP), f.scan(one, PPP)
        return ("sum",) + self._tail(xl, yl, P, R, PP, PPP) + (zz, zzz, P, R)

    def peel_ok(self, l):
        """field29.hpp peel_ok29 on a limb list (32-bit words)"""
        n, mod = self.N, self.H["MOD"]
        t1, t0 = l[n - 1], l[n - 2]
        lo = t1 != 0 or t0 >= self.H["PEEL_LO"]
        hi = t1 < mod[n - 1] or (t1 == mod[n - 1] and t0 < mod[n - 2])
        return lo and hi

    def canon(self, l):
        v = F.value29(l)
        assert v < 2 * self.p, "canon29's range"
        return F.limbs29(v % self.p, self.N)

    def first_peeled(self, x, y, qx, qy, sign):
        """The peel -> ("sum", ...) or ("fallback", which guard), guards in the kernel's order."""
        f, H, n = self.f, self.H, self.N
        L, M32 = f.L, 0xFFFFFFFF
        xl, yl, qxl = L(x), L(y), L(qx)
        if sign:      # sub29(0, q.y, B1) in 32-bit words: wraps for q.y > p
            S2, c = [], 0
            for i, (b, l) in enumerate(zip(H["B1"], L(qy))):
                w = (b + c - l) & M32
                S2.append(w & M29 if i < n - 1 else w)
                c = w >> 29 if i < n - 1 else 0
        else:
            S2 = L(qy)
        if not self.peel_ok(qxl):
            return ("fallback", "q.x")
        if not self.peel_ok(S2):
            return ("fallback", "S2")
        P = f.sub29(qxl, xl, H["ACC_P"])
        R = f.sub29(S2, yl, H["ACC_R"])
        if self.zero29(P):
            return ("fallback", "P = 0")
        PP = f.scan(P, None, square=True)
        PPP = f.scan(P, PP)
        zz, zzz = self.canon(PP), self.canon(PPP)
        if not self.peel_ok(zz):
            return ("fallback", "PP")
        if not self.peel_ok(zzz):
            return ("fallback", "PPP")
        return ("sum",) + self._tail(xl, yl, P, R, PP, PPP) + (zz, zzz, P, R)

    def check_first(self, x, y, qx, qy, sign, fault=None):
        """-> (None or what differs, the peel's outcome).  Where the peel does not fall back its
        words are the generic body's; where it does, the generic body has an outcome of its own."""
        g, q = self.first_generic(x, y, qx, qy, sign), self.first_peeled(x, y, qx, qy, sign)
        if fault and q[0] == "sum":
            q = fault(q)
        if q[0] == "fallback":
            return (None if g[0] in ("sum", "inf", "dbl") else "generic body: %r" % (g,)), q
        return (None if q == g else "peel %s, generic %s" % (q, g)), q

    def threshold(self):
        """The least integer whose two top limbs reach PEEL_LO, and p's two top limbs as an integer."""
        s = 29 * (self.N - 2)
        return self.H["PEEL_LO"] << s, (self.p >> s) << s


_cache = {}


def model(curve):
    if curve not in _cache:
        _cache[curve] = RowArith(curve)
    return _cache[curve]
