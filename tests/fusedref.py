"""Limb-level model and operand generator of the fused product-and-subtract forms of
csrc/field29.hpp -- mulsub29(a, b, x, B) = a b / R29 + B - x and sqrsub3_29(a, s, t, C) =
a^2 / R29 + C - s - 2t -- for tests/test_field29_fused_cpu.py and tests/test_gpu_field29_fused.py.

The model is plain product scanning in radix 2^29 with one 64-bit column accumulator, written
from the algorithm and not from the device code: low column K takes the limb products, the m p
terms of the m already known, m_K = acc (-p^-1) mod 2^29, and m_K p_0; high column K takes the
limb products, the m p terms and (fused forms only) the 32-bit addend B[K - N] - x[K - N], then
gives result limb K - N = acc mod 2^29.  The top limb is what is left, plus the top limbs' term
in 32-bit wrap-around arithmetic.  Every column is asserted below 2^64 and every addend in
[0, 2^32).  The two-pass compositions the fused forms replace -- sub29(mont29(a, b), x, B) and
sub3_29(sqr29(a), s, t, C) -- are modelled pass by pass in 32-bit arithmetic beside them.

The sites are the call sites of msm.hpp (acc_loop29 and x29_add), each with the bias it names and
the input bounds tools/gen_params29.py check_bounds gives its operands.
"""
import random
from fractions import Fraction

import fieldref as F

M29, M32 = F.M29, 0xFFFFFFFF
NEDGE_RANDOM = 300   # seeded random cases of the CPU comparison
NRANDOM = F.NRANDOM  # and of the GPU probe, as the existing field tests


class Fused29:
    def __init__(self, curve):
        self.curve = curve
        self.m = m = F.layer("f29", curve)
        self.p, self.N, self.H = m.p, m.N, m.H
        self.peak = 0  # largest column sum seen

    # ------------------------------------------------------------------ product scanning
    def scan(self, a, b, square=False, addend=None, top=0):
        """(a b + m p) / R29 limb by limb (a, b limb lists; square: a^2 with the off-diagonal
        products taken once against the pre-doubled operand, as sqr29 does); addend(i) joins high
        column N + i, `top` the top limb (mod 2^32)."""
        n, mod, inv = self.N, self.H["MOD"], self.H["INV"]
        a2 = [(2 * v) & M32 for v in a]
        m, t, acc = [0] * n, [0] * n, 0
        for K in range(2 * n - 1):
            lo, hi = max(0, K - n + 1), min(K, n - 1)
            if square:
                acc += sum(a2[i] * a[K - i] for i in range(lo, hi + 1) if i < K - i)
                if K % 2 == 0:
                    acc += a[K // 2] * a[K // 2]
            else:
                acc += sum(a[i] * b[K - i] for i in range(lo, hi + 1))
            if K < n:
                acc += sum(m[i] * mod[K - i] for i in range(K))
                m[K] = (((acc & M32) * inv) & M32) & M29
                acc += m[K] * mod[0]
                assert acc & M29 == 0
            else:
                acc += sum(m[i] * mod[K - i] for i in range(lo, n))
                if addend is not None:
                    e = addend(K - n)
                    assert 0 <= e <= M32, "addend of limb %d is negative or too wide: %d" % (K - n, e)
                    acc += e
                t[K - n] = acc & M29
            assert acc < 1 << 64, "column %d overflows" % K
            self.peak = max(self.peak, acc)
            acc >>= 29
        t[n - 1] = (acc + top) & M32
        return t

    def sub29(self, a, x, B):
        """sub29's carry pass: a + B - x in 32-bit words."""
        r, c = [], 0
        for i in range(self.N):
            v = (a[i] + B[i] + c - x[i]) & M32
            assert a[i] + B[i] + c - x[i] >= 0 or i == self.N - 1
            r.append(v & M29 if i < self.N - 1 else v)
            c = v >> 29
        return r

    def sub3_29(self, a, s, t, C):
        r, c = [], 0
        for i in range(self.N):
            v = ((a[i] + C[i] + c) - (s[i] + 2 * t[i])) & M32
            r.append(v & M29 if i < self.N - 1 else v)
            c = v >> 29
        return r

    # ------------------------------------------------------------------ the ops, on integers
    def L(self, v):
        return F.limbs29(v, self.N)

    def mulsub_fused(self, bias, a, b, x):
        B, xl, n = self.H[bias], self.L(x), self.N
        return self.scan(self.L(a), self.L(b), addend=lambda i: B[i] - xl[i], top=B[n - 1] - xl[n - 1])

    def mulsub_two_pass(self, bias, a, b, x):
        return self.sub29(self.scan(self.L(a), self.L(b)), self.L(x), self.H[bias])

    def sqrsub3_fused(self, bias, a, s, t):
        C, sl, tl, n = self.H[bias], self.L(s), self.L(t), self.N
        return self.scan(self.L(a), None, square=True, addend=lambda i: C[i] - sl[i] - 2 * tl[i],
                         top=C[n - 1] - sl[n - 1] - 2 * tl[n - 1])

    def sqrsub3_two_pass(self, bias, a, s, t):
        return self.sub3_29(self.scan(self.L(a), None, square=True), self.L(s), self.L(t), self.H[bias])

    def value(self, kind, bias, case):
        """The integer the op returns: the Montgomery product plus the bias minus the subtrahend."""
        k = F.value29(self.H[bias])
        assert k % self.p == 0
        if kind == "mulsub":
            a, b, x = case
            return self.m.mont(a, b) + k - x
        a, s, t = case
        return self.m.mont(a, a) + k - s - 2 * t

    # ------------------------------------------------------------------ call sites and operands
    def sites(self):
        """name -> (kind, bias constant, bounds of the three operands in units of p).  The
        subtrahend of a mulsub site goes up to its bias (sub29's precondition), the others to
        the bounds check_bounds walks through."""
        m, B, rec = self.m, self.m.bounds, self.m.rec
        ro = {k: Fraction(v) for k, v in m.roles.items()}
        q2 = B["acc_D"] - ro["ACC_QX"]                      # Q2 of the loop
        u1, s1 = m.mont_bound(rec["x"], rec["z"]), m.mont_bound(rec["y"], rec["z"])
        P, R = u1 + 2, s1 + 2                                # x29_add's P and R (bias B2)
        PP = m.mont_bound(P, P)
        assert ro["ACC_X3"] >= B["acc_PPP"] + 2 * q2 and 8 >= m.mont_bound(P, PP) + 2 * m.mont_bound(u1, PP)
        return {
            "mulsub_ACC_P": ("mulsub", "ACC_P", (B["qin"], B["Z"], ro["ACC_P"])),
            "mulsub_ACC_R": ("mulsub", "ACC_R", (ro["ACC_NEG"], B["Z"], ro["ACC_R"])),
            "mulsub_B2": ("mulsub", "B2", (Fraction(rec["y"]), Fraction(rec["z"]), Fraction(2))),
            "sqrsub3_ACC_X3": ("sqrsub3", "ACC_X3", (B["acc_R"], B["acc_PPP"], q2)),
            "sqrsub3_C8": ("sqrsub3", "C8", (R, m.mont_bound(P, PP), m.mont_bound(u1, PP))),
        }

    def cases(self, site, nrandom):
        """Edge families of every operand (k p and k p +- 1 up to the bound, bound - 1, all-ones
        lower limbs, alternating limbs, 0 and 1 -- F.Mod29.family), each pair of operands in full
        with the third cycling through its own family, then seeded random cases."""
        kind, bias, bounds = self.sites()[site]
        m = self.m
        rng = random.Random("%d fused %s %s" % (F.SEED, self.curve, site))
        fam = [m.family(k) for k in bounds]
        out = []
        for i, j, k in ((0, 2, 1), (1, 2, 0), (0, 1, 2)):
            n = 0
            for u in fam[i]:
                for v in fam[j]:
                    c = [0, 0, 0]
                    c[i], c[j], c[k] = u, v, fam[k][n % len(fam[k])]
                    n += 1
                    out.append(tuple(c))
        out += [tuple(m.rand_below(rng, k) for k in bounds) for _ in range(nrandom)]
        out = F.dedupe(out)
        for c in out:  # preconditions: every operand within its bound, the result not negative
            assert all(v < k * self.p for v, k in zip(c, bounds))
            assert self.value(kind, bias, c) >= 0
        return kind, bias, out

    def fused(self, kind, bias, case):
        return (self.mulsub_fused if kind == "mulsub" else self.sqrsub3_fused)(bias, *case)

    def two_pass(self, kind, bias, case):
        return (self.mulsub_two_pass if kind == "mulsub" else self.sqrsub3_two_pass)(bias, *case)


SITES = ["mulsub_ACC_P", "mulsub_ACC_R", "mulsub_B2", "sqrsub3_ACC_X3", "sqrsub3_C8"]
_cache = {}


def model(curve):
    if curve not in _cache:
        _cache[curve] = Fused29(curve)
    return _cache[curve]
