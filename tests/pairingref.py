"""Plain big-integer reference of the pairing interpreter's ops (csrc/pairing_par.hpp running the
tables of csrc/bilinear_gen.hpp) and the operand families their probe tests run
(tests/test_gpu_pairing.py on the GPU, tests/test_pairingref_cpu.py without).

The reference is Fp2 / Fp6 / Fp12 arithmetic written out here on top of oracle/pyspec (flat
f12_mul, flat_to_tower and its inverse); it never reads the generated tables or
gen_bilinear.evaluate, which are what is under test.  Elements are lists of Fp integers in the
tower coefficient order of the register file: c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each
(re, im).

Registers hold x R with R = 2^(29 N): a row of integer value v stands for v R^-1 mod p.  A round
output must be congruent to op(...) R, lie within the bound tests/fieldref.py holds lp_reduce to
(|v| < 0.51 p) and have limbs within LP_OUT_LO / LP_OUT_HI with the lanes above N zero.  A K_COPY
block is the same limbs, a K_INV result an lp_mul output (|v| < 1.5 p), 0 -> 0; CONJ outputs pass
through lp_reduce like every round output.

Operand rows satisfy |v| < 1.5 p, the lp_mul output bound: the widest class the shipped programs
feed to any operand (K, E, P and the K_INV result; round outputs are below 0.51 p).
"""
import os
import random

import numpy as np

import fieldref as F
from oracle.pyspec import curves as pc
from oracle.pyspec.pairing import f12_mul, f12_pow, flat_to_tower

G = F._load(os.path.join(F.PKG, "tools", "gen_bilinear.py"), "gen_bilinear")
OP_NAMES = [name for name, _ in G.OPS]
NRANDOM = 256
NSIGNS = 64
W_ORDER = [0, 2, 4, 1, 3, 5]  # tower slot j (an Fp2) is the coefficient of w^W_ORDER[j]
# (rows read from A, rows read from B, rows written) of each op, from its definition
SHAPES = {"MUL": (12, 12, 12), "SQR": (12, 0, 12), "CYC": (12, 0, 12), "CONJ": (12, 0, 12), "LINE": (12, 6, 12),
          "LL": (6, 6, 12), "FROB1": (12, 0, 12), "FROB2": (12, 0, 12), "FROB3": (12, 0, 12), "INV_NORM": (12, 0, 6),
          "INV6_T": (6, 0, 6), "INV6_D": (6, 6, 2), "INV2_N": (2, 0, 1), "INV2_FIN": (2, 1, 2), "INV6_FIN": (6, 2, 6),
          "INV12_FIN": (12, 6, 12), "LEVAL": (4, 3, 6)}


def tower_to_flat(t, C):
    """Inverse of flat_to_tower: the w^k coefficient (x, y) gives f[k] = x - beta y, f[k + 6] = y."""
    f = [0] * 12
    for j, k in enumerate(W_ORDER):
        x, y = t[2 * j], t[2 * j + 1]
        f[k + 6] = y % C.p
        f[k] = (x - C.beta * y) % C.p
    return f


class TowerRef:
    """Fp2 / Fp6 / Fp12 over one curve, elements as described in the module docstring."""

    def __init__(self, curve):
        self.curve, self.C = curve, pc.CURVES[curve]
        self.p, self.xi = self.C.p, self.C.xi
        self._gamma = {}

    # ---- Fp2 (u^2 = -1), tuples
    def add(self, a, b): return pc.fp2_add(a, b, self.p)
    def sub(self, a, b): return pc.fp2_sub(a, b, self.p)
    def neg(self, a): return pc.fp2_neg(a, self.p)
    def mul(self, a, b): return pc.fp2_mul(a, b, self.p)
    def mxi(self, a): return pc.fp2_mul(a, self.xi, self.p)
    def conj2(self, a): return (a[0] % self.p, -a[1] % self.p)
    def smul(self, a, k): return (a[0] * k % self.p, a[1] * k % self.p)

    def pow2(self, a, e):
        r = (1, 0)
        for bit in bin(e)[2:]:
            r = self.mul(r, r)
            if bit == "1":
                r = self.mul(r, a)
        return r

    @staticmethod
    def f2s(t):
        return [(t[2 * k], t[2 * k + 1]) for k in range(len(t) // 2)]

    @staticmethod
    def flat(f2s):
        return [v for x in f2s for v in x]

    # ---- Fp6 = Fp2[v] / (v^3 - xi), lists of three Fp2
    def mul6(self, a, b):
        m, ad = self.mul, self.add
        return [ad(m(a[0], b[0]), self.mxi(ad(m(a[1], b[2]), m(a[2], b[1])))),
                ad(ad(m(a[0], b[1]), m(a[1], b[0])), self.mxi(m(a[2], b[2]))),
                ad(ad(m(a[0], b[2]), m(a[1], b[1])), m(a[2], b[0]))]

    def mulv6(self, a):
        return [self.mxi(a[2]), a[0], a[1]]

    # ---- Fp12 through the pyspec's flat representation
    def f12mul(self, a, b):
        C = self.C
        return flat_to_tower(f12_mul(tower_to_flat(a, C), tower_to_flat(b, C), C), C)

    def f12pow(self, a, e):
        C = self.C
        return flat_to_tower(f12_pow(tower_to_flat(a, C), e, C), C)

    def one(self):
        return [1] + [0] * 11

    def line_full(self, l):
        """The sparse line (a, b, c) as an Fp12: M-type a + b w^2 + c w^3 (BLS12-381), D-type
        a + b w + c w^3 (BN254)."""
        a, b, c = self.f2s(l)
        slots = [(0, 0)] * 6
        slots[0] = a
        slots[W_ORDER.index(2 if self.C.twist == "M" else 1)] = b
        slots[W_ORDER.index(3)] = c
        return self.flat(slots)

    def gamma(self, k, i):
        """xi^(i (p^k - 1) / 6): w^i to the power p^k is gamma w^i."""
        if (k, i) not in self._gamma:
            self._gamma[(k, i)] = self.pow2(self.xi, i * (self.p ** k - 1) // 6)
        return self._gamma[(k, i)]

    # ---- the ops
    def op(self, name, A, B=None):
        p = self.p
        s2, fl = self.f2s, self.flat
        if name == "MUL":
            return self.f12mul(A, B)
        if name == "SQR":
            return self.f12mul(A, A)
        if name == "CYC":
            return self.cyc(A)
        if name == "CONJ":
            return [v % p for v in A[:6]] + [-v % p for v in A[6:]]
        if name == "LINE":
            return self.f12mul(A, self.line_full(B))
        if name == "LL":
            return self.f12mul(self.line_full(A), self.line_full(B))
        if name.startswith("FROB"):
            k = int(name[4])
            out = []
            for j, c in enumerate(s2(A)):
                y = self.conj2(c) if k & 1 else c
                out.append(self.mul(y, self.gamma(k, W_ORDER[j])))
            return fl(out)
        if name == "INV_NORM":   # f -> c0^2 - v c1^2
            c0, c1 = s2(A[:6]), s2(A[6:])
            t0, t1 = self.mul6(c0, c0), self.mulv6(self.mul6(c1, c1))
            return fl([self.sub(x, y) for x, y in zip(t0, t1)])
        if name == "INV6_T":     # a -> (a0^2 - xi a1 a2, xi a2^2 - a0 a1, a1^2 - a0 a2)
            a = s2(A)
            m = self.mul
            return fl([self.sub(m(a[0], a[0]), self.mxi(m(a[1], a[2]))),
                       self.sub(self.mxi(m(a[2], a[2])), m(a[0], a[1])),
                       self.sub(m(a[1], a[1]), m(a[0], a[2]))])
        if name == "INV6_D":     # a, t -> a0 t0 + xi (a2 t1 + a1 t2)
            a, t = s2(A), s2(B)
            m = self.mul
            return fl([self.add(m(a[0], t[0]), self.mxi(self.add(m(a[2], t[1]), m(a[1], t[2]))))])
        if name == "INV2_N":     # d -> d0^2 + d1^2
            return [(A[0] * A[0] + A[1] * A[1]) % p]
        if name == "INV2_FIN":   # d, ninv -> (d0 ninv, -d1 ninv)
            return [A[0] * B[0] % p, -A[1] * B[0] % p]
        if name == "INV6_FIN":   # t, dinv -> t dinv
            di = (B[0], B[1])
            return fl([self.mul(x, di) for x in s2(A)])
        if name == "INV12_FIN":  # f, tinv -> (c0 tinv, -c1 tinv)
            c0, c1, ti = s2(A[:6]), s2(A[6:]), s2(B)
            return fl(self.mul6(c0, ti) + [self.neg(x) for x in self.mul6(c1, ti)])
        if name == "LEVAL":      # (c, lam), (X, Y, Z) -> M-type (c Z, lam X, -Y), D-type (-Y, lam X, c Z)
            c, lam = s2(A)
            X, Y, Z = B
            parts = [self.smul(c, Z), self.smul(lam, X), (-Y % p, 0)]
            return fl(parts if self.C.twist == "M" else parts[::-1])
        raise KeyError(name)

    def cyc(self, A):
        """Granger-Scott squaring of the compressed-squaring form, for any input: with the Fp4
        squaring (a, b) -> (a^2 + xi b^2, 2 a b) of the pairs (z0, z1) = (c0.c0, c1.c1),
        (z2, z3) = (c1.c0, c0.c2), (z4, z5) = (c0.c1, c1.c2)."""
        c = self.f2s(A)
        z0, z4, z3, z2, z1, z5 = c
        m, ad = self.mul, self.add

        def sq4(a, b):
            return ad(m(a, a), self.mxi(m(b, b))), self.smul(m(a, b), 2)
        t0, t1 = sq4(z0, z1)
        t2, t3 = sq4(z2, z3)
        t4, t5 = sq4(z4, z5)
        tri = lambda t, z, s: ad(self.smul(t, 3), self.smul(z, 2 * s))  # noqa: E731  3 t +- 2 z
        r00, r01, r02 = tri(t0, z0, -1), tri(t2, z4, -1), tri(t4, z3, -1)
        r10, r11, r12 = tri(self.mxi(t5), z2, 1), tri(t1, z1, 1), tri(t3, z5, 1)
        return self.flat([r00, r01, r02, r10, r11, r12])

    def inverse(self, f):
        """f^-1 by the seven stages and one Fp inversion (0 -> 0), with every stage's value."""
        st = {}
        st["INV_NORM"] = self.op("INV_NORM", f)
        st["INV6_T"] = self.op("INV6_T", st["INV_NORM"])
        st["INV6_D"] = self.op("INV6_D", st["INV_NORM"], st["INV6_T"])
        st["INV2_N"] = self.op("INV2_N", st["INV6_D"])
        st["K_INV"] = [pow(st["INV2_N"][0], -1, self.p) if st["INV2_N"][0] else 0]
        st["INV2_FIN"] = self.op("INV2_FIN", st["INV6_D"], st["K_INV"])
        st["INV6_FIN"] = self.op("INV6_FIN", st["INV6_T"], st["INV2_FIN"])
        st["INV12_FIN"] = self.op("INV12_FIN", f, st["INV6_FIN"])
        return st

    def cyclotomic(self, f):
        """f^((p^6 - 1)(p^2 + 1)): conj(f) / f, then times its p^2 power."""
        g = self.f12mul(self.op("CONJ", f), self.inverse(f)["INV12_FIN"])
        return self.f12mul(self.op("FROB2", g), g)


class PairRef:
    """Rows, families and output checks of one curve."""

    def __init__(self, curve):
        self.curve = curve
        self.lp = F.layer("lp", curve)
        self.T = TowerRef(curve)
        self.p, self.N, self.R = self.lp.p, self.lp.N, self.lp.R
        self.Rinv = pow(self.R, -1, self.p)
        self.b_red = (51 * self.p - 1) // 100 + 1   # lp_reduce: 100 |v| < 51 p  <=>  |v| < b_red
        self.b_mul = (3 * self.p - 1) // 2 + 1      # lp_mul:    2 |v| < 3 p     <=>  |v| < b_mul
        self._fam = {}

    # ---- rows and values
    def elem(self, v):
        """The field element a row of integer value v stands for."""
        return v * self.Rinv % self.p

    def mont(self, x):
        return x * self.R % self.p

    def values(self, rows):
        return [self.lp.value([int(v) for v in l]) for l in rows]

    def check_operand_row(self, l):
        assert len(l) == 16 and not any(l[self.N:]) and all(abs(v) <= F.LP_LIMB_MAX for v in l), l
        assert abs(self.lp.value(l)) < self.b_mul, "operand row not below 1.5 p"
        return l

    def edge_values(self):
        p, top = self.p, 1 << (F.W29 * (self.N - 1))
        v = [0, 1, -1, p, -p, p + 1, p - 1, -p + 1, -p - 1, self.b_red - 1, 1 - self.b_red, self.b_mul - 1,
             1 - self.b_mul, top, -top]
        return [x for x in v if abs(x) < self.b_mul]  # BN254: 2^(29 (N - 1)) is ~169 p, outside every operand class

    def clipped_edge_rows(self, rng):
        """ModLp.edge_rows within the operand bound, and the all-limbs-at-maximum rows cut to the
        longest run of maximal limbs that stays below 1.5 p."""
        rows = [l for l in self.lp.edge_rows(rng) if abs(self.lp.value(l)) < self.b_mul]
        for s in (1, -1):
            for alt in (False, True):
                k = self.N - 1
                while True:
                    l = [s * F.LP_LIMB_MAX * ((-1) ** i if alt else 1) for i in range(k)] + [0] * (16 - k)
                    if abs(self.lp.value(l)) < self.b_mul:
                        break
                    k -= 1
                rows.append(l)
        return F.dedupe(rows)

    # ---- operand families: a case is (rows of A, rows of B)
    def family(self, name):
        if name in self._fam:
            return self._fam[name]
        wa, wb, _ = SHAPES[name]
        n, lp, p = wa + wb, self.lp, self.p
        rng = random.Random("%d pairing %s %s" % (F.SEED, self.curve, name))
        rv = lambda: rng.randrange(1 - self.b_mul, self.b_mul)  # noqa: E731
        plain = []  # lists of n integer values
        ev = self.edge_values()
        for i in range(n):                       # every coefficient in turn, the others random
            for v in ev:
                c = [rv() for _ in range(n)]
                c[i] = v
                plain.append(c)
        plain += [[v] * n for v in ev]           # all coefficients together
        one = self.R % p

        def unit(w, u):                          # u in the first coefficient of a w-wide operand
            return [u] + [0] * (w - 1) if w else []
        for ua, ub in ((one, one), (-one, -one), (one, -one), (0, 0), (one, None), (None, one), (-one, None),
                       (0, None), (None, 0)):
            a = unit(wa, ua) if ua is not None else [rv() for _ in range(wa)]
            b = unit(wb, ub) if ub is not None else [rv() for _ in range(wb)]
            plain.append(a + b)
        for k in (1, 2, 6):                      # Fp, Fp2, Fp6: the other coefficients zero
            for which in ("a", "b", "ab"):
                for _ in range(4):
                    a = [rv() if (i < k or "a" not in which) else 0 for i in range(wa)]
                    b = [rv() if (i < k or "b" not in which) else 0 for i in range(wb)]
                    plain.append(a + b)
        for _ in range(NSIGNS):                  # every coefficient at +- a bound
            plain.append([rng.choice((1, -1)) * (rng.choice((self.b_red, self.b_mul)) - 1) for _ in range(n)])
        cases = []
        for c in plain:
            rows = [lp.row(v) for v in c]
            cases.append(rows)
            cases.append([lp.jiggle(rng, l) for l in rows])
        er = self.clipped_edge_rows(rng)
        for k in range(len(er)):                 # each edge row in every position
            cases.append([er[(k + i) % len(er)] for i in range(n)])
        cyc = self.cyclotomic_values(NRANDOM // 2, rng) if name == "CYC" else []
        for k in range(NRANDOM):
            c = cyc[k // 2] if name == "CYC" and k % 2 else [rv() for _ in range(n)]
            rows = [lp.row(v) for v in c]
            cases.append([lp.jiggle(rng, l) for l in rows] if rng.randrange(2) else rows)
        for rows in cases:
            for l in rows:
                self.check_operand_row(l)
        self._fam[name] = [(rows[:wa], rows[wa:]) for rows in cases]
        return self._fam[name]

    def cyclotomic_values(self, count, rng):
        """Register values (x R + e p, e in {-1, 0}) of `count` elements of the cyclotomic subgroup:
        g, g^2, g^3, ... for g = f^((p^6 - 1)(p^2 + 1)), f random."""
        T, p = self.T, self.p
        g = T.cyclotomic([rng.randrange(p) for _ in range(12)])
        out, cur = [], g
        for _ in range(count):
            out.append([self.mont(x) - rng.randrange(2) * p for x in cur])
            cur = T.f12mul(cur, g)
        return out

    # ---- expectations
    def want(self, name, case):
        A, B = ([self.elem(v) for v in self.values(rows)] for rows in case)
        return self.T.op(name, A, B)

    def check_round_rows(self, rows, want):
        """rows: the output block as read back; want: field elements.  None or a message."""
        if len(rows) != len(want):
            return "%d rows for %d outputs" % (len(rows), len(want))
        for k, (l, w) in enumerate(zip(rows, want)):
            l = [int(v) for v in l]
            g = self.lp.value(l)
            if (g - w * self.R) % self.p:
                return "output %d not congruent to op(...) R: row %s" % (k, F.hexs(l))
            if not abs(g) < self.b_red:
                return "output %d: |v| = %.4f p, lp_reduce bound 0.51 p" % (k, abs(g) / self.p)
            err = self.lp.norm_ok(l)
            if err:
                return "output %d: %s" % (k, err)
        return None

    def check_inv_row(self, l, src_value):
        """K_INV: an lp_mul output congruent to x^-1 R for the source's x (0 -> 0)."""
        l = [int(v) for v in l]
        x = self.elem(src_value)
        w = pow(x, -1, self.p) if x else 0
        g = self.lp.value(l)
        if (g - w * self.R) % self.p:
            return "K_INV result not congruent to x^-1 R: row %s" % F.hexs(l)
        if not abs(g) < self.b_mul:
            return "K_INV: |v| = %.4f p, lp_mul bound 1.5 p" % (abs(g) / self.p)
        return self.lp.norm_ok(l)


_refs = {}


def ref(curve):
    if curve not in _refs:
        _refs[curve] = PairRef(curve)
    return _refs[curve]


# ---------------------------------------------------------------------------- programs and images
def new_prog(curve):
    return G.Prog(curve)


def images(prog, cases_rows):
    """cases_rows: per case a list of (first register row, rows).  int32 [n][NR - R_P][16]."""
    img = np.zeros((len(cases_rows), prog.NR - prog.R_P, 16), dtype=np.int32)
    for k, placements in enumerate(cases_rows):
        for reg, rows in placements:
            if rows:
                assert prog.R_P <= reg and reg + len(rows) <= prog.NR
                img[k, reg - prog.R_P:reg - prog.R_P + len(rows)] = np.array(rows, dtype=np.int64)
    return img


def untouched(prog, img_in, img_out, written):
    """None, or a message naming the first case whose rows outside the `written` (start, n) blocks changed."""
    keep = np.ones(img_in.shape[1], dtype=bool)
    for reg, n in written:
        keep[reg - prog.R_P:reg - prog.R_P + n] = False
    bad = np.nonzero((img_in[:, keep] != img_out[:, keep]).any(axis=(1, 2)))[0]
    return None if not len(bad) else "case %d: a register outside the output blocks changed" % bad[0]


# ---------------------------------------------------------------------------- bound walk
def parse_header_array(name):
    """A `static __constant__ ... NAME[n] = {...};` array of csrc/bilinear_gen.hpp as a list of ints."""
    import re
    with open(os.path.join(F.PKG, "csrc", "bilinear_gen.hpp")) as f:
        text = f.read()
    m = re.search(r"\b%s\[\d+\] = \{([^}]*)\};" % re.escape(name), text)
    return [int(x) for x in m.group(1).split(",")]


def header_info(curve):
    """{name: value} of the curve's OpsInfo struct in csrc/bilinear_gen.hpp."""
    import re
    with open(os.path.join(F.PKG, "csrc", "bilinear_gen.hpp")) as f:
        text = f.read()
    body = text[text.index("struct %sOpsInfo {" % {"bls12_381": "Bls", "bn254": "Bn"}[curve]):]
    body = body[:body.index("\n};")]
    return {k: int(v) for k, v in re.findall(r"(\w+) = (\d+)", body)}


def stated_output_bound():
    """k of the comment `|sum| < k * 1.5 p` above lp_terms_chunk in csrc/pairing_par.hpp."""
    import re
    with open(os.path.join(F.PKG, "csrc", "pairing_par.hpp")) as f:
        m = re.search(r"\|sum\| < (\d+) \* 1\.5 p", f.read())
    return int(m.group(1))


def shipped_program(curve):
    P, res = G.build_program(curve)
    G.compress_cyc_runs(P)
    return P, res


def op_tables(curve):
    return {name: G.build_op(fn, curve) for name, fn in G.OPS}


MUL, RED = "mul", "red"  # magnitude classes: |v| < 1.5 p (lp_mul outputs), |v| < 0.51 p (lp_reduce outputs)


def bound_walk(curve, code, tables, head=None, stated=None):
    """Dataflow over a program's bytecode: every register carries the magnitude class of what wrote
    it (K, E, P and the K_INV result: lp_mul outputs; round outputs: lp_reduce outputs; K_COPY
    keeps the class).  Asserts for every round that each factor form and each output sum is below
    2^HEAD p (lp_mul's and lp_reduce's tested domains), that each output sum is within the bound
    pairing_par.hpp states, that the per-lane 64-bit accumulators stay below 2^58 and that the top
    lane fits 32 bits.  Returns the largest sums met, in units of p."""
    r = ref(curve)
    lp, p, N = r.lp, r.p, r.N
    head = lp.HEAD if head is None else head
    stated = stated_output_bound() if stated is None else stated
    P = G.Prog(curve)
    bound = {MUL: r.b_mul, RED: r.b_red}
    cls = [None] * P.NR
    for i in list(range(P.R_K, P.R_K + 36)) + list(range(P.R_E, P.R_P + 6)):
        cls[i] = MUL
    limb = F.LP_LIMB_MAX
    top_unit = 1 << (F.W29 * (N - 1))
    worst = {"factor": 0, "output": 0}

    def form_bound(form, a, b, what):
        tot, ncoef = 0, 0
        for (src, i), c in form.items():
            if src == "P":
                bd = r.b_mul
            else:
                reg = {"A": a, "B": b, "K": P.R_K}[src]
                assert reg is not None and reg != G.NONE, "%s reads a missing operand" % what
                assert cls[reg + i] is not None, "%s reads register %d before it is written" % (what, reg + i)
                bd = bound[cls[reg + i]]
            tot += abs(c) * bd
            ncoef += abs(c)
        assert tot < (1 << head) * p, "%s: sum up to %.1f p, not below 2^%d p" % (what, tot / p, head)
        assert ncoef * limb < 1 << 58, "%s: a lane accumulator can reach 2^58" % what
        # top lane: its own limbs (a value below B with limbs within LP_OUT has a top limb below
        # B / 2^(29 (N - 1)) + 2) plus the carry of the lane below (at most ncoef + 1)
        assert tot // top_unit + 2 * ncoef + ncoef + 1 < 1 << 31, "%s: top lane does not fit 32 bits" % what
        return tot

    def round_(opn, a, b, o):
        name = OP_NAMES[opn]
        prods, outs = tables[name]
        for j, (L, R_) in enumerate(prods):
            for f in (L, R_):
                worst["factor"] = max(worst["factor"], form_bound(f, a, b, "%s product %d" % (name, j)))
        sums = [form_bound(out.d, a, b, "%s output %d" % (name, k)) for k, out in enumerate(outs)]
        for k, s in enumerate(sums):
            assert s <= stated * r.b_mul, "%s output %d: sum up to %.1f p, pairing_par.hpp states %d * 1.5 p" % (
                name, k, s / p, stated)
        worst["output"] = max([worst["output"]] + sums)
        return [(o + k, RED) for k in range(len(outs))]

    for ins in code:
        kind = ins[0]
        if kind == G.K_ROUND:
            writes = round_(*ins[1:5])
        elif kind == G.K_ROUND2:
            writes = round_(*ins[1:5]) + round_(*ins[5:9])
        elif kind == G.K_CYCRUN:
            writes, src, dst = [], ins[2], ins[3]
            for _ in range(ins[1]):
                for reg, c in round_(OP_NAMES.index("CYC"), src, G.NONE, dst):
                    cls[reg] = c
                src, dst = dst, (ins[4] if dst == ins[3] else ins[3])
        elif kind == G.K_COPY:
            writes = [(ins[4] + k, cls[ins[2] + k]) for k in range(12)]
        else:
            assert kind == G.K_INV and cls[ins[2]] is not None
            writes = [(ins[4], MUL)]
        for reg, c in writes:
            cls[reg] = c
    return {k: v / p for k, v in worst.items()}


def family_forms_ok(curve, name, tables):
    """Every factor form of `name` on every case of its family, as exact integers and limb by limb:
    |form| < 2^HEAD p (lp_mul's domain), lane accumulators below 2^58, top lane within 32 bits."""
    r = ref(curve)
    lp, N = r.lp, r.N
    prods, _ = tables[name]
    Kc = None
    for A, B in r.family(name):
        rows = {"A": A, "B": B}
        for L, R_ in prods:
            for form in (L, R_):
                if any(src == "K" for src, _ in form):
                    if Kc is None:
                        Kc = [lp.row(r.mont(k)) for k in G.consts(curve)]
                    rows["K"] = Kc
                acc = [sum(c * rows[src][i][lane] for (src, i), c in form.items()) for lane in range(16)]
                assert all(abs(v) < 1 << 58 for v in acc)
                assert abs(lp.value(acc)) < lp.bound, (name, form)
                assert abs(acc[N - 1] + (acc[N - 2] >> 29)) < 1 << 31
    return True
