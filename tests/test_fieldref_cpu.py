"""Keeps tests/fieldref.py -- the big-integer reference and the operand generator of
tests/test_gpu_field.py -- honest without a GPU: its model products are Montgomery products,
its outputs sit within the bounds tools/gen_params29.py check_bounds assigns, every generated
operand meets the precondition of the op it is fed to, the listed edge values are all emitted,
and its checkers accept the output of an independent limb-by-limb emulation of the device
algorithms (which also asserts the 64-bit column headroom) and reject it once one word is off."""
import random
from fractions import Fraction

import pytest

import fieldref as F

M29 = F.M29
LAYERS = [(k, c) for c in F.CURVES for k in ("fp", "fr", "f29", "lp")]


def cases_of(kind, curve, op):
    return F.ops_of(kind, curve)[op].cases


def test_registry_lists_exactly_the_generated_ops():
    want = {(k, c): set() for k, c in LAYERS}
    for k, c, o in F.all_op_ids():
        want[(k, c)].add(o)
    for k, c in LAYERS:
        assert set(F.ops_of(k, c)) == want[(k, c)], (k, c)
        assert all(len(o.cases) >= F.NRANDOM for o in F.ops_of(k, c).values()), "2048 random cases per op"


def test_probe_table_matches_the_encoders():
    """The probe library's op table (no GPU needed to ask it) against the generator's encoders,
    and its argument checks: they return before any HIP call."""
    import fieldprobe
    for k, c, o in F.all_op_ids():
        spec = F.ops_of(k, c)[o]
        wi, wo = fieldprobe.words(c, o)
        assert {len(spec.encode(x)) for x in spec.cases[:8] + spec.cases[-8:]} == {wi} and wo > 0, (c, o)
    with pytest.raises(KeyError):
        fieldprobe.words("bn254", "f29.no_such_op")
    run = fieldprobe.lib().kzgmi_fieldprobe_run
    assert run(2, b"fp.add", None, 4, None) == -1      # unknown curve
    assert run(0, b"fp.no_such_op", None, 4, None) == -2
    assert run(0, b"lp.mul", None, 3, None) == -3      # row ops take whole waves: multiples of 4
    assert run(1, b"fp.add", None, 0, None) == -3


# ---------------------------------------------------------------------------- the model products
@pytest.mark.parametrize("curve", F.CURVES)
@pytest.mark.parametrize("which", ["fp", "fr"])
def test_model32_products_are_montgomery_products(curve, which):
    m = F.layer(which, curve)
    p, R = m.p, m.R
    rinv = pow(R, -1, p)
    for a, b in cases_of(which, curve, which + ".mul")[::3]:
        t = m.mont_scan(a, b)
        assert t % p == a * b * rinv % p and t < 2 * p
        assert m.mul(a, b) == a * b * rinv % p
    if m.lazy:
        for a, b in cases_of(which, curve, which + ".mul_lazy")[::3]:
            t = m.mont_scan(a, b)
            assert t % p == a * b * rinv % p and t < 2 * p, "lazy product leaves [0, 2p)"
        for a, b, c, d in cases_of(which, curve, which + ".mul2_lazy")[::3]:
            t = m.mont_scan(a, b, c, d)
            assert t % p == (a * b + c * d) * rinv % p and t < R
            assert t < 2 * p if 8 * p < R else t < 4 * p  # one fold of 2p brings it back


@pytest.mark.parametrize("curve", F.CURVES)
def test_model29_products_and_bounds(curve):
    m = F.layer("f29", curve)
    p, R, B = m.p, m.R, m.bounds
    rinv = pow(R, -1, p)
    kmax = m.kmax
    for a, b in cases_of("f29", curve, "f29.mul")[::5]:
        t = m.mont(a, b)
        assert t % p == a * b * rinv % p and t < m.mont_bound(kmax, kmax) * p
    k2 = m.rec["y"] + 2
    for a, b, c, d in cases_of("f29", curve, "f29.mul2")[::5]:
        t = m.mont(a, b, c, d)
        assert t % p == (a * b + c * d) * rinv % p and t < m.mont_bound(k2, k2, k2, k2) * p
    kppp = m.bias("ACC_PPP")
    y3 = m.mont_bound(B["acc_R"], B["acc_D"], B["Y"], kppp)
    assert y3 <= B["Y"], "the loop's y bound is a fixed point"
    for r, d, y, q in cases_of("f29", curve, "f29.mul2_neg")[::3]:
        t = m.mont(r, d, y, kppp * p - q)
        assert t % p == (r * d - y * q) * rinv % p and t < y3 * p
    k3 = m.bias("ACC_X3")
    for a, s, t in cases_of("f29", curve, "f29.sub3_ACC_X3"):
        v = a + k3 * p - s - 2 * t
        assert 0 <= v < (2 + k3) * p <= m.rec["x"] * p and v % p == (a - s - 2 * t) % p


@pytest.mark.parametrize("curve", F.CURVES)
def test_bound_model_is_check_bounds(curve):
    """fieldref's walk through the value bounds is the generator's: same fixed point, and the
    record formulas stay inside the record bounds on both curves; on BLS12-381 within the
    figures csrc/msm.hpp documents."""
    m = F.layer("f29", curve)
    B = m.bounds
    cb = F.gen29.check_bounds(m.p, m.N, m.nkp, m.roles)
    assert (float(B["X"]), float(B["Y"]), float(B["Z"])) == (cb["X"], cb["Y"], cb["Z"])
    rec = m.rec
    for pre in ("add", "x29dbl", "dbl"):
        assert B[pre + "_x"] < rec["x"] and B[pre + "_y"] < rec["y"]
        assert B[pre + "_zz"] < rec["z"] and B[pre + "_zzz"] < rec["z"]
    if curve == "bls12_381":
        assert B["add_x"] < Fraction(91, 10) and max(B["add_y"], B["add_zz"], B["add_zzz"]) < Fraction(101, 100)
        assert B["x29dbl_x"] < Fraction(51, 10) and max(B["x29dbl_y"], B["x29dbl_zz"], B["x29dbl_zzz"]) < Fraction(101, 100)
        assert B["dbl_x"] < 10 and B["dbl_y"] < 10 and max(B["dbl_zz"], B["dbl_zzz"]) < 2
    for nm in ("B2", "B4", "B8", "B16", "ACC_NEG", "ACC_P", "ACC_R", "ACC_QX", "ACC_PPP", "DBL_X", "DBL_QX", "DBL_Y", "ACC_X3"):
        assert m.bias(nm) >= 1  # the generated limbs are that multiple of p (asserted inside)


# ---------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("curve", F.CURVES)
def test_operands_meet_preconditions_32(curve):
    for which in ("fp", "fr"):
        m = F.layer(which, curve)
        p, R = m.p, m.R
        lim = {"csub_mod": R, "csub_mod2": R, "raw_lt_mod": R, "mul_lazy": 2 * p, "add_lazy": 2 * p, "sub_lazy": 2 * p,
               "neg_lazy": 2 * p, "is_zero_lazy": 2 * p, "canon": 2 * p, "mul2_lazy": 2 * p + 1, "rsub_mod": p + 1}
        for name, op in F.ops_of(which, curve).items():
            bound = lim.get(name.split(".")[1], p)
            assert all(0 <= v < bound for c in op.cases for v in c), name


@pytest.mark.parametrize("curve", F.CURVES)
def test_operands_meet_preconditions_29(curve):
    m = F.layer("f29", curve)
    p, n, B = m.p, m.N, m.bounds
    ops = F.ops_of("f29", curve)
    word_ops = ("f29.limbs29", "f29.fp_to29")
    for name, op in ops.items():
        if name in word_ops or name in ("f29.x29_add", "f29.x29_dbl"):
            continue
        for c in op.cases:  # normalised limbs: every operand is below R29, so its top limb is below 2^29
            assert all(0 <= v < m.R and max(F.limbs29(v, n)) <= M29 for v in c), name
    kmax = m.kmax
    assert kmax >= 2 * m.rec["y"] and (kmax == 76) == (curve == "bls12_381")
    assert all(v < kmax * p for c in ops["f29.mul"].cases + ops["f29.sqr"].cases for v in c)
    assert ("B64" in m.sub_biases) == (curve == "bls12_381")
    for nm in m.sub_biases:
        assert all(a < m.minuend_bound(nm) * p and b <= m.bias(nm) * p for a, b in ops["f29.sub_" + nm].cases), nm
    assert all(v < m.nkp * p for v, in ops["f29.is_zero"].cases)
    assert ops["f29.is_zero"].cases is ops["f29.is_zero_mf"].cases
    assert all(v < 2 * p for v, in ops["f29.canon"].cases)
    btop = m.H["ACC_PPP"][n - 1]
    for r, d, y, q in ops["f29.mul2_neg"].cases:
        assert r < B["acc_R"] * p and d < B["acc_D"] * p and y < B["Y"] * p and q < B["acc_PPP"] * p
        assert F.limbs29(q, n)[n - 1] <= btop
    lim = [m.rec["x"], m.rec["y"], m.rec["z"], m.rec["z"]]
    for c in ops["f29.x29_add"].cases + ops["f29.x29_dbl"].cases:
        for r in c:
            assert all(v < k * p for v, k in zip(r[:4], lim)) and (r[4] == 0 or r[2] == 0)
    assert all(x < B["qin"] * p and y < m.bias("ACC_NEG") * p for x, y in ops["f29.dbl_affine"].cases)
    assert all(v < p for v, in ops["f29.fp_to29"].cases)


@pytest.mark.parametrize("curve", F.CURVES)
def test_operands_meet_preconditions_lp(curve):
    m = F.layer("lp", curve)
    ops = F.ops_of("lp", curve)
    for name in ("lp.mul", "lp.reduce", "lp.row_is_zero", "lp.to_fp", "lp.canon"):
        for c in ops[name].cases:
            for row in c:
                m.check_row_in(row)
    assert all(abs(m.value(c[0])) < (1 << min(13, m.HEAD)) * m.p for c in ops["lp.canon"].cases)
    for row, in ops["lp.norm"].cases:
        assert len(row) == 16 and not any(row[m.N:]) and all(abs(v) < 2 ** 30.6 for v in row)
    # all four rows of a wave carry different cases
    for name in ("lp.norm", "lp.mul", "lp.reduce", "lp.row_is_zero", "lp.to_fp", "lp.canon", "lp.raw_from_words"):
        cs = ops[name].cases
        same = [i for i in range(0, len(cs) - 3, 4) if len({repr(c) for c in cs[i:i + 4]}) < 4]
        assert not same, (name, same[:3])
        assert ops[name].pad_to == 4


# ---------------------------------------------------------------------------- the listed edge values
@pytest.mark.parametrize("curve", F.CURVES)
def test_edge_values_emitted_32(curve):
    for which in ("fp", "fr"):
        m = F.layer(which, curve)
        p, R, N = m.p, m.R, m.N
        ops = F.ops_of(which, curve)
        edge = {0, 1, 2, p - 2, p - 1, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p}
        edge |= {v for j in range(1, N) for v in ((1 << (32 * j)) - 1, 1 << (32 * j)) if v < p}
        edge |= {v for i in range(N) for v in (p & ~(0xFFFFFFFF << (32 * i)), p | (0xFFFFFFFF << (32 * i))) if v < p}
        for name in ("add", "sub", "mul", "mul_ps"):
            assert {(a, b) for a in edge for b in edge} <= set(ops[which + "." + name].cases), name
        assert {p - 1, p, p + 1, R - 1} <= {v for v, in ops[which + ".csub_mod"].cases}
        assert {p - 1, p, p + 1, R - 1} <= {v for v, in ops[which + ".raw_lt_mod"].cases}
        inv = {v for v, in ops[which + ".inv"].cases}
        ys = [1, 2, 3, p - 1, p - 2, (p + 1) // 2, 1 << 200, 1 << (p.bit_length() - 1), (1 << 64) - 1]
        assert {0} | set(ys) | {y * R % p for y in ys} <= inv
        if m.lazy:
            lazy = edge | {p, p + 1, 2 * p - 2, 2 * p - 1}
            for name in ("mul_lazy", "add_lazy", "sub_lazy"):
                assert {(a, b) for a in lazy for b in lazy} <= set(ops[which + "." + name].cases), name
            assert lazy <= {v for v, in ops[which + ".neg_lazy"].cases}
            assert {v for c in ops[which + ".mul2_lazy"].cases for v in c} >= lazy | {2 * p}
            assert (2 * p, 2 * p) in {c[:2] for c in ops[which + ".mul2_lazy"].cases}
            assert {2 * p - 1, 2 * p, 2 * p + 1} <= {v for v, in ops[which + ".csub_mod2"].cases}
            assert {0, p} <= {v for v, in ops[which + ".rsub_mod"].cases}


@pytest.mark.parametrize("curve", F.CURVES)
def test_edge_values_emitted_29(curve):
    m = F.layer("f29", curve)
    p, n, B = m.p, m.N, m.bounds
    ops = F.ops_of("f29", curve)
    s = 29 * (n - 1)
    low = (1 << s) - 1
    kmax = m.kmax
    top = kmax * p - 1
    ones = ((top >> s) << s | low) if ((top >> s) << s | low) <= top else (((top >> s) - 1) << s | low)
    assert ones < kmax * p and all(v == M29 for v in F.limbs29(ones, n)[:n - 1])
    edge = {0, 1, p - 1, p, p + 1, top, ones, low} | {j * p + e for j in range(1, kmax) for e in (-1, 0, 1)}
    edge |= {F.value29([M29 * (i % 2) for i in range(n - 1)] + [0]), F.value29([M29 * (1 - i % 2) for i in range(n - 1)] + [0])}
    assert {(a, b) for a in edge for b in edge} <= set(ops["f29.mul"].cases)
    assert edge <= {v for v, in ops["f29.sqr"].cases}
    assert all((v, v, v, v) in set(ops["f29.mul2"].cases) for v in edge if v < (m.rec["y"] + 2) * p and v != ones)
    # PPP at 0, all ones, its bound - 1, with the other three operands at their bounds
    at = (m.below(B["acc_R"]), m.below(B["acc_D"]), m.below(B["Y"]))
    assert {at + (q,) for q in (0, low, m.below(B["acc_PPP"]))} <= set(ops["f29.mul2_neg"].cases)
    for nm in m.sub_biases:
        k = m.bias(nm)
        want = {(a, b) for a in (0, m.minuend_bound(nm) * p - 1) for b in (0, k * p - 1, k * p, low)}
        assert want <= set(ops["f29.sub_" + nm].cases), nm
    z = {v for v, in ops["f29.is_zero"].cases}
    kp_lo = set(m.H["KP_LO"])
    for j in range(m.nkp):
        assert {j * p, j * p + 1} <= z and (j == 0 or j * p - 1 in z)
        assert any(v % p and v & M29 == (j * p) & M29 and v >> 29 != (j * p) >> 29 for v in z), "filter hit, row differs"
        assert all(j * p + (1 << (29 * i)) in z or j * p + (1 << (29 * i)) >= m.nkp * p for i in range(1, n))
    assert kp_lo == {(j * p) & M29 for j in range(m.nkp)}
    kneg = m.bias("ACC_NEG")
    assert any(y == kneg * p - 1 for _, y in ops["f29.dbl_affine"].cases)
    kinds = set()
    for a, b in ops["f29.x29_add"].cases:
        if a[4] or b[4]:
            kinds.add("O+Q" if a[4] and not b[4] else "P+O" if b[4] and not a[4] else "O+O")
            continue
        A, Bp = m.rec_affine(a), m.rec_affine(b)
        if A == Bp:
            kinds.add("P+P scaled" if a[2] % p != b[2] % p else "P+P")
        elif A[0] == Bp[0]:
            kinds.add("P-P")
        if a[0] >= (m.rec["x"] - 1) * p and a[1] >= (m.rec["y"] - 1) * p and a[2] >= (m.rec["z"] - 1) * p:
            kinds.add("top shifts")
    assert kinds == {"O+Q", "P+O", "O+O", "P+P scaled", "P+P", "P-P", "top shifts"}


@pytest.mark.parametrize("curve", F.CURVES)
def test_edge_values_emitted_lp(curve):
    m = F.layer("lp", curve)
    p, N = m.p, m.N
    ops = F.ops_of("lp", curve)
    vals = {m.value(c[0]) for c in ops["lp.reduce"].cases}
    top = (1 << m.HEAD) - 1
    for j in (0, 1, -1, 2, -2, top, -top):
        assert {j * p - 1, j * p, j * p + 1} <= vals, j
        h = (2 * j + 1) * p // 2
        assert {h, h + 1} <= vals and 2 * h < (2 * j + 1) * p < 2 * (h + 1)
    assert len({v // p for v in vals if v % p == 0}) >= 20, "a seeded sample of j p between"
    assert {m.bound - 1, 1 - m.bound} <= vals
    limbs = {v for c in ops["lp.mul"].cases for row in c for v in row}
    assert {F.LP_LIMB_MAX, -F.LP_LIMB_MAX} <= limbs and F.LP_LIMB_MAX == (1 << 29) + 3
    nl = {v for row, in ops["lp.norm"].cases for v in row[:N - 1]}
    assert {F.LP_NORM_IN - 1, 1 - F.LP_NORM_IN} <= nl and F.LP_NORM_IN - 1 < 2 ** 30.6 <= F.LP_NORM_IN + 1
    assert set(map(repr, ops["lp.reduce"].cases)) <= set(map(repr, ops["lp.row_is_zero"].cases))
    # lp_canon's own family: its floor boundary up to the top of its contract, plain and redundant rows
    crow = [c[0] for c in ops["lp.canon"].cases]
    cvals = {m.value(l) for l in crow}
    ctop = (1 << min(13, m.HEAD)) - 1
    for j in (0, 1, -1, 2, -2, ctop, -ctop):
        assert {j * p - 1, j * p, j * p + 1} <= cvals, j
        assert any(m.value(l) == j * p and l == m.row(j * p) for l in crow)
    assert {(ctop + 1) * p - 1, 1 - (ctop + 1) * p} <= cvals
    assert len({v // p for v in cvals if v % p == 0}) >= 40, "a seeded sample of j p between"
    assert sum(1 for l in crow if l != m.row(m.value(l))) >= 512, "redundant (jiggled) rows"
    assert sum(1 for v in cvals if abs(v) > (ctop + 1) * p // 2) >= 512, "random rows reach the upper half of the range"
    zero_rows = [c[0] for c in ops["lp.row_is_zero"].cases if m.value(c[0]) == 0]
    assert any(all(zero_rows_i[:N]) for zero_rows_i in zero_rows), "zero held as a rippling carry"
    kinds = set()
    for P, _, Q, _ in ops["lp.xyzz_add"].cases:
        kinds.add("O" if P is None or Q is None else "P+P" if P == Q else "P-P" if P[0] == Q[0] else "P+Q")
    assert kinds == {"O", "P+P", "P-P", "P+Q"}


# ---------------------------------------------------------------------------- checkers vs an emulation
def emu_mont29(m, a, b, c=None, d=None):
    """field29.hpp's product scan limb by limb (29-bit m_k, one accumulator per column)."""
    n, P, inv = m.N, m.H["MOD"], m.H["INV"]
    acc, mm, t = 0, [0] * n, [0] * n
    for k in range(2 * n - 1):
        lo, hi = max(0, k - n + 1), min(k, n - 1)
        for i in range(lo, hi + 1):
            acc += a[i] * b[k - i] + (c[i] * d[k - i] if c else 0)
        for i in range(lo, k if k < n else n):
            acc += mm[i] * P[k - i]
        if k < n:
            mm[k] = ((acc & 0xFFFFFFFF) * inv) & M29
            acc += mm[k] * P[0]
            assert acc & M29 == 0
        else:
            t[k - n] = acc & M29
        assert acc < 1 << 64, "column overflow"
        acc >>= 29
    assert acc < 1 << 32
    t[n - 1] = acc
    return t


def emu_sub29(m, a, b, bias):
    out, c = [], 0
    for i in range(m.N):
        x = a[i] + bias[i] + c - b[i]
        assert 0 <= x < 1 << 32, "limb went negative"
        out.append(x & M29 if i < m.N - 1 else x)
        c = x >> 29
    return out


def tampered(out):
    return [out[0] ^ 1] + list(out[1:])


@pytest.mark.parametrize("curve", F.CURVES)
def test_checkers_accept_the_emulation_and_reject_one_bit(curve):
    m = F.layer("f29", curve)
    n = m.N
    ops = F.ops_of("f29", curve)
    L = lambda v: F.limbs29(v, n)  # noqa: E731
    rng = random.Random(5)

    def sample(op, k=400):
        cs = ops[op].cases
        return cs[:k] + rng.sample(cs, k)

    for op, f in (("f29.mul", lambda a, b: emu_mont29(m, L(a), L(b))),
                  ("f29.sqr", lambda a: emu_mont29(m, L(a), L(a))),
                  ("f29.mul2", lambda a, b, c, d: emu_mont29(m, L(a), L(b), L(c), L(d))),
                  ("f29.mul2_neg", lambda r, d, y, q: emu_mont29(
                      m, L(r), L(d), L(y), [x - z for x, z in zip(m.H["ACC_PPP"], L(q))])),
                  ("f29.sub_B2", lambda a, b: emu_sub29(m, L(a), L(b), m.H["B2"])),
                  ("f29.sub_" + m.sub_biases[5], lambda a, b: emu_sub29(m, L(a), L(b), m.H[m.sub_biases[5]])),
                  ("f29.sub_ACC_QX", lambda a, b: emu_sub29(m, L(a), L(b), m.H["ACC_QX"]))):
        for case in sample(op):
            out = f(*case)
            assert ops[op].check(case, out) is None, (op, F.hexs(case))
            assert ops[op].check(case, tampered(out)), (op, "a wrong low bit passes")
    # the extreme column of the accumulation's Y3: every operand at its bound, PPP = 0 (the
    # un-normalised ACC_PPP - PPP limbs at their largest)
    B = m.bounds
    case = (m.below(B["acc_R"]), m.below(B["acc_D"]), m.below(B["Y"]), 0)
    assert ops["f29.mul2_neg"].check(case, emu_mont29(m, L(case[0]), L(case[1]), L(case[2]), m.H["ACC_PPP"])) is None
    for v in (0, m.p, 2 * m.p, (m.nkp - 1) * m.p):
        assert ops["f29.is_zero"].check((v,), [1]) is None and ops["f29.is_zero"].check((v,), [0])
        assert ops["f29.is_zero"].check((v + 1,), [0]) is None and ops["f29.is_zero"].check((v + 1,), [1])


def emu_lp_mul(m, a, b):
    """lpfield.hpp's systolic product and one carry pass on a 16-lane row of signed limbs."""
    N, P, inv = m.N, m.H["MOD"], m.H["INV"]
    acc = [0] * 16
    for i in range(N):
        acc = [x + a[i] * bj for x, bj in zip(acc, b)]
        mq = ((acc[0] & 0xFFFFFFFF) * inv) & M29
        acc = [x + mq * pj for x, pj in zip(acc, P)]
        assert acc[0] & M29 == 0 and all(abs(x) < 1 << 63 for x in acc)
        lo, hi = [x & M29 for x in acc], [x >> 29 for x in acc]
        acc = [hi[j] + (lo[j + 1] if j < 15 else 0) for j in range(16)]
    assert all(abs(x) < 1 << 31 for x in acc)
    carry = [(x >> 29) if j < N - 1 else 0 for j, x in enumerate(acc)]
    return [((x & M29) if j < N - 1 else x) + (carry[j - 1] if j else 0) for j, x in enumerate(acc)]


@pytest.mark.parametrize("curve", F.CURVES)
def test_lp_checkers_accept_the_emulation_and_reject_one_bit(curve):
    m = F.layer("lp", curve)
    ops = F.ops_of("lp", curve)
    cs = ops["lp.mul"].cases
    for case in cs[:300] + cs[-300:]:
        out = [v & 0xFFFFFFFF for v in emu_lp_mul(m, *case)]
        assert ops["lp.mul"].check(case, out) is None, F.hexs(case)
        assert ops["lp.mul"].check(case, tampered(out))
    row = m.row(3 * m.p)
    assert ops["lp.row_is_zero"].check((row,), [1]) is None and ops["lp.row_is_zero"].check((row,), [0])
    assert ops["lp.canon"].check((row,), F.to_words(0, m.W)) is None
    assert ops["lp.canon"].check((row,), F.to_words(m.p, m.W)), "an uncanonical p passes"
    wide = (F.LP_NORM_LO, F.LP_NORM_HI)  # lp.norm alone; lp_mul / lp_reduce keep [-2, 2^29 + 2)
    assert m.norm_ok([-4] + [0] * 15, *wide) is None and m.norm_ok([-5] + [0] * 15, *wide)
    assert m.norm_ok([(1 << 29) + 2] + [0] * 15, *wide) is None and m.norm_ok([(1 << 29) + 3] + [0] * 15, *wide)
    assert m.norm_ok([-2] + [0] * 15) is None and m.norm_ok([-3] + [0] * 15)
    assert m.norm_ok([(1 << 29) + 1] + [0] * 15) is None and m.norm_ok([(1 << 29) + 2] + [0] * 15)
