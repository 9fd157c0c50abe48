"""The pairing interpreter, op by op, on its fast and generic paths.

The test-only probe (tests/native/pairing_probe.hip, tests/pairingprobe.py) runs the shipped
par_load_consts and par_run of csrc/pairing_par.hpp on a caller-supplied program and register
image (programs are built with tools/gen_bilinear.py's Prog, so its alias assertions hold for
them too), and the body of k_pairing_check_par behind k_precompute_lines with the result rows
copied out.  Every value is compared, as an exact integer, with the plain big-integer tower
reference of tests/pairingref.py: a round output must be congruent to op(...) R, lie within the
bound lp_reduce is held to and have normalised limbs; a copied block keeps its limbs; a K_INV
result is an lp_mul output.  Registers outside an instruction's output blocks must come back
unchanged.  The operand families (every coefficient in turn and all together at 0, +-1, +-p,
+-p +- 1 and +- each operand bound, the units, subfield elements, sign patterns at the bounds,
all-limbs-at-maximum and ripple rows, each plain and with redundant limbs, 256 seeded random
cases) are generated and precondition-checked in pairingref.py; none is dropped here.  Each test
is one probe launch.  A probe kernel first fills its whole LDS with a poison word, so no result
can rest on what an earlier workgroup left there; test_lds_independent runs every op under
three poisons and requires the same bits.

What this pins: the shipped par_run, the shipped tables and both round bodies -- par_round_fast
(MUL, LL, CYC, SQR + LL, K_CYCRUN), which production takes for those ops (fast_ok is asserted 1
on the shipped tables), and the generic round body with its chunked reader (lp_eval_terms /
lp_terms_chunk), which production runs for CONJ, FROB1/2/3 and the seven inversion stages and
would run for everything if a list outgrew its slot: every one of the 17 ops through it,
including the generic forms of MUL / SQR / CYC / LL and the K_CYCRUN fallback that no production
call reaches today -- on operands at the edge of their bounds; LINE, LEVAL and BLS12-381's
FROB3, which no shipped program uses; K_COPY, K_INV and the inversion chain stage by stage; and k_pairing_check_par's
value (not only its verdict) on homogeneous points with arbitrary ZZ / ZZZ, two pairs, and
every skip flag, which also covers csrc/tower.hpp's Fp2 line precomputation over random Q.
The public kzgmi_pairing is compared with the oracle on seeded random points and at infinity.

What it does not pin: the serial tower pairing (k_pairing_check / k_pairing_one of
csrc/kernels.hpp), which the shipped build launches nowhere; and the probe kernels are their
own compilation of par_run, not the register allocation of the copy inside libkzgmi.so (the
parity tests and the public-API tests here stay that copy's end-to-end check).
"""
import functools
import random

import numpy as np
import pytest

import fieldref as F
import pairingprobe
import pairingref as PR
from oracle import oracle as O  # checker only
from oracle.pyspec import curves as pc
from oracle.pyspec import kzg as pk

pytestmark = pytest.mark.gpu

G = PR.G
CURVES = F.CURVES
PATHS = ["fast", "generic"]
RUN_LENGTHS = [1, 2, 3, 5, 9, 32]
NRAND_INV = 128


def run(curve, P, code, placements, generic):
    """One launch: (images in, images out); asserts the fast_ok every block reports."""
    img = PR.images(P, placements)
    out, fast = pairingprobe.run_program(curve, code, img, generic)
    assert fast == [0 if generic else 1] * len(placements), "fast_ok: %r" % sorted(set(fast))
    return img, out


def rows_at(P, out, k, reg, n):
    return out[k, reg - P.R_P:reg - P.R_P + n]


def check_blocks(curve, P, img, out, cases, blocks):
    """blocks: (output register, op name, case -> (A rows, B rows)) per output block of the program."""
    r = PR.ref(curve)
    bad = []
    for k, case in enumerate(cases):
        for reg, name, pick in blocks:
            want = r.want(name, pick(case))
            msg = r.check_round_rows(rows_at(P, out, k, reg, len(want)), want)
            if msg:  # the whole evidence goes into the message: operands as integers, rows as read back
                A, B = pick(case)
                bad.append((k, name, "%s; A = %s; B = %s; rows read back: %s" % (
                    msg, F.hexs(r.values(A)), F.hexs(r.values(B)), rows_at(P, out, k, reg, len(want)).tolist())))
    assert not bad, "%d results of %d cases wrong (cases %s); first: case %d %s -- %s" % (
        (len(bad), len(cases), sorted({b[0] for b in bad})[:16]) + bad[0])
    msg = PR.untouched(P, img, out, [(reg, PR.SHAPES[name][2]) for reg, name, _ in blocks])
    assert msg is None, msg


def one_op_test(curve, name, generic):
    r = PR.ref(curve)
    P = PR.new_prog(curve)
    wa, wb, _ = PR.SHAPES[name]
    a, b, o = P.g(0), (P.g(1) if wb else None), P.g(2)
    P.op(name, a, b, o)
    cases = r.family(name)
    img, out = run(curve, P, P.code, [[(a, A), (b or a, B)] for A, B in cases], generic)
    check_blocks(curve, P, img, out, cases, [(o, name, lambda c: c)])


# ---------------------------------------------------------------------------- static
@pytest.mark.parametrize("curve", CURVES)
def test_info_matches_header(curve):
    info, hdr = pairingprobe.info(curve, PR.OP_NAMES), PR.header_info(curve)
    for k in ("NPROG", "NR", "R_K", "R_E", "R_P", "R_SCAL", "R_G", "R_RES"):
        assert info[k] == hdr[k], k
    assert info["OP_COUNT"] == len(PR.OP_NAMES) and info["PAR_THREADS"] == 1024
    assert info["NL"] == G.num_lines(curve)
    for name in PR.OP_NAMES:
        assert (info["NP"][name], info["NO"][name]) == (hdr[name + "_NP"], hdr[name + "_NO"]), name


@pytest.mark.parametrize("curve", CURVES)
def test_program_check_refuses(curve):
    """The host-side bytecode check: nothing out of range reaches a launch."""
    P = PR.new_prog(curve)
    img = PR.images(P, [[]])
    NONE, last = G.NONE, P.NR - 11
    mul = G.OPNUM["MUL"]
    bad = [
        [[5, 0, P.g(0), NONE, P.g(1), 0, 0, 0, 0, 0]],                       # kind
        [[G.K_ROUND, len(PR.OP_NAMES), P.g(0), NONE, P.g(1), 0, 0, 0, 0, 0]],  # op
        [[G.K_ROUND, mul, last, P.g(1), P.g(2), 0, 0, 0, 0, 0]],             # A block past NR
        [[G.K_ROUND, mul, P.g(0), last, P.g(2), 0, 0, 0, 0, 0]],             # B block past NR
        [[G.K_ROUND, mul, P.g(0), NONE, P.g(2), 0, 0, 0, 0, 0]],             # B missing
        [[G.K_ROUND, mul, P.g(0), P.g(1), last, 0, 0, 0, 0, 0]],             # output block past NR
        [[G.K_ROUND2, G.OPNUM["SQR"], P.g(0), NONE, P.g(1), G.OPNUM["LL"], P.g(2), P.g(2) + 6, last, 0]],
        [[G.K_COPY, 0, P.g(0), NONE, last, 0, 0, 0, 0, 0]],
        [[G.K_COPY, 0, last, NONE, P.g(0), 0, 0, 0, 0, 0]],
        [[G.K_INV, 0, P.NR, NONE, P.R_SCAL, 0, 0, 0, 0, 0]],
        [[G.K_INV, 0, P.R_SCAL, NONE, P.NR, 0, 0, 0, 0, 0]],
        [[G.K_CYCRUN, 0, P.g(0), P.g(1), P.g(2), 0, 0, 0, 0, 0]],            # count
        [[G.K_CYCRUN, 65, P.g(0), P.g(1), P.g(2), 0, 0, 0, 0, 0]],
        [[G.K_CYCRUN, 2, P.g(0), P.g(1), last, 0, 0, 0, 0, 0]],
        [[G.K_COPY, 0, P.g(0), NONE, P.g(0), 0, 0, 0, 0, 0]] * (pairingprobe.info(curve, PR.OP_NAMES)["NPROG"] + 1),
    ]
    for code in bad:
        with pytest.raises(pairingprobe.ProgramRejected):
            pairingprobe.run_program(curve, code, img, False)
    ok = [[G.K_COPY, 0, last - 1, NONE, last - 1, 0, 0, 0, 0, 0]]  # the last block that fits
    out, _ = pairingprobe.run_program(curve, ok, img, False)
    assert np.array_equal(out, img)


# ---------------------------------------------------------------------------- single ops
@pytest.mark.parametrize("curve,name", [(c, o) for c in CURVES for o in PR.OP_NAMES],
                         ids=["%s-%s" % (c, o) for c in CURVES for o in PR.OP_NAMES])
def test_op_generic(curve, name):
    """Every op as a one-instruction program through the generic reader (fast_ok cleared)."""
    one_op_test(curve, name, True)


@pytest.mark.parametrize("name", ["MUL", "LL", "CYC"])
@pytest.mark.parametrize("curve", CURVES)
def test_op_fast(curve, name):
    """The fast single-op rounds; fast_ok comes back 1: the shipped tables fit the fast slots, so
    this is the path production takes."""
    one_op_test(curve, name, False)


# ---------------------------------------------------------------------------- two-op rounds
def round2_test(curve, n1, n2, generic):
    r = PR.ref(curve)
    P = PR.new_prog(curve)
    (wa1, wb1, _), (wa2, wb2, _) = PR.SHAPES[n1], PR.SHAPES[n2]
    a1, b1, o1 = P.g(0), (P.g(1) if wb1 else None), P.g(2)
    a2 = P.g(3)
    b2 = (a2 + 6 if wa2 == 6 else P.g(4)) if wb2 else None  # LL's operands lie side by side, as E[idx] does
    o2 = P.g(5)
    P.op2(n1, a1, b1, o1, n2, a2, b2, o2)
    f1, f2 = r.family(n1), r.family(n2)
    cases = [(f1[k % len(f1)], f2[k % len(f2)]) for k in range(max(len(f1), len(f2)))]
    place = [[(a1, c1[0]), (b1 or a1, c1[1]), (a2, c2[0]), (b2 or a2, c2[1])] for c1, c2 in cases]
    img, out = run(curve, P, P.code, place, generic)
    check_blocks(curve, P, img, out, cases, [(o1, n1, lambda c: c[0]), (o2, n2, lambda c: c[1])])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("curve", CURVES)
def test_round2_sqr_ll(curve, path):
    """SQR + LL in one round: the Miller loop's step, the only fast pair."""
    round2_test(curve, "SQR", "LL", path == "generic")


@pytest.mark.parametrize("curve", CURVES)
def test_round2_conj_frob1(curve):
    """A pair with no fast form (CONJ has no products, FROB1 reads K): the generic K_ROUND2."""
    round2_test(curve, "CONJ", "FROB1", True)


# ---------------------------------------------------------------------------- K_CYCRUN
@functools.lru_cache(maxsize=None)
def cyc_chains(curve):
    """Per case of the CYC family: the field elements of 0..max(RUN_LENGTHS) chained squarings."""
    r = PR.ref(curve)
    chains = []
    for A, _ in r.family("CYC"):
        cur = [r.elem(v) for v in r.values(A)]
        ch = [cur]
        for _ in range(max(RUN_LENGTHS)):
            cur = r.T.cyc(cur)
            ch.append(cur)
        chains.append(ch)
    return chains


@pytest.mark.parametrize("n", RUN_LENGTHS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("curve", CURVES)
def test_cycrun(curve, path, n):
    """n chained squarings s0 -> u -> v -> u ...: the last destination holds the n-th squaring, the
    other register the (n - 1)-th (for n = 1, v is not written)."""
    r = PR.ref(curve)
    P = PR.new_prog(curve)
    s0, u, v = P.g(0), P.g(1), P.g(2)
    cur = s0
    for k in range(n):  # the chain as cyclo_pow emits it, folded by the generator's own pass
        P.op("CYC", cur, None, u if k % 2 == 0 else v)
        cur = u if k % 2 == 0 else v
    if n >= 2:
        G.compress_cyc_runs(P)
        assert P.code == [[G.K_CYCRUN, n, s0, u, v, 0, 0, 0, 0, 0]]
    code = [[G.K_CYCRUN, n, s0, u, v, 0, 0, 0, 0, 0]]
    cases = r.family("CYC")
    img, out = run(curve, P, code, [[(s0, A)] for A, _ in cases], path == "generic")
    last, other = (u, v) if n % 2 else (v, u)
    bad = []
    for k, ch in enumerate(cyc_chains(curve)):
        msg = r.check_round_rows(rows_at(P, out, k, last, 12), ch[n])
        if msg is None and n >= 2:
            msg = r.check_round_rows(rows_at(P, out, k, other, 12), ch[n - 1])
            msg = msg and "other register: " + msg
        if msg:
            bad.append((k, msg))
    assert not bad, "%d of %d cases wrong; first: case %d -- %s" % ((len(bad), len(cases)) + bad[0])
    msg = PR.untouched(P, img, out, [(u, 12)] + ([(v, 12)] if n >= 2 else []))
    assert msg is None, msg


# ---------------------------------------------------------------------------- K_COPY, K_INV
@pytest.mark.parametrize("curve", CURVES)
def test_copy(curve):
    """K_COPY moves twelve rows limb for limb, whatever their form."""
    r = PR.ref(curve)
    P = PR.new_prog(curve)
    P.copy(P.g(1), P.g(0))
    cases = r.family("CONJ")
    img, out = run(curve, P, P.code, [[(P.g(0), A)] for A, _ in cases], False)
    src = img[:, P.g(0) - P.R_P:P.g(0) - P.R_P + 12]
    assert np.array_equal(out[:, P.g(1) - P.R_P:P.g(1) - P.R_P + 12], src)
    assert PR.untouched(P, img, out, [(P.g(1), 12)]) is None


@pytest.mark.parametrize("curve", CURVES)
def test_inv(curve):
    """K_INV at 0, +-1, p - 1, at values held as +-p and +-p +- 1, at the operand bounds, at the
    field elements 1 and -1, and on random rows; 0 -> 0."""
    r = PR.ref(curve)
    lp, p = r.lp, r.p
    rng = random.Random("%d K_INV %s" % (F.SEED, curve))
    vals = r.edge_values() + [r.mont(1), r.mont(p - 1), r.mont(1) - p, r.mont(2), r.mont(pow(2, -1, p))]
    vals += [rng.randrange(1 - r.b_mul, r.b_mul) for _ in range(NRAND_INV)]
    rows = []
    for v in vals:
        rows += [lp.row(v), lp.jiggle(rng, lp.row(v))]
    rows += r.clipped_edge_rows(rng)
    rows = [r.check_operand_row(l) for l in F.dedupe(rows)]
    P = PR.new_prog(curve)
    src, dst = P.R_SCAL, P.R_SCAL + 1
    P.inv(dst, src)
    img, out = run(curve, P, P.code, [[(src, [l])] for l in rows], False)
    bad = [(k, msg) for k, msg in ((k, r.check_inv_row(rows_at(P, out, k, dst, 1)[0], lp.value(l)))
                                   for k, l in enumerate(rows)) if msg]
    assert not bad, "%d of %d cases wrong; first: %s -- %s" % (len(bad), len(rows), F.hexs(rows[bad[0][0]]), bad[0][1])
    zero = [k for k, l in enumerate(rows) if lp.value(l) % p == 0]
    assert len(zero) >= 4 and all(lp.value([int(x) for x in rows_at(P, out, k, dst, 1)[0]]) % p == 0 for k in zero)
    assert PR.untouched(P, img, out, [(dst, 1)]) is None


# ---------------------------------------------------------------------------- the inversion chain
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("curve", CURVES)
def test_inversion_chain(curve, path):
    """INV_NORM ... INV12_FIN with K_INV in the shipped program's order, every stage kept in a
    register of its own, then f f^-1 by MUL."""
    r = PR.ref(curve)
    lp, p, T = r.lp, r.p, r.T
    rng = random.Random("%d inversion %s" % (F.SEED, curve))
    rv = lambda: rng.randrange(1 - r.b_mul, r.b_mul)  # noqa: E731
    one = r.R % p
    fs = [[rv() for _ in range(12)] for _ in range(32)]
    fs += [[one] + [0] * 11, [-one] + [0] * 11, [one - p] + [0] * 11]
    for k in (1, 2, 6):                                    # f in Fp, Fp2, Fp6 (c1 = 0)
        fs += [[rv() for _ in range(k)] + [0] * (12 - k) for _ in range(4)]
    fs += [[0] * 6 + [rv() for _ in range(6)] for _ in range(4)]   # c0 = 0
    fs += [[p, -p] * 3 + [rv() for _ in range(6)], [rv() for _ in range(6)] + [p, -p] * 3]  # zero halves held as +-p
    cases = []
    for f in fs:
        rows = [lp.row(v) for v in f]
        cases += [rows, [lp.jiggle(rng, l) for l in rows]]
    P = PR.new_prog(curve)
    f, sc = P.g(0), P.R_SCAL
    reg = {"INV_NORM": P.g(3), "INV6_T": P.g(4), "INV6_D": P.g(5), "INV2_N": sc, "K_INV": sc + 1, "INV2_FIN": P.g(6),
           "INV6_FIN": P.g(7), "INV12_FIN": P.g(8), "MUL": P.g(9)}
    P.op("INV_NORM", f, None, reg["INV_NORM"])
    P.op("INV6_T", reg["INV_NORM"], None, reg["INV6_T"])
    P.op("INV6_D", reg["INV_NORM"], reg["INV6_T"], reg["INV6_D"])
    P.op("INV2_N", reg["INV6_D"], None, sc)
    P.inv(sc + 1, sc)
    P.op("INV2_FIN", reg["INV6_D"], sc + 1, reg["INV2_FIN"])
    P.op("INV6_FIN", reg["INV6_T"], reg["INV2_FIN"], reg["INV6_FIN"])
    P.op("INV12_FIN", f, reg["INV6_FIN"], reg["INV12_FIN"])
    P.op("MUL", f, reg["INV12_FIN"], reg["MUL"])
    img, out = run(curve, P, P.code, [[(f, rows)] for rows in cases], path == "generic")
    bad = []
    for k, rows in enumerate(cases):
        x = [r.elem(v) for v in r.values(rows)]
        st = T.inverse(x)
        assert any(x) and st["INV2_N"][0], "a case of this test is not invertible"
        st["MUL"] = T.one()
        for name, want in st.items():
            got = rows_at(P, out, k, reg[name], len(want))
            if name == "K_INV":
                nrm = lp.value([int(v) for v in rows_at(P, out, k, sc, 1)[0]])
                msg = r.check_inv_row(got[0], nrm)
            else:
                msg = r.check_round_rows(got, want)
            if msg:
                bad.append((k, name, msg))
    assert not bad, "%d stage results wrong; first: case %d %s -- %s" % ((len(bad),) + bad[0])
    written = [(reg[n], PR.SHAPES[n][2]) for n in reg if n != "K_INV"] + [(sc + 1, 1)]
    assert PR.untouched(P, img, out, written) is None


# ---------------------------------------------------------------------------- leftover LDS
POISONS = [pairingprobe.POISON, 0x00000000, 0xFFFFFFFF]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("curve", CURVES)
def test_lds_independent(curve, path):
    """One program holding every op, K_CYCRUN, K_COPY and K_INV, and the whole pairing checks, each
    run with the kernel's LDS pre-filled with three different words: the register file, fast_ok,
    values and verdicts must come back bit for bit the same (the shipped kernel starts on whatever
    LDS the workgroup before it left)."""
    r = PR.ref(curve)
    rng = random.Random("%d lds %s" % (F.SEED, curve))
    P = PR.new_prog(curve)
    g, sc = P.g, P.R_SCAL
    P.op("MUL", g(0), g(1), g(2))
    P.op2("SQR", g(0), None, g(3), "LL", g(1), g(1) + 6, g(4))
    P.code.append([G.K_CYCRUN, 3, g(0), g(5), g(8), 0, 0, 0, 0, 0])
    P.op("CONJ", g(0), None, g(6))
    P.op("LINE", g(0), g(1), g(7))
    for k in (1, 2, 3):
        P.op("FROB%d" % k, g(0), None, g(8 + k))
    P.op("INV_NORM", g(0), None, g(12))
    P.op("INV6_T", g(12), None, g(13))
    P.op("INV6_D", g(12), g(13), g(14))
    P.op("INV2_N", g(14), None, sc)
    P.inv(sc + 1, sc)
    P.op("INV2_FIN", g(14), sc + 1, g(15))
    P.op("INV6_FIN", g(13), g(15), g(12))
    P.op("INV12_FIN", g(0), g(12), g(14))
    P.op("LEVAL", g(1), g(1) + 4, g(15) + 6)
    P.copy(g(13), g(14))
    assert {ins[1] for ins in P.code if ins[0] == G.K_ROUND} | {G.OPNUM["SQR"], G.OPNUM["LL"], G.OPNUM["CYC"]} \
        == set(range(len(PR.OP_NAMES)))
    cases = []
    for _ in range(64):
        rows = [r.lp.row(rng.randrange(1 - r.b_mul, r.b_mul)) for _ in range(24)]
        cases.append([(g(0), [r.lp.jiggle(rng, l) for l in rows])])
    img = PR.images(P, cases)
    runs = [pairingprobe.run_program(curve, P.code, img, path == "generic", poison) for poison in POISONS]
    for out, fast in runs[1:]:
        assert fast == runs[0][1] and np.array_equal(out, runs[0][0]), "the result depends on the LDS left behind"
    pcs = pairing_cases(curve)
    xyzz = [r.lp.xyzz(A, la) + r.lp.xyzz(B, lb) for A, la, B, lb, _, _, _, _ in pcs]
    g2 = [g2_words(Q0, r) + g2_words(Q1, r) for _, _, _, _, Q0, Q1, _, _ in pcs]
    pruns = [pairingprobe.run_pairing(curve, xyzz, g2, [c[6] for c in pcs], path == "generic", poison)
             for poison in POISONS]
    for verdict, rows in pruns[1:]:
        assert verdict == pruns[0][0] and np.array_equal(rows, pruns[0][1]), "the pairing depends on the LDS left behind"


# ---------------------------------------------------------------------------- whole pairing checks
def g2_words(Q, r):
    W, R32, p = r.lp.W, r.lp.R32, r.p
    return [w for c in (Q[0][0], Q[0][1], Q[1][0], Q[1][1]) for w in F.to_words(c * R32 % p, W)]


def oracle_pairing(curve, P, Q):
    """e(P, Q) (cubed on BLS12-381, as the pairing program computes it) in tower order."""
    C = pc.CURVES[curve]
    if P is None or Q is None:
        return [1] + [0] * 11
    e = O.pairing(curve, pk.g1_to_bytes(P, C), pk.g2_to_bytes(Q, C))
    fb = C.fp_bytes
    return [int.from_bytes(e[i * fb:(i + 1) * fb], "big") for i in range(12)]


@functools.lru_cache(maxsize=None)
def pairing_cases(curve):
    """(A, lambda_A, B, lambda_B, Q0, Q1, q_inf flags, expected value) for the eight cases."""
    r = PR.ref(curve)
    C, T = r.lp.C, r.T
    rng = random.Random("%d run_pairing %s" % (F.SEED, curve))
    k = lambda: rng.randrange(1, C.r)       # noqa: E731
    lam = lambda: rng.randrange(2, r.p)     # noqa: E731
    g1 = lambda: pc.g1_mul(C.g1, k(), C)    # noqa: E731
    g2 = lambda: pc.g2_mul(C.g2, k(), C)    # noqa: E731
    tau = k()
    A = g1()
    tq, tb = pc.g2_mul(C.g2, tau, C), pc.g1_mul(A, tau, C)
    near = pc.g1_add(tb, C.g1, C)
    raw = [
        (g1(), g1(), g2(), g2(), (0, 0)),          # random pairs
        (tb, A, C.g2, tq, (0, 0)),                 # e([tau] A, G2) e(-A, [tau] G2) = 1: the KZG relation
        (near, A, C.g2, tq, (0, 0)),               # its near miss
        (None, g1(), g2(), g2(), (0, 0)),          # A at infinity
        (g1(), None, g2(), g2(), (0, 0)),          # B at infinity
        (g1(), g1(), g2(), g2(), (1, 0)),          # Q0 flagged at infinity
        (g1(), g1(), g2(), g2(), (0, 1)),          # Q1 flagged at infinity
        (None, None, g2(), g2(), (1, 1)),          # all of them
    ]
    out = []
    for Ap, Bp, Q0, Q1, inf in raw:
        e0 = oracle_pairing(curve, Ap, None if inf[0] else Q0)
        e1 = oracle_pairing(curve, None if Bp is None else pc.g1_neg(Bp, C), None if inf[1] else Q1)
        out.append((Ap, lam(), Bp, lam(), Q0, Q1, inf, T.f12mul(e0, e1)))
    return out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("curve", CURVES)
def test_run_pairing(curve, path):
    """k_pairing_check_par's body on XYZZ records with ZZ = lambda^2, ZZZ = lambda^3: the value
    e(A, Q0) e(-B, Q1) (cubed on BLS12-381) against the oracle, and the verdict.  A pair with its G1
    point at infinity or its q_inf flag set contributes one, so each of those cases alone leaves
    the other pair's value (verdict 0) and all of them together give one (verdict 1), as the true
    KZG relation does."""
    r = PR.ref(curve)
    cases = pairing_cases(curve)
    xyzz = [r.lp.xyzz(A, la) + r.lp.xyzz(B, lb) for A, la, B, lb, _, _, _, _ in cases]
    g2 = [g2_words(Q0, r) + g2_words(Q1, r) for _, _, _, _, Q0, Q1, _, _ in cases]
    verdict, rows = pairingprobe.run_pairing(curve, xyzz, g2, [c[6] for c in cases], path == "generic")
    one = r.T.one()
    want_verdict = [int(c[7] == one) for c in cases]
    assert want_verdict == [0, 1, 0, 0, 0, 0, 0, 1]
    for k, c in enumerate(cases):
        got = [r.elem(v) for v in r.values(rows[k])]
        assert got == c[7], "case %d: value differs from the oracle's" % k
        msg = r.check_round_rows(rows[k], c[7])
        assert msg is None, "case %d: %s" % (k, msg)
    assert verdict == want_verdict


# ---------------------------------------------------------------------------- public API
@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 1)
    yield c
    c.close()


def public_reference(curve, Pb, Qb):
    """What kzgmi_pairing returns: e(P, Q); the oracle gives e^3 on BLS12-381, so it is asked for
    e([3^-1 mod r] P, Q)^3 there (as tests/test_gpu_parity.py test_pairing_golden does)."""
    if curve == "bls12_381":
        inv3 = pow(3, -1, pc.CURVES[curve].r).to_bytes(32, "big")
        Pb = O.msm_g1(curve, Pb, inv3, 1)
    return O.pairing(curve, Pb, Qb)


@pytest.mark.parametrize("curve", CURVES)
def test_public_pairing_random(ctx, curve):
    C = pc.CURVES[curve]
    rng = random.Random("%d public pairing %s" % (F.SEED, curve))
    for _ in range(32):
        Pb = pk.g1_to_bytes(pc.g1_mul(C.g1, rng.randrange(1, C.r), C), C)
        Qb = O.g2_mul(curve, pk.g2_to_bytes(C.g2, C), rng.randrange(1, C.r))
        assert ctx.pairing(curve, Pb, Qb) == public_reference(curve, Pb, Qb)


@pytest.mark.parametrize("curve", CURVES)
def test_public_pairing_infinity_and_bilinearity(ctx, curve):
    C = pc.CURVES[curve]
    fb = C.fp_bytes
    one = (1).to_bytes(fb, "big") + bytes(11 * fb)
    rng = random.Random("%d public bilinear %s" % (F.SEED, curve))
    G1, G2 = pk.g1_to_bytes(C.g1, C), pk.g2_to_bytes(C.g2, C)
    assert ctx.pairing(curve, pk.g1_to_bytes(None, C), G2) == one
    assert ctx.pairing(curve, G1, pk.g2_to_bytes(None, C)) == one
    assert ctx.pairing(curve, pk.g1_to_bytes(None, C), pk.g2_to_bytes(None, C)) == one
    for _ in range(4):
        a = rng.randrange(1, C.r)
        Pb = pk.g1_to_bytes(pc.g1_mul(C.g1, rng.randrange(1, C.r), C), C)
        Qb = O.g2_mul(curve, G2, rng.randrange(1, C.r))
        aP = pk.g1_to_bytes(pc.g1_mul(pk.g1_from_bytes(Pb, C), a, C), C)
        aQ = O.g2_mul(curve, Qb, a)
        e = ctx.pairing(curve, aP, Qb)
        assert e == ctx.pairing(curve, Pb, aQ) and e != one
