"""CPU side of the pairing interpreter tests (tests/test_gpu_pairing.py runs the same families on
the GPU): the plain reference of tests/pairingref.py against the generated tables and against
f12_pow, the magnitude bounds the interpreter rests on walked over the shipped bytecode, the
operand families' preconditions, and the probe's constants against the generated header."""
import os
import random
import re

import pytest

import fieldref as F
import pairingref as PR

G = PR.G
CURVES = F.CURVES
OPS = [(c, o) for c in CURVES for o in PR.OP_NAMES]
OP_IDS = ["%s-%s" % co for co in OPS]
STRUCT = {"bls12_381": "Bls", "bn254": "Bn"}


@pytest.fixture(scope="module")
def tables():
    return {c: PR.op_tables(c) for c in CURVES}


# ---------------------------------------------------------------------------- reference vs tables
@pytest.mark.parametrize("curve,op", OPS, ids=OP_IDS)
def test_reference_matches_tables(curve, op, tables):
    """On every case of the op's family the plain reference and the generated table agree mod p."""
    r = PR.ref(curve)
    prods, outs = tables[curve][op]
    K = G.consts(curve)
    assert PR.SHAPES[op] == G.op_shape(op, curve)
    for case in r.family(op):
        A, B = ([r.elem(v) for v in r.values(rows)] for rows in case)
        got = G.evaluate(prods, outs, A + [0] * 12, B + [0] * 12, K, r.p)
        assert got == r.T.op(op, A, B), (op, F.hexs(A), F.hexs(B))


@pytest.mark.parametrize("curve", CURVES)
def test_reference_matches_f12_pow(curve):
    """Frobenius maps, a whole inverse and the cyclotomic squaring against f12_pow / f12_mul."""
    r = PR.ref(curve)
    T, p = r.T, r.p
    rng = random.Random("%d f12_pow %s" % (F.SEED, curve))
    for f in ([rng.randrange(p) for _ in range(12)], [rng.randrange(p) for _ in range(6)] + [0] * 6):
        for k in (1, 2, 3):
            assert T.op("FROB%d" % k, f) == T.f12pow(f, p ** k), k
        inv = T.inverse(f)["INV12_FIN"]
        assert inv == T.f12pow(f, p ** 12 - 2)
        assert T.f12mul(f, inv) == T.one()
        g = T.cyclotomic(f)
        assert T.f12pow(g, p ** 4 - p ** 2 + 1) == T.one()      # in the cyclotomic subgroup
        assert T.op("CYC", g) == T.f12mul(g, g)
        assert T.op("CYC", f) != T.f12mul(f, f)                 # defined, but no square, elsewhere
    for vals in r.cyclotomic_values(4, rng):
        g = [r.elem(v) for v in vals]
        assert T.op("CYC", g) == T.op("SQR", g)
    assert T.inverse([0] * 12)["INV12_FIN"] == [0] * 12


# ---------------------------------------------------------------------------- bound walk
def _shipped(curve):
    P, res = PR.shipped_program(curve)
    flat = [v for ins in P.code for v in ins]
    assert flat == PR.parse_header_array("k%s_PROG" % STRUCT[curve]), "bilinear_gen.hpp holds another program"
    return P


@pytest.mark.parametrize("curve", CURVES)
def test_bound_walk(curve, tables):
    """The shipped bytecode keeps every factor form and output sum inside lp_mul's and lp_reduce's
    domain, inside the bound pairing_par.hpp states, and inside the accumulators."""
    P = _shipped(curve)
    worst = PR.bound_walk(curve, P.code, tables[curve])
    stated = PR.stated_output_bound()
    # the figures the bound rests on: sum |coef| of the largest output list times 1.5 p, and of the
    # largest factor form times 1.5 p (E, P and K operands are lp_mul outputs)
    big = max(sum(abs(c) for c in o.d.values()) for name in PR.OP_NAMES for o in tables[curve][name][1])
    assert worst["output"] <= big * 1.5 <= stated * 1.5
    if curve == "bn254":
        assert big == stated == 252, (big, stated)   # reached at its edge by BN254's MUL
    assert worst["factor"] <= 24 * 1.5


@pytest.mark.parametrize("curve", CURVES)
def test_bound_walk_rejects_low_head(curve, tables):
    """The same walk with HEAD lowered below the largest output sum must fail, and pass one above."""
    P = _shipped(curve)
    worst = PR.bound_walk(curve, P.code, tables[curve])
    need = int(worst["output"]).bit_length()  # smallest HEAD with 2^HEAD p above the largest sum
    assert need <= PR.ref(curve).lp.HEAD
    PR.bound_walk(curve, P.code, tables[curve], head=need)
    with pytest.raises(AssertionError, match="not below 2\\^%d p" % (need - 1)):
        PR.bound_walk(curve, P.code, tables[curve], head=need - 1)


@pytest.mark.parametrize("curve", CURVES)
def test_bound_walk_rejects_scaled_coefficient(curve, tables):
    """One coefficient of the largest MUL output list multiplied: the sum passes the stated bound."""
    P = _shipped(curve)
    stated = PR.stated_output_bound()
    prods, outs = tables[curve]["MUL"]
    k = max(range(len(outs)), key=lambda i: sum(abs(c) for c in outs[i].d.values()))
    total = sum(abs(c) for c in outs[k].d.values())
    atom, coef = max(outs[k].d.items(), key=lambda kv: abs(kv[1]))
    factor = (stated - total) // abs(coef) + 2          # the smallest multiple that lifts the sum past `stated`
    mutated = list(outs)
    mutated[k] = G.S({**outs[k].d, atom: coef * factor})
    assert sum(abs(c) for c in mutated[k].d.values()) > stated
    bad = dict(tables[curve], MUL=(prods, mutated))
    with pytest.raises(AssertionError, match="pairing_par.hpp states"):
        PR.bound_walk(curve, P.code, bad)


def test_bound_walk_rejects_unwritten_register(tables):
    """A program that reads a G register nothing wrote is refused by the walk."""
    P = PR.new_prog("bn254")
    P.op("MUL", P.g(0), P.g(1), P.g(2))
    with pytest.raises(AssertionError, match="before it is written"):
        PR.bound_walk("bn254", P.code, tables["bn254"])


# ---------------------------------------------------------------------------- operand preconditions
@pytest.mark.parametrize("curve,op", OPS, ids=OP_IDS)
def test_family_preconditions(curve, op, tables):
    r = PR.ref(curve)
    fam = r.family(op)
    wa, wb, _ = PR.SHAPES[op]
    assert len(fam) >= PR.NRANDOM + 2 * PR.NSIGNS and all(len(A) == wa and len(B) == wb for A, B in fam)
    vals = {v for A, B in fam for v in r.values(A + B)}
    for v in r.edge_values():
        assert v in vals
    assert max(vals) == r.b_mul - 1 and min(vals) == 1 - r.b_mul
    assert PR.family_forms_ok(curve, op, tables[curve])


# ---------------------------------------------------------------------------- static agreement
@pytest.mark.parametrize("curve", CURVES)
def test_static_agreement(curve, tables):
    """bilinear_gen.hpp, gen_bilinear.Prog, pairing_par.hpp's op enum and the probe's info() layout
    agree (source level: the built library is compared with the header in test_gpu_pairing.py)."""
    info = PR.header_info(curve)
    P, res = PR.shipped_program(curve)
    assert (info["NPROG"], info["R_RES"]) == (len(P.code), res)
    for k in ("R_K", "R_E", "R_P", "R_SCAL", "R_G", "NR"):
        assert info[k] == getattr(P, k), k
    assert info["R_P"] - info["R_E"] == 12 * G.num_lines(curve) and info["NR"] - info["R_G"] == 12 * P.NG
    for name in PR.OP_NAMES:
        prods, outs = tables[curve][name]
        assert (info[name + "_NP"], info[name + "_NO"]) == (len(prods), len(outs)), name
        assert PR.SHAPES[name][2] == len(outs)
    with open(os.path.join(F.PKG, "csrc", "pairing_par.hpp")) as f:
        par = f.read()
    enum = re.search(r"enum ParOp \{([^}]*)\}", par).group(1)
    assert [s.strip() for s in enum.split(",")] == ["OP_" + n for n in PR.OP_NAMES] + ["OP_COUNT"]
    kinds = dict(re.findall(r"(K_\w+) = (\d)", par[par.index("constexpr int K_ROUND"):][:200]))
    assert {k: int(v) for k, v in kinds.items()} == {k: getattr(G, k) for k in
                                                     ("K_ROUND", "K_ROUND2", "K_COPY", "K_INV", "K_CYCRUN")}
    with open(os.path.join(F.ROOT, "tests", "native", "pairing_probe.hip")) as f:
        probe = f.read()
    import pairingprobe
    head = re.search(r"const int head\[INFO_HEAD\] = \{([^}]*)\}", probe).group(1)
    head = [s.strip().replace("I::", "") for s in head.replace("\n", " ").split(",")]
    want = {"OP_COUNT": "OP_COUNT", "PAR_THREADS": "PAR_THREADS", "NL": "num_lines<Cv>()"}
    assert head == [want.get(n, n) for n in pairingprobe.INFO_HEAD]
    for suffix in ("NP", "NO"):
        lst = re.search(r"constexpr int k%s\[OP_COUNT\] = \{([^}]*)\}" % suffix, probe).group(1)
        assert re.findall(r"I::(\w+)_%s" % suffix, lst) == PR.OP_NAMES


@pytest.mark.parametrize("curve", CURVES)
def test_fast_round_widths_hold_the_lists(curve, tables):
    """par_load_consts only checks a fast list against the table slots FW_P / FW_O; par_round_fast
    reads the WL, WR, WO terms of its template arguments.  Every list of a fast op must fit those
    (a longer regenerated list would pass fast_ok and be read short), and FW_P / FW_O are exact."""
    with open(os.path.join(F.PKG, "csrc", "pairing_par.hpp")) as f:
        par = f.read()
    const = lambda n: int(re.search(r"constexpr int (?:\w+ = \d+, )*%s = (\d+)" % n, par).group(1))  # noqa: E731
    calls = re.findall(r"par_round_fast<Cv, OP_(\w+), (-1|OP_\w+), (\w+), (\w+), (\w+)>", par)
    widths = {}
    for op1, op2, wl, wr, wo in calls:
        w = tuple(int(x) if x.isdigit() else const(x) for x in (wl, wr, wo))
        assert widths.setdefault((op1, op2), w) == w
    assert set(widths) == {("MUL", "-1"), ("LL", "-1"), ("CYC", "-1"), ("SQR", "OP_LL")}
    longest = {}
    for name in ("MUL", "SQR", "CYC", "LL"):
        prods, outs = tables[curve][name]
        longest[name] = (max(len(L) for L, _ in prods), max(len(R_) for _, R_ in prods), max(len(o.d) for o in outs))
    for (op1, op2), w in widths.items():
        for name in [op1] + ([op2[3:]] if op2 != "-1" else []):
            assert all(n <= k for n, k in zip(longest[name], w)), (name, longest[name], w)
    assert max(max(v[:2]) for v in longest.values()) <= const("FW_P")
    assert max(v[2] for v in longest.values()) <= const("FW_O")
    if curve == "bn254":  # the widest lists are BN254's: the slots are exact there
        assert max(max(v[:2]) for v in longest.values()) == const("FW_P")
        assert max(v[2] for v in longest.values()) == const("FW_O")
