"""The fused product-and-subtract forms of csrc/field29.hpp (mulsub29, sqrsub3_29) return, limb
for limb, what the two passes they replace return: a plain-Python product-scanning model with the
subtraction's limb added in every high column (tests/fusedref.py) against the same scan followed
by sub29's / sub3_29's carry pass, on both curves, at every call site of csrc/msm.hpp with its own
bias and input bounds.  Operands: k p and k p +- 1 up to each bound, bound - 1 (so a subtrahend
whose top limb exceeds the biased constant's), all-ones limbs, subtrahend 0, a = 0 (columns as
small as they get: a wrong borrow shows), and seeded random cases.  Both forms are also held to
the integer they stand for in its one normal form, and every column to 64 bits.

tools/gen_params29.py check_bounds carries the fused sites' assertions: the shipped roles pass,
a bias too small for a fused site's subtrahend does not."""
import pytest

import fieldref as F
import fusedref as R


@pytest.mark.parametrize("curve", F.CURVES)
@pytest.mark.parametrize("site", R.SITES)
def test_fused_equals_two_pass(curve, site):
    md = R.model(curve)
    kind, bias, cases = md.cases(site, R.NEDGE_RANDOM)
    p, n = md.p, md.N
    bounds = md.sites()[site][2]
    # the families the comparison rests on are really there
    assert any(c[0] == 0 for c in cases), "a = 0"
    assert any(c[2] == 0 for c in cases) and any(c[1] == 0 for c in cases), "subtrahend 0"
    sub = 2 if kind == "mulsub" else 1
    assert any(c[sub] == md.m.below(bounds[sub]) for c in cases), "subtrahend at bound - 1"
    assert any(c[0] == k * p + d for c in cases for k in (1, int(bounds[0]) - 1) for d in (-1, 0, 1))
    low = (1 << (29 * (n - 1))) - 1
    assert any(c[0] & low == low for c in cases) and any(c[sub] & low == low for c in cases), "all-ones limbs"
    if kind == "mulsub":  # the top limb wraps: the biased constant's top limb is below the subtrahend's
        assert any(F.limbs29(c[2], n)[-1] > md.H[bias][-1] for c in cases)
    for c in cases:
        got, want = md.fused(kind, bias, c), md.two_pass(kind, bias, c)
        assert got == want, "%s %s: fused %s, two passes %s, case %s" % (curve, site, got, want, F.hexs(c))
        assert got == F.limbs29(md.value(kind, bias, c), n), "not the normal form of the integer"
    assert md.peak < 1 << 64


@pytest.mark.parametrize("curve", F.CURVES)
def test_model_scan_is_montgomery(curve):
    """The scan without an addend is the Montgomery product fieldref checks the GPU against."""
    md = R.model(curve)
    fam = md.m.family(md.m.kmax)
    for a, b in zip(fam, reversed(fam)):
        assert md.scan(md.L(a), md.L(b)) == F.limbs29(md.m.mont(a, b), md.N)
        assert md.scan(md.L(a), None, square=True) == F.limbs29(md.m.mont(a, a), md.N)


@pytest.mark.parametrize("curve", F.CURVES)
def test_model_rejects_a_negative_addend(curve):
    """A subtrahend limb above the bias limb (an unnormalised subtrahend) is outside the contract:
    the model refuses it instead of wrapping."""
    md = R.model(curve)
    xl = md.L(md.p)
    xl[1] = md.H["B2"][1] + 1
    with pytest.raises(AssertionError):
        md.scan(md.L(1), md.L(1), addend=lambda i: md.H["B2"][i] - xl[i])


@pytest.mark.parametrize("idx", [0, 1])
def test_check_bounds_covers_the_fused_sites(idx):
    g = F.gen29
    name, p, n, r32, b, nkp, roles = g.CURVES[idx]
    g.check_bounds(p, n, nkp, roles)
    # a bias one step too small for what the fused site subtracts: the running sum's x under
    # ACC_P, its y under ACC_R, PPP + 2 Q2 under ACC_X3
    for role in ("ACC_P", "ACC_R", "ACC_X3"):
        bad = dict(roles, **{role: 1})
        with pytest.raises(AssertionError):
            g.check_bounds(p, n, nkp, bad)
