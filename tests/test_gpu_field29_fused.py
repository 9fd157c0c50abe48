"""The fused product-and-subtract forms of csrc/field29.hpp on the GPU, op by op: mulsub29 and
sqrsub3_29 with each bias constant csrc/msm.hpp passes them, one kernel per op and curve
(tests/native/field29_fused_probe.hip), over the operand families of
tests/test_field29_fused_cpu.py plus 2048 seeded random cases, compared limb for limb with the
CPU model (tests/fusedref.py).  The contract is one integer in one normal form, so there is no
tolerance."""
import pytest

pytestmark = pytest.mark.gpu

import fieldref as F  # noqa: E402
import fusedref as R  # noqa: E402


@pytest.mark.parametrize("curve", F.CURVES)
@pytest.mark.parametrize("site", R.SITES)
def test_fused_op_matches_model(curve, site):
    import fusedprobe
    md = R.model(curve)
    kind, bias, cases = md.cases(site, R.NRANDOM)
    n = md.N
    got = fusedprobe.run(curve, site, [[w for v in c for w in md.L(v)] for c in cases], n)
    bad = []
    for c, out in zip(cases, got):
        want = md.fused(kind, bias, c)
        assert want == F.limbs29(md.value(kind, bias, c), n)
        if out != want:
            bad.append("case %s: got %s, want %s" % (F.hexs(c), [hex(x) for x in out], [hex(x) for x in want]))
    assert not bad, "%s %s: %d of %d cases differ\n%s" % (curve, site, len(bad), len(cases), "\n".join(bad[:5]))
