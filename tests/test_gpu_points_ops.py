"""The G1 point layer, device function by device function and launcher by launcher.

The 32-bit XYZZ formulas of csrc/g1.hpp, the radix-2^29 Jacobian chain of the subgroup check with
its zero test, square root and encoding helpers (csrc/points.hpp), the GLV split (csrc/glv.hpp) and
the launchers of csrc/launch_io.hip are called through the test-only probe library
(tests/native/points_probe.hip, tests/pointsprobe.py) and compared with the plain big-integer model
of tests/pointref.py: the affine point a projective result stands for, with canonical coordinates and
ZZ^3 = ZZZ^2 (XYZZ) or normalised limbs below the bound of the branch taken (radix 29); bytes, flags,
error words and half scalars exactly.  The cases (P + Q, P + P, P - P and infinity on either side
under independently scaled coordinates, the order-3 points of BLS12-381, x = 1 and p - 1 on BN254,
coordinates at k = 0 and at their input bound, every multiple of p zero29 must recognise, members and
non-members of every cofactor order, every class of encoding, the Babai and Barrett boundaries of the
split) are generated and precondition-checked in pointref.py; none is dropped here.

test_op: one kernel launch per id, one case per thread.  test_stage: one probe call per id -- "each"
enqueues the shipped launcher once per case with n = 1 and that case's own error word, so every
case has its own verdict; "single" is one launch over at least 300 cases, which tests the indexing
(subgroup_check: 600 members with one non-member at index 0, 255, 256 or 599).  Every output buffer
has its exact size, is poisoned first and must leave its guard intact.
"""
import pytest

import pointref as R
import pointsprobe

pytestmark = pytest.mark.gpu

OPS = R.all_op_ids()
STAGES = R.all_stage_ids()


@pytest.mark.parametrize("curve,op", OPS, ids=["%s-%s" % (c, o) for c, o in OPS])
def test_op(curve, op):
    spec = R.op_of(curve, op)
    outs = pointsprobe.run(curve, op, [spec.encode(c) for c in spec.cases])
    assert len(outs) == len(spec.cases)
    bad = [(c, msg) for c, msg in ((c, spec.check(c, o)) for c, o in zip(spec.cases, outs)) if msg]
    assert not bad, "%s (%s): %d of %d cases wrong; first operands: %s -- %s" % (
        op, curve, len(bad), len(spec.cases), R.hexs(bad[0][0]), bad[0][1])


@pytest.mark.parametrize("curve,stage,mode", STAGES, ids=["%s-%s-%s" % s for s in STAGES])
def test_stage(curve, stage, mode):
    st = R.stage_of(curve, stage, mode)
    per_elem = mode == "each"
    out = st.call(pointsprobe, per_elem)
    assert all(out["guards"].values()) and out["guards"], out["guards"]
    bad = st.check(out, per_elem)
    assert not bad, "%s %s (%s): %d of %d cases wrong; first: %s" % (stage, mode, curve, len(bad), st.n, "; ".join(bad[:3]))
