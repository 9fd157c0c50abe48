"""The three GPU prime-field layers, op by op, at the edges of their bounds.

csrc/field.hpp (Fp<P>, all four moduli), csrc/field29.hpp (F29<Q>, with the record formulas
x29_add / x29_dbl / dbl_affine29 of csrc/msm.hpp) and csrc/lpfield.hpp (lane-parallel rows and
its XYZZ formulas) are called one device function per kernel through the test-only probe
library (tests/native/field_probe.hip, tests/fieldprobe.py) and compared with the plain
big-integer reference of tests/fieldref.py: exactly where the contract defines one integer,
by residue or affine point plus the documented output bound where the form is redundant.  The
operand families (k p and k p +- 1 up to each call site's bound, all-ones limbs, subtrahends at
their bias, quotient estimates on their rounding boundary, the exceptional point cases, 2048
seeded random cases) are generated and precondition-checked in fieldref.py; none is dropped on
the GPU side.  Each test is one probe launch.

Output bounds are the documented ones where the documentation holds; two comments did not and
were corrected with the bound's derivation (fieldref.py): lp_norm's carry v >> 29 lies in [-4, 3]
for |v| < 2^30.6, so its limbs land in [-4, 2^29 + 3), not [-2, 2^29 + 2) (lp_mul and lp_reduce,
whose last carry pass sees small limbs, are held to [-2, 2^29 + 2)); and the record
formulas' "x < 9.1p / 5.1p, y, zz, zzz < 1.01p" are BLS12-381's figures -- each curve is held to
what tools/gen_params29.py check_bounds' steps give for it (BN254, R29 / p ~ 169: y < 1.4p after
x29_add), and always to the record bounds.

What this pins: the semantics and the column / carry headroom of each inline function as
instantiated in the probe's own register-allocation context -- not that the copy inlined into
k_accumulate got the same registers; acc_loop29's mixed addition is written inline and is
covered through its primitives at the loop's bounds (the parity tests stay its end-to-end check).
"""
import pytest

import fieldprobe
import fieldref as F

pytestmark = pytest.mark.gpu

IDS = F.all_op_ids()


@pytest.mark.parametrize("layer,curve,op", IDS, ids=["%s-%s" % (c, o) for _, c, o in IDS])
def test_op(layer, curve, op):
    spec = F.ops_of(layer, curve)[op]
    mod = F.layer(layer, curve)
    outs = fieldprobe.run(curve, op, [spec.encode(c) for c in spec.cases], spec.pad_to)
    assert len(outs) == len(spec.cases)
    bad = [(c, msg) for c, msg in ((c, spec.check(c, o)) for c, o in zip(spec.cases, outs)) if msg]
    assert not bad, "%s (%s, p = %#x): %d of %d cases wrong; first operands: %s -- %s" % (
        op, mod.name, mod.p, len(bad), len(spec.cases), F.hexs(bad[0][0]), bad[0][1])
