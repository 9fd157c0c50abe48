"""The transforms over Fr without a GPU: the roots, the big-integer model against itself
(tests/nttref.py), the shipped pass plan (csrc/ntt_plan.hpp through tests/native/ntt_plan_probe.hip) for
every size and bound, the plan run by the model against the definitions, and the tie of the conventions
to the EIP-7594 model (tests/recoverref.py)."""
import itertools
import random

import pytest

import nttplanprobe as P
import nttref as N

CURVES = ["bls12_381", "bn254"]
FLAGS = [0, N.INVERSE, N.BITREV, N.INVERSE | N.BITREV]


@pytest.mark.parametrize("curve", CURVES)
def test_roots(curve):
    r, g = N.MODULUS[curve], N.GENERATOR[curve]
    assert pow(g, (r - 1) // 2, r) == r - 1  # g generates the whole 2-power subgroup
    for logn in range(1, 27):
        w = N.root(r, g, logn)
        assert pow(w, 1 << logn, r) == 1 and pow(w, 1 << (logn - 1), r) == r - 1, logn
    assert N.root(r, g, 0) == 1


def test_root_matches_the_cell_model():
    import cellref
    assert cellref.R == N.MODULUS["bls12_381"]
    assert cellref.OMEGA == N.root(cellref.R, 7, 13)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("flags", FLAGS)
def test_recursive_form_equals_the_definition(curve, flags):
    r, g = N.MODULUS[curve], N.GENERATOR[curve]
    rng = random.Random(100 + flags)
    for logn in range(0, 9):
        vals = [rng.randrange(r) for _ in range(1 << logn)]
        for shift in (1, rng.randrange(1, r)):
            kw = dict(inverse=bool(flags & N.INVERSE), bitrev=bool(flags & N.BITREV), shift=shift)
            assert N.dft(vals, logn, r, g, **kw) == N.dft_naive(vals, logn, r, g, **kw), (logn, shift)


def test_constants():
    c = P.constants()
    assert c["max_logn"] == 26 and c["min_pass_bits"] == 2
    assert c["min_tile_bits"] <= c["tile_bits"] <= c["max_tile_bits"]
    assert c["max_bits"] == c["tile_bits"] - 2  # a tile holds at least four columns of the widest pass
    assert c["max_passes"] == 13


def test_plan_structure_every_size_and_bound():
    B = P.constants()["max_bits"]
    for logn, bound in itertools.product(range(27), range(2, B + 1)):
        for flags, shift in itertools.product(FLAGS, (False, True)):
            passes, scratch = P.plan(logn, 1, flags, shift, bound)
            npass = max(1, -(-logn // bound))
            assert len(passes) == npass
            widths = [p["bits"] for p in passes]
            assert sum(widths) == logn and all(w <= bound for w in widths)
            assert max(widths) - min(widths) <= 1 and widths == sorted(widths, reverse=True)  # balanced, wider first
            prev = 0
            for k, p in enumerate(passes):
                assert p["lprev"] == prev and p["lstride"] == logn - prev - p["bits"]
                assert p["tw_step"] == (0 if k == 0 else 1 << (26 - prev - p["bits"]))
                assert bool(p["flags"] & N.P_TWIDDLE) == (k > 0)
                assert bool(p["flags"] & N.P_INVERSE) == bool(flags & N.INVERSE)
                assert bool(p["flags"] & N.P_LAST) == (k == npass - 1)
                assert bool(p["flags"] & N.P_READ_BE) == (k == 0)
                assert bool(p["flags"] & N.P_WRITE_BE) == (k == npass - 1)
                prev += p["bits"]
            first, last = passes[0]["flags"], passes[-1]["flags"]
            inv, rev = bool(flags & N.INVERSE), bool(flags & N.BITREV)
            assert bool(first & N.P_BITREV_IN) == (inv and rev) and bool(last & N.P_BITREV_OUT) == (rev and not inv)
            assert bool(last & N.P_SCALE) == (inv and logn > 0)
            assert bool((last if inv else first) & N.P_SHIFT) == shift
            for p in passes[1:-1]:  # nothing but twiddles is folded into a middle pass
                assert p["flags"] & ~(N.P_TWIDDLE | N.P_INVERSE) == 0
            assert scratch == (32 << logn if npass > 1 else 0)


def test_plan_refuses_bad_arguments():
    B = P.constants()["max_bits"]
    assert P.plan(27) is None
    assert P.plan(26, 2) is None and P.plan(26, 1) is not None
    assert P.plan(10, (1 << 16) + 1) is None and P.plan(10, 1 << 16) is not None
    assert P.plan(4, 1, 4) is None
    assert P.plan(4, 1, 0, False, 1) is None and P.plan(4, 1, 0, False, 11) is None
    assert P.plan(4, 1, 0, False, B) is not None
    assert P.plan(5, 0) == P.plan(5, 0)  # count 0 plans (the entry points enqueue nothing)
    assert P.plan(12, 7)[1] == 7 * 32 * 4096


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("flags", FLAGS)
def test_planned_transform_equals_the_definition(curve, flags):
    r, g = N.MODULUS[curve], N.GENERATOR[curve]
    rng = random.Random(200 + flags)
    B = P.constants()["max_bits"]
    kw = dict(inverse=bool(flags & N.INVERSE), bitrev=bool(flags & N.BITREV))
    for logn in range(0, 11):
        vals = [rng.randrange(r) for _ in range(1 << logn)]
        for shift in (1, rng.randrange(1, r)):
            want = N.dft_naive(vals, logn, r, g, shift=shift, **kw)
            for bound in sorted({2, 3, 5, B}):
                passes, _ = P.plan(logn, 1, flags, shift != 1, bound)
                assert N.transform_planned(vals, passes, logn, r, g, shift) == want, (logn, bound, shift)


@pytest.mark.parametrize("curve", CURVES)
def test_inverse_of_forward_is_the_identity(curve):
    r, g = N.MODULUS[curve], N.GENERATOR[curve]
    rng = random.Random(300)
    for logn in (0, 1, 5, 9):
        vals = [rng.randrange(r) for _ in range(1 << logn)]
        for bitrev, shift, bound in itertools.product((False, True), (1, rng.randrange(1, r)), (2, 3)):
            fwd, _ = P.plan(logn, 1, N.BITREV if bitrev else 0, shift != 1, bound)
            inv, _ = P.plan(logn, 1, N.INVERSE | (N.BITREV if bitrev else 0), shift != 1, bound)
            ev = N.transform_planned(vals, fwd, logn, r, g, shift)
            assert N.transform_planned(ev, inv, logn, r, g, shift) == vals
            assert N.dft(N.dft(vals, logn, r, g, False, bitrev, shift), logn, r, g, True, bitrev, shift) == vals


def test_forward_bitrev_is_the_cell_extension():
    """the forward BITREV transform at logn = 13 of a blob polynomial's coefficients, padded with zeros,
    is the blob's extended cells; the coset of w_8192 gives their second half"""
    import recoverref as RR
    r = N.MODULUS["bls12_381"]
    rng = random.Random(400)
    blob = [rng.randrange(r) for _ in range(4096)]
    coeffs = N.dft(blob, 12, r, 7, inverse=True, bitrev=True)
    assert coeffs == RR.blob_to_coeffs(blob)
    cells = [x for cell in RR.compute_cells(blob) for x in cell]
    assert N.dft(coeffs + [0] * 4096, 13, r, 7, bitrev=True) == cells
    assert cells[:4096] == blob
    assert N.dft(coeffs, 12, r, 7, bitrev=True, shift=N.root(r, 7, 13)) == cells[4096:]
