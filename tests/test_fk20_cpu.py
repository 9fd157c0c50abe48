"""CPU checks of the FK20 cell proof pipeline's definitions (tests/fk20ref.py, in the exponent under a
toy tau) against the quotient definition of tests/cellref.py, and of the C ABI's new entry points."""
import random

import pytest

import cellref as K
import fk20ref as F

TAU = 0x7594_0000_1234_5678_9ABC_DEF1


@pytest.fixture(scope="module")
def poly():
    rng = random.Random(0xF20)
    coeffs = [rng.randrange(K.R) for _ in range(K.BLOB_N)]
    srs = F.srs_scalars(TAU)
    return {"coeffs": coeffs, "srs": srs, "h": F.h_full(coeffs, srs)}


def test_vectors():
    coeffs = list(range(1, K.BLOB_N + 1))
    srs = [10_000 + m for m in range(K.BLOB_N)]
    for b in (0, 5, 63):
        a = F.a_vec(coeffs, b)
        assert a[:64] == [64 * v + b + 1 for v in range(64)] and a[64:] == [0] * 64
        x = F.x_vec(srs, b)
        assert x[0] == srs[b]
        assert [x[128 - u] for u in range(1, 63)] == [srs[64 * u + b] for u in range(1, 63)]
        assert x[1:66] == [0] * 65                         # S_m for m >= 4032 is never used
    assert [K.rev(i, 7) for i in (0, 1, 2, 64, 127)] == [0, 64, 32, 1, 127]


def test_dft_is_its_own_inverse():
    rng = random.Random(1)
    v = [rng.randrange(K.R) for _ in range(F.N)]
    assert F.dft(F.dft(v), inverse=True) == v
    assert F.dft([1] + [0] * 127) == [1] * 128
    assert F.dft([0, 1] + [0] * 126) == [pow(F.OMEGA128, k, K.R) for k in range(128)]


def test_h_equals_its_double_sum(poly):
    for t in (0, 31, 62):
        assert poly["h"][t + 1] == F.h_direct(poly["coeffs"], poly["srs"], t)


def test_discarded_entries_are_not_zero(poly):
    """Entry 0 and entries 66..127 of the inverse transform are wrapped-around sums, not zero (64
    and 65 are empty sums): the shift has to drop them before the forward transform."""
    h = poly["h"]
    assert h[0] != 0 and all(h[66:])
    assert h[64] == 0 and h[65] == 0
    assert F.shift(h)[:63] == h[1:64] and F.shift(h)[63:] == [0] * 65


def test_proofs_equal_the_quotient(poly):
    got = F.proofs(poly["coeffs"], TAU)
    p_tau = K.horner(poly["coeffs"], TAU)
    for i in (0, 1, 63, 64, 127):
        q = F.quotient_scalar(poly["coeffs"], i, TAU, p_tau)
        assert got[i] == q
        assert K.open_cell(poly["coeffs"], i, TAU)[1] == F.proof_bytes(q)


def test_low_degree_has_zero_quotients():
    rng = random.Random(2)
    coeffs = [rng.randrange(K.R) for _ in range(64)] + [0] * (K.BLOB_N - 64)
    assert F.proofs(coeffs, TAU) == [0] * 128
    x64 = [0] * K.BLOB_N
    x64[64] = 1
    assert F.proofs(x64, TAU) == [1] * 128


def test_symbols_and_methods():
    import kzgmi
    new = ["kzgmi_cell_pk_load", "kzgmi_cell_pk_free", "kzgmi_cell_pk_device_bytes",
           "kzgmi_compute_cells_and_proofs", "kzgmi_compute_cells_and_proofs_device",
           "kzgmi_compute_cells_and_proofs_device_async", "kzgmi_recover_cells_and_proofs",
           "kzgmi_recover_cells_and_proofs_device", "kzgmi_recover_cells_and_proofs_device_async",
           "kzgmi_fk20_scalars_device", "kzgmi_g1_fft128_device"]
    lib = kzgmi.lib()
    for s in new:
        assert s in kzgmi.exported_symbols(), s
        assert hasattr(lib, s), s
    assert kzgmi.ABI_VERSION == 6 and lib.kzgmi_abi_version() == 6
    for m in ("load_cell_proof_key", "compute_cells_and_proofs", "compute_cells_and_proofs_async",
              "recover_cells_and_proofs", "recover_cells_and_proofs_async", "fk20_scalars", "g1_fft128"):
        assert callable(getattr(kzgmi.Context, m)), m
    assert callable(kzgmi.compute_cells_and_proofs) and callable(kzgmi.recover_cells_and_proofs)
    assert kzgmi.CellProofKey.__name__ == "CellProofKey"
    assert lib.kzgmi_cell_pk_device_bytes(None) == 0
