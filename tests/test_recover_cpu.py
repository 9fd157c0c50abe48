"""CPU checks of EIP-7594 cell extension and recovery: the reference of tests/recoverref.py against
plain polynomial arithmetic and the verifier's conventions (tests/cellref.py), and the new boundary
symbols."""
import random

import pytest

import cellref as K
import recoverref as RR

TAU = 0x7594_0000_1234_5678_9ABC_DEF1

RECOVER_SYMBOLS = ["kzgmi_compute_cells", "kzgmi_compute_cells_device", "kzgmi_compute_cells_device_async",
                   "kzgmi_recover_cells", "kzgmi_recover_cells_device", "kzgmi_recover_cells_device_async"]
RECOVER_METHODS = ["compute_cells", "compute_cells_async", "recover_cells", "recover_cells_async"]


@pytest.fixture(scope="module")
def blob():
    rng = random.Random(0x7594_C)
    return [rng.randrange(K.R) for _ in range(K.BLOB_N)]


@pytest.fixture(scope="module")
def cells(blob):
    return RR.compute_cells(blob)


def test_first_half_is_the_blob(blob, cells):
    assert len(cells) == K.NUM_CELLS and all(len(c) == K.CELL_N for c in cells)
    assert [v for c in cells[:64] for v in c] == blob
    assert all(K.rev(k, 13) == 2 * K.rev(k, 12) for k in (0, 1, 2, 100, 4095))


@pytest.mark.parametrize("i,j", [(64, 0), (127, 63), (3, 17), (90, 33)])
def test_cells_are_horner_values(blob, cells, i, j):
    coeffs = RR.blob_to_coeffs(blob)
    assert cells[i][j] == K.horner(coeffs, K.coset_points(i)[j])


@pytest.mark.parametrize("deg", [4095, 100])
def test_cells_match_the_verifier_convention(deg):
    """The cell of compute_cells is the cell cellref.open_cell opens (and the verifier accepts)."""
    rng = random.Random(deg)
    coeffs = [rng.randrange(K.R) for _ in range(deg + 1)]
    got = RR.coeffs_to_cells(coeffs)
    for i in (0, 77, 127):
        cell, _ = K.open_cell(coeffs, i, TAU)
        assert K.cell_to_ints(cell) == got[i]
    # and through the blob: the evaluation form of the same polynomial
    blob = [v for c in got[:64] for v in c]
    assert RR.blob_to_coeffs(blob) == coeffs + [0] * (K.BLOB_N - len(coeffs))
    assert RR.compute_cells(blob) == got


def _index_sets():
    rng = random.Random(64)
    some = rng.sample(range(K.NUM_CELLS), 64)
    return {"random64": some, "upper": list(range(64, 128)), "all-but-5": [i for i in range(128) if i != 5]}


@pytest.mark.parametrize("name", ["random64", "upper", "all-but-5"])
def test_reference_recovers(blob, cells, name):
    idx = _index_sets()[name]
    given = [cells[i] for i in idx]
    assert RR.consistent(idx, given)
    assert RR.recover_cells(idx, given) == cells
    assert RR.recover_coeffs(idx, given)[:K.BLOB_N] == RR.blob_to_coeffs(blob)


def test_reference_detects_inconsistency(cells):
    rng = random.Random(65)
    idx = rng.sample(range(K.NUM_CELLS), 65)
    given = [list(cells[i]) for i in idx]
    given[7][3] = (given[7][3] + 1) % K.R
    assert not RR.consistent(idx, given)
    with pytest.raises(ValueError):
        RR.recover_cells(idx, given)
    # with 64 cells any values are consistent: they define another polynomial
    assert RR.consistent(idx[:64], given[:64])
    other = RR.recover_cells(idx[:64], given[:64])
    assert other != cells and all(other[i] == g for i, g in zip(idx[:64], given[:64]))


def test_library_exports_recover_entry_points():
    import kzgmi
    lib = kzgmi.lib()
    for s in RECOVER_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in kzgmi.exported_symbols()
    for m in RECOVER_METHODS:
        assert callable(getattr(kzgmi.Context, m)), m
    assert callable(kzgmi.compute_cells) and callable(kzgmi.recover_cells)
    assert kzgmi.ABI_VERSION == 6 and lib.kzgmi_abi_version() == 6
