"""CPU checks of the EIP-7594 cell front end: the reference of tests/cellref.py against plain
polynomial arithmetic and the oracle's pairing, the generated root of unity, and the new boundary
symbols."""
import os
import random
import re

import pytest

import cellref as K
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kzg-batch-verification-scheme_amd")
TAU = 0x7594_0000_1234_5678_9ABC_DEF1

CELL_SYMBOLS = ["kzgmi_cell_srs_load", "kzgmi_cell_srs_free", "kzgmi_cell_batch_challenge_device",
                "kzgmi_cell_interp_device", "kzgmi_verify_cell_batch", "kzgmi_verify_cell_batch_device",
                "kzgmi_verify_cell_batch_device_async"]
CELL_METHODS = ["load_cell_srs", "cell_batch_challenge", "cell_interp", "verify_cell_batch", "verify_cell_batch_async"]


@pytest.mark.parametrize("i", [0, 1, 64, 127])
def test_coset_identities(i):
    h = K.coset_shift(i)
    pts = K.coset_points(i)
    assert pts == [h * pow(K.OMEGA64, K.rev(j, 6), K.R) % K.R for j in range(K.CELL_N)]
    assert pow(h, K.CELL_N, K.R) == K.coset_shift_pow64(i)
    assert all(pow(x, K.CELL_N, K.R) == K.coset_shift_pow64(i) for x in pts)
    assert len(set(pts)) == K.CELL_N
    assert pow(K.OMEGA64, 64, K.R) == 1 and pow(K.OMEGA64, 32, K.R) == K.R - 1


def test_cosets_partition_the_extended_domain():
    seen = {K.coset_shift_pow64(i) for i in range(K.NUM_CELLS)}
    assert len(seen) == K.NUM_CELLS
    assert K.coset_points(0)[0] == 1 and K.coset_shift(0) == 1


@pytest.mark.parametrize("i", [0, 1, 64, 127])
def test_interpolation_forms_agree(i):
    rng = random.Random(7594 + i)
    coeffs = [rng.randrange(K.R) for _ in range(200)]
    interp = K.poly_mod_coset(coeffs, i)
    pts = K.coset_points(i)
    vals = [K.horner(coeffs, x) for x in pts]
    assert [K.horner(interp, x) for x in pts] == vals  # I reproduces the cell at all 64 points
    assert K.interpolate(i, vals) == interp
    assert K.interpolate_dit(i, vals) == interp


def test_open_cell_reproduces_the_polynomial():
    rng = random.Random(1)
    coeffs = [rng.randrange(K.R) for _ in range(K.BLOB_N)]
    cell, _ = K.open_cell(coeffs, 77, TAU)
    assert K.cell_to_ints(cell) == [K.horner(coeffs, x) for x in K.coset_points(77)]


def test_transcript_length():
    c48 = bytes([0xC0]) + bytes(47)
    cell = K.cell_from_ints([0] * K.CELL_N)
    for m, n in [(0, 0), (1, 1), (3, 7), (2, 65)]:
        msg = K.transcript([c48] * m, [0] * n, [5] * n, [cell] * n, [c48] * n)
        assert len(msg) == 48 + 48 * m + 2112 * n
        assert msg[:16] == b"RCKZGCBATCH__V1_"
        assert msg[16:48] == (4096).to_bytes(8, "big") + (64).to_bytes(8, "big") + m.to_bytes(8, "big") + n.to_bytes(8, "big")
    a = K.challenge([c48], [0], [1], [cell], [c48])
    assert 0 <= a < K.R and a != K.challenge([c48], [0], [2], [cell], [c48])


def _batch(n, seed):
    rng = random.Random(seed)
    polys = [[rng.randrange(K.R) for _ in range(100)] for _ in range(2)]
    cs = [K.commit(p, TAU) for p in polys]
    cidx = [k % 2 for k in range(n)]
    cells_i = [rng.randrange(K.NUM_CELLS) for _ in range(n)]
    opened = [K.open_cell(polys[c], i, TAU) for c, i in zip(cidx, cells_i)]
    return cs, cidx, cells_i, [o[0] for o in opened], [o[1] for o in opened]


def test_batch_equation_under_the_oracle_pairing():
    cs, cidx, cells_i, cells, proofs = _batch(5, 11)
    g1m, g2, t64 = K.toy_cell_srs(TAU)
    r = K.challenge(cs, cidx, cells_i, cells, proofs)
    A, Bc = K.expected_combination(cs, cidx, cells_i, cells, proofs, r, g1m)
    assert O.pairing_check(K.CURVE, A, Bc, g2, t64) is True
    vals = K.cell_to_ints(cells[3])
    vals[17] = (vals[17] + 1) % K.R
    bad = cells[:3] + [K.cell_from_ints(vals)] + cells[4:]
    A2, B2 = K.expected_combination(cs, cidx, cells_i, bad, proofs, r, g1m)
    assert A2 == A and B2 != Bc
    assert O.pairing_check(K.CURVE, A2, B2, g2, t64) is False


def test_root_of_unity_and_committed_constant():
    w = K.OMEGA
    assert pow(w, 4096, K.R) == K.R - 1
    assert w == pow(7, (K.R - 1) // 8192, K.R)
    with open(os.path.join(PKG, "csrc", "params_gen.hpp")) as f:
        src = f.read()
    frp = src[src.index("struct Bls12_381FrParams"):]
    frp = frp[:frp.index("\n};")]
    limbs = {}
    for name in ("ROOT4096_M", "ROOT8192_M"):
        m = re.search(name + r"\[N\] = \{([^}]*)\}", frp)
        v = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
        assert len(v) == 8
        limbs[name] = sum(x << (32 * i) for i, x in enumerate(v))
    assert limbs["ROOT8192_M"] == w * (1 << 256) % K.R  # Montgomery form
    assert limbs["ROOT4096_M"] == w * w * (1 << 256) % K.R
    assert "ROOT8192_M" not in src[src.index("struct Bn254FrParams"):]


def test_library_exports_cell_entry_points():
    import kzgmi
    lib = kzgmi.lib()
    for s in CELL_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in kzgmi.exported_symbols()
    for m in CELL_METHODS:
        assert callable(getattr(kzgmi.Context, m)), m
    assert callable(kzgmi.verify_cell_batch)
    assert kzgmi.ABI_VERSION == 6 and lib.kzgmi_abi_version() == 6
