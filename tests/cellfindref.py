"""Pure-Python reference of the search for a rejected cell batch's invalid cells (csrc/host_find.hip,
include/kzgmi.h): the counter-mode randomisers, the combination of an index range and one cell's
validity.  hashlib and Python ints over tests/cellref.py; G1 sums and pairings from the C oracle.
Test infrastructure only.

  r_k = int_be(SHA256(seed || le64(k))[0:16]) >> 1, 1 if that is 0          (k: the global index)
  A_g = sum_{k in g} r_k pi_k
  B_g = sum_{k in g} r_k C_{cidx[k]} + sum_{k in g} (r_k h_k^64) pi_k - sum_{m < 64} c_m(g) [tau^m]_1
  c_m(g) = sum_{k in g} r_k coef_k[m],  coef_k = the 64 coefficients of I_k
  cell k is valid iff e(pi_k, [tau^64]_2) = e(C_k + h_k^64 pi_k - [I_k(tau)]_1, [1]_2)
"""
import hashlib

import cellref as K
from oracle import oracle as O

R = K.R


def randomizer(seed, i):
    v = int.from_bytes(hashlib.sha256(bytes(seed) + int(i).to_bytes(8, "little")).digest()[:16], "big") >> 1
    return v or 1


_COEFFS = {}


def coeffs(cell_index, cell):
    """The 64 coefficients of the cell's interpolation polynomial (memoised: ranges overlap)."""
    key = (cell_index, cell)
    if key not in _COEFFS:
        _COEFFS[key] = K.interpolate_dit(cell_index, K.cell_to_ints(cell))
    return _COEFFS[key]


def _be(xs):
    return b"".join((x % R).to_bytes(32, "big") for x in xs)


def combination(weights, commitments, commitment_indices, cell_indices, cells, proofs, g1_monomial):
    """K.expected_combination with the given weights in place of the powers of r: (A, B) as 96-byte
    encodings, through the oracle's MSM."""
    n = len(cells)
    pi = K.decompress(proofs)
    cm = K.decompress([commitments[i] for i in commitment_indices])
    A = O.msm_g1(K.CURVE, pi, _be(weights), n)
    agg = [0] * K.CELL_N
    for w, i, cell in zip(weights, cell_indices, cells):
        for m, c in enumerate(coeffs(i, cell)):
            agg[m] = (agg[m] + w * c) % R
    scal = list(weights) + [w * K.coset_shift_pow64(i) for w, i in zip(weights, cell_indices)] + [-c for c in agg]
    B = O.msm_g1(K.CURVE, cm + pi + g1_monomial, _be(scal), 2 * n + K.CELL_N)
    return A, B


def range_combination(seed, offset, lo, hi, commitments, commitment_indices, cell_indices, cells, proofs, g1_monomial):
    """(A_g, B_g) of the cells [lo, hi) of a batch whose first cell has global index offset."""
    w = [randomizer(seed, offset + k) for k in range(lo, hi)]
    return combination(w, commitments, commitment_indices[lo:hi], cell_indices[lo:hi], cells[lo:hi], proofs[lo:hi],
                       g1_monomial)


_VALID = {}


def cell_valid(commitment, cell_index, cell, proof, toy):
    """One cell's validity: the n = 1 combination with weight 1 through the oracle's pairing check
    (memoised: the oracle's pairing takes ~0.2 s and tests ask about the same cells again).
    toy: (g1_monomial, [1]_2, [tau^64]_2)."""
    key = (commitment, cell_index, cell, proof, toy)
    if key not in _VALID:
        A, B = combination([1], [commitment], [0], [cell_index], [cell], [proof], toy[0])
        _VALID[key] = O.pairing_check(K.CURVE, A, B, toy[1], toy[2])
    return _VALID[key]
