"""Pure-Python restatement of EIP-7594 (PeerDAS) verify_cell_kzg_proof_batch as csrc/cell.hpp
implements it: hashlib and Python ints; G1 / G2 arithmetic from the C oracle.  Test infrastructure
only.

  w = 7^((r-1)/8192); cell i (0 <= i < 128) holds p at w^rev13(64 i + j) = h_i * w64^rev6(j), j < 64,
  with h_i = w^rev7(i) and w64 = w^128; h_i^64 = (w^64)^rev7(i)
  I_k = p_k mod (X^64 - h^64): c_m = h^-m / 64 * sum_j e_j w64^(-rev6(j) m)
  r = int_be(SHA256("RCKZGCBATCH__V1_" || be64(4096) || be64(64) || be64(m) || be64(n) || C_0 .. C_{m-1}
        || for k < n: be64(commitment_indices[k]) || be64(cell_indices[k]) || cells[k] || proofs[k])) mod r
  e(sum r^k pi_k, [tau^64]_2) = e(sum r^k C_k + sum r^k h_k^64 pi_k - [sum r^k I_k(tau)]_1, [1]_2)
"""
import hashlib

from oracle import oracle as O
from oracle.pyspec import curves as pc
from oracle.pyspec import kzg as pk

CURVE = "bls12_381"
R = pc.CURVES[CURVE].r
BLOB_N = 4096          # FIELD_ELEMENTS_PER_BLOB
EXT_N = 8192           # FIELD_ELEMENTS_PER_EXT_BLOB
CELL_N = 64            # FIELD_ELEMENTS_PER_CELL
NUM_CELLS = 128        # CELLS_PER_EXT_BLOB
CELL_BYTES = 32 * CELL_N
CELL_TAG = b"RCKZGCBATCH__V1_"

OMEGA = pow(7, (R - 1) // EXT_N, R)
OMEGA64 = pow(OMEGA, NUM_CELLS, R)  # order 64
INV64 = pow(CELL_N, -1, R)


def rev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def coset_shift(i):
    """h_i = w^rev7(i)."""
    return pow(OMEGA, rev(i, 7), R)


def coset_shift_pow64(i):
    """h_i^64 = (w^64)^rev7(i)."""
    return pow(pow(OMEGA, CELL_N, R), rev(i, 7), R)


def coset_points(i):
    """The 64 points of cell i, in the cell's element order."""
    return [pow(OMEGA, rev(CELL_N * i + j, 13), R) for j in range(CELL_N)]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def interpolate(i, vals):
    """The 64 coefficients of I with I(coset_points(i)[j]) = vals[j]: the closed form."""
    hinv = pow(coset_shift(i), -1, R)
    winv = pow(OMEGA64, -1, R)
    out = []
    for m in range(CELL_N):
        s = sum(e * pow(winv, rev(j, 6) * m, R) for j, e in enumerate(vals)) % R
        out.append(pow(hinv, m, R) * INV64 % R * s % R)
    return out


def interpolate_dit(i, vals):
    """interpolate() the way k_cell_fold_intt computes it: the cell's bit-reversed element order is
    the input order of a decimation-in-time transform, so six radix-2 stages run on vals as they
    are (root w64^-1), then the scale by h^-m / 64."""
    x = list(vals)
    winv = pow(OMEGA64, -1, R)
    half = 1
    while half < CELL_N:
        y = list(x)
        for t in range(CELL_N):
            k = t & (half - 1)
            w = pow(winv, k * (CELL_N // (2 * half)), R)
            if t & half:
                y[t] = (x[t - half] - w * x[t]) % R
            else:
                y[t] = (x[t] + w * x[t + half]) % R
        x = y
        half *= 2
    hinv = pow(coset_shift(i), -1, R)
    return [pow(hinv, m, R) * INV64 % R * x[m] % R for m in range(CELL_N)]


def poly_mod_coset(coeffs, i):
    """p mod (X^64 - h_i^64): X^(64 q + m) -> (h^64)^q X^m."""
    a = coset_shift_pow64(i)
    out = [0] * CELL_N
    aq = 1
    for q in range(0, len(coeffs), CELL_N):
        for m, c in enumerate(coeffs[q:q + CELL_N]):
            out[m] = (out[m] + aq * c) % R
        aq = aq * a % R
    return out


def cell_from_ints(vals):
    assert len(vals) == CELL_N
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def cell_to_ints(cell):
    assert len(cell) == CELL_BYTES
    return [int.from_bytes(cell[32 * j:32 * j + 32], "big") for j in range(CELL_N)]


def transcript(commitments, commitment_indices, cell_indices, cells, proofs):
    """commitments: the m unique 48-byte encodings; the other four lists have n entries."""
    m, n = len(commitments), len(cells)
    msg = CELL_TAG + BLOB_N.to_bytes(8, "big") + CELL_N.to_bytes(8, "big") + m.to_bytes(8, "big") + n.to_bytes(8, "big")
    msg += b"".join(commitments)
    for ci, ce, cell, p in zip(commitment_indices, cell_indices, cells, proofs):
        msg += ci.to_bytes(8, "big") + ce.to_bytes(8, "big") + cell + p
    assert len(msg) == 48 + 48 * m + 2112 * n
    return msg


def challenge(commitments, commitment_indices, cell_indices, cells, proofs):
    msg = transcript(commitments, commitment_indices, cell_indices, cells, proofs)
    return int.from_bytes(hashlib.sha256(msg).digest(), "big") % R


def powers(r, n):
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * r % R
    return out


def aggregate(cell_indices, cells, r):
    """c_m of sum_k r^k I_k."""
    agg = [0] * CELL_N
    for rk, i, cell in zip(powers(r, len(cells)), cell_indices, cells):
        for m, c in enumerate(interpolate_dit(i, cell_to_ints(cell))):
            agg[m] = (agg[m] + rk * c) % R
    return agg


def g1_of(k):
    """compress(k G1), 48 bytes."""
    return O.g1_compress(CURVE, O.g1_mul_gen(CURVE, (k % R).to_bytes(32, "big"), 1), 1)


def commit(coeffs, tau):
    return g1_of(horner(coeffs, tau))


def open_cell(coeffs, i, tau):
    """(cell, proof48) of a valid opening of p on coset i under the toy secret tau:
    I = p mod (X^64 - h^64), proof = ((p(tau) - I(tau)) / (tau^64 - h^64)) G1."""
    interp = poly_mod_coset(coeffs, i)
    cell = cell_from_ints([horner(interp, x) for x in coset_points(i)])
    den = (pow(tau, CELL_N, R) - coset_shift_pow64(i)) % R
    q = (horner(coeffs, tau) - horner(interp, tau)) * pow(den, -1, R) % R
    return cell, g1_of(q)


def decompress(points48):
    rc, out = O.g1_decompress(CURVE, b"".join(points48), len(points48))
    assert rc == 0
    return out


def toy_cell_srs(tau):
    """(g1_monomial: [tau^m]_1 for m < 64, 64 x 96 B; [1]_2; [tau^64]_2)."""
    C = pc.CURVES[CURVE]
    g2 = pk.g2_to_bytes(C.g2, C)
    scal = b"".join(t.to_bytes(32, "big") for t in powers(tau % R, CELL_N))
    return O.g1_mul_gen(CURVE, scal, CELL_N), g2, O.g2_mul(CURVE, g2, pow(tau, CELL_N, R))


def expected_combination(commitments, commitment_indices, cell_indices, cells, proofs, r, g1_monomial):
    """(A, B) = (sum r^k pi_k,  sum r^k C_k + sum r^k h_k^64 pi_k - sum_m c_m [tau^m]_1), 96-byte
    encodings, through the oracle's MSM."""
    n = len(cells)
    rk = powers(r, n)
    pi = decompress(proofs)
    cm = decompress([commitments[i] for i in commitment_indices])
    be = lambda xs: b"".join((x % R).to_bytes(32, "big") for x in xs)  # noqa: E731
    A = O.msm_g1(CURVE, pi, be(rk), n)
    agg = aggregate(cell_indices, cells, r)
    scal = rk + [x * coset_shift_pow64(i) for x, i in zip(rk, cell_indices)] + [-c for c in agg]
    Bc = O.msm_g1(CURVE, cm + pi + g1_monomial, be(scal), 2 * n + CELL_N)
    return A, Bc
