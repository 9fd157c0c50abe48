"""Pure-Python restatement of EIP-7594 (PeerDAS) compute_cells and recover_cells (the cells, not
their proofs) as csrc/recover.hpp implements them: Python ints only, the constants and the cell
order of cellref.py.  Test infrastructure only.

  w = 7^((r-1)/8192); a blob is p on dom[k] = (w^2)^rev12(k), k < 4096; cell i (i < 128), element j
  (j < 64), is p(w^rev13(64 i + j)): the extended blob is p on w^rev13(q), q < 8192.
  rev13(k) = 2 rev12(k) for k < 4096, so cells 0..63 are the blob; cells 64..127 are p on w dom[k].

recover_cells is the specification's route: the vanishing polynomial Z of the missing cells, E Z to
coefficients, E Z and Z on the coset shifted by 7, the pointwise quotient, back to coefficients.
"""
from cellref import CELL_N, BLOB_N, EXT_N, NUM_CELLS, OMEGA, R, coset_shift_pow64, rev

SHIFT = 7                        # the coset of the quotient: 7 is not a root of unity of order 8192
OMEGA2 = OMEGA * OMEGA % R       # order 4096: the blob's domain


def fft(vals, root):
    """[sum_m vals[m] root^(k m) for k < n], natural order in and out; root of order n = len(vals)."""
    n = len(vals)
    if n == 1:
        return list(vals)
    r2 = root * root % R
    ev, od = fft(vals[0::2], r2), fft(vals[1::2], r2)
    out = [0] * n
    x = 1
    for k in range(n // 2):
        t = x * od[k] % R
        out[k] = (ev[k] + t) % R
        out[k + n // 2] = (ev[k] - t) % R
        x = x * root % R
    return out


def ifft(vals, root):
    n = len(vals)
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in fft(vals, pow(root, -1, R))]


def bitrev_perm(vals):
    n = len(vals)
    bits = n.bit_length() - 1
    return [vals[rev(k, bits)] for k in range(n)]


def blob_to_coeffs(blob_ints):
    """The 4096 coefficients of p with p(dom[k]) = blob_ints[k]."""
    assert len(blob_ints) == BLOB_N
    return ifft(bitrev_perm(blob_ints), OMEGA2)


def coeffs_to_cells(coeffs):
    """All 128 cells (lists of 64 ints) of a polynomial of degree < 4096."""
    assert len(coeffs) <= BLOB_N
    ext = bitrev_perm(fft(list(coeffs) + [0] * (EXT_N - len(coeffs)), OMEGA))
    return [ext[CELL_N * i:CELL_N * (i + 1)] for i in range(NUM_CELLS)]


def compute_cells(blob_ints):
    return coeffs_to_cells(blob_to_coeffs(blob_ints))


def vanishing_poly(missing):
    """Coefficients in Y = X^64 of Z = prod over the missing cells i of (Y - h_i^64), low first."""
    z = [1]
    for i in missing:
        a = coset_shift_pow64(i)
        nz = [0] * (len(z) + 1)
        for d, c in enumerate(z):
            nz[d + 1] = (nz[d + 1] + c) % R
            nz[d] = (nz[d] - a * c) % R
        z = nz
    return z


def recover_coeffs(indices, cells):
    """The 8192 coefficients of (E Z) / Z, computed on the coset shifted by 7: for a consistent input
    the upper 4096 are zero and the lower are p.  indices: distinct, each < 128, 64 <= len <= 128."""
    assert len(indices) == len(cells) and 64 <= len(indices) <= NUM_CELLS
    assert len(set(indices)) == len(indices) and all(0 <= i < NUM_CELLS for i in indices)
    missing = [i for i in range(NUM_CELLS) if i not in set(indices)]
    zy = vanishing_poly(missing)
    zx = [0] * EXT_N                      # Z as a polynomial in X (degree 64 * len(missing) <= 4096)
    for d, c in enumerate(zy):
        zx[CELL_N * d] = c
    z_eval = fft(zx, OMEGA)               # natural order
    ext = [0] * EXT_N                     # E in cell order, the missing cells zero
    for i, cell in zip(indices, cells):
        ext[CELL_N * i:CELL_N * (i + 1)] = cell
    e_nat = bitrev_perm(ext)              # natural order: e_nat[e] = E(w^e)
    ez = ifft([a * b % R for a, b in zip(e_nat, z_eval)], OMEGA)
    sp = 1
    ez_s, z_s = [], []
    for m in range(EXT_N):
        ez_s.append(ez[m] * sp % R)
        z_s.append(zx[m] * sp % R)
        sp = sp * SHIFT % R
    ez_c, z_c = fft(ez_s, OMEGA), fft(z_s, OMEGA)
    q = ifft([a * pow(b, -1, R) % R for a, b in zip(ez_c, z_c)], OMEGA)
    sinv = pow(SHIFT, -1, R)
    sp = 1
    out = []
    for m in range(EXT_N):
        out.append(q[m] * sp % R)
        sp = sp * sinv % R
    return out


def consistent(indices, cells):
    """Some polynomial of degree < 4096 takes all the given values."""
    c = recover_coeffs(indices, cells)
    if any(c[BLOB_N:]):
        return False
    got = coeffs_to_cells(c[:BLOB_N])
    return all(got[i] == list(cell) for i, cell in zip(indices, cells))


def recover_cells(indices, cells):
    """All 128 cells of the polynomial of degree < 4096 through the given cells; ValueError if the
    input is inconsistent."""
    c = recover_coeffs(indices, cells)
    got = coeffs_to_cells(c[:BLOB_N])
    if any(c[BLOB_N:]) or any(got[i] != list(cell) for i, cell in zip(indices, cells)):
        raise ValueError("inconsistent cells")
    return got


def cells_to_bytes(cells):
    return b"".join(int(v).to_bytes(32, "big") for cell in cells for v in cell)


def blob_to_bytes(blob_ints):
    return b"".join(int(v).to_bytes(32, "big") for v in blob_ints)
