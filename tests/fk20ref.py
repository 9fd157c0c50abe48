"""Pure-Python restatement of the FK20 cell proof pipeline of csrc/fk20.hpp, in the exponent: under
a toy secret tau every G1 point is a scalar times the generator, so the whole pipeline is Fr
arithmetic on Python ints.  Test infrastructure only.

  p(X) = sum_{j < 4096} c_j X^j, omega = w^64 (order 128), S_m = [tau^m]_1
  proof_i = [floor(p / (X^64 - h_i^64))(tau)]_1 = P_{rev7(i)},  P_e = sum_{t < 63} omega^(e t) H_t
  H_t = sum_{b < 64} sum_{u = 0}^{62 - t} c_{64 (u + t + 1) + b} S_{64 u + b}
  a^(b) = (c_b, c_{64 + b}, .., c_{64 63 + b}, 0 x 64);  x^(b)[0] = S_b, x^(b)[128 - u] = S_{64 u + b}
  (u = 1 .. 62), infinity elsewhere;  hhat[pos] = sum_b DFT(a^(b))[pos] DFT(x^(b))[pos];
  H_t = IDFT(hhat)[t + 1]
"""
import cellref as K

R = K.R
N = 128
OMEGA128 = pow(K.OMEGA, K.CELL_N, R)  # w^64, order 128


def dft(vals, inverse=False):
    """[sum_j vals[j] omega^(k j) for k < 128], natural order in and out (inverse: omega^-1 and 1/128)."""
    assert len(vals) == N
    root = pow(OMEGA128, -1, R) if inverse else OMEGA128
    pw = [pow(root, e, R) for e in range(N)]
    out = [sum(v * pw[k * j % N] for j, v in enumerate(vals) if v) % R for k in range(N)]
    if inverse:
        ninv = pow(N, -1, R)
        out = [v * ninv % R for v in out]
    return out


def srs_scalars(tau):
    """tau^m for m < 4096: the discrete logarithms of the monomial SRS."""
    return K.powers(tau % R, K.BLOB_N)


def a_vec(coeffs, b):
    return [coeffs[64 * v + b] for v in range(64)] + [0] * 64


def x_vec(srs, b):
    x = [0] * N
    x[0] = srs[b]
    for u in range(1, 63):
        x[N - u] = srs[64 * u + b]
    return x


def scalars(coeffs):
    """ahat[pos][b] = DFT(a^(b))[pos]: what kzgmi_fk20_scalars_device writes (32 B big-endian at
    32 ((128 blob + pos) 64 + b))."""
    cols = [dft(a_vec(coeffs, b)) for b in range(64)]
    return [[cols[b][pos] for b in range(64)] for pos in range(N)]


def key_scalars(srs):
    """xhat[pos][b] = DFT(x^(b))[pos], in the exponent."""
    cols = [dft(x_vec(srs, b)) for b in range(64)]
    return [[cols[b][pos] for b in range(64)] for pos in range(N)]


def pointwise(ahat, xhat):
    return [sum(a * x for a, x in zip(ahat[pos], xhat[pos])) % R for pos in range(N)]


def h_full(coeffs, srs):
    """The whole inverse transform: entries 1 .. 63 are H_0 .. H_62, the others are discarded."""
    return dft(pointwise(scalars(coeffs), key_scalars(srs)), inverse=True)


def h_direct(coeffs, srs, t):
    return sum(coeffs[64 * (u + t + 1) + b] * srs[64 * u + b] for b in range(64) for u in range(63 - t)) % R


def shift(h):
    """D = (H_0, .., H_62, 0 x 65)."""
    return h[1:64] + [0] * 65


def proofs(coeffs, tau):
    """The 128 quotient scalars q_i(tau), cell order."""
    P = dft(shift(h_full(coeffs, srs_scalars(tau))))
    return [P[K.rev(i, 7)] for i in range(N)]


def quotient_scalar(coeffs, i, tau, p_tau=None):
    """q_i(tau) by the definition cellref.open_cell uses."""
    interp = K.poly_mod_coset(coeffs, i)
    den = (pow(tau, K.CELL_N, R) - K.coset_shift_pow64(i)) % R
    if p_tau is None:
        p_tau = K.horner(coeffs, tau)
    return (p_tau - K.horner(interp, tau)) * pow(den, -1, R) % R


def proof_bytes(q):
    """compress([q]_1): infinity is 0xC0 and 47 zero bytes."""
    return K.g1_of(q)
