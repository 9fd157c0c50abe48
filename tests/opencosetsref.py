"""Big-integer model of kzgmi_open_cosets (include/kzgmi.h, csrc/host_g1ntt.hip, csrc/cosets.hpp): FK20
multi-proofs of p = sum_{i<m} c_i X^i, m <= N = 2^logN, on the K = 2^logk cosets of l = 2^logl points of the
n = K l-th roots of unity, in the exponent (a point is its discrete log to the base G1 under a toy tau;
S_j = tau^j).  R = N / l.

    h_e = w_n^e,  z_e = h_e^l = w_K^e,  coset e = { h_e w_l^j : j < l },  w_l = w_n^K
    proof_e = q_e(tau),  q_e = floor(p / (X^l - z_e)),  I_e = p mod (X^l - z_e)
    ys[e][j] = p(w_n^(e + K j))
    proof_e = sum_{t<R-1} w_K^(e t) H_t,   H_t = sum_{b<l} sum_{u <= R-2-t} c_{l(u+t+1)+b} S_{l u + b}

    a^(b) = (c_b, c_{l+b}, .., c_{l(R-1)+b}, 0 x R);  x^(b)[0] = S_b, x^(b)[2R - u] = S_{l u + b} (u = 1 .. R-2)
    hhat[pos] = sum_b DFT_2R(a^(b))[pos] DFT_2R(x^(b))[pos];  H_t = IDFT_2R(hhat)[t + 1]

open_cosets() runs every step the way the job does: the key (the staged forward transforms of the l vectors
x^(b), each put in natural order), the strided pad with 1 / 2R folded in, the Fr transforms, the pointwise
sums, the unscaled inverse stages, the shift through the bit reversal with its padding to K, the forward
K-point transform, and ys as the forward Fr transform of the coefficients padded to n, gathered coset-major.
"""
import g1nttref as G
import nttref as N

BITREV = N.BITREV
MAX_LOGN = 19         # logN, and count * N <= 2^19
MAX_LOG_POINTS = 20   # count * K * l <= 2^20


def divide_coset(coeffs, l, z, r):
    """(q, I): p = q (X^l - z) + I, deg I < l, by synthetic division"""
    c = list(coeffs)
    q = [0] * max(0, len(c) - l)
    for i in range(len(c) - 1, l - 1, -1):
        q[i - l] = c[i]
        c[i - l] = (c[i - l] + z * c[i]) % r
    return q, c[:l]


def h_direct(coeffs, logN, logl, tau, r):
    N_, l = 1 << logN, 1 << logl
    R = N_ >> logl
    c = list(coeffs) + [0] * (N_ - len(coeffs))
    return [sum(c[l * (u + t + 1) + b] * pow(tau, l * u + b, r) for b in range(l) for u in range(R - 1 - t)) % r
            for t in range(max(0, R - 1))]


def key(logN, logl, tau, r, g):
    """DFT_2R(x^(b)) for every b, each in natural order: key[b][pos]"""
    l, R = 1 << logl, 1 << (logN - logl)
    out = []
    for b in range(l):
        x = [0] * (2 * R)
        for i in range(2 * R):
            u = (2 * R - i) & (2 * R - 1)
            if u + 1 < R:
                x[i] = pow(tau, l * u + b, r)
        G.stages(x, logN - logl + 1, r, g, False)
        out.append(N.bitrev_perm(x, logN - logl + 1))
    return out


def open_cosets(coeffs, logN, logl, logk, tau, r, g, flags=0, xhat=None):
    """(proof exponents, ys) of one polynomial in the order of `flags`: K proofs and K l evaluations"""
    N_, l, K, m = 1 << logN, 1 << logl, 1 << logk, len(coeffs)
    logr2 = logN - logl + 1
    R = N_ >> logl
    assert m <= N_ and logl <= logN and logk >= logN - logl
    if xhat is None:
        xhat = key(logN, logl, tau, r, g)
    inv2r = pow(2 * R, r - 2, r)
    c = list(coeffs) + [0] * (N_ - m)
    hhat = [0] * (2 * R)
    for b in range(l):
        a = [c[l * u + b] * inv2r % r for u in range(R)] + [0] * R
        ahat = N.dft(a, logr2, r, g)
        for pos in range(2 * R):
            hhat[pos] = (hhat[pos] + ahat[pos] * xhat[b][pos]) % r
    G.stages(hhat, logr2, r, g, True)  # bit-reversed out, unscaled: the 1 / 2R is in the scalars
    d = [hhat[N.rev(j + 1, logr2)] if j + 1 < R else 0 for j in range(K)]
    assert d[:max(0, R - 1)] == h_direct(coeffs, logN, logl, tau, r)
    proofs = G.transform_staged(d, logk, r, g, flags & BITREV)
    logn = logk + logl
    y = N.dft(list(coeffs) + [0] * ((1 << logn) - m), logn, r, g, bitrev=bool(flags & BITREV))
    if not flags & BITREV:
        y = [y[e + K * j] for e in range(K) for j in range(l)]
    return proofs, y
