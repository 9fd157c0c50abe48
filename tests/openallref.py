"""Big-integer model of kzgmi_open_all (include/kzgmi.h, csrc/host_g1ntt.hip): all n = 2^logn openings of
p = sum_{i<m} c_i X^i on <w_n>, the FK20 single-proof construction, in the exponent (a point is its discrete
log to the base G1 under a toy tau; S_j = tau^j).

    proof_e = sum_{t<n-1} w_n^(e t) h_t,   h_t = sum_{j <= n-2-t} c_{t+1+j} S_j,   h_{n-1} = infinity
    a = (c_0 .. c_{n-1}, 0 x n);  x[0] = S_0, x[2n - u] = S_u (u = 1 .. n-2), infinity elsewhere
    h_t = IDFT_2n(DFT_2n(a) . DFT_2n(x))[t + 1],  t <= n - 2

open_all() runs every step the way the job does: the key (the staged forward transform of x, put in natural
order), ahat = DFT_2n(a / 2n) over Fr, the pointwise products, the unscaled inverse stages, the shift through
the bit reversal, the forward n-point transform, and ys as the forward Fr transform of the coefficients.
"""
import g1nttref as G
import nttref as N

BITREV = N.BITREV
MAX_LOGN = 19


def h_direct(coeffs, n, tau, r):
    c = list(coeffs) + [0] * (n - len(coeffs))
    return [sum(c[t + 1 + j] * pow(tau, j, r) for j in range(n - 1 - t)) % r for t in range(n - 1)] + [0]


def key(logn, tau, r, g):
    """DFT_2n(x) in natural order, as kzgmi_open_all_key_load leaves it"""
    n = 1 << logn
    x = [0] * (2 * n)
    for i in range(2 * n):
        u = (2 * n - i) & (2 * n - 1)
        if u + 1 < n:
            x[i] = pow(tau, u, r)
    G.stages(x, logn + 1, r, g, False)
    return N.bitrev_perm(x, logn + 1)


def open_all(coeffs, logn, tau, r, g, flags=0, xhat=None):
    """(proof exponents, ys) in the order of `flags`"""
    n, m = 1 << logn, len(coeffs)
    assert m <= n
    if xhat is None:
        xhat = key(logn, tau, r, g)
    inv2n = pow(2 * n, r - 2, r)
    a = [c * inv2n % r for c in coeffs] + [0] * (2 * n - m)
    ahat = N.dft(a, logn + 1, r, g)
    hhat = [s * p % r for s, p in zip(ahat, xhat)]
    G.stages(hhat, logn + 1, r, g, True)  # bit-reversed out, unscaled: the 1 / 2n is in ahat
    d = [hhat[N.rev(t + 1, logn + 1)] if t + 1 < n else 0 for t in range(n)]
    assert d == h_direct(coeffs, n, tau, r)
    proofs = G.transform_staged(d, logn, r, g, flags & BITREV)
    ys = N.dft(list(coeffs) + [0] * (n - m), logn, r, g, bitrev=bool(flags & BITREV))
    return proofs, ys
