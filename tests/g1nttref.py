"""Big-integer model of the power-of-two transforms over G1 (include/kzgmi.h, kzgmi_g1_ntt*), working in
the exponent as fk20ref.py does: a point k G is its discrete log k mod r, infinity is 0, [w] P is a product
mod r.  The definitions:

    forward:  out[j] = sum_i [w_n^(i j)] in[i]
    inverse:  out[i] = [n^-1] sum_j [w_n^(-i j)] in[j]
    bitrev:   the evaluation side (forward output, inverse input) holds point rev_logn(k) at index k

transform() is straight from nttref.dft; transform_staged() runs the stages the way csrc/g1ntt.hpp does:
radix-2 decimation in frequency in place (natural order in, bit-reversed out), the twiddle of butterfly k
of span `half` taken as w_{2^26}^(k << (25 - log2 half)) (negated mod 2^26 for the inverse), a scaling by
n^-1 per point behind the stages, and the gathers the order flags ask for before and after.
"""
import nttref as N

INVERSE, BITREV = N.INVERSE, N.BITREV
ROOT_BITS = N.ROOT_BITS
MAX_LOGN = 20  # G1NTT_MAX_LOGN


def transform(vals, logn, r, g, flags=0):
    return N.dft(vals, logn, r, g, inverse=bool(flags & INVERSE), bitrev=bool(flags & BITREV))


def stages(data, logn, r, g, inverse):
    """the logn stages in place: natural in, position p holds X[rev(p)]; the inverse unscaled.  Returns
    the number of scalar multiplications the kernel runs (twiddle != 1 and difference != infinity)."""
    n = 1 << logn
    w26 = N.root(r, g, ROOT_BITS)
    muls = 0
    for ls in range(logn - 1, -1, -1):
        half = 1 << ls
        for j in range(n // 2):
            k = j & (half - 1)
            i0 = ((j - k) << 1) | k
            a, b = data[i0], data[i0 + half]
            data[i0] = (a + b) % r
            d = (a - b) % r
            e = k << (ROOT_BITS - 1 - ls)
            if e and d:
                if inverse:
                    e = (1 << ROOT_BITS) - e
                d = d * pow(w26, e, r) % r
                muls += 1
            data[i0 + half] = d
    return muls


def transform_staged(vals, logn, r, g, flags=0):
    n = 1 << logn
    inverse = bool(flags & INVERSE)
    data = N.bitrev_perm(vals, logn) if inverse and flags & BITREV else list(vals)
    stages(data, logn, r, g, inverse)
    if inverse:
        ninv = (r - (r - 1) // n) % r  # as the kernel takes it: r - (r - 1) / n
        assert ninv * n % r == 1
        data = [x * ninv % r for x in data]
    if not inverse and flags & BITREV:
        return data
    return N.bitrev_perm(data, logn)
