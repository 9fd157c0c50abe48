"""Big-integer model of the power-of-two transforms over Fr (include/kzgmi.h, kzgmi_fr_ntt*):

    w_n = g^((r-1)/n), g = 7 (BLS12-381) / 5 (BN254), n = 2^logn
    forward:  out[j] = sum_i in[i] (s w_n^j)^i
    inverse:  out[i] = s^-i n^-1 sum_j v[j] w_n^(-i j)
    bitrev:   the evaluation side (forward output, inverse input) holds point rev_logn(k) at index k

dft_naive is straight from these definitions; dft is the recursive radix-2 form; transform_planned runs
a pass plan of csrc/ntt_plan.hpp the way csrc/ntt.hpp does: sub-transforms that leave their digit
bit-reversed, twiddles and the shift folded into a pass's load, scaling folded into the last store, bit
reversal in the indices.  Values are Python ints.
"""

MODULUS = {
    "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    "bn254": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
}
GENERATOR = {"bls12_381": 7, "bn254": 5}
INVERSE, BITREV = 1, 2  # KZGMI_NTT_INVERSE, KZGMI_NTT_BITREV

# NTT_P_* of csrc/ntt_plan.hpp
P_READ_BE, P_SHIFT, P_SCALE, P_BITREV_IN, P_BITREV_OUT, P_WRITE_BE, P_TWIDDLE, P_LAST, P_INVERSE = (
    1, 2, 4, 8, 16, 32, 64, 128, 256)
ROOT_BITS = 26


def root(r, g, logn):
    return pow(g, (r - 1) >> logn, r)


def rev(x, bits):
    y = 0
    for _ in range(bits):
        y = (y << 1) | (x & 1)
        x >>= 1
    return y


def bitrev_perm(vals, logn):
    return [vals[rev(k, logn)] for k in range(1 << logn)]


def dft_naive(vals, logn, r, g, inverse=False, bitrev=False, shift=1):
    n = 1 << logn
    assert len(vals) == n
    w = root(r, g, logn)
    if not inverse:
        pts = [shift * pow(w, j, r) % r for j in range(n)]
        out = []
        for x in pts:
            acc = 0
            for c in reversed(vals):
                acc = (acc * x + c) % r
            out.append(acc)
        return bitrev_perm(out, logn) if bitrev else out
    v = bitrev_perm(vals, logn) if bitrev else list(vals)
    wi, ni, si = pow(w, r - 2, r), pow(n, r - 2, r), pow(shift, r - 2, r)
    out = []
    for i in range(n):
        x = pow(wi, i, r)
        acc = 0
        for c in reversed(v):
            acc = (acc * x + c) % r
        out.append(acc * ni % r * pow(si, i, r) % r)
    return out


def _fft(vals, w, r):
    n = len(vals)
    if n == 1:
        return list(vals)
    w2 = w * w % r
    even, odd = _fft(vals[0::2], w2, r), _fft(vals[1::2], w2, r)
    out = [0] * n
    x = 1
    for k in range(n // 2):
        t = x * odd[k] % r
        out[k] = (even[k] + t) % r
        out[k + n // 2] = (even[k] - t) % r
        x = x * w % r
    return out


def dft(vals, logn, r, g, inverse=False, bitrev=False, shift=1):
    """the same map as dft_naive in O(n log n)"""
    n = 1 << logn
    assert len(vals) == n
    w = root(r, g, logn)
    if not inverse:
        v, x = [], 1
        for c in vals:
            v.append(c * x % r)
            x = x * shift % r
        out = _fft(v, w, r)
        return bitrev_perm(out, logn) if bitrev else out
    v = bitrev_perm(vals, logn) if bitrev else list(vals)
    out = _fft(v, pow(w, r - 2, r), r)
    si, x = pow(shift, r - 2, r), pow(n, r - 2, r)
    res = []
    for c in out:
        res.append(c * x % r)
        x = x * si % r
    return res


def _dif(col, w, r):
    """radix-2 decimation in frequency, in place: natural order in, position p holds X[rev(p)]"""
    n = len(col)
    h = n // 2
    while h >= 1:
        wh = pow(w, n // (2 * h), r)  # w_{2h}
        for base in range(0, n, 2 * h):
            x = 1
            for kk in range(h):
                a, b = col[base + kk], col[base + kk + h]
                col[base + kk] = (a + b) % r
                col[base + kk + h] = (a - b) * x % r
                x = x * wh % r
        h //= 2
    return col


def transform_planned(vals, passes, logn, r, g, shift=1):
    """One transform of 2^logn values through `passes` (dicts with bits, lstride, lprev, tw_step, flags):
    pass 0 reads `vals`, every later pass the array the one before wrote; the last one's output is
    returned.  Mirrors k_ntt_pass of csrc/ntt.hpp index by index."""
    n = 1 << logn
    w26 = root(r, g, ROOT_BITS)
    data = list(vals)
    for p in passes:
        b, ls, lp, fl = p["bits"], p["lstride"], p["lprev"], p["flags"]
        assert b + ls + lp == logn
        inv, last = bool(fl & P_INVERSE), bool(fl & P_LAST)
        R, lt = 1 << b, logn - b
        wR = root(r, g, b)
        if inv:
            wR = pow(wR, r - 2, r)
        base = pow(shift, r - 2, r) if inv else shift
        out = list(data) if not last else [None] * n
        for colw in range(1 << lt):
            if last:
                kappa, h, lo = colw, rev(colw, lp), 0
            else:
                lo, h = colw & ((1 << ls) - 1), colw >> ls
                kappa = rev(h, lp)
            col = [0] * R
            for rm in range(R):
                if fl & P_BITREV_IN:
                    a, pos = rev(rm, b), (rev(lo, ls) << b) | rm
                else:
                    a, pos = rm, (((h << b) | rm) << ls) | lo
                x = data[pos]
                if (fl & P_SHIFT) and not inv:
                    x = x * pow(base, (a << ls) | lo, r) % r
                if fl & P_TWIDDLE:
                    e = a * kappa * p["tw_step"]
                    if inv:
                        e = -e % (1 << ROOT_BITS)
                    x = x * pow(w26, e, r) % r
                col[a] = x
            _dif(col, wR, r)
            for pp in range(R):
                x = col[pp]
                if last and not (fl & P_BITREV_OUT):
                    pos = kappa + (rev(pp, b) << lt)
                else:
                    pos = (((h << b) | pp) << ls) | lo
                if last and inv:
                    if fl & P_SHIFT:
                        x = x * pow(base, pos, r) % r
                    if fl & P_SCALE:
                        x = x * pow(n, r - 2, r) % r
                out[pos] = x
        data = out
    return data


def to_bytes(vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]
