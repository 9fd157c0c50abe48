"""Big-integer models of the opening scan (csrc/open.hpp): plain synthetic division, and the tiled
three-pass scan with the tile parameters as arguments.

For p = sum_{i<m} c_i X^i and a point z:  Q_m = 0, Q_i = c_i + z Q_{i+1};  y = p(z) = Q_0 and
(p - y) / (X - z) = sum_{1<=i<m} Q_i X^(i-1).
"""


def divide(coeffs, z, r):
    """(y, q): y = p(z) and the m - 1 coefficients of (p - y) / (X - z), lowest first."""
    m = len(coeffs)
    q = [0] * max(m - 1, 0)
    acc = 0
    for i in range(m - 1, -1, -1):
        acc = (coeffs[i] + z * acc) % r
        if i >= 1:
            q[i - 1] = acc
    return acc, q


def evaluate(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (c + x * acc) % r
    return acc


def _scan(vals, w, r):
    """The workgroup scan S_t = v_t + w S_{t+1} as the kernel takes it: log2(len) steps, step s adding
    w^(2^s) times the value 2^s places up."""
    n = len(vals)
    assert n & (n - 1) == 0
    v = list(vals)
    d, p = 1, w
    while d < n:
        v = [(v[t] + p * v[t + d]) % r if t + d < n else v[t] for t in range(n)]
        d, p = 2 * d, p * p % r
    return v


def divide_tiled(coeffs, z, r, run=16, block=256, span=256):
    """divide() in the kernel's three passes: runs of `run` coefficients, tiles of `block` runs, the
    tile aggregates scanned `span` at a time from the top; all three powers of two.  The coefficient
    array reads as zeros above m, so every run and tile is full."""
    m = len(coeffs)
    tile = run * block
    tiles = (m + tile - 1) // tile
    c = lambda i: coeffs[i] if i < m else 0  # noqa: E731
    z_run, z_tile = pow(z, run, r), pow(z, tile, r)

    def horner(lo, acc, out=None):
        for e in range(run - 1, -1, -1):
            i = lo + e
            if i >= m:
                continue
            acc = (c(i) + z * acc) % r
            if out is not None and i >= 1:
                out[i - 1] = acc
        return acc

    # pass 1: run values, tile aggregates
    runv = [[horner(b * tile + t * run, 0) for t in range(block)] for b in range(tiles)]
    tilev = [_scan(runv[b], z_run, r)[0] for b in range(tiles)]
    # pass 2: the carry into every tile, y
    tilec = [0] * tiles
    carry = 0
    base = (tiles + span - 1) // span * span
    while base > 0:
        base -= span
        v = [tilev[base + t] if base + t < tiles else 0 for t in range(span)]
        v[span - 1] = (v[span - 1] + z_tile * carry) % r
        s = _scan(v, z_tile, r)
        for t in range(span):
            if base + t < tiles:
                tilec[base + t] = s[t + 1] if t + 1 < span else carry
        carry = s[0]
    y = carry
    # pass 3: every run's true carry-in, the quotient
    q = [0] * max(m - 1, 0)
    for b in range(tiles):
        v = list(runv[b])
        v[block - 1] = (v[block - 1] + z_run * tilec[b]) % r
        s = _scan(v, z_run, r)
        for t in range(block):
            lo = b * tile + t * run
            if lo >= m:
                continue
            horner(lo, s[t + 1] if t + 1 < block else tilec[b], q)
    return y, q
