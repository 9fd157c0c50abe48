"""Hand-made sorted lists for the row accumulation's arithmetic paths (tests/test_gpu_msm_rows_arith.py,
held to the model without a GPU by tests/test_row_arith_cpu.py): sign patterns, the degenerate buckets
whose first addition doubles or cancels, and a point whose x is a tiny residue in the radix-29
Montgomery domain.  Built with tests/msmcases.py's Entries at the stage tests' item length; seeded."""
import fieldref as F
import msmcases as MC
import msmref as R
from oracle.pyspec import curves as pc

L = 8           # the item length the stage tests force (tests/msmrowscases.py)
WBITS = 13
TOTAL = 2600    # entries: the size of the existing row test's lists (2 500 - 6 000)
PATTERNS = ["all_negative", "alternating", "mixed"]


def tiny_x_points(curve, n=2):
    """n curve points whose x is c / R29 mod p for the smallest c >= 1 that give a point: the
    kernels hold x as the residue c itself (or c + p), far below p 2^-22.  Not in the r-torsion
    subgroup in general, which the accumulation does not ask for."""
    C, M = pc.CURVES[curve], R.layers(curve)[0]
    p, out, c = C.p, [], 0
    assert p % 4 == 3
    rinv = pow(M.R, -1, p)
    while len(out) < n:
        c += 1
        x = c * rinv % p
        rhs = (pow(x, 3, p) + C.b) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs and y:
            out.append((x, y))
            assert pc.g1_on_curve(out[-1], C) and x * M.R % p == c
    return out


def small_pp_point(curve, P1):
    """A curve point Q whose first addition to P1 has PP = (q.x - x)^2 / R29 a residue just below the
    peel's threshold (csrc/field29.hpp peel_ok29, PEEL_LO): q.x = x + sqrt(t R29) for the first t
    under the threshold that gives a point.  None on a curve without the peel."""
    C, M = pc.CURVES[curve], R.layers(curve)[0]
    if "PEEL_LO" not in M.H:
        return None
    p = C.p
    rinv = pow(M.R, -1, p)
    t = M.H["PEEL_LO"] << (F.W29 * (M.N - 2))
    x1 = P1[0] * M.R % p
    while True:
        t -= 1
        s = pow(t * M.R % p, (p + 1) // 4, p)
        if s * s % p != t * M.R % p:
            continue
        for d in (s, p - s):
            x = (x1 + d) * rinv % p
            rhs = (pow(x, 3, p) + C.b) % p
            y = pow(rhs, (p + 1) // 4, p)
            if y * y % p == rhs and y:
                return (x, y)


def _signed(vals, pattern, at):
    """The values of a bucket that starts at list position `at` under a sign pattern."""
    if pattern == "all_negative":
        return [v | 1 for v in vals]
    if pattern == "alternating":
        return [(v & ~1) | ((at + i) & 1) for i, v in enumerate(vals)]
    return [(v | 1) if i == 0 else (v & ~1) for i, v in enumerate(vals)]     # a negative first entry


def arith_list(curve, pattern, total=TOTAL):
    """Buckets of 1, 2 and 3 entries (many of each: whole rows of them), one of every length up to L,
    one of 3 L + 2 entries (cut into 4 items and joined), then -- in the mixed list, under explicit
    signs -- (P, P) alone and with more behind it, (-P, -P), (P, -P) alone, (P, -P, Q), (-P, P, Q, Q),
    a sum that meets its next entry at the second addition, a pair whose PP is a residue under the
    peel's threshold (where the curve peels), and the tiny-x points as second entry (every sign
    pair), as first entry and between others -- each of these makes a wave take the generic body for
    its first addition; random short buckets up to `total`."""
    assert pattern in PATTERNS
    b = MC.Entries(curve, L)
    b.rng = MC.rng_of("rows arith", curve, pattern)
    some = b.some

    def bucket(vals, gap=0, keep=False):
        b.bucket(vals if keep else _signed(vals, pattern, len(b)), gap=gap)

    for n in (1, 2, 3) * 70:
        bucket(some(n), gap=int(b.rng.randrange(5) == 0))
    for n in range(1, L + 1):
        bucket(some(n), gap=1)
    bucket(some(3 * L + 2), gap=2)
    if pattern == "mixed":
        x, y, z = (v & ~1 for v in b.distinct(3))
        for vals in ([x, x], [x, x, y, z], [x ^ 1, x ^ 1], [x ^ 1, x ^ 1, y], [x, x ^ 1], [x ^ 1, x],
                     [x, x ^ 1, y], [x ^ 1, x, y, y], [x, x ^ 1, y, y ^ 1, z]):
            bucket(vals, gap=1, keep=True)
        s = b.v(R.add(b.point(x), b.point(y), curve))
        bucket([x, y, s, z], keep=True)                     # the doubling at the second addition
        bucket([x, y, s ^ 1, z], keep=True)                 # ... and O there, then a restart
        Qp = small_pp_point(curve, b.point(x))              # PP below the peel's threshold: both signs of both
        if Qp is not None:
            q = b.v(Qp)
            for first in (x, x ^ 1):
                for second in (q, q ^ 1):
                    bucket([first, second], keep=True)
                    bucket([first, second, z], gap=1, keep=True)
        for T in tiny_x_points(curve):
            t = b.v(T)
            for first in (y, y ^ 1):
                for second in (t, t ^ 1):
                    bucket([first, second], keep=True)
                    bucket([first, second, z, x ^ 1], gap=1, keep=True)
            bucket([t, y], keep=True)
            bucket([t ^ 1, t ^ 1, y], keep=True)
            bucket([t, t ^ 1, z], keep=True)
            bucket([x, z, t, y ^ 1, t ^ 1], keep=True)
    while len(b) < total - 1:
        bucket(some(min(b.rng.randrange(1, 4), total - 1 - len(b))), gap=int(b.rng.randrange(8) == 0))
    bucket(some(total - len(b)), gap=3)
    assert len(b) == total and b.key <= R.Win(WBITS).nbuckets
    return b


def classes(total):
    """A term list that plans the list: one class, one window, as many terms as entries."""
    return [[total, 0, 4, 1, 0, 4, 0, 0]]


def signs_hold(b, pattern):
    """What the pattern promises, read back from the list."""
    vals = [v & ~R.SV_FIRST for v in b.sval]
    if pattern == "all_negative":
        return all(v & 1 for v in vals)
    if pattern == "alternating":
        n = sum((v & 1) == (i & 1) for i, v in enumerate(vals))
        return n == len(vals)
    firsts = [v for v in b.sval if v & R.SV_FIRST]
    return sum(v & 1 for v in firsts) > len(firsts) * 3 // 4 and any(not v & 1 for v in vals)


def limb_top_is_tiny(curve, P):
    """x of P as the kernels hold it has no bits in its two top limbs."""
    M = R.layers(curve)[0]
    return (P[0] * M.R % M.p) >> (F.W29 * (M.N - 2)) == 0
