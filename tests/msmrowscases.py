"""The hand-made sorted list of the row accumulation's stage tests (tests/test_gpu_msm_rows.py,
held to the model without a GPU by tests/test_msm_rows_cpu.py), built with tests/msmcases.py's
helpers: the order inside every bucket is fixed, everything is seeded."""
import msmcases as MC
import msmref as R

L = 8           # the item length the stage tests force (MsmTuning::row_len; 256 as shipped)
WBITS = 13
TOTAL = 5000    # entries: the plan launches two blocks for it, and the list makes some 40 rows


def rows_list(curve, total=TOTAL):
    """Buckets of 1, 2, L, L + 1 and 2 L + 1 entries; empty buckets between full ones; the in-item
    doubling at offset 1, at the last offset of an item, and in the second piece of a cut bucket;
    P + (-P) and then more entries (a run through O); items that sum to O, whole and as a piece of a
    cut bucket; negated entries (every random value carries a random sign); buckets cut into 4 and 6
    items, one of them with equal pieces (the join's doubling) and one with cancelling pieces; random
    short buckets up to `total`, which is no multiple of 64 items: the last row is not full and the
    rows between the classes mix lengths."""
    b = MC.Entries(curve, L)
    some, curve_add = b.some, lambda x, y: R.add(b.point(x), b.point(y), curve)
    for n in (1, 2, L, L + 1, 2 * L + 1):
        b.bucket(some(n), gap=2)                                # (gap: empty buckets in front)
    x, y, z = b.distinct(3)
    b.bucket([x, x] + some(3), gap=1)                           # doubling at offset 1
    s = b.v(curve_add(x, y))
    b.bucket([x, y, s], gap=3)                                  # doubling at the item's last offset
    b.bucket([x, y, s ^ 1, z], gap=1)                           # ... its negation: O at offset 2, then on
    b.bucket([x, x ^ 1, y, z])                                  # P + (-P), then more entries
    b.bucket([x, x ^ 1])                                        # an item that sums to O
    b.bucket([x, y, y ^ 1, x ^ 1], gap=1)                       # ... passing through x on the way
    a = some(L)
    b.bucket(a + a + some(L) + some(2), gap=1)                  # 4 items, the first two equal: the join doubles
    b.bucket(a + MC.neg_vals(a) + some(L) + some(L) + a + some(3))   # 6 items: O after two, equal ones apart
    o = [v for w in some(L // 2) for v in (w, w ^ 1)]
    b.bucket(some(L) + o + some(1), gap=2)                      # 3 items, the middle one O
    b.bucket(o + o[::-1])                                       # 2 items, both O: the bucket is O
    t = b.v(curve_add(a[0], a[1]))
    b.bucket(some(L) + [a[0], a[1], t] + some(2))               # doubling inside the second piece
    b.bucket(some(3 * L + 2), gap=5)                            # 4 items, the last one short
    while len(b) < total - 1:                                   # (Entries.fill's gaps would leave the set)
        b.bucket(some(min(b.rng.randrange(1, 4), total - 1 - len(b))), gap=int(b.rng.randrange(8) == 0))
    b.bucket(some(total - len(b)), gap=4000 - b.key)            # the last bucket far up the set
    assert len(b) == total and b.key <= R.Win(WBITS).nbuckets
    return b


def classes(total):
    """A term list that plans the list: one class, one window, as many terms as entries."""
    return [[total, 0, 4, 1, 0, 4, 0, 0]]
