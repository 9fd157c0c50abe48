"""The inputs of the MSM stage tests (tests/test_gpu_msm_stages.py), built without a GPU so that
tests/test_msmref_cpu.py can hold them to the stage probe's preconditions and run the model on them:
the 64 points, the term lists of the digit / sort cases, the hand-written sorted lists of the
accumulation cases (the order inside every bucket fixed), the record stores of the merge and
reduction cases and the window sums of the combination cases.  Everything is seeded."""
import random

import fieldref as F
import msmref as R
from oracle import oracle as O
from oracle.pyspec import curves as pc, kzg as pk

CURVES = F.CURVES
WBITS = [13, 16]
_points = {}


def rng_of(*what):
    return random.Random("%d msm stages %s" % (F.SEED, " ".join(str(w) for w in what)))


def base_points(curve):
    """(k_j, P_j = k_j G) for 64 distinct j, from the oracle's generator multiplication."""
    if curve not in _points:
        C = pc.CURVES[curve]
        rng = rng_of("points", curve)
        ks = [rng.randrange(1, C.r) for _ in range(64)]
        raw = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(k) for k in ks), 64)
        g = pk.g1_size(C)
        _points[curve] = (ks, [pk.g1_from_bytes(raw[i * g:(i + 1) * g], C) for i in range(64)])
        assert len(set(_points[curve][1])) == 64
    return _points[curve]


def windows(wbits):
    """(windows of a 127-bit magnitude, of a full scalar): windows_half, windows_full of msm_plan.hpp."""
    return (128 + wbits - 1) // wbits, (256 + wbits - 1) // wbits


def half_words(mag, sign):
    assert mag < 1 << 127
    return F.to_words(mag | (sign << 127), 4)


class Scalars:
    """The scalar array of a call: word offsets of each class's scalars (16-byte aligned)."""

    def __init__(self):
        self.words = []

    def full(self, ks):
        o = len(self.words)
        for k in ks:
            self.words += F.to_words(k, 8)
        return o

    def half(self, ks):      # (magnitude, sign flag)
        o = len(self.words)
        for m, s in ks:
            self.words += half_words(m, s)
        return o


# ------------------------------------------------------------------------------ digits and sort
def sort_edges(curve, wbits):
    """Edge scalars through low, top (narrow at c = 13) and shared windows in 3 sets: classes of
    different nwin sharing sets, win_off > 0, a shared scalar, an empty class, infinity flags."""
    C, c = pc.CURVES[curve], wbits
    H, Fw = windows(c)
    rng = rng_of("sort edges", curve, wbits)
    full = [0, 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << 255) - 1, C.r - 1, (1 << 127) - 1]
    full += [rng.randrange(C.r) for _ in range(300 - len(full))]
    mags = [0, 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << 127) - 1, (1 << 127) - (1 << (c - 1))]
    half = [(m, s) for m in mags for s in (0, 1)] + [(rng.randrange(1 << 127), rng.randrange(2)) for _ in range(188)]
    sc = Scalars()
    of, oh, os_ = sc.full(full), sc.half(half), sc.full([C.r - 1 - (1 << (2 * c - 1))])
    classes = [[300, 0, 8, 2, 0, 8, of, 0],              # low windows (every carry case)
               [300, 100, 8, 3, 0, 8, of, Fw - 3],       # the top windows of full scalars
               [0, 0, 8, 1, 0, 8, 0, 0],                 # an empty class in the middle
               [200, 50, 4, 2, 1, 4, oh, H - 2],         # the top windows of 127-bit magnitudes
               [100, 300, 8, 1, 0, 0, os_, 1]]           # one shared scalar
    inf = [1 if j % 37 == 5 else 0 for j in range(400)]
    return dict(classes=classes, scalars=sc.words, inf=inf, nsets=3, mw=[1, 0, 0, 3, 0])


def sort_tiles(curve, wbits):
    """Class counts on both sides of the 4096-term tile."""
    rng = rng_of("sort tiles", curve, wbits)
    sc, classes = Scalars(), []
    for count in (1, 4095, 4096, 4097):
        o = sc.half([(rng.randrange(1 << 127), rng.randrange(2)) for _ in range(count)])
        classes.append([count, 0, 4, 1, 0, 4, o, 0])
    return dict(classes=classes, scalars=sc.words, inf=[0] * 4097, nsets=1, mw=[1, 0, 0, 1, 0])


def sort_big_bin(curve, wbits):
    """About 9000 entries in one coarse bin (above FINE_STAGE: fine_sort_chunks), several buckets."""
    rng = rng_of("sort big bin", curve, wbits)
    ks = [(rng.choice((1, 2, 3, 5, 100, 128)), rng.randrange(2)) for _ in range(8900)]
    ks += [(rng.choice((129, 1000, 0)), 0) for _ in range(100)]
    rng.shuffle(ks)
    sc = Scalars()
    o = sc.half(ks)
    assert sum(1 for m, s in ks if 1 <= m <= 128) > R.FINE_STAGE
    return dict(classes=[[9000, 0, 4, 1, 0, 4, o, 0]], scalars=sc.words, inf=[0] * 9000, nsets=1, mw=[1, 0, 0, 1, 0])


# ------------------------------------------------------------------------------ accumulation
class Entries:
    """A hand-written sorted list: buckets in key order, the order inside a bucket as given.  L is the
    chunk length the list is laid out for; positions count from the list's own start."""

    def __init__(self, curve, L, key0=0, points=None):
        self.curve, self.L = curve, L
        self.points = points if points is not None else list(base_points(curve)[1])
        self.index = {P: i for i, P in enumerate(self.points)}
        self.sval, self.skey, self.key = [], [], key0
        self.rng = rng_of("entries", curve, L, key0)

    def __len__(self):
        return len(self.sval)

    def v(self, P, sign=0):
        """The value of +-P, P a point (added to the point array if new)."""
        if P not in self.index:
            self.index[P] = len(self.points)
            self.points.append(P)
        return (self.index[P] << 1) | sign

    def some(self, n):
        return [self.rng.randrange(64) << 1 | self.rng.randrange(2) for _ in range(n)]

    def distinct(self, n):
        """n values of n different points"""
        idx = self.rng.sample(range(64), n)
        return [i << 1 | self.rng.randrange(2) for i in idx]

    def point(self, v):
        return R.value_point(v, self.points, self.curve)

    def bucket(self, vals, gap=0):
        self.key += gap
        self.sval += [vals[0] | R.SV_FIRST] + list(vals[1:])
        self.skey += [self.key] * len(vals)
        self.key += 1

    def pad(self, r):
        """Single-entry buckets until the next entry stands at offset r of its chunk."""
        while len(self) % self.L != r % self.L:
            self.bucket(self.some(1), gap=self.rng.randrange(2))

    def fill(self, upto):
        while len(self) < upto:
            self.bucket(self.some(min(self.rng.randrange(1, 4), upto - len(self))), gap=self.rng.randrange(3))


def neg_vals(vals):
    return [v ^ 1 for v in vals]


def standard_list(curve, L, T, key0=0, points=None):
    """T entries laid out for chunks of L: buckets cut into 2, 3, 4 (serial join), 5 and 9 pieces
    (crowded list) at three offsets; pieces that are O on either side and on both; equal and cancelling
    pieces in the serial and the crowded join; the in-chunk doubling at every chunk offset, after one
    entry and after two, last in its chunk and last in its bucket; a run returning to O and going on;
    a last bucket cut by the last chunk boundary that ends at the list's end."""
    b = Entries(curve, L, key0, points)
    some = b.some

    def cut(offset, pieces, tail):
        b.pad(offset)
        b.bucket(some((L - offset) + (pieces - 2) * L + tail))

    for pieces in (2, 3, 4, 5, 9):
        cut(0, pieces, L)
        cut(L - 1, pieces, 1)
        cut(1, pieces, L // 2)
    a, c = some(L), some(L)
    o = [v for x in some(L // 2) for v in (x, x ^ 1)]          # L entries summing to O, passing O on the way
    e, f = some(L), some(L)
    for pcs in ([o, a], [a, o], [o, o[::-1]], [a, a[::-1]], [a, neg_vals(a)], [a, c, a[::-1]],
                [a, a[::-1], o, c, neg_vals(c), e],            # crowded: doubling, + O, cancelling later
                [a, neg_vals(a), c, o, c[::-1], e, f],         # crowded: O first, then O + P
                [a, a, a, a, a, a, a, a, a]):                  # crowded: a chain of equal pieces
        b.pad(0)
        b.bucket([v for pc_ in pcs for v in pc_])
    for off in range(1, L):
        x, y = b.distinct(2)
        b.pad(off - 1)
        b.bucket([x, x])                                        # doubling at chunk offset `off`, then a bucket change
        if off >= 2:
            s = b.v(R.add(b.point(x), b.point(y), curve))
            b.pad(off - 2)
            b.bucket([x, y, s] + some(off % 3))                 # running sum x + y meets the point x + y
    for off in range(0, L - 3):
        x, y, z = b.distinct(3)
        b.pad(off)
        b.bucket([x, x ^ 1, y, z])                              # back to O mid-chunk, then on
        s = b.v(R.add(b.point(x), b.point(y), curve))
        b.pad(off)
        b.bucket([x, y, s ^ 1, z])
    X = T - 3
    X -= (X - (L - 2)) % L                                      # the last bucket starts 2 before a chunk boundary
    assert len(b) <= X, (len(b), T)
    b.fill(X)
    b.bucket(some(T - X))                                       # ... and ends at the list's end
    assert len(b) == T and X // L != (T - 1) // L
    return b


def whole_chunks(curve, L, nchunks):
    """Every bucket exactly one chunk."""
    b = Entries(curve, L)
    for _ in range(nchunks):
        b.bucket(b.some(L), gap=b.rng.randrange(2))
    return b


# ------------------------------------------------------------------------------ records
def edge_shifts(curve):
    M = R.layers(curve)[0]
    top = (M.rec["x"] - 1, M.rec["y"] - 1, M.rec["z"] - 1, M.rec["z"] - 1)
    return [(0, 0, 0, 0), top, (top[0], 0, top[2], 0), (0, top[1], 0, top[3])]


def record_store(curve, S, NB, rng):
    """{key: point} as a store of NB records (numpy uint32 words) and its counts: ZZ random, the
    coordinates shifted to the edges of the record bounds or by random multiples of p inside them."""
    import numpy as np
    M = R.layers(curve)[0]
    n = 4 * M.N
    acc, cnt = np.zeros(NB * n, dtype=np.uint32), [0] * NB
    shifts = edge_shifts(curve)
    for i, (key, P) in enumerate(sorted(S.items())):
        sh = shifts[i % 4] if i % 8 < 4 else tuple(rng.randrange(t + 1) for t in shifts[1])
        w = R.encode_record(P, curve, sh, 1 if i % 5 == 0 else rng.randrange(1, M.p))
        assert R.check_record(w, curve) is None and R.decode_record(w, curve)[0] == P
        acc[key * n:(key + 1) * n] = w
        cnt[key] = 1 + i % 3
    return acc, cnt


def reduce_store(curve, wbits, nsets):
    """Bucket sums for the reduction: only bucket 0 (set 0); only the top bucket (the last set); a
    whole segment of equal points; adjacent buckets that cancel; a bucket whose sum is O (cnt > 0);
    scattered random buckets; with 3 sets the middle one stays empty (its window sum is O)."""
    W = R.Win(wbits)
    rng = rng_of("reduce", curve, wbits, nsets)
    pts = base_points(curve)[1]
    S = {}
    last = (nsets - 1) * W.nbuckets
    if nsets == 1:
        S[0] = pts[0]
        for i in range(R.SEG):
            S[3 * R.SEG + i] = pts[1]                      # one whole segment of equal points
        for g, i in ((7, 2), (9, 7), (11, 3), (12, 11), (13, 15)):
            S[g * R.SEG + i] = pts[2 + i]                  # adjacent buckets that cancel: inside a half, a
            if i < 15:                                     # quarter, across the halves
                S[g * R.SEG + i + 1] = R.neg(pts[2 + i], curve)
        S[20 * R.SEG + 5] = None                           # a non-empty bucket that sums to O
        S[21 * R.SEG + 4], S[21 * R.SEG + 5] = pts[20], pts[20]   # adjacent equal sums
        for _ in range(40):
            S[rng.randrange(24 * R.SEG, W.nbuckets - 1)] = rng.choice(pts)
        S[W.nbuckets - 1] = pts[30]
    else:
        S[0] = pts[0]                                      # only bucket 0 in set 0
        S[last + W.nbuckets - 1] = pts[1]                  # only the top bucket in the last set
    return S


def combine_cases(curve, wbits):
    """{name: (window sums as points, mw, nsets)}"""
    pts = base_points(curve)[1]
    P, Q, T = pts[3], pts[4], pts[5]
    sh = R.mul(P, 1 << wbits, curve)
    return {
        "top O": ([P, Q, None], [1, 0, 0, 3, 0], 3),
        "middle O": ([P, None, Q], [1, 0, 0, 3, 0], 3),
        "all O": ([None, None, None], [1, 0, 0, 3, 0], 3),
        "cancel": ([T, R.neg(sh, curve), P], [1, 0, 0, 3, 0], 3),     # acc = -ws after the doublings, then O + T
        "double": ([T, sh, P], [1, 0, 0, 3, 0], 3),                   # 2^c acc = ws: the doubling branch
        "nwin 1": ([P], [1, 0, 0, 1, 0], 1),
        "two msms": ([P, Q, T], [2, 0, 1, 1, 2], 3),
        "second first": ([P, Q, T], [2, 2, 0, 1, 2], 3),              # MSM#0 reads set 2, MSM#1 sets 0..1
    }


# ------------------------------------------------------------------------------ small path
def small_edges(curve):
    """(8-word scalars, 4-word (magnitude, sign flag) pairs) every small case set must run: 0, 1, r - 1
    and the Booth extremes 0x88..8, 0x77..7, 0xff..f masked to the class width (255 and 127 bits)."""
    C = pc.CURVES[curve]
    booth8 = [int(d * 64, 16) & ((1 << 255) - 1) for d in "87f"]
    booth4 = [int(d * 32, 16) & ((1 << 127) - 1) for d in "87f"]
    return [0, 1, C.r - 1] + booth8, [(m, s) for m in [0, 1] + booth4 for s in (0, 1)]


def small_cases(curve):
    """{name: (classes, scalar words, points, inf, mw, nsets, [expected scalar, point index per MSM])}
    for k_small_msm: leaf counts 1, 2, 3, 5, 64, 65 of full scalars, the first leaves taking the
    8-word edges in order (5 leaves: 0, 1, r - 1, 0x088..8, 0x77..7; 64 and 65: all six, and leaves 6, 7
    siblings that cancel); two MSMs of unequal size with every 4-word edge under both signs."""
    C = pc.CURVES[curve]
    pts = base_points(curve)[1]
    rng = rng_of("small", curve)
    edge8, edge4 = small_edges(curve)
    out = {}
    for n in (1, 2, 3, 5, 64, 65):
        sc = Scalars()
        ks = (edge8 + [rng.randrange(1, C.r) for _ in range(n)])[:n]
        idx = list(range(n))
        if n >= 8:
            ks[7], idx[7] = C.r - ks[6], idx[6]            # leaves 6, 7: siblings that cancel (k P and -k P)
        o = sc.full(ks)
        out["leaves %d" % n] = ([[n, 0, 8, 1, 0, 8, o, 0]], sc.words, [pts[i % 64] for i in idx], [0] * n,
                                [1, 0, 0, 1, 0], 1, [[(k, i) for k, i in zip(ks, range(n))]])
    # two MSMs of unequal size: 4-word signed scalars and an infinity point in MSM#0; equal siblings,
    # a shared scalar and an infinity point in MSM#1
    sc = Scalars()
    n0, n1, n2 = len(edge4) + 3, 9, 4
    h = edge4 + [(rng.randrange(1 << 127), rng.randrange(2)) for _ in range(3)]
    k1 = [rng.randrange(C.r) for _ in range(n1)]
    k1[1] = k1[0]
    ks_shared = rng.randrange(C.r)
    o0, o1, o2 = sc.half(h), sc.full(k1), sc.full([ks_shared])
    points = [pts[i] for i in range(n0)] + [pts[20]] * 2 + [pts[22 + i] for i in range(n1 - 2)] + [pts[40 + i] for i in range(n2)]
    inf = [0] * len(points)
    inf[n0 - 1] = inf[n0 + 4] = 1                          # (a random term's point: every edge scalar runs)
    classes = [[n0, 0, 4, 2, 0, 4, o0, 0], [n1, n0, 8, 1, 2, 8, o1, 0], [n2, n0 + n1, 8, 1, 2, 0, o2, 0]]
    want0 = [((C.r - m) % C.r if s else m, i) for i, (m, s) in enumerate(h)]
    want1 = [(k, n0 + i) for i, k in enumerate(k1)] + [(ks_shared, n0 + n1 + i) for i in range(n2)]
    out["two msms"] = (classes, sc.words, points, inf, [2, 0, 2, 2, 1], 3, [want0, want1])
    return out


# ------------------------------------------------------------------------------ chained
def chained(curve, wbits, n=96):
    """A mixed term list in 3 sets whose two MSMs are plain sums sum_i k_i P_i the oracle can check:
    the windows of a scalar read by classes with win_off over tables of shifted points 2^(c w) P_i
    (the fixed-base form).  MSM#0: signed 127-bit scalars, two windows a class (sets 0, 1); MSM#1:
    full scalars below 2^(6 c - 1), one window a class (set 2), with an empty class and a class of
    one shared scalar.  -> classes, scalars, points, inf, nsets, mw, and per MSM (scalars mod r,
    points) for the oracle."""
    C, c = pc.CURVES[curve], wbits
    H, _ = windows(c)
    ks, pts = base_points(curve)
    rng = rng_of("chained", curve, wbits)
    base = [j % 64 for j in range(n)]
    rows = max(H, 6)
    # table row w: 2^(c w) P_i, from the oracle's generator multiplication
    raw = O.g1_mul_gen(curve, b"".join(pk.fr_to_bytes(ks[j] * (1 << (c * w)) % C.r) for w in range(rows) for j in base),
                       rows * n)
    g = pk.g1_size(C)
    points = [pk.g1_from_bytes(raw[i * g:(i + 1) * g], C) for i in range(rows * n)]
    inf = [0] * len(points)
    half = [(rng.randrange(1 << 127), rng.randrange(2)) for _ in range(n)]
    half[:4] = [(0, 0), ((1 << 127) - 1, 1), (1, 1), (1 << (c - 1), 0)]
    full = [rng.randrange(1 << (6 * c - 1)) for _ in range(n)]
    full[:3] = [(1 << (6 * c - 1)) - 1, 0, (1 << (c - 1)) + 1]
    shared = rng.randrange(1 << (c - 2))
    sc = Scalars()
    oh, of, os_ = sc.half(half), sc.full(full), sc.full([shared])
    classes = []
    for w in range(0, H, 2):
        classes.append([n, w * n, 4, min(2, H - w), 0, 4, oh, w])
    classes.append([0, 0, 8, 1, 2, 8, 0, 0])
    for w in range(6):
        classes.append([n, w * n, 8, 1, 2, 8, of, w])
    classes.append([n // 2, 5, 8, 1, 2, 0, os_, 0])
    assert len(classes) <= 16
    for j in range(3):                                      # a few points at infinity (every row of them)
        for w in range(rows):
            inf[w * n + 7 * j + 1] = 1
    dead = {7 * j + 1 for j in range(3)}
    want0 = [((C.r - m) % C.r if s else m, pts[base[i]]) for i, (m, s) in enumerate(half) if i not in dead]
    want1 = [(k, pts[base[i]]) for i, k in enumerate(full) if i not in dead]
    want1 += [(shared, pts[base[5 + i]]) for i in range(n // 2) if 5 + i not in dead]
    return dict(classes=classes, scalars=sc.words, points=points, inf=inf, nsets=3, mw=[2, 0, 2, 2, 1], want=[want0, want1])


def oracle_msm(curve, want):
    """sum k P of (scalar, point) pairs through the C oracle -> affine point or None"""
    C = pc.CURVES[curve]
    raw = O.msm_g1(curve, b"".join(pk.g1_to_bytes(P, C) for k, P in want), b"".join(pk.fr_to_bytes(k) for k, P in want),
                   len(want))
    return pk.g1_from_bytes(raw, C)


# ------------------------------------------------------------------------------ accumulation cases
QUEUE_TUNING = dict(acc_threads_env=256, acc_queue=4, acc_queue_min=4, acc_queue_from=1024)


def acc_cases(curve):
    """{name: (entries, wbits, nsets, tuning, [(lo, end, chunk length)] per launch)}: the static grid
    at chunk lengths 4 and 8, every bucket one whole chunk, the work-queue form (256 threads taking
    1024 chunks, half of them past the list's end), and two sets for the split accumulation (the
    second launch's range starting off a 16-byte boundary)."""
    out = {
        "len4": (standard_list(curve, 4, 1000), 13, 1, {}, [(0, 1000, 4)]),
        "len8": (standard_list(curve, 8, 1800), 13, 1, {}, [(0, 1800, 8)]),
        "whole": (whole_chunks(curve, 4, 256), 13, 1, {}, [(0, 1024, 4)]),
        "queue": (standard_list(curve, 8, 4200), 16, 1, QUEUE_TUNING, [(0, 4200, 8)]),
    }
    a = standard_list(curve, 4, 999)
    b = standard_list(curve, 8, 1800, key0=R.Win(13).nbuckets, points=a.points)
    a.sval += b.sval
    a.skey += b.skey
    out["split"] = (a, 13, 2, dict(split_acc=1), [(0, 999, 4), (999, 2799, 8)])
    return out


def acc_classes(launches, nsets):
    """A term list that plans the hand-made list: one class per set, one window, as many terms as entries."""
    return [[end - lo, 0, 4, 1, s, 4, 0, 0] for s, (lo, end, L) in enumerate(launches)]
