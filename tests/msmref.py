"""Plain big-integer model of the bucket MSM pipeline (csrc/msm.hpp, csrc/msm_small.hpp), stage by
stage, and the executable form of the contracts its kernels pass each other.  Used by
tests/test_msmref_cpu.py (the model against the oracle, no GPU) and tests/test_gpu_msm_stages.py
(every stage of the GPU pipeline against the model).

  digits        the signed window recoding of term_digits and the digit array's layout
  sort_contract what the four sort kernels hand the accumulation: per bucket the multiset of
                values, cnt / off of every bucket of every set, skey, SV_FIRST, total, the coarse bins
  accumulate    which record every chunk's bucket pieces go to, each piece's sum, the crowded list
  segments      R', U, V of every reduction segment, in the two- and the four-thread form
  winsum, combine   sum_b (b + 1) S_b per set, sum_w 2^(c w) winsum[set_base + w] per MSM
  records       radix-29 XYZZ records: encode_record / decode_record / check_record

Points are affine (x, y) tuples of integers or None (oracle.pyspec.curves); limb encodings and the
per-curve record bounds come from tests/fieldref.py (Mod29, ModLp).  Term classes are lists
[count, pt_base, scal_words, nwin, set_base, scal_stride, scal word offset, win_off]."""
import fieldref as F
from oracle.pyspec import curves as pc

COARSE_SHIFT, FINE, SEG, FINE_STAGE, FIX_LP_FROM = 7, 128, 16, 8192, 4
SV_FIRST = 1 << 31
_layers = {}


def layers(curve):
    if curve not in _layers:
        _layers[curve] = (F.Mod29(curve), F.ModLp(curve))
    return _layers[curve]


class Win:
    def __init__(self, wbits):
        self.c = wbits
        self.nbuckets = 1 << (wbits - 1)
        self.bins = self.nbuckets >> COARSE_SHIFT
        self.bins_log2 = wbits - 1 - COARSE_SHIFT
        self.nseg = self.nbuckets // SEG
        self.maxw = 256 // wbits + 1


# ------------------------------------------------------------------------------ group helpers
def neg(P, curve):
    return pc.g1_neg(P, pc.CURVES[curve])


def add(P, Q, curve):
    return pc.g1_add(P, Q, pc.CURVES[curve])


def mul(P, k, curve):
    """[k]P for 0 <= k < r"""
    return pc.g1_mul(P, k, pc.CURVES[curve])


def total(points, curve):
    acc = None
    for P in points:
        acc = add(acc, P, curve)
    return acc


# ------------------------------------------------------------------------------ digits
def scalar_of(words, scal_words):
    """(magnitude, sign flag) of a class's scalar: 4-word scalars carry their sign in bit 127."""
    v = F.from_words(words[:scal_words])
    if scal_words == 4:
        return v & ((1 << 127) - 1), bool(v >> 127)
    return v, False


def term_codes(k, negf, is_inf, win_off, nwin, wbits):
    """term_digits: the codes of windows win_off .. win_off + nwin - 1 of magnitude k.  d > 2^(c-1)
    gives d - 2^c and a carry; code = |d| | (d < 0) xor sign flag << 31, or 0 (zero digit, infinity)."""
    W = Win(wbits)
    out, carry = [], 0
    for w in range(W.maxw):
        if w >= win_off + nwin:
            break
        d = ((k >> (w * wbits)) & ((1 << wbits) - 1)) + carry
        carry = 0
        if d > W.nbuckets:
            d -= 1 << wbits
            carry = 1
        if w >= win_off:
            out.append(0 if d == 0 or is_inf else abs(d) | (((d < 0) != negf) << 31))
    return out


def digits(classes, scalars, inf, wbits, dig_base=None):
    """The digit array: digit (w, i) of class k at dig_base[k] + w * count + i (dig_base: classes back
    to back when not given, as plan_msm lays them out)."""
    if dig_base is None:
        dig_base, n = [], 0
        for c in classes:
            dig_base.append(n)
            n += c[0] * c[3]
    ndig = max([0] + [b + c[0] * c[3] for b, c in zip(dig_base, classes)])
    out = [None] * ndig
    for b, (count, pt_base, sw, nwin, set_base, stride, so, win_off) in zip(dig_base, classes):
        for i in range(count):
            k, negf = scalar_of(scalars[so + i * stride: so + i * stride + sw], sw)
            for w, code in enumerate(term_codes(k, negf, bool(inf[pt_base + i]), win_off, nwin, wbits)):
                out[b + w * count + i] = code
    assert None not in out
    return out


# ------------------------------------------------------------------------------ sort
def set_shifts(classes, nsets, wbits, full_bins=False):
    """set_shifts_host: per set the coarse-bin width (log2 buckets per bin)."""
    W = Win(wbits)
    if full_bins:
        return [COARSE_SHIFT] * nsets
    ss = [0] * nsets
    for count, pt_base, sw, nwin, set_base, stride, so, win_off in classes:
        if not count:
            continue
        bits = 127 if sw == 4 else 255
        for w in range(nwin):
            tb = min(wbits, max(0, bits - (win_off + w) * wbits))
            need = COARSE_SHIFT if tb >= wbits - 1 else max(0, tb - W.bins_log2)
            ss[set_base + w] = max(ss[set_base + w], need)
    return ss


def entries(classes, digs, wbits, dig_base=None):
    """{global key: [values]}: key = set * 2^(c-1) + |d| - 1, value = (pt_base + i) << 1 | sign."""
    W = Win(wbits)
    if dig_base is None:
        dig_base, n = [], 0
        for c in classes:
            dig_base.append(n)
            n += c[0] * c[3]
    out = {}
    for b, (count, pt_base, sw, nwin, set_base, stride, so, win_off) in zip(dig_base, classes):
        for w in range(nwin):
            for i in range(count):
                code = digs[b + w * count + i]
                if code:
                    key = (set_base + w) * W.nbuckets + (code & 0x7fffffff) - 1
                    out.setdefault(key, []).append(((pt_base + i) << 1) | (code >> 31))
    return out


def sort_contract(ents, nsets, shifts, wbits):
    """From the entries per key: cnt and off of every bucket (off of a bucket no narrowed bin covers
    = the start of the bin that owns it, k_fine_sort), skey, the positions that carry SV_FIRST,
    total, and the coarse counts and offsets."""
    W = Win(wbits)
    NB = nsets * W.nbuckets
    cnt, off = [0] * NB, [0] * NB
    ccnt = [0] * (nsets * W.bins)
    for key, vals in ents.items():
        s, m1 = divmod(key, W.nbuckets)
        sh = shifts[s]
        assert (m1 >> sh) < W.bins, "an entry in a bucket no coarse bin covers: scalar above its class's bound"
        cnt[key] = len(vals)
        ccnt[s * W.bins + (m1 >> sh)] += len(vals)
    coff, run = [], 0
    for v in ccnt:
        coff.append(run)
        run += v
    run = 0
    skey = []
    for s in range(nsets):
        sh = shifts[s]
        covered = W.bins << sh
        for b in range(W.nbuckets):
            key = s * W.nbuckets + b
            if b < covered:
                off[key] = run
                run += cnt[key]
                skey += [key] * cnt[key]
            else:
                assert cnt[key] == 0
                off[key] = coff[s * W.bins + (b - covered) // (FINE - (1 << sh))]
    first = sorted(off[k] for k in ents)
    return dict(cnt=cnt, off=off, skey=skey, first=first, total=run, coarse_cnt=ccnt, coarse_off=coff)


def bucket_sums(ents, points, curve):
    """{key: S_key}: the sum of the bucket's points, each negated where its value's sign bit is set."""
    out = {}
    for key, vals in ents.items():
        out[key] = total([neg(points[v >> 1], curve) if v & 1 else points[v >> 1] for v in vals], curve)
    return out


def sorted_list(ents, order=None):
    """(sval, skey, first positions) of the entries in key order, the values of a bucket in the order
    given (hand-made lists fix it; `order` may reorder a bucket's values)."""
    sval, skey = [], []
    for key in sorted(ents):
        vals = order(key, ents[key]) if order else ents[key]
        sval += [vals[0] | SV_FIRST] + list(vals[1:])
        skey += [key] * len(vals)
    return sval, skey


def off_cnt(skey, NB):
    """off / cnt of a hand-made key list as the sort would write them under full-width bins."""
    cnt, off = [0] * NB, [0] * NB
    for k in skey:
        cnt[k] += 1
    run = 0
    for k in range(NB):
        off[k] = run
        run += cnt[k]
    return off, cnt


# ------------------------------------------------------------------------------ accumulation
def acc_chunk_len(n, nthreads):
    per = ((n + nthreads - 1) // nthreads + 3) & ~3
    return max(per, 4)


def value_point(v, points, curve):
    P = points[(v & ~SV_FIRST) >> 1]
    return neg(P, curve) if v & 1 else P


def accumulate(sval, skey, points, curve, nthreads, nb, lo=0, end=None):
    """One accumulation launch over the sorted entries [lo, end) with nthreads chunks, its piece
    records behind record nb.  -> (flushed, joined, cuts, length): flushed {record index: partial
    sum} after k_accumulate alone, joined {key: bucket sum} for every bucket of the range, cuts
    {key: (c0, c1)} the first and last chunk of every bucket cut by a chunk boundary (crowded():
    those k_fixup lists), and the chunk length."""
    end = len(skey) if end is None else end
    ln = acc_chunk_len(end - lo, nthreads)
    flushed, joined, pieces = {}, {}, {}
    c = 0
    while c * ln < end - lo:
        start = lo + c * ln
        stop = min(start + ln, end)
        e = start
        while e < stop:
            key, run = skey[e], None
            e0 = e
            while e < stop and skey[e] == key:
                run = add(run, value_point(sval[e], points, curve), curve)
                e += 1
            before = e0 == start and start > 0 and skey[start - 1] == key
            after = e == stop and stop < end and skey[stop] == key
            rec = nb + c if before else nb + nthreads + c if after else key
            assert rec not in flushed
            flushed[rec] = run
            joined[key] = add(joined.get(key), run, curve)
            pieces.setdefault(key, []).append(c)
        c += 1
    for k, cs in pieces.items():
        assert cs == list(range(cs[0], cs[-1] + 1))
    return flushed, joined, {k: (cs[0], cs[-1]) for k, cs in pieces.items() if len(cs) > 1}, ln


def crowded(cuts):
    """The (key, c0, c1) of the buckets of FIX_LP_FROM + 1 pieces or more: k_fixup's crowded list."""
    return {(k, c0, c1) for k, (c0, c1) in cuts.items() if c1 - c0 >= FIX_LP_FROM}


# ------------------------------------------------------------------------------ reduction
def segments(S, nsets, wbits, curve, four):
    """{segment g: (R', U, V)} of the non-empty segments (every other segment is (O, O, O)):
    two threads per segment: R' + 8 V = sum_i i S_(16 g + i), V = the upper half's sum; four:
    R' + 4 V, V = u_1 + 2 u_2 + 3 u_3.  U = the segment's sum in both."""
    out = {}
    for g in sorted({k // SEG for k in S}):
        s = [S.get(g * SEG + i) for i in range(SEG)]
        U = total(s, curve)
        if four:
            r = [total([mul(s[4 * h + i], i, curve) for i in range(4)], curve) for h in range(4)]
            u = [total(s[4 * h:4 * h + 4], curve) for h in range(4)]
            V = total([u[1], mul(u[2], 2, curve), mul(u[3], 3, curve)], curve)
            m = 4
        else:
            r = [total([mul(s[8 * h + i], i, curve) for i in range(8)], curve) for h in range(2)]
            V = total(s[8:], curve)
            m = 8
        Rp = total(r, curve)
        assert add(Rp, mul(V, m, curve), curve) == total([mul(s[i], i, curve) for i in range(SEG)], curve)
        out[g] = (Rp, U, V)
    return out


def winsums(S, nsets, wbits, curve):
    """winsum[set] = sum_b (b + 1) S_b over the set's buckets b = |d| - 1."""
    W = Win(wbits)
    out = [None] * nsets
    for key, P in S.items():
        s, b = divmod(key, W.nbuckets)
        out[s] = add(out[s], mul(P, b + 1, curve), curve)
    return out


def winsum_from_segments(segs, nsets, wbits, curve, four):
    """The window sums as k_reduce_bits and k_reduce_bits_finish assemble them from the segment
    records: sum_g (R'_g + U_g) + m sum_g V_g + 16 sum_g g U_g (g within the set)."""
    W = Win(wbits)
    out = [None] * nsets
    for g, (Rp, U, V) in segs.items():
        s, gl = divmod(g, W.nseg)
        t = total([Rp, U, mul(V, 4 if four else 8, curve), mul(U, SEG * gl, curve)], curve)
        out[s] = add(out[s], t, curve)
    return out


def combine(ws, mw, wbits, curve):
    """res[m] = sum_w 2^(c w) winsum[set_base_m + w] (Horner from the top window)."""
    nmsm, sb, nw = mw[0], mw[1:3], mw[3:5]
    res = []
    for m in range(nmsm):
        acc = None
        for w in range(nw[m] - 1, -1, -1):
            for _ in range(wbits):
                acc = add(acc, acc, curve)
            acc = add(acc, ws[sb[m] + w], curve)
        res.append(acc)
    return res


def msm(classes, scalars, points, inf, nsets, mw, wbits, curve):
    """The whole pipeline: digits, sort, bucket sums, segments (both forms), window sums, combination."""
    digs = digits(classes, scalars, inf, wbits)
    ents = entries(classes, digs, wbits)
    S = bucket_sums(ents, points, curve)
    ws = winsums(S, nsets, wbits, curve)
    for four in (False, True):
        assert winsum_from_segments(segments(S, nsets, wbits, curve, four), nsets, wbits, curve, four) == ws
    return combine(ws, mw, wbits, curve)


# ------------------------------------------------------------------------------ records and points
def decode_record(words, curve):
    """-> (affine point or None, (x, y, zz, zzz) as integers); infinity is zz = 0."""
    M, _ = layers(curve)
    n = M.N
    assert len(words) == 4 * n
    v = tuple(F.value29(words[i * n:(i + 1) * n]) for i in range(4))
    return M.rec_affine(v + (v[2] == 0,)), v


def encode_record(P, curve, shifts=(0, 0, 0, 0), lam=1):
    """The record of P with ZZ = lam^2, ZZZ = lam^3 and shifts[i] multiples of p added to coordinate
    i (inside the record bounds, which make_rec asserts); O: zz = 0 under the same shifts of x, y."""
    M, _ = layers(curve)
    if P is None:
        r = (shifts[0] * M.p, shifts[1] * M.p, 0, shifts[3] * M.p)
    else:
        r = M.make_rec(P, lam, shifts)[:4]
    return [w for v in r for w in F.limbs29(v, M.N)]


def check_record(words, curve):
    """None, or what is wrong: limbs normalised (all but a coordinate's top limb below 2^29), every
    coordinate inside the record bounds x29_add, x29_dbl and the lane-parallel loads read under
    (fieldref.Mod29.rec: x, y, zz = zzz, in units of p), and a point unless zz = 0."""
    M, _ = layers(curve)
    n = M.N
    if len(words) != 4 * n:
        return "record of %d words" % len(words)
    for i, w in enumerate(words):
        if (i + 1) % n and w > F.M29:
            return "limb %d not normalised: %#x" % (i, w)
    v = [F.value29(words[i * n:(i + 1) * n]) for i in range(4)]
    for nm, x, b in zip(("x", "y", "zz", "zzz"), v, (M.rec["x"], M.rec["y"], M.rec["z"], M.rec["z"])):
        if not x < b * M.p:
            return "%s = %.4f p, record bound %d p" % (nm, x / M.p, b)
    if v[2] == 0:
        return None
    if v[2] % M.p == 0:
        return "zz is a nonzero multiple of p: infinity must be zz = 0"
    try:
        M.rec_affine(tuple(v) + (False,))
    except AssertionError as e:
        return str(e)
    return None


def records(arr, idx, curve):
    """The words of record idx of a flat record array (numpy or list)."""
    n = 4 * layers(curve)[0].N
    return [int(w) for w in arr[idx * n:(idx + 1) * n]]


def affine_words(P, curve):
    """A point as the probe takes it: the words of an Affine<Cv> slot (csrc/g1.hpp), x then y in
    32-bit Montgomery form, the 96 bytes of BLS12-381 padded to the slot's 128 (O: zeros, flagged
    apart)."""
    _, L = layers(curve)
    pad = [0] * (8 if 2 * L.W == 24 else 0)
    if P is None:
        return [0] * (2 * L.W) + pad
    return F.to_words(P[0] * L.R32 % L.p, L.W) + F.to_words(P[1] * L.R32 % L.p, L.W) + pad


def xyzz_words(P, curve, lam=1):
    return layers(curve)[1].xyzz(P, lam)


def xyzz_point(arr, idx, curve):
    """Affine point of Xyzz record idx (field.hpp words), asserting canonical coordinates."""
    L = layers(curve)[1]
    n = 4 * L.W
    return L.xyzz_affine([int(w) for w in arr[idx * n:(idx + 1) * n]])
