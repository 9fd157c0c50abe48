"""CPU side of the MSM stage tests (tests/test_gpu_msm_stages.py runs the stages on the GPU): the
big-integer model of tests/msmref.py chained from the digits to the combination against the C
oracle's MSM, its pieces against each other, the record encoding, and the inputs of the GPU tests
(tests/msmcases.py) against the stage probe's preconditions and the plan the probe will make."""
import random

import pytest

import fieldref as F
import msmcases as MC
import msmprobe as MP
import msmref as R
from oracle.pyspec import curves as pc

CURVES = F.CURVES
CW = [(c, w) for c in CURVES for w in MC.WBITS]
CW_IDS = ["%s-c%d" % cw for cw in CW]


# ---------------------------------------------------------------------------- model vs oracle
@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_model_chain_matches_oracle_mixed(curve, wbits):
    """The mixed-class term list of the chained GPU test, stage by stage through the model, gives
    the oracle's MSMs (the model's own stage identities are asserted inside msm())."""
    case = MC.chained(curve, wbits)
    got = R.msm(case["classes"], case["scalars"], case["points"], case["inf"], case["nsets"], case["mw"], wbits, curve)
    assert got == [MC.oracle_msm(curve, w) for w in case["want"]]


@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_model_chain_matches_oracle_batch_form(curve, wbits):
    """Two MSMs over every window, as batch_terms lays a batch out: signed 127-bit scalars in H sets,
    full scalars (and a shared one) in F more, with the scalar edges and infinity flags."""
    C = pc.CURVES[curve]
    H, Fw = MC.windows(wbits)
    pts = MC.base_points(curve)[1]
    rng = MC.rng_of("batch form", curve, wbits)
    n = 24
    c = wbits
    half = [(0, 0), (1, 1), (1 << (c - 1), 0), ((1 << (c - 1)) + 1, 1), ((1 << 127) - 1, 0), ((1 << 127) - 1, 1)]
    half += [(rng.randrange(1 << 127), rng.randrange(2)) for _ in range(n - len(half))]
    full = [0, 1, 1 << (c - 1), (1 << (c - 1)) + 1, C.r - 1, (1 << 127) - 1, int("f" * 63, 16) % C.r]
    full += [rng.randrange(C.r) for _ in range(n - len(full))]
    shared = rng.randrange(C.r)
    sc = MC.Scalars()
    oh, of, os_ = sc.half(half), sc.full(full), sc.full([shared])
    classes = [[n, 0, 4, H, 0, 4, oh, 0], [n, n, 8, Fw, H, 8, of, 0], [n, 0, 4, H, H, 4, oh, 0], [5, 2 * n, 8, Fw, H, 0, os_, 0]]
    points = pts[:n] + pts[n:2 * n] + pts[50:55]
    inf = [0] * len(points)
    inf[3] = inf[n + 4] = 1
    got = R.msm(classes, sc.words, points, inf, H + Fw, [2, 0, H, H, Fw], wbits, curve)
    sgn = [((C.r - m) % C.r if s else m) for m, s in half]
    want0 = [(k, points[i]) for i, k in enumerate(sgn) if not inf[i]]
    want1 = [(k, points[n + i]) for i, k in enumerate(full) if not inf[n + i]] + want0 + [(shared, P) for P in points[2 * n:]]
    assert got == [MC.oracle_msm(curve, want0), MC.oracle_msm(curve, want1)]


@pytest.mark.parametrize("wbits", MC.WBITS)
def test_digits_recompose_the_scalar(wbits):
    """sum_w d_w 2^(c w) = k with every |d_w| <= 2^(c-1), the sign flag flipping every digit, a
    point at infinity giving code 0 everywhere, and win_off / nwin selecting a range of the windows."""
    W = R.Win(wbits)
    rng = random.Random("%d digits %d" % (F.SEED, wbits))
    c = wbits
    ks = [0, 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << 255) - 1, (1 << 127) - 1] + [rng.randrange(1 << 255) for _ in range(64)]
    for k in ks:
        for negf in (False, True):
            codes = R.term_codes(k, negf, False, 0, W.maxw, wbits)
            assert len(codes) == W.maxw and all((x & 0x7fffffff) <= W.nbuckets for x in codes)
            val = sum((-1 if (x >> 31) != negf else 1) * (x & 0x7fffffff) << (c * w) for w, x in enumerate(codes))
            assert val == k
            assert R.term_codes(k, negf, False, 3, 2, wbits) == codes[3:5]
            assert R.term_codes(k, negf, True, 0, 4, wbits) == [0] * 4
    assert R.term_codes(1 << (c - 1), False, False, 0, 2, wbits) == [W.nbuckets, 0]                  # no carry
    assert R.term_codes((1 << (c - 1)) + 1, False, False, 0, 2, wbits) == [(W.nbuckets - 1) | 1 << 31, 1]  # carry


# ---------------------------------------------------------------------------- records
@pytest.mark.parametrize("curve", CURVES)
def test_record_round_trip_and_check(curve):
    M = R.layers(curve)[0]
    rng = MC.rng_of("records", curve)
    pts = MC.base_points(curve)[1]
    for i, sh in enumerate(MC.edge_shifts(curve)):
        for lam in (1, rng.randrange(1, M.p)):
            for P in (pts[i], None):
                w = R.encode_record(P, curve, sh, lam)
                assert R.check_record(w, curve) is None
                got, v = R.decode_record(w, curve)
                assert got == P and all(v[j] // M.p >= sh[j] for j in (0, 1))
    w = R.encode_record(pts[0], curve)
    n = M.N
    bad = list(w)
    bad[0] += 1 << 29                                    # same value ...
    bad[1] -= 1 if bad[1] else 0
    assert "normalised" in R.check_record(bad, curve)
    over = F.limbs29(R.decode_record(w, curve)[1][0] + M.rec["x"] * M.p, n) + w[n:]
    assert "record bound" in R.check_record(over, curve)
    zzp = w[:2 * n] + F.limbs29(M.p, n) + w[3 * n:]
    assert "multiple of p" in R.check_record(zzp, curve)
    off_curve = w[:n] + F.limbs29(R.decode_record(w, curve)[1][1] + 1, n) + w[2 * n:]
    assert R.decode_record(off_curve, curve)[0] != pts[0]


# ---------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("curve", CURVES)
def test_hand_made_lists_meet_the_probe_preconditions(curve):
    """Every accumulation case is a list the sort could have produced, the plan gives it the chunk
    length it was laid out for, and the model's joined sums are the plain bucket sums.  The check is
    the probe's own (the one its accumulate stage makes before it launches; host code, no GPU)."""
    for name, (lst, wbits, nsets, tuning, launches) in MC.acc_cases(curve).items():
        call = MP.Call(MC.acc_classes(launches, nsets), nsets, [nsets, 0, nsets - 1, 1, nsets - 1], wbits, tuning=tuning)
        p = MP.plan(curve, call)
        NB, T = p["NB"], len(lst)
        assert not p["small"] and NB == nsets * R.Win(wbits).nbuckets and bool(p["split"]) == (nsets == 2), name
        assert bool(p["acc_threads"]) == (name == "queue") and (not p["acc_threads"] or p["acc_threads"] < p["nchunks"])
        off, cnt = R.off_cnt(lst.skey, NB)
        assert MP.check_sorted(curve, call, len(lst.points), lst.sval, lst.skey, off, cnt, T, mid=launches[-1][0]), name
        ents = {}
        for v, k in zip(lst.sval, lst.skey):
            ents.setdefault(k, []).append(v & ~R.SV_FIRST)
        S = R.bucket_sums(ents, lst.points, curve)
        cuts = set()
        for s, (lo, end, L) in enumerate(launches):
            assert R.acc_chunk_len(end - lo, p["nchunks"]) == L, name
            assert all(s * R.Win(wbits).nbuckets <= k < (s + 1) * R.Win(wbits).nbuckets for k in lst.skey[lo:end])
            flushed, joined, cut, ln = R.accumulate(lst.sval, lst.skey, lst.points, curve, p["nchunks"], NB, lo, end)
            assert ln == L and all(S[k] == P for k, P in joined.items())
            assert 1 + 3 * len(R.crowded(cut)) <= p["crowd_words"]                       # the crowd list's planned size
            cuts |= {c1 - c0 + 1 for c0, c1 in cut.values()}
            assert name == "whole" or lst.skey[end - 1] in cut                           # a cut bucket that ends at `end`
        assert cuts == (set() if name == "whole" else {2, 3, 4, 5, 6, 7, 9}), name


@pytest.mark.parametrize("curve", CURVES)
def test_probe_refuses_inconsistent_lists(curve):
    """Each kind of list the sort could not have written is refused by the probe's check, and by the
    accumulate stage itself before it allocates or launches anything (so this needs no GPU)."""
    lst, wbits, nsets, tuning, launches = MC.acc_cases(curve)["len4"]
    call = MP.Call(MC.acc_classes(launches, nsets), nsets, [1, 0, 0, 1, 0], wbits)
    NB, T, npts = MP.plan(curve, call)["NB"], len(lst), len(lst.points)
    pts = [w for P in lst.points for w in R.affine_words(P, curve)]
    off, cnt = R.off_cnt(lst.skey, NB)
    swapped = list(lst.skey)
    swapped[10], swapped[11] = swapped[11] + 1, swapped[10]             # keys not non-decreasing
    stray = list(lst.sval)
    stray[next(e for e in range(1, T) if lst.skey[e] == lst.skey[e - 1])] |= R.SV_FIRST
    missing = list(lst.sval)
    missing[0] &= ~R.SV_FIRST
    off2 = list(off)
    off2[lst.skey[40]] += 1                                             # off disagrees with skey
    cnt2 = list(cnt)
    cnt2[next(k for k in range(NB) if not cnt[k])] = 1                  # a count for a bucket without entries
    beyond = list(lst.skey)
    beyond[-1] = NB                                                     # a key outside the sets
    assert MP.check_sorted(curve, call, npts, lst.sval, lst.skey, off, cnt, T)
    for what, (c, n, sval, skey, o, k) in {
            "keys": (call, npts, lst.sval, swapped, off, cnt), "stray SV_FIRST": (call, npts, stray, lst.skey, off, cnt),
            "missing SV_FIRST": (call, npts, missing, lst.skey, off, cnt), "off": (call, npts, lst.sval, lst.skey, off2, cnt),
            "cnt": (call, npts, lst.sval, lst.skey, off, cnt2), "key range": (call, npts, lst.sval, beyond, off, cnt),
            "point index": (call, 3, lst.sval, lst.skey, off, cnt),
            "emax": (call.but(emax=T + 15), npts, lst.sval, lst.skey, off, cnt)}.items():
        assert not MP.check_sorted(curve, c, n, sval, skey, o, k, T), what
        with pytest.raises(MP.Refused):
            MP.accumulate(curve, c, pts[:n * len(pts) // npts], sval, skey, o, k, T)


@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_sort_cases_stay_inside_their_bins(curve, wbits):
    """The sort cases' scalars respect their classes' bounds (the contract asserts that no entry
    falls into a bucket the narrowed bins do not cover), the narrow top windows do narrow a set at
    c = 13, and the big-bin case does pass FINE_STAGE."""
    for build in (MC.sort_edges, MC.sort_tiles, MC.sort_big_bin):
        case = build(curve, wbits)
        digs = R.digits(case["classes"], case["scalars"], case["inf"], wbits)
        ents = R.entries(case["classes"], digs, wbits)
        for full in (False, True):
            sh = R.set_shifts(case["classes"], case["nsets"], wbits, full)
            want = R.sort_contract(ents, case["nsets"], sh, wbits)
            assert want["total"] == sum(len(v) for v in ents.values()) == len(want["skey"])
            if build is MC.sort_edges and not full:
                assert (min(sh) < R.COARSE_SHIFT) == (wbits == 13)
            if build is MC.sort_big_bin:
                assert max(want["coarse_cnt"]) > R.FINE_STAGE
        call = MP.Call(case["classes"], case["nsets"], case["mw"], wbits)
        p = MP.plan(curve, call)
        assert not p["small"] and p["ndig"] == len(digs) and want["total"] + 16 <= call.emax


@pytest.mark.parametrize("curve", CURVES)
def test_small_cases_plan_small(curve):
    """Every small case plans small, and the cases together run every named scalar edge: 0, 1, r - 1
    and the three Booth extremes as 8-word scalars, and as 4-word scalars under both signs."""
    full, half = set(), set()
    for name, (classes, scal, points, inf, mw, nsets, want) in MC.small_cases(curve).items():
        p = MP.plan(curve, MP.Call(classes, nsets, mw, 16, tuning=dict(small_terms=4096)))
        assert p["small"] and p["n_small_terms"] == len(points) == len(inf) and len(want) == mw[0], name
        for count, pt_base, sw, nwin, set_base, stride, so, win_off in classes:
            for i in range(count):
                if not inf[pt_base + i]:
                    k = R.scalar_of(scal[so + i * stride: so + i * stride + sw], sw)
                    (full if sw == 8 else half).add(k[0] if sw == 8 else k)
    edge8, edge4 = MC.small_edges(curve)
    assert len(set(edge8)) == 6 and len(set(edge4)) == 10
    assert set(edge8) <= full and {(m, bool(s)) for m, s in edge4} <= half
    sizes = {len(c[1]) // 8 for n, c in MC.small_cases(curve).items() if n.startswith("leaves")}
    assert sizes == {1, 2, 3, 5, 64, 65}


@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_segment_forms_and_window_sums(curve, wbits):
    """The reduction stores of the GPU tests through the model: both segment forms recombine to
    sum_b (b + 1) S_b, and the stores' records are inside their bounds (record_store asserts it)."""
    for nsets in (1, 3):
        S = MC.reduce_store(curve, wbits, nsets)
        NB = nsets * R.Win(wbits).nbuckets
        acc, cnt = MC.record_store(curve, S, NB, MC.rng_of("store", curve, wbits, nsets))
        assert sum(1 for x in cnt if x) == len(S)
        ws = R.winsums(S, nsets, wbits, curve)
        for four in (False, True):
            assert R.winsum_from_segments(R.segments(S, nsets, wbits, curve, four), nsets, wbits, curve, four) == ws
        if nsets == 3:
            assert ws[1] is None and ws[0] == MC.base_points(curve)[1][0]
