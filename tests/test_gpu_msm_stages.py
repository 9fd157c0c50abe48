"""The bucket MSM pipeline stage by stage on the GPU against the big-integer model of
tests/msmref.py: the shipped launchers of csrc/launch_msm.hip run one stage per call through the
test-only probe (tests/native/msm_probe.hip, tests/msmprobe.py) on the inputs of tests/msmcases.py.
Every buffer has the size plan_msm gives it and a guard behind it; the buffers a stage writes hold
a poison word first.  Every comparison is exact: integers equal, points equal as affine group
elements, record coordinates inside the bounds tests/fieldref.py states; no tolerance anywhere."""
import numpy as np
import pytest

import fieldref as F
import msmcases as MC
import msmprobe as MP
import msmref as R

pytestmark = pytest.mark.gpu

CURVES = F.CURVES
CW = [(c, w) for c in CURVES for w in MC.WBITS]
CW_IDS = ["%s-c%d" % cw for cw in CW]
ONE_WINDOW = [1, 0, 0, 1, 0]


def word(poison):
    return 0x01010101 * poison


def intact(out):
    assert out["guards"] and all(out["guards"].values()), "a kernel wrote past a planned size: %s" % out["guards"]


def record_ok(arr, idx, want, curve, what):
    w = R.records(arr, idx, curve)
    msg = R.check_record(w, curve)
    assert msg is None, "%s: %s" % (what, msg)
    assert R.decode_record(w, curve)[0] == want, what


# ------------------------------------------------------------------------------ digits and sort
def check_sort(curve, case, wbits, tuning):
    classes, nsets = case["classes"], case["nsets"]
    call = MP.Call(classes, nsets, case["mw"], wbits, tuning=tuning)
    p = MP.plan(curve, call)
    out = MP.sort(curve, call, case["scalars"], case["inf"])
    intact(out)
    digs = R.digits(classes, case["scalars"], case["inf"], wbits, p["dig_base"])
    assert out["digits"].tolist() == digs
    ents = R.entries(classes, digs, wbits, p["dig_base"])
    want = R.sort_contract(ents, nsets, R.set_shifts(classes, nsets, wbits, tuning.get("sort_full_bins")), wbits)
    nb, T = nsets * p["bins"], want["total"]
    coarse = out["coarse"].tolist()
    assert coarse[:nb] == want["coarse_cnt"] and coarse[nb:2 * nb] == want["coarse_off"]
    assert coarse[2 * nb:] == [o + c for o, c in zip(want["coarse_off"], want["coarse_cnt"])]   # the cursors, spent
    assert out["total"] == T
    assert out["cnt"].tolist() == want["cnt"]
    assert out["off"].tolist() == want["off"]              # every bucket, the uncovered ones of a narrowed set too
    sval, skey = out["sval"].tolist(), out["skey"].tolist()
    assert skey[:T] == want["skey"]
    assert [e for e in range(T) if sval[e] & R.SV_FIRST] == want["first"]
    for key, vals in ents.items():
        o = want["off"][key]
        assert sorted(v & ~R.SV_FIRST for v in sval[o:o + len(vals)]) == sorted(vals), key
    assert set(sval[T:]) | set(skey[T:]) <= {word(call.poison)}      # nothing written past `total`
    return out, p


@pytest.mark.parametrize("flags", [{}, {"sort_split": 1}, {"sort_full_bins": 1}], ids=["packed", "split", "fullbins"])
@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_sort_edge_scalars(curve, wbits, flags):
    """0, 1, 2^(c-1) (no carry), 2^(c-1) + 1 (carry), all ones, r - 1, 2^127 - 1 with and without the
    sign flag; low and top windows (the narrowed SetShift path at c = 13, and forced off), win_off
    > 0, a shared scalar, infinity flags, an empty class, classes of different nwin sharing sets."""
    check_sort(curve, MC.sort_edges(curve, wbits), wbits, flags)


@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_sort_tile_edges(curve, wbits):
    """Class counts 1, 4095, 4096 and 4097."""
    check_sort(curve, MC.sort_tiles(curve, wbits), wbits, {})


@pytest.mark.parametrize("flags", [{}, {"sort_split": 1}], ids=["packed", "split"])
@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_sort_chunked_bin(curve, wbits, flags):
    """One coarse bin above FINE_STAGE entries (fine_sort_chunks), several buckets inside it."""
    check_sort(curve, MC.sort_big_bin(curve, wbits), wbits, flags)


# ------------------------------------------------------------------------------ accumulation and joins
@pytest.fixture(scope="module")
def acc_cases():
    return {c: MC.acc_cases(c) for c in CURVES}


def check_accumulate(curve, lst, wbits, nsets, tuning, launches, order):
    """order: the launches in the order they run (a split's second launch keeps its pieces behind
    the first's: NB + 2 nchunks)."""
    call = MP.Call(MC.acc_classes(launches, nsets), nsets, [nsets, 0, nsets - 1, 1, nsets - 1], wbits, tuning=tuning)
    p = MP.plan(curve, call)
    NB, nch, T = p["NB"], p["nchunks"], len(lst)
    off, cnt = R.off_cnt(lst.skey, NB)
    out = MP.accumulate(curve, call, [w for P in lst.points for w in R.affine_words(P, curve)], lst.sval, lst.skey, off,
                        cnt, T, mid=launches[-1][0])
    intact(out)
    flushed, joined, crowds = {}, {}, []
    for i, li in enumerate(order):
        lo, end, L = launches[li]
        f, j, cuts, ln = R.accumulate(lst.sval, lst.skey, lst.points, curve, nch, NB + 2 * nch * i, lo, end)
        assert ln == L
        assert not set(f) & set(flushed)
        flushed.update(f)
        joined.update(j)
        crowds.append(R.crowded(cuts))
    nw = p["rec_words"]
    mid = out["acc_mid"].reshape(-1, nw)
    assert mid.shape[0] == NB + 2 * p["pieces"]
    for rec, want in flushed.items():                       # whole buckets and flushed pieces, after k_accumulate alone
        record_ok(out["acc_mid"], rec, want, curve, "record %d after k_accumulate" % rec)
    unflushed = np.ones(mid.shape[0], dtype=bool)           # piece records no chunk flushes (buckets with cnt == 0
    unflushed[:NB] = False                                  # are not asserted on)
    unflushed[[r for r in flushed if r >= NB]] = False
    assert (mid[unflushed] == word(call.poison)).all(), "k_accumulate wrote a piece record no chunk flushes"
    for key, want in joined.items():                        # every bucket with cnt > 0, after the joins
        record_ok(out["acc"], key, want, curve, "bucket %d after the joins" % key)
    assert set(joined) == {k for k in range(NB) if cnt[k]}
    crowd = out["crowd"].tolist()
    for i, want in enumerate(crowds):
        lst_ = crowd[i * p["crowd_words"]:(i + 1) * p["crowd_words"]]
        assert lst_[0] == len(want)
        assert {tuple(lst_[1 + 3 * k:4 + 3 * k]) for k in range(lst_[0])} == want


@pytest.mark.parametrize("name", ["len4", "len8", "whole", "queue"])
@pytest.mark.parametrize("curve", CURVES)
def test_accumulate_and_joins(curve, name, acc_cases):
    """Hand-written sorted lists, the order inside every bucket fixed (tests/msmcases.py
    standard_list): buckets cut into 2 .. 9 pieces, O / equal / cancelling pieces, the in-chunk
    doubling at every offset, runs through O; the static grid at two chunk lengths, whole-chunk
    buckets, and the work-queue form."""
    lst, wbits, nsets, tuning, launches = acc_cases[curve][name]
    check_accumulate(curve, lst, wbits, nsets, tuning, launches, [0])


@pytest.mark.parametrize("rev", [1, 0], ids=["msm0-first", "msm1-first"])
@pytest.mark.parametrize("curve", CURVES)
def test_accumulate_split(curve, rev, acc_cases):
    """Two launches over the two sets' ranges (lo non-null, off a 16-byte boundary), in both orders."""
    lst, wbits, nsets, tuning, launches = acc_cases[curve]["split"]
    check_accumulate(curve, lst, wbits, nsets, dict(tuning, split_rev=rev), launches, [0, 1] if rev else [1, 0])


@pytest.mark.parametrize("curve", CURVES)
def test_merge_buckets(curve):
    """(ka, kb) in {(0, n), (n, 0), (n, m)}; sums that differ, coincide (the doubling branch), cancel,
    and O on either side; the records of empty buckets are poison going in and not asserted on."""
    wbits, nsets = 13, 1
    call = MP.Call([[100, 0, 4, 1, 0, 4, 0, 0]], nsets, ONE_WINDOW, wbits, part=3)
    NB = MP.plan(curve, call)["NB"]
    pts = MC.base_points(curve)[1]
    rng = MC.rng_of("merge", curve)
    A = {1: pts[1], 2: pts[2], 3: pts[3], 4: pts[4], 5: None, 6: pts[6], NB - 1: pts[9]}
    B = {0: pts[0], 2: pts[12], 3: pts[3], 4: R.neg(pts[4], curve), 5: pts[5], 6: None, NB - 1: pts[9]}
    for _ in range(24):
        k = rng.randrange(16, NB - 1)
        A[k], B[k] = rng.choice(pts), rng.choice(pts)
    acc_a, cnt_a = MC.record_store(curve, A, NB, rng)
    acc_b, cnt_b = MC.record_store(curve, B, NB, rng)
    out = MP.merge(curve, call, acc_a, cnt_a, acc_b, cnt_b)
    intact(out)
    assert out["cnt"].tolist() == [a + b for a, b in zip(cnt_a, cnt_b)]
    nw = 4 * R.layers(curve)[0].N
    got, before = out["acc"].reshape(-1, nw), acc_a.reshape(-1, nw)
    for k in range(NB):
        if cnt_b[k]:
            record_ok(out["acc"], k, R.add(A.get(k), B[k], curve), curve, "bucket %d" % k)
        elif cnt_a[k]:
            assert (got[k] == before[k]).all()


# ------------------------------------------------------------------------------ reduction
def check_reduce(curve, wbits, nsets, four, low_prio, S, acc, cnt):
    call = MP.Call([[100, 0, 4, 1, 0, 4, 0, 0]], nsets, [1, 0, 0, nsets, 0], wbits, tuning=dict(seg4_waves=64 if four else 0))
    out = MP.reduce(curve, call, cnt, acc, low_prio)
    intact(out)
    again = MP.reduce(curve, call.but(poison=MP.POISON2), cnt, acc, low_prio)     # every cnt == 0 record: another poison
    intact(again)
    assert (out["winsum"] == again["winsum"]).all(), "the window sums depend on records of empty buckets"
    assert (out["R"] == again["R"]).all() and (out["U"] == again["U"]).all()
    W = R.Win(wbits)
    nseg = nsets * W.nseg
    segs = R.segments(S, nsets, wbits, curve, four)
    for g, (Rp, U, V) in segs.items():
        record_ok(out["R"], g, Rp, curve, "R' of segment %d" % g)
        record_ok(out["U"], g, U, curve, "U of segment %d" % g)
        record_ok(out["U"], nseg + g, V, curve, "V of segment %d" % g)
    nw = 4 * R.layers(curve)[0].N
    empty = np.ones(nseg, dtype=bool)
    empty[list(segs)] = False
    Rr, Ur = out["R"].reshape(-1, nw), out["U"].reshape(-1, nw)
    assert Rr.shape[0] == nseg and Ur.shape[0] == 2 * nseg
    n29 = nw // 4
    for name, rows in (("R'", Rr[empty]), ("U", Ur[:nseg][empty]), ("V", Ur[nseg:][empty])):
        assert not rows[:, 2 * n29:3 * n29].any(), "%s of an empty segment is not O (zz != 0)" % name
        for row in rows[rows.any(axis=1)]:                  # (an all-zero record is inside every bound)
            assert R.check_record(row.tolist(), curve) is None, name
    want = R.winsums(S, nsets, wbits, curve)
    assert [R.xyzz_point(out["winsum"], s, curve) for s in range(nsets)] == want
    return out


@pytest.mark.parametrize("nsets", [1, 3])
@pytest.mark.parametrize("four", [False, True], ids=["seg2", "seg4"])
@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_reduce_hand_made_records(curve, wbits, four, nsets):
    """Records at the edges of their bounds and in non-canonical form (random ZZ, shifted by
    multiples of p): only bucket 0, only the top bucket, a whole segment of equal points, adjacent
    buckets that cancel, an empty set; both segment forms, both priorities; every record of an empty
    bucket is poison, and a second poison must not change a word of R, U, V or the window sums."""
    S = MC.reduce_store(curve, wbits, nsets)
    NB = nsets * R.Win(wbits).nbuckets
    acc, cnt = MC.record_store(curve, S, NB, MC.rng_of("store", curve, wbits, nsets))
    check_reduce(curve, wbits, nsets, four, low_prio=(nsets == 3) != four, S=S, acc=acc, cnt=cnt)


# ------------------------------------------------------------------------------ window combination
@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_window_combine(curve, wbits):
    """The top, a middle and every window O; acc = -ws after the doublings; 2^c acc = ws (the
    doubling branch); one window; two MSMs with different set_base.  Window sums with ZZ != 1."""
    rng = MC.rng_of("combine", curve, wbits)
    p = R.layers(curve)[1].p
    for i, (name, (ws, mw, nsets)) in enumerate(MC.combine_cases(curve, wbits).items()):
        call = MP.Call([[100, 0, 4, 1, 0, 4, 0, 0]], nsets, mw, wbits)
        words = [w for P in ws for w in R.xyzz_words(P, curve, rng.randrange(1, p))]
        out = MP.combine(curve, call, words, low_prio=bool(i & 1))
        intact(out)
        want = R.combine(ws, mw, wbits, curve)
        assert [R.xyzz_point(out["res"], m, curve) for m in range(mw[0])] == want, name
        nx = len(words) // nsets
        assert set(out["res"][mw[0] * nx:].tolist()) <= {word(call.poison)}, name


# ------------------------------------------------------------------------------ small path
@pytest.mark.parametrize("curve", CURVES)
def test_small_msm(curve):
    """k_small_msm: 1, 2, 3, 5, 64 and 65 leaves and two MSMs of unequal size; scalars 0, 1, r - 1 and
    the Booth extremes 0x88..8, 0x77..7, 0xff..f masked to the class width; 4-word classes with the
    sign flag (bit 127, as its class handling documents); infinity points; siblings that cancel and
    siblings that are equal."""
    C = R.pc.CURVES[curve]
    for name, (classes, scal, points, inf, mw, nsets, wants) in MC.small_cases(curve).items():
        call = MP.Call(classes, nsets, mw, 16, tuning=dict(small_terms=4096))
        out = MP.small(curve, call, scal, [w for P in points for w in R.affine_words(P, curve)], inf)
        intact(out)
        want = [R.total([R.pc.g1_mul(points[i], k, C) for k, i in w if not inf[i]], curve) for w in wants]
        assert [R.xyzz_point(out["res"], m, curve) for m in range(mw[0])] == want, name


# ------------------------------------------------------------------------------ chained
@pytest.mark.parametrize("curve,wbits", CW, ids=CW_IDS)
def test_chained_stages_give_the_oracle_msm(curve, wbits):
    """One mixed term list, each stage fed by the previous one's output as the probe copied it back:
    sort -> accumulate and joins -> reduce -> combine ends at the C oracle's MSMs, and the buckets,
    segment records and window sums on the way are the model's."""
    case = MC.chained(curve, wbits)
    classes, nsets, mw = case["classes"], case["nsets"], case["mw"]
    call = MP.Call(classes, nsets, mw, wbits)
    srt, p = check_sort(curve, case, wbits, {})
    T = srt["total"]
    acc = MP.accumulate(curve, call, [w for P in case["points"] for w in R.affine_words(P, curve)], srt["sval"],
                        srt["skey"], srt["off"], srt["cnt"], T)
    intact(acc)
    ents = {}
    for v, k in zip(srt["sval"][:T].tolist(), srt["skey"][:T].tolist()):
        ents.setdefault(k, []).append(v & ~R.SV_FIRST)
    S = R.bucket_sums(ents, case["points"], curve)
    for key, want in S.items():
        record_ok(acc["acc"], key, want, curve, "bucket %d" % key)
    red = check_reduce(curve, wbits, nsets, four=wbits == 13, low_prio=False, S=S, acc=acc["acc"], cnt=srt["cnt"])
    res = MP.combine(curve, call, red["winsum"])
    intact(res)
    got = [R.xyzz_point(res["res"], m, curve) for m in range(2)]
    assert got == [MC.oracle_msm(curve, w) for w in case["want"]]
