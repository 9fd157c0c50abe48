"""CPU side of the row accumulation's tests (tests/test_gpu_msm_rows.py runs it on the GPU): the
model of tests/msmrowsref.py on the hand-made list of tests/msmrowscases.py, the plan's row fields
(csrc/msm_plan.hpp, through the host-only plan call of tests/native/msm_rows_probe.hip) against the
model's sizes, and the planner's choice of path -- above all that every call of the existing stage
tests keeps the equal-chunk kernels."""
import pytest

import fieldref as F
import msmcases as MC
import msmprobe as MP
import msmref as R
import msmrowscases as RC
import msmrowsprobe as RP
import msmrowsref as RR
import planprobe as PP

CURVES = F.CURVES
ONE_WINDOW = [1, 0, 0, 1, 0]


def rows_call(total, **kw):
    return MP.Call(RC.classes(total), 1, ONE_WINDOW, RC.WBITS, **kw)


@pytest.fixture(scope="module")
def lists():
    return {c: RC.rows_list(c) for c in CURVES}


@pytest.mark.parametrize("curve", CURVES)
def test_list_meets_the_probe_and_holds_every_case(curve, lists):
    """The hand-made list passes the check the probe makes before it launches, and holds what its
    docstring promises: the lengths, the cut buckets, a last row that is not full, mixed rows."""
    b = lists[curve]
    call = rows_call(len(b))
    p = RP.plan(curve, call, acc_rows=1, row_len=RC.L)
    assert p["rows"] == 1 and p["row_len"] == RC.L and p["nchunks"] == 512          # two blocks
    off, cnt = R.off_cnt(b.skey, p["NB"])
    assert MP.check_sorted(curve, call, len(b.points), b.sval, b.skey, off, cnt, len(b))
    its = RR.items(off, cnt, RC.L)
    lens = sorted((it[3] for it in its), reverse=True)
    assert {1, 2, RC.L, RC.L + 1, 2 * RC.L + 1} <= set(cnt)
    assert max(RR.cut_buckets(cnt, RC.L).values()) >= 4 and any(c == 0 for c in cnt[:b.key])
    assert len(its) % 64 and len(its) > 128
    rows = RR.rows(lens)
    assert rows[-1][1] < 64 and any(idle for _, _, idle in rows[:-1])           # a short last row, mixed rows
    assert sum(h * ln for ln, h in enumerate(RR.histogram(its, RC.L))) == len(b)
    S = R.bucket_sums({k: [v & ~R.SV_FIRST for v, kk in zip(b.sval, b.skey) if kk == k] for k in set(b.skey)},
                      b.points, curve)
    assert any(P is None for P in S.values())                                   # a bucket that sums to O
    for key, piece, first, ln in its:                                           # the pieces of a bucket add up to it
        if piece == 0:
            n = RR.cut_buckets(cnt, RC.L)[key]
            parts = [RR.item_sum(b.sval, first + j * RC.L, min(RC.L, cnt[key] - j * RC.L), b.points, curve) for j in range(n)]
            assert R.total(parts, curve) == S[key]


def test_items_and_rows_model():
    off, cnt = [0, 0, 3, 3, 11, 28, 28], [0, 3, 0, 8, 17, 0, 9]
    its = RR.items(off, cnt, 8)
    assert its == [(1, None, 0, 3), (3, None, 3, 8), (4, 0, 11, 8), (4, 1, 19, 8), (4, 2, 27, 1), (6, 0, 28, 8), (6, 1, 36, 1)]
    assert RR.cut_buckets(cnt, 8) == {4: 3, 6: 2}
    h = RR.histogram(its, 8)
    assert h == [0, 2, 0, 1, 0, 0, 0, 0, 4] and RR.class_runs(h) == {8: (0, 4), 3: (4, 5), 1: (5, 7)}
    assert RR.classes(its)[8] == [(3, 3, None), (11, 4, 0), (19, 4, 1), (28, 6, 0)]
    assert RR.record_index(3, None, 100, {}) == 3 and RR.record_index(4, 2, 100, {4: 2, 6: 0}) == 104
    assert RR.slots_ok({(4, 2, 3), (6, 0, 2)}, {4: 3, 6: 2}, 5)
    assert not RR.slots_ok({(4, 1, 3), (6, 0, 2)}, {4: 3, 6: 2}, 5)              # overlapping runs
    assert not RR.slots_ok({(4, 2, 3)}, {4: 3, 6: 2}, 5)
    assert RR.rows([9] * 64 + [9, 8, 1]) == [(9, 64, 0), (9, 3, 9)]
    with pytest.raises(AssertionError):
        RR.rows([1, 2])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("L,emax", [(8, 5016), (8, 1 << 12), (256, 1 << 20), (256, (1 << 25) + 16), (1, 100)])
def test_plan_sizes_follow_the_model(curve, L, emax):
    """row_items / row_pieces / row_cuts and the byte sizes are the model's; the worst lists of emax - 16
    entries fit them: every bucket one entry longer than L, one bucket holding everything, all single."""
    nsets = 24 if emax > 1 << 22 else 1
    wbits = 16 if emax > 1 << 20 else 13
    H = 8
    classes = [[(emax - 16) // (3 * H), 0, 4, H, 0, 4, 0, 0]] * 3 if nsets > 1 else RC.classes(emax - 16)
    call = MP.Call(classes, nsets, [2, 0, 8, 8, 16] if nsets > 1 else ONE_WINDOW, wbits, emax=emax, alone=False, sync_call=False)
    p = RP.plan(curve, call, acc_rows=1, row_len=L)
    assert p["rows"] == 1
    rec = 4 * R.layers(curve)[0].N * 4
    want = RR.sizes(p["NB"], emax, L, rec, p["pieces"])
    assert {k: p[k] for k in want} == want
    if emax <= 1 << 20:
        T, NB = emax - 16, p["NB"]
        for cnt in ([L + 1] * min(NB, T // (L + 1)), [T], [1] * min(NB, T), [2 * L] * min(NB, T // (2 * L))):
            cnt = cnt + [0] * (NB - len(cnt))
            off, run = [], 0
            for c in cnt:
                off.append(run)
                run += c
            assert RR.sizes_hold(off, cnt, emax, L, want)
    off_rows = RP.plan(curve, call, acc_rows=0, row_len=L)
    assert off_rows["rows"] == 0 and off_rows["rowq"] == off_rows["items"] == off_rows["cuts"] == 0
    assert off_rows["acc29"] == (p["NB"] + 2 * p["pieces"]) * rec                 # the parent's size


def _stage_test_calls(curve):
    """Every call the existing stage tests plan (tests/test_gpu_msm_stages.py): sort, accumulation and
    joins, merge, reduction, combination, the chained pipeline."""
    for wbits in MC.WBITS:
        for case, flags in ((MC.sort_edges(curve, wbits), {}), (MC.sort_edges(curve, wbits), {"sort_split": 1}),
                            (MC.sort_edges(curve, wbits), {"sort_full_bins": 1}), (MC.sort_tiles(curve, wbits), {}),
                            (MC.sort_big_bin(curve, wbits), {})):
            yield MP.Call(case["classes"], case["nsets"], case["mw"], wbits, tuning=flags)
        ch = MC.chained(curve, wbits)
        yield MP.Call(ch["classes"], ch["nsets"], ch["mw"], wbits)
        for nsets in (1, 3):
            yield MP.Call([[100, 0, 4, 1, 0, 4, 0, 0]], nsets, [1, 0, 0, nsets, 0], wbits)
    for name, (lst, wbits, nsets, tuning, launches) in MC.acc_cases(curve).items():
        yield MP.Call(MC.acc_classes(launches, nsets), nsets, [nsets, 0, nsets - 1, 1, nsets - 1], wbits, tuning=tuning)
    yield MP.Call([[100, 0, 4, 1, 0, 4, 0, 0]], 1, ONE_WINDOW, 13, part=3)


@pytest.mark.parametrize("curve", CURVES)
def test_stage_test_calls_keep_the_chunk_kernels(curve):
    """With the shipped tuning (acc_rows = -1) no call of the existing stage tests takes the row path,
    whichever way it is issued, and its bucket store keeps the parent's size."""
    n = 0
    for call in _stage_test_calls(curve):
        for sync_call in (True, False):
            for async_call in (False, True):
                p = RP.plan(curve, call.but(sync_call=sync_call), async_call=async_call)
                assert p["rows"] == 0 and p["rowq"] == p["items"] == p["cuts"] == 0, call.classes
                assert p["acc29"] == MP.plan(curve, call)["acc29"]
        n += 1
    assert n >= 20


@pytest.mark.parametrize("curve", CURVES)
def test_selection_rule(curve):
    """MsmPlan::rows against the model: asynchronous BLS12-381 batches of at least 2^23 entries on the
    unsplit static launch; synchronous calls, split launches, the work-queue grid (>= 2^26 entries),
    chunked ranges and smaller calls keep the chunk kernels; the tuning key forces either."""
    H = 8
    for tuples in (1 << 15, 1 << 17, (1 << 18) - 1, 1 << 18, 1 << 20, 1 << 21):
        classes = [[tuples, 0, 4, H, 0, 4, 0, 0], [tuples, tuples, 4, H, H, 4, 0, 0], [tuples, 0, 8, 2 * H, H, 8, 0, 0]]
        emax = 32 * tuples + 16
        for acc_rows in (-1, 0, 1):
            for part in (0, 1, 3):
                for alone in (True, False):
                    for sync_call, async_call in ((True, True), (False, True), (False, False), (True, False)):
                        call = MP.Call(classes, 3 * H, [2, 0, H, H, 2 * H], 16, emax=emax, part=part, alone=alone,
                                       sync_call=sync_call, tuning=dict(split_acc=-1))
                        p = RP.plan(curve, call, acc_rows=acc_rows, async_call=async_call)
                        want = RR.selects_rows(curve, acc_rows, emax, part, p["split"], p["acc_threads"], sync_call,
                                               async_call)
                        assert p["rows"] == int(want), (tuples, acc_rows, part, alone, sync_call, async_call)
                        if sync_call and alone and part == 0 and emax >= 1 << 25:
                            assert p["split"] == 1 and not want
    # the work-queue grid: 2^26 entries
    tuples = 1 << 22
    call = MP.Call([[tuples, 0, 8, 16, 0, 8, 0, 0]], 16, [1, 0, 0, 16, 0], 16, emax=16 * tuples + 16, alone=False,
                   sync_call=False)
    p = RP.plan(curve, call, acc_rows=1, async_call=True)
    assert p["acc_threads"] and p["rows"] == 0
    # the flagship shape takes rows on BLS12-381 only, and its bucket store keeps the parent's size
    tuples = 1 << 20
    classes = [[tuples, 0, 4, H, 0, 4, 0, 0], [tuples, tuples, 4, H, H, 4, 0, 0], [tuples, 0, 8, 2 * H, H, 8, 0, 0]]
    call = MP.Call(classes, 3 * H, [2, 0, H, H, 2 * H], 16, emax=32 * tuples + 16, alone=False, sync_call=False)
    p = RP.plan(curve, call, async_call=True)
    assert p["rows"] == int(curve == "bls12_381")
    assert p["acc29"] == RP.plan(curve, call, acc_rows=0, async_call=True)["acc29"]


def test_the_forced_slot_test_plans_rows():
    """The call of tests/test_gpu_msm_rows.py's 4-slot test -- a 2^15-tuple BLS12-381 batch as batch_terms
    lays it out (no GLV, 127-bit randomisers, 16-bit windows), asynchronous, alone or beside other slots --
    takes the row path under KZGMI_ACC_ROWS=1 with L = 256, and the chunk kernels without the key: that
    test's verdicts and combination come from k_accumulate_rows."""
    n = 1 << 15
    tuning = dict(MP.TUNING, small_terms=4096, split_acc=-1)
    wb = PP.call_wbits(tuning, 32 * n, 1 << 22)
    H, Fw = PP.windows(wb)
    bt = PP.batch_terms(False, False, 0, H, Fw, n, 0, 0, n, True)
    classes = [c[:6] + [0, c[7]] for c in bt["tl"]["c"]]
    assert wb == 16 and bt["emax"] == 32 * n + Fw + 16
    for alone in (True, False):
        call = MP.Call(classes, bt["nsets"], bt["mw"], wb, emax=bt["emax"], alone=alone, sync_call=False, tuning=tuning)
        forced = RP.plan("bls12_381", call, acc_rows=1, async_call=True)
        assert forced["small"] == 0 and forced["rows"] == 1 and forced["row_len"] == RP.ROW_LEN and not forced["split"]
        assert RP.plan("bls12_381", call, acc_rows=-1, async_call=True)["rows"] == 0      # below 2^23 entries
