"""The row accumulation on the GPU (csrc/msm.hpp k_items_hist / k_items_scan / k_items_scatter,
k_accumulate_rows, k_join_rows through Launch<Cv>::row_items and accumulate_rows) against the
big-integer model of tests/msmref.py and tests/msmrowsref.py: the stage probe pattern of
tests/test_gpu_msm_stages.py (every buffer at its planned size behind a guard, outputs poisoned
first) on the hand-made list of tests/msmrowscases.py with the item length forced to 8, the chained
pipeline against the C oracle's MSM, and one batch over the slots of a context that is forced onto
the path.  Every comparison is exact."""
import hashlib
import os

import numpy as np
import pytest

import fieldref as F
import msmcases as MC
import msmprobe as MP
import msmref as R
import msmrowscases as RC
import msmrowsprobe as RP
import msmrowsref as RR
from oracle import oracle as O
from oracle.pyspec import curves as pc, kzg as pk

pytestmark = pytest.mark.gpu

CURVES = F.CURVES
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


@pytest.mark.parametrize("curve", CURVES)
def test_items_rows_and_joins(curve):
    """The hand-made list (lengths 1, 2, L, L + 1, 2 L + 1, empty buckets between, a short last row,
    mixed rows, the in-item doubling at offset 1 and at the last offset, runs through O, items and
    pieces that sum to O, negated entries, buckets cut into 4 and 6 items) at L = 8.  The item list is
    the model's, class by class, lengths never increasing; every bucket with cnt > 0 is the model's
    sum in a record inside the bounds; every piece record is its piece's sum; the records of the
    buckets the chunk kernels do not cut either are theirs word for word; nothing else is written."""
    b = RC.rows_list(curve)
    T, L = len(b), RC.L
    call = MP.Call(RC.classes(T), 1, ONE_WINDOW, RC.WBITS)
    points = [w for P in b.points for w in R.affine_words(P, curve)]
    NB = MP.plan(curve, call)["NB"]
    off, cnt = R.off_cnt(b.skey, NB)
    out = RP.accumulate(curve, call, points, b.sval, b.skey, off, cnt, T, row_len=L)
    intact(out)
    p, nw = out["plan"], out["rec_words"]
    poison = word(call.poison)
    # ---- the items
    its = RR.items(off, cnt, L)
    want_cut = RR.cut_buckets(cnt, L)
    assert out["nitems"] == len(its) and out["hist"] == RR.histogram(its, L)
    assert out["ncut"] == len(want_cut) and out["pieces"] == sum(want_cut.values())
    assert RR.slots_ok(out["cuts"], want_cut, out["pieces"]), out["cuts"]
    slots = {k: s for k, s, _ in out["cuts"]}
    got = out["items"]
    lens = [ln for _, _, ln in got]
    rows = RR.rows(lens)                                                       # (asserts: lengths never increase)
    assert rows[-1][1] < 64 and len(rows) == (len(its) + 63) // 64
    runs, model = RR.class_runs(out["hist"]), RR.classes(its)
    for ln, (lo, hi) in runs.items():
        want = sorted((first, RR.record_index(key, piece, NB, slots)) for first, key, piece in model[ln])
        assert sorted((first, rec) for rec, first, _ in got[lo:hi]) == want, "class %d" % ln
    assert (out["items_rest"] == poison).all() and (out["cuts_rest"] == poison).all()
    # ---- the records
    ents = {}
    for v, k in zip(b.sval, b.skey):
        ents.setdefault(k, []).append(v & ~R.SV_FIRST)
    S = R.bucket_sums(ents, b.points, curve)
    assert set(S) == {k for k in range(NB) if cnt[k]}
    for key, want in S.items():
        record_ok(out["acc"], key, want, curve, "bucket %d" % key)
    for key, piece, first, ln in its:
        if piece is not None:
            record_ok(out["acc"], NB + slots[key] + piece, RR.item_sum(b.sval, first, ln, b.points, curve), curve,
                      "piece %d of bucket %d" % (piece, key))
    acc = out["acc"].reshape(-1, nw)
    assert acc.shape[0] == NB + max(2 * p["pieces"], p["row_pieces"])
    untouched = np.ones(acc.shape[0], dtype=bool)
    untouched[[k for k in S]] = False
    untouched[NB:NB + out["pieces"]] = False
    assert (acc[untouched] == poison).all(), "a record of an empty bucket or a free piece slot was written"
    # ---- the chunk kernels on the same list: the buckets neither path cuts agree word for word
    old = MP.accumulate(curve, call, points, b.sval, b.skey, off, cnt, T)
    intact(old)
    _, _, old_cuts, _ = R.accumulate(b.sval, b.skey, b.points, curve, MP.plan(curve, call)["nchunks"], NB)
    same = [k for k in S if k not in want_cut and k not in old_cuts]
    assert len(same) > 1000 and any(cnt[k] == L for k in same)
    old_acc = old["acc"].reshape(-1, nw)
    assert (acc[same] == old_acc[same]).all()


@pytest.mark.parametrize("wbits", MC.WBITS)
@pytest.mark.parametrize("curve", CURVES)
def test_chained_rows_give_the_oracle_msm(curve, wbits):
    """sort -> items -> rows -> joins -> reduce -> combine in one chain on a mixed term list of some
    3000 window entries in 3 sets (tests/msmcases.py chained), at L = 8 so that its crowded buckets are
    cut and joined: the two results are the C oracle's MSMs."""
    case = MC.chained(curve, wbits, n=192)
    call = MP.Call(case["classes"], case["nsets"], case["mw"], wbits)
    assert 2500 < call.emax < 6000
    out = RP.msm(curve, call, case["scalars"], [w for P in case["points"] for w in R.affine_words(P, curve)],
                 case["inf"], row_len=RC.L)
    intact(out)
    assert out["ncut"] > 0 and out["nitems"] > 64
    got = [R.xyzz_point(out["res"], m, curve) for m in range(2)]
    assert got == [MC.oracle_msm(curve, w) for w in case["want"]]


def _context_env(slots, **env):
    import kzgmi
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzgmi.Context(0, slots)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_one_batch_over_the_slots_forced_onto_rows():
    """One 2^15-tuple BLS12-381 batch enqueued asynchronously on the 4 slots of a context whose tuning
    key forces the row path (L = 256 as shipped), the copy on slot 2 with a corrupted y: three verdicts
    True and one False, and every accepted slot's combination bit-exact against the oracle."""
    import torch
    curve = "bls12_381"
    C = pc.CURVES[curve]
    n, tau = 1 << 15, 0xC0FFEE + 29
    g1b = 2 * C.fp_bytes
    ctx = _context_env(4, KZGMI_ACC_ROWS="1")
    try:
        d = [torch.empty(n * w, dtype=torch.uint8, device="cuda") for w in (g1b, 32, 32, g1b)]
        ctx.gen_tuples(curve, tau, hashlib.sha256(b"rows-slots").digest(), n, *d)
        host = [t.cpu().numpy() for t in d]
        bad_y = d[2].clone()
        bad_y[32 * (n // 3) + 31] ^= 1
        g2 = pk.g2_to_bytes(C.g2, C)
        tg2 = O.g2_mul(curve, g2, tau)
        srs = ctx.load_srs(curve, g2, tg2)
        seed = hashlib.sha256(b"rows-slots-verify").digest()
        for slot in range(4):
            ctx.batch_verify_async(srs, slot, d[0], d[1], bad_y if slot == 2 else d[2], d[3], n, seed=seed)
        ok_o, Ao, Bo = O.batch_verify(curve, *(a.tobytes() for a in host), n, g2, tg2, seed, want_ab=True)
        bad = [host[0], host[1], bad_y.cpu().numpy(), host[3]]
        assert ok_o is True and O.batch_verify(curve, *(a.tobytes() for a in bad), n, g2, tg2, seed) is False
        assert [ctx.wait(slot) for slot in range(4)] == [True, True, False, True]
        assert ctx.last_combination(curve) == (Ao, Bo)                         # (slot 0's)
        del srs
    finally:
        ctx.close()
