"""The row accumulation's arithmetic paths on the GPU (csrc/msm.hpp acc_row29: the lazily negated
q.y of the hot loop, the normalised forms of the prologue, the restart after P + (-P) and the
doubling) through the unchanged probe of tests/msmrowsprobe.py, on the hand-made lists of
tests/msmrowsarithcases.py at L = 8: every entry negative, alternating signs, and a mixed list with a
negative first entry in every bucket, buckets of 1, 2 and 3 entries by the row, a bucket cut and
joined, buckets that double or cancel at their first and second addition, and points whose x is a
tiny residue as first and as second entry.  The last three kinds, and a pair whose PP is a residue
under the threshold, make a wave leave the peeled first addition (BLS12-381) for the generic body;
every other row takes the peel.  Both curves: the lazy negation runs on both.  Every
record decodes to the big-integer sum inside the record bounds, the records of buckets that neither
path cuts equal the chunk kernels' word for word, and nothing outside the planned sizes is written."""
import numpy as np
import pytest

import fieldref as F
import msmprobe as MP
import msmref as R
import msmrowsarithcases as AC
import msmrowsprobe as RP
import msmrowsref as RR

pytestmark = pytest.mark.gpu

ONE_WINDOW = [1, 0, 0, 1, 0]


def intact(out):
    assert out["guards"] and all(out["guards"].values()), "a kernel wrote past a planned size: %s" % out["guards"]


def record_ok(arr, idx, want, curve, what):
    w = R.records(arr, idx, curve)
    msg = R.check_record(w, curve)
    assert msg is None, "%s: %s" % (what, msg)
    assert R.decode_record(w, curve)[0] == want, what


@pytest.mark.parametrize("pattern", AC.PATTERNS)
@pytest.mark.parametrize("curve", F.CURVES)
def test_rows_on_sign_patterns_and_degenerate_buckets(curve, pattern):
    b = AC.arith_list(curve, pattern)
    T, L = len(b), AC.L
    assert 2500 <= T <= 6000 and AC.signs_hold(b, pattern)
    call = MP.Call(AC.classes(T), 1, ONE_WINDOW, AC.WBITS)
    points = [w for P in b.points for w in R.affine_words(P, curve)]
    NB = MP.plan(curve, call)["NB"]
    off, cnt = R.off_cnt(b.skey, NB)
    assert {1, 2, 3} <= set(cnt) and max(cnt) > L
    if pattern == "mixed":
        assert all(AC.limb_top_is_tiny(curve, P) for P in b.points[64:][-2:])
    out = RP.accumulate(curve, call, points, b.sval, b.skey, off, cnt, T, row_len=L)
    intact(out)
    p, nw = out["plan"], out["rec_words"]
    poison = 0x01010101 * call.poison
    # ---- the items: the model's count and histogram, the one long bucket cut
    its = RR.items(off, cnt, L)
    want_cut = RR.cut_buckets(cnt, L)
    assert out["nitems"] == len(its) and out["hist"] == RR.histogram(its, L)
    assert len(want_cut) == 1 and RR.slots_ok(out["cuts"], want_cut, out["pieces"]), out["cuts"]
    slots = {k: s for k, s, _ in out["cuts"]}
    RR.rows([ln for _, _, ln in out["items"]])                                 # (asserts: lengths never increase)
    # ---- every record is the big-integer sum, inside the record bounds
    ents = {}
    for v, k in zip(b.sval, b.skey):
        ents.setdefault(k, []).append(v & ~R.SV_FIRST)
    S = R.bucket_sums(ents, b.points, curve)
    assert set(S) == {k for k in range(NB) if cnt[k]}
    if pattern == "mixed":
        assert sum(1 for P in S.values() if P is None) >= 3, "buckets that sum to O"
    for key, want in S.items():
        record_ok(out["acc"], key, want, curve, "bucket %d" % key)
    for key, piece, first, ln in its:
        if piece is not None:
            record_ok(out["acc"], NB + slots[key] + piece, RR.item_sum(b.sval, first, ln, b.points, curve), curve,
                      "piece %d of bucket %d" % (piece, key))
    acc = out["acc"].reshape(-1, nw)
    assert acc.shape[0] == NB + max(2 * p["pieces"], p["row_pieces"])
    untouched = np.ones(acc.shape[0], dtype=bool)
    untouched[list(S)] = False
    untouched[NB:NB + out["pieces"]] = False
    assert (acc[untouched] == poison).all(), "a record of an empty bucket or a free piece slot was written"
    # ---- the chunk kernels on the same list: the buckets neither path cuts agree word for word
    old = MP.accumulate(curve, call, points, b.sval, b.skey, off, cnt, T)
    intact(old)
    _, _, old_cuts, _ = R.accumulate(b.sval, b.skey, b.points, curve, MP.plan(curve, call)["nchunks"], NB)
    same = [k for k in S if k not in want_cut and k not in old_cuts]
    assert len(same) > 500
    old_acc = old["acc"].reshape(-1, nw)
    assert (acc[same] == old_acc[same]).all()
