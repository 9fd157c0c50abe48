"""The row accumulation (csrc/msm.hpp k_items_*, k_accumulate_rows, k_join_rows) in the big-integer
model of tests/msmref.py: the items of a sorted list, their size-sorted order, the rows a wave
walks, the record every item is stored in, the plan's sizes and the planner's choice of path."""
import msmref as R

ROW_LEN_MAX = 256
ROWS_FROM = 1 << 23          # MsmTuning::ROWS_FROM
RQ_WORDS = 4 + 2 * (ROW_LEN_MAX + 1)


def items(off, cnt, L):
    """[(key, piece, first entry, length)] in key order: a bucket of cnt <= L entries is one item
    (piece None), a longer one ceil(cnt / L) pieces of L entries, the last one the rest."""
    out = []
    for key, (o, c) in enumerate(zip(off, cnt)):
        if 0 < c <= L:
            out.append((key, None, o, c))
        for j in range((c + L - 1) // L if c > L else 0):
            out.append((key, j, o + j * L, min(L, c - j * L)))
    return out


def cut_buckets(cnt, L):
    """{key: pieces} of the buckets longer than L"""
    return {k: (c + L - 1) // L for k, c in enumerate(cnt) if c > L}


def histogram(its, L):
    h = [0] * (L + 1)
    for _, _, _, ln in its:
        h[ln] += 1
    return h


def classes(its):
    """{length: sorted [(first entry, key, piece)]}: the list holds each class as a run, in any order"""
    out = {}
    for key, piece, first, ln in its:
        out.setdefault(ln, []).append((first, key, piece))
    return {ln: sorted(v, key=lambda t: t[0]) for ln, v in out.items()}


def class_runs(h):
    """{length: (start, end)} of the descending list"""
    out, run = {}, 0
    for ln in range(len(h) - 1, 0, -1):
        if h[ln]:
            out[ln] = (run, run + h[ln])
            run += h[ln]
    return out


def rows(lengths):
    """[(trip count, live lanes, idle lane slots)] of a list of lengths, which must not increase:
    row r is items [64 r, 64 r + 64), walked for as long as its first (longest) item."""
    assert all(a >= b for a, b in zip(lengths, lengths[1:])), "lengths increase"
    out = []
    for r in range(0, len(lengths), 64):
        row = lengths[r:r + 64]
        out.append((row[0], len(row), sum(row[0] - ln for ln in row)))
    return out


def record_index(key, piece, NB, slots):
    """The record an item is stored in: the bucket's own, or piece slot `piece` of the bucket's run
    of slots behind the NB bucket records (slots: {key: first slot}, handed out by the device)."""
    return key if piece is None else NB + slots[key] + piece


def slots_ok(cuts, want, pieces):
    """cuts: the device's {(key, first slot, pieces)}; want: cut_buckets().  The runs of slots are
    disjoint and fill [0, pieces)."""
    if {(k, n) for k, _, n in cuts} != set(want.items()):
        return False
    used = sorted((s, s + n) for _, s, n in cuts)
    return all(a[1] == b[0] for a, b in zip(used, used[1:])) and (not used or (used[0][0] == 0 and used[-1][1] == pieces)) \
        and (bool(used) or pieces == 0)


def item_sum(sval, first, ln, points, curve):
    run = None
    for e in range(first, first + ln):
        run = R.add(run, R.value_point(sval[e], points, curve), curve)
    return run


def sizes(NB, emax, L, rec_bytes, old_pieces):
    """The plan's row fields for a call of NB buckets and at most emax entries."""
    cuts = emax // L + 1
    pieces = 2 * cuts
    cap = (NB + pieces + 63) // 64 * 64
    return dict(row_len=L, row_cuts=cuts, row_pieces=pieces, row_items=cap, rowq=4 * RQ_WORDS, items=12 * cap,
                cuts=12 * cuts, acc29=(NB + max(2 * old_pieces, pieces)) * rec_bytes)


def sizes_hold(off, cnt, emax, L, s):
    """No list of at most emax entries overruns the sizes: checked on this one."""
    its = items(off, cnt, L)
    cut = cut_buckets(cnt, L)
    return len(its) <= s["row_items"] and len(cut) <= s["row_cuts"] and sum(cut.values()) <= s["row_pieces"]


def selects_rows(curve, acc_rows, emax, part, split, acc_threads, sync_call, async_call):
    """MsmPlan::rows: only the unsplit static launch into the one store; forced, or by default the
    asynchronous BLS12-381 batches of at least ROWS_FROM entries."""
    if part != 0 or split or acc_threads:
        return False
    if acc_rows > 0:
        return True
    return acc_rows < 0 and curve == "bls12_381" and async_call and not sync_call and emax >= ROWS_FROM
