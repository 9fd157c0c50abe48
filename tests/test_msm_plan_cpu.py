"""The MSM plan (csrc/msm_plan.hpp) without a GPU, through tests/planprobe.py.

1. plan_msm reproduces, value for value, what run_msm_core decided before the plan existed:
   tests/golden/msm_plan_parent.json, recorded from that commit on an MI355X (its `about` says how).
2. batch_terms builds the term lists, windows, set count and entry bound that enqueue_batch and
   enqueue_batch_chunked built there, for every (glv, powers, cell) form and the ranges of a chunked batch.
3. A context reserved for n tuples has every buffer a smaller batch of the same mode plans, as
   long as both take the same window width.  Pairs across the width switch are computed and
   printed, not asserted (test_reserve_across_the_width_switch's docstring has the figures).
"""
import json
import os

import pytest

import planprobe as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(ROOT, "tests", "golden", "msm_plan_parent.json")) as f:
        return json.load(f)["cases"]


def _plan(c):
    return P.plan(c["curve"], c["tuning"], c["tl"], c["nsets"], c["emax"], c["mw"], c["wbits"], c["part"], c["own_pts"],
                  c["alone"], c["sync_call"])


def test_golden_covers_the_switches(cases):
    """The recorded table holds what the checks below are meant to see."""
    by = lambda f: [c for c in cases if f(c)]  # noqa: E731

    def reserved(curve, glv):  # {n: case} of the reserves with 127-bit r_i
        return {c["batch"]["n"]: c for c in cases if c["dry"] and c["curve"] == curve and
                (c["batch"]["glv"], c["batch"]["powers"]) == (glv, 0)}
    b, g = reserved(0, 0), reserved(1, 1)
    assert b[1365]["out"]["small"] and not b[1366]["out"]["small"]  # 3n + 1 <= 4096 terms
    assert g[1023]["out"]["small"] and not g[1024]["out"]["small"]  # 4n + 2
    for r in (b, g, reserved(0, 1)):
        assert [r[n]["wbits"] for n in (32768, 32769, 131072, 131073)] == [16, 13, 13, 16]
    assert b[32767]["emax"] == 1 << 20 and b[32768]["emax"] > 1 << 20       # ACC_SMALL_ENTRIES
    assert (1 << 25) <= b[1 << 20]["emax"] < (1 << 26) <= b[1 << 21]["emax"]  # SPLIT_FROM, ACC_QUEUE_FROM
    assert b[1 << 20]["out"]["nchunks"] == 256 * 4 * 4 * 64 and not b[1 << 20]["out"]["acc_threads"]  # the grid at its cap
    assert b[1 << 21]["out"]["acc_threads"]                                  # the work-queue form
    assert by(lambda c: not c["alone"]) and by(lambda c: c["sync_call"]) and by(lambda c: c["out"].get("split"))
    assert {c["part"] for c in cases} == {0, 1, 2, 3}
    assert by(lambda c: c["batch"] is None and c["tl"]["c"][0][7] == 0 and c["tl"]["nclass"] == 16)  # a commit-key call
    assert by(lambda c: c["batch"] is None and c["wbits"] == 13) and by(lambda c: c["batch"] is None and c["wbits"] == 16)
    forms = {(c["batch"]["glv"], c["batch"]["powers"], c["batch"]["cell"]) for c in cases if c["batch"]}
    assert forms == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)}


def test_plan_reproduces_parent(cases):
    for c in cases:
        p, want, ctx = _plan(c), c["out"], c["tag"]
        assert p["refuse"] is None and p["small"] == want["small"], ctx
        k = c["tl"]["nclass"]
        own = max([t[1] + t[0] for t in c["tl"]["c"] if t[0]] or [0]) if c["own_pts"] else 0
        assert p["own_npts"] == own, ctx
        assert p["tl"] == c["tl"], ctx
        if want["small"]:
            assert (p["small_terms"], p["small_nodes"], p["small_flags"]) == (want["terms"], want["nodes"], want["flags"]), ctx
            for name, v in want["sp"].items():
                assert (p["sp"][name][:k] if name in ("term_base", "leaf_base", "msm") else p["sp"][name]) == v, (ctx, name)
            got = {b: v for b, v in p["bytes"].items() if v}
            assert got == want["bytes"], ctx
            continue
        assert p["dig_base"] == want["dig_base"], ctx
        for name in P.COUNTS:
            if name != "own_npts":
                assert p[name] == want[name], (ctx, name)
        assert p["bytes"] == {"small_nodes": 0, "small_flags": 0, **want["bytes"]}, ctx


def test_too_many_digits_is_refused(cases):
    c = dict(next(c for c in cases if not c["out"]["small"] and c["batch"] is None and c["tl"]["nclass"] == 1))
    cls = list(c["tl"]["c"][0])
    cls[0], cls[3] = 1 << 28, 16  # 2^32 digits
    c["tl"] = {"nclass": 1, "total": 1 << 28, "c": [cls]}
    assert _plan(c)["refuse"] == "too many window digits for one call"
    cls[0] -= 1
    c["tl"] = {"nclass": 1, "total": cls[0], "c": [cls]}
    assert _plan(c)["refuse"] is None


def test_batch_terms_reproduce_parent(cases):
    seen = set()
    for c in cases:
        b = c["batch"]
        if not b:
            continue
        assert P.call_wbits(c["tuning"], (48 if b["powers"] else 32) * b["n"], 1 << 22) == b["wb"] == c["wbits"], c["tag"]
        H, F = P.windows(b["wb"])
        got = P.batch_terms(b["glv"], b["powers"], 64 if b["cell"] else 0, H, F, b["n"], b["m"], b["lo"], b["nj"], b["last"])
        assert got == {"tl": c["tl"], "mw": c["mw"], "nsets": c["nsets"], "emax": c["emax"]}, c["tag"]
        seen.add((b["form"], b["glv"], b["last"], b["lo"] > 0))
    assert {("chunked", g, last, inner) for g in (0, 1) for last in (0, 1) for inner in (0, 1)} <= seen


def test_msm_widths(cases):
    """Plain MSMs: 16 entries per point, 13-bit windows in (2^16, 2^17] points."""
    t = cases[0]["tuning"]
    assert [P.call_wbits(t, 16 * n, 1 << 21) for n in (65536, 65537, 131072, 131073)] == [16, 13, 13, 16]
    assert P.windows(16) == (8, 16) and P.windows(13) == (10, 20)
    for forced in (13, 16):
        assert {P.call_wbits({**t, "wbits_env": forced}, e, 1 << 22) for e in (1, 1 << 21, 1 << 30)} == {forced}


# ---- reserve dominates
MODES = {"plain": (0, 0, 0), "trusted": (1, 0, 0), "powers": (0, 1, 0), "checked": (1, 0, 1)}  # glv on BLS12-381, powers, own_pts
RESERVED = [1365, 1366, 5000, 21845, 32768, 32769, 87381, 131072, 131073, 1 << 18, 1 << 20, 1 << 21]
SWITCHES = [1023, 1024, 1365, 1366, 21845, 21846, 32767, 32768, 32769, 87381, 87382, 131072, 131073]


def _pairs(tuning):
    """(curve, mode, n, n', same width, reserve plan, [(alone, sync_call, plan of n')])"""
    for curve in (0, 1):
        for mode, (glv, powers, own) in MODES.items():
            glv = glv or curve == 1
            for n in RESERVED:
                res = P.reserve(curve, tuning, glv, powers, n, own)
                wb_n = P.call_wbits(tuning, (48 if powers else 32) * n, 1 << 22)
                grid = {n, n - 17, 1, 256, 4096} | {s for s in SWITCHES} | {1 << k for k in range(10, 22)}
                for m in sorted(x for x in grid if 0 < x <= n):
                    wb = P.call_wbits(tuning, (48 if powers else 32) * m, 1 << 22)
                    H, F = P.windows(wb)
                    bt = P.batch_terms(glv, powers, 0, H, F, m, 0, 0, m, 1)
                    plans = [(a, s, P.plan(curve, tuning, bt["tl"], bt["nsets"], bt["emax"], bt["mw"], wb, 0, own, a, s))
                             for a in (0, 1) for s in (0, 1)]
                    yield curve, mode, n, m, wb == wb_n, res, plans


def _excess(res, p):
    return {b: (v, res["bytes"][b]) for b, v in p["bytes"].items() if v > res["bytes"][b]}


def test_reserve_dominates_within_a_width(cases):
    """Reserved for n, a batch of n' <= n tuples of the same mode and window width plans no buffer
    larger than the reserved one, whether or not other slots are busy or the call is synchronous.
    This includes n' small enough for the small form, whose tree plan_reserve sizes too."""
    tuning = cases[0]["tuning"]
    assert tuning["ncu"] == 256
    checked = 0
    for curve, mode, n, m, same, res, plans in _pairs(tuning):
        if same:
            for a, s, p in plans:
                assert not _excess(res, p), (curve, mode, n, m, a, s, _excess(res, p))
                checked += 1
    assert checked > 3000  # the grid did not collapse


def test_reserve_across_the_width_switch(cases):
    """Not asserted: which buffers a smaller batch at the other window width plans larger than a
    context reserved for n holds (it then allocates inside the call); printed per curve, mode,
    reserved size and buffer with the n' that needs most.  Found at 256 CUs, BLS12-381 without GLV
    (the other modes and BN254 alike):
    - reserved at 16 bits above the 13-bit range (n > 2^17), a 13-bit n' has 30 sets against 24:
      winsum 5760 B against 4608 and scratch 80640 against 78336 at every such n; reserved just above
      the range (131073), n' = 131072 also has 5/4 the digits and entries (digits 20971600 B against
      16777408, ent 41943328 against 33554944, sval, skey).
    - reserved at 13 bits (2^15 < n <= 2^17), a 16-bit n' <= 2^15 has 8x the buckets per set: cnt and
      off 3145728 B against 491520, coarse 73728 against 11520, R 11010048 against 1720320, U twice
      that, and at n' = 32767 acc29 235110400 against 86245376 (reserved 32769; 144965632 reserved
      131072) and crowd 789560 against 786488."""
    tuning = cases[0]["tuning"]
    found = {}
    for curve, mode, n, m, same, res, plans in _pairs(tuning):
        if not same:
            for a, s, p in plans:
                for b, (need, have) in _excess(res, p).items():
                    key = (curve, mode, n, b)
                    if key not in found or need > found[key][1]:
                        found[key] = (m, need, have)
    for (curve, mode, n, b), (m, need, have) in sorted(found.items()):
        print("reserve crosses width: curve %d %s reserved %d, n' %d: %s %d > %d" % (curve, mode, n, m, b, need, have))
