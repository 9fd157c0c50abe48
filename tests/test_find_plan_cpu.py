"""The search plan of csrc/find_plan.hpp through its test-only probe (tests/findprobe.py): the split of a
range, the search driven by a predicate (tests/findref.py), the layout of a grouped launch and the
path of a level.  No GPU."""
import math
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import findprobe  # noqa: E402
import findref  # noqa: E402


@pytest.mark.parametrize("F", [2, 3, 16])
def test_split_tiles_the_range(F):
    for L in range(1, 41):
        for lo in (0, 7, (1 << 33) + 5):
            parts = findprobe.split(lo, lo + L, F)
            assert len(parts) == min(F, L)
            assert parts[0][0] == lo and parts[-1][1] == lo + L
            assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
            lens = [hi - l for l, hi in parts]
            assert min(lens) >= 1 and max(lens) - min(lens) <= 1
            k = len(parts)
            assert parts == [(lo + j * L // k, lo + (j + 1) * L // k) for j in range(k)]


def _bad_sets(n, F, rng):
    sets = [set(), {0}, {n - 1}, set(range(n))]
    if n > 1:
        b = findprobe.split(0, n, F)[0][1]  # the first level-0 boundary: b - 1 and b lie in different parts
        sets.append({b - 1, b})
    for k in (1, 2, 5, 12, n // 2):
        if 0 < k <= n:
            sets.append(set(rng.sample(range(n), k)))
    return sets


@pytest.mark.parametrize("n", [1, 2, 17, 257, 4099])
@pytest.mark.parametrize("F", [2, 16])
@pytest.mark.parametrize("max_bad", [1, 3, 8])
def test_search_model_returns_the_lowest_invalid_indices(n, F, max_bad):
    rng = random.Random(1000 * n + 10 * F + max_bad)
    for bad in _bad_sets(n, F, rng):
        got, more, levels = findref.search(n, F, max_bad, findref.contains(bad), findprobe.split, findprobe.next_level)
        assert got == sorted(bad)[:max_bad], (n, F, max_bad, sorted(bad))
        assert more == (len(bad) > max_bad)
        assert levels <= math.ceil(math.log(n, F)) + 1 if n > 1 else levels == 1


def test_level_fanout_and_the_shipped_search():
    """The wide fan-out in the levels the grouped kernel takes, the narrow one above; the search model
    under that rule finds the same indices."""
    t = findprobe.tuning()
    F, Fb = t["fanout"], t["bucket_fanout"]
    assert 2 <= Fb <= F
    longest = (t["group_terms"] - 1) // 3  # the longest part the grouped kernel takes
    assert findprobe.level_fanout([(0, 1)], t) == F
    assert findprobe.level_fanout([(7, 7 + Fb * longest)], t) == F
    assert findprobe.level_fanout([(7, 7 + Fb * longest + 1)], t) == Fb
    assert findprobe.level_fanout([(0, 5), (9, 10 + Fb * longest)], t) == Fb  # by the longest suspect
    assert findprobe.level_path(findprobe.split(7, 7 + Fb * longest, F), t) == 1
    assert findprobe.level_path(findprobe.split(7, 7 + Fb * longest + 1, Fb), t) == 0
    n = 4 * F * longest + 3
    paths = []

    def fanout(suspects):
        f = findprobe.level_fanout(suspects, t)
        paths.append(findprobe.level_path([p for lo, hi in suspects for p in findprobe.split(lo, hi, f)], t))
        return f
    rng = random.Random(n)
    for bad in ([], [0], [n - 1], sorted(rng.sample(range(n), 9))):
        del paths[:]
        got, more, levels = findref.search(n, fanout, 4, findref.contains(bad), findprobe.split, findprobe.next_level)
        assert (got, more) == (bad[:4], len(bad) > 4)
        assert paths == sorted(paths) and paths[0] == 0  # bucket levels first, then grouped ones, never back
        assert levels <= math.ceil(math.log(n, Fb)) + 1


def test_next_level_keeps_found_tuples_in_order():
    # a found tuple above a failing part competes with it for the max_bad places
    sus, bad, more = findprobe.next_level([(0, 2), (2, 4), (4, 6)], [False, True, False], 2, [9], False)
    assert (sus, bad, more) == ([(0, 2), (4, 6)], [], True)
    sus, bad, more = findprobe.next_level([(4, 6), (6, 7)], [True, False], 2, [1], False)
    assert (sus, bad, more) == ([], [1, 6], False)
    sus, bad, more = findprobe.next_level([(4, 6)], [True], 2, [1], True)
    assert (sus, bad, more) == ([], [1], True)  # sticky


def _tree(leaves):
    nodes = flags = 0
    while leaves > 1:
        nodes += leaves
        flags += (leaves + 1) // 2
        leaves = (leaves + 1) // 2
    return nodes, flags


def test_group_plan_layout():
    lens = [1, 2, 3, 5, 64, 65]
    ranges, lo = [], 3
    for L in lens:
        ranges.append((lo, lo + L))
        lo += L
    plan, groups = findprobe.group_plan(ranges)
    node_bytes = findprobe.tuning()["node_bytes"]
    assert node_bytes == 272
    # the waves partition the terms: group g's 3 len + 1 waves follow group g - 1's
    wave = 0
    regions_n, regions_f = [], []
    for (lo, hi), g in zip(ranges, groups):
        L = hi - lo
        assert (g["lo"], g["len"], g["wave_base"]) == (lo, L, wave)
        wave += 3 * L + 1
        for leaves, nb, fb in ((L, g["node_base_a"], g["flag_base_a"]), (2 * L + 1, g["node_base_b"], g["flag_base_b"])):
            nodes, flags = _tree(leaves)
            regions_n.append((nb, nb + nodes))
            regions_f.append((fb, fb + flags))
    assert plan["waves"] == wave == sum(3 * L + 1 for L in lens)
    for regions, total in ((regions_n, plan["nodes"]), (regions_f, plan["flags"])):
        nonempty = sorted(r for r in regions if r[1] > r[0])
        assert all(a[1] <= b[0] for a, b in zip(nonempty, nonempty[1:])), "tree regions overlap"
        assert max(r[1] for r in regions) <= total
    # the reported bytes cover the highest index
    assert plan["bytes_nodes"] >= plan["nodes"] * node_bytes
    assert plan["bytes_flags"] >= plan["flags"] * 4
    assert plan["bytes_table"] >= len(lens) * 32 and plan["bytes_negt"] >= len(lens) * 32
    assert plan["bytes"] == plan["bytes_nodes"] + plan["bytes_flags"] and plan["fits"] == 1


def test_level_path_and_chunks_follow_the_tuning():
    t = findprobe.tuning()
    assert t["fanout"] >= 2 and t["max_bad"] == 4096 and t["max_ranges"] == 65536
    longest = (t["group_terms"] - 1) // 3  # 3 len + 1 <= group_terms
    assert findprobe.level_path([(0, longest), (longest, longest + 1)], t) == 1
    assert findprobe.level_path([(0, 1), (5, 5 + longest + 1)], t) == 0
    # a launch's trees stay within the bound, and a launch always takes at least one range
    ranges = [(i * longest, (i + 1) * longest) for i in range(64)]
    one, _ = findprobe.group_plan(ranges[:1])
    small = dict(t, group_bytes=3 * one["bytes"])
    k = findprobe.group_chunk(ranges, small)
    assert 1 <= k < len(ranges)
    assert findprobe.group_plan(ranges[:k])[0]["bytes"] <= small["group_bytes"]
    assert findprobe.group_plan(ranges[:k + 1])[0]["bytes"] > small["group_bytes"]
    assert findprobe.group_chunk(ranges, dict(t, group_bytes=1)) == 1
    assert findprobe.group_chunk(ranges, t) == len(ranges)
    # the shipped bound holds a level of fanout x max_bad single tuples in one launch
    singles = [(i, i + 1) for i in range(t["fanout"] * 4)]
    assert findprobe.group_chunk(singles, t) == len(singles)
