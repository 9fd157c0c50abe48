"""The search plan of csrc/find_plan.hpp with a tail (the 64 tail terms of a range of EIP-7594 cells)
through its test-only probe (tests/cellfindprobe.py): the layout of a grouped launch, the tail-1 form
against the probe of the plan as it was (tests/findprobe.py), and the cut of a level.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cellfindprobe  # noqa: E402
import findprobe  # noqa: E402

T = cellfindprobe.CELL_TAIL
LENS = [1, 2, 3, 64, 65, 1365]


def _ranges(lens, lo=3):
    out = []
    for L in lens:
        out.append((lo, lo + L))
        lo += L
    return out


def _tree(leaves):
    nodes = flags = 0
    while leaves > 1:
        nodes += leaves
        flags += (leaves + 1) // 2
        leaves = (leaves + 1) // 2
    return nodes, flags


def test_tail_is_64():
    assert T == 64
    for L in LENS:
        assert cellfindprobe.wave_terms(L, T) == 3 * L + 64
        assert cellfindprobe.wave_terms(L, 1) == 3 * L + 1


def test_group_plan_with_the_cell_tail():
    ranges = _ranges(LENS)
    plan, groups = cellfindprobe.group_plan(ranges, T)
    node_bytes = findprobe.tuning()["node_bytes"]
    wave = nodes = flags = 0
    for (lo, hi), g in zip(ranges, groups):
        L = hi - lo
        assert (g["lo"], g["len"], g["wave_base"]) == (lo, L, wave)
        wave += 3 * L + 64
        na, fa = _tree(L)
        nb, fb = _tree(2 * L + 64)  # tree B: r C, s pi and the 64 tail terms
        assert (g["node_base_a"], g["node_base_b"]) == (nodes, nodes + na)
        assert (g["flag_base_a"], g["flag_base_b"]) == (flags, flags + fa)
        nodes += na + nb
        flags += fa + fb
    assert plan["waves"] == wave == sum(3 * L + 64 for L in LENS)
    assert (plan["nodes"], plan["flags"]) == (nodes, flags)
    assert plan["bytes_negt"] == (64 * len(LENS) + 1) * 32
    assert plan["bytes_nodes"] == (nodes + 1) * node_bytes and plan["bytes_flags"] == (flags + 1) * 4
    assert plan["bytes"] == plan["bytes_nodes"] + plan["bytes_flags"] and plan["fits"] == 1
    assert plan["bytes_table"] == (len(LENS) + 1) * 32


def test_tail_1_is_the_plan_as_it_was():
    for ranges in (_ranges(LENS), _ranges(LENS[::-1], lo=(1 << 20) + 1), _ranges([1365]), []):
        assert cellfindprobe.group_plan(ranges, 1) == findprobe.group_plan(ranges)
    plan1, _ = cellfindprobe.group_plan(_ranges(LENS), 1)
    assert plan1["bytes_negt"] == (len(LENS) + 1) * 32
    t = findprobe.tuning()
    ranges = [(i * 1365, (i + 1) * 1365) for i in range(64)]
    one, _ = findprobe.group_plan(ranges[:1])
    for gb in (1, 3 * one["bytes"], t["group_bytes"]):
        tt = dict(t, group_bytes=gb)
        assert cellfindprobe.group_chunk(ranges, tt, 1) == findprobe.group_chunk(ranges, tt)


@pytest.mark.parametrize("lens", [[1365] * 64, LENS * 8, [1] * 300, [4096] * 16, [65536]])
def test_group_chunk_with_the_cell_tail(lens):
    """A launch takes at least one range and its trees stay within group_bytes, unless its first range
    alone passes the bound; one range more would pass it."""
    t = findprobe.tuning()
    ranges = _ranges(lens, lo=0)
    one, _ = cellfindprobe.group_plan(ranges[:1], T)
    for gb in (1, one["bytes"], 3 * one["bytes"], 3 * one["bytes"] + 1, t["group_bytes"]):
        tt = dict(t, group_bytes=gb)
        g0, launches = 0, 0
        while g0 < len(ranges):
            k = cellfindprobe.group_chunk(ranges[g0:], tt, T)
            assert 1 <= k <= len(ranges) - g0
            used = cellfindprobe.group_plan(ranges[g0:g0 + k], T)[0]["bytes"]
            assert used <= gb or k == 1
            if g0 + k < len(ranges):
                assert cellfindprobe.group_plan(ranges[g0:g0 + k + 1], T)[0]["bytes"] > gb
            g0 += k
            launches += 1
        if gb == 1:
            assert launches == len(ranges)
    # level 0 of the largest cell search (65 536 cells at the shipped fan-out) is one launch
    parts = findprobe.split(0, 65536, t["fanout"])
    assert cellfindprobe.group_chunk(parts, t, T) == len(parts)
    assert cellfindprobe.group_plan(parts, T)[0]["waves"] == 3 * 65536 + 64 * len(parts)
