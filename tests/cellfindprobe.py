"""ctypes binding of the test-only probe of the search plan's tail parameter
(tests/native/cellfind_probe.hip, built by the package Makefile into kzgmi/libkzgmi_cellfindprobe.so):
find_wave_terms, find_group_plan and find_group_chunk of csrc/find_plan.hpp with the tail length given.
Host code only: no GPU, no HIP call.  Ranges are (lo, hi) tuples, half open; the plan and group
dictionaries are those of tests/findprobe.py."""
import ctypes
import os

from findprobe import GROUP, PLAN, TUNING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGMI_CELLFINDPROBE_LIB") or os.path.join(
    ROOT, "kzg-batch-verification-scheme_amd", "kzgmi", "libkzgmi_cellfindprobe.so")
CELL_TAIL = 64  # the tail terms of a range of EIP-7594 cells: -c_m(g) [tau^m]_1, m < 64
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libkzgmi_cellfindprobe.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        u64, u32 = ctypes.c_uint64, ctypes.c_uint32
        L.kzgmi_cellfindprobe_wave_terms.argtypes = [u64, u32]
        L.kzgmi_cellfindprobe_wave_terms.restype = u64
        L.kzgmi_cellfindprobe_group_plan.argtypes = [u64p, u64, u32, u32p, u64p]
        L.kzgmi_cellfindprobe_group_plan.restype = None
        L.kzgmi_cellfindprobe_group_chunk.argtypes = [u64p, u64, u64p, u32]
        L.kzgmi_cellfindprobe_group_chunk.restype = u64
        _lib = L
    return _lib


def _ranges(rs):
    flat = [v for r in rs for v in r]
    return (ctypes.c_uint64 * max(1, len(flat)))(*flat)


def wave_terms(length, tail):
    return lib().kzgmi_cellfindprobe_wave_terms(length, tail)


def group_plan(ranges, tail):
    """-> (plan dict, [group dict])"""
    G = len(ranges)
    table = (ctypes.c_uint32 * (8 * max(1, G)))()
    out = (ctypes.c_uint64 * 9)()
    lib().kzgmi_cellfindprobe_group_plan(_ranges(ranges), G, tail, table, out)
    return dict(zip(PLAN, list(out))), [dict(zip(GROUP, table[8 * g: 8 * g + 8])) for g in range(G)]


def group_chunk(ranges, t, tail):
    tuning = (ctypes.c_uint64 * len(TUNING))(*[int(t[k]) for k in TUNING])
    return lib().kzgmi_cellfindprobe_group_chunk(_ranges(ranges), len(ranges), tuning, tail)
