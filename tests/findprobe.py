"""ctypes binding of the test-only probe of the search plan (tests/native/find_probe.hip, built by the
package Makefile into kzgmi/libkzgmi_findprobe.so): find_split, find_next_level, find_group_plan,
find_level_fanout, find_level_path, find_group_chunk and the shipped FindTuning of
csrc/find_plan.hpp.  Host code only: no GPU, no HIP call.  Ranges are (lo, hi) tuples, half open."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGMI_FINDPROBE_LIB") or os.path.join(
    ROOT, "kzg-batch-verification-scheme_amd", "kzgmi", "libkzgmi_findprobe.so")
TUNING = ["fanout", "bucket_fanout", "group_terms", "group_bytes"]
GROUP = ["lo", "len", "wave_base", "node_base_a", "node_base_b", "flag_base_a", "flag_base_b", "pad"]
PLAN = ["waves", "nodes", "flags", "bytes_nodes", "bytes_flags", "bytes_table", "bytes_negt", "bytes", "fits"]
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libkzgmi_findprobe.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        u64p, u32p, i32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32))
        u64 = ctypes.c_uint64
        L.kzgmi_findprobe_tuning.argtypes = [u64p]
        L.kzgmi_findprobe_tuning.restype = None
        L.kzgmi_findprobe_split.argtypes = [u64, u64, ctypes.c_uint32, u64p]
        L.kzgmi_findprobe_split.restype = ctypes.c_uint32
        L.kzgmi_findprobe_next_level.argtypes = [u64p, i32p, u64, u64, u64p, u64, ctypes.c_int, u64p, u64p, u64p]
        L.kzgmi_findprobe_next_level.restype = None
        L.kzgmi_findprobe_group_plan.argtypes = [u64p, u64, u32p, u64p]
        L.kzgmi_findprobe_group_plan.restype = None
        L.kzgmi_findprobe_level_path.argtypes = [u64p, u64, u64p]
        L.kzgmi_findprobe_level_path.restype = ctypes.c_int
        L.kzgmi_findprobe_level_fanout.argtypes = [u64p, u64, u64p]
        L.kzgmi_findprobe_level_fanout.restype = ctypes.c_uint32
        L.kzgmi_findprobe_group_chunk.argtypes = [u64p, u64, u64p]
        L.kzgmi_findprobe_group_chunk.restype = u64
        _lib = L
    return _lib


def _ranges(rs):
    flat = [v for r in rs for v in r]
    return (ctypes.c_uint64 * max(1, len(flat)))(*flat)


def _tuning(t):
    return (ctypes.c_uint64 * len(TUNING))(*[int(t[k]) for k in TUNING])


def tuning():
    """the shipped FindTuning, with max_bad, max_ranges and node_bytes beside it"""
    out = (ctypes.c_uint64 * 7)()
    lib().kzgmi_findprobe_tuning(out)
    return dict(zip(TUNING + ["max_bad", "max_ranges", "node_bytes"], list(out)))


def split(lo, hi, F):
    out = (ctypes.c_uint64 * (2 * F))()
    k = lib().kzgmi_findprobe_split(lo, hi, F, out)
    return [(out[2 * j], out[2 * j + 1]) for j in range(k)]


def next_level(parts, verdicts, max_bad, bad, more):
    """-> (suspects, bad, more) after a level whose part j passed iff verdicts[j]"""
    ok = (ctypes.c_int32 * max(1, len(parts)))(*[int(bool(v)) for v in verdicts])
    bad_in = (ctypes.c_uint64 * max(1, len(bad)))(*bad)
    bad_out = (ctypes.c_uint64 * max_bad)()
    sus = (ctypes.c_uint64 * (2 * max_bad))()
    out3 = (ctypes.c_uint64 * 3)()
    lib().kzgmi_findprobe_next_level(_ranges(parts), ok, len(parts), max_bad, bad_in, len(bad), int(bool(more)), bad_out,
                                     sus, out3)
    ns, nb, m = list(out3)
    return [(sus[2 * j], sus[2 * j + 1]) for j in range(ns)], list(bad_out[:nb]), bool(m)


def group_plan(ranges):
    """-> (plan dict, [group dict])"""
    G = len(ranges)
    table = (ctypes.c_uint32 * (8 * max(1, G)))()
    out = (ctypes.c_uint64 * 9)()
    lib().kzgmi_findprobe_group_plan(_ranges(ranges), G, table, out)
    return dict(zip(PLAN, list(out))), [dict(zip(GROUP, table[8 * g: 8 * g + 8])) for g in range(G)]


def level_path(parts, t):
    """1: the grouped kernel, 0: bucket partial jobs"""
    return lib().kzgmi_findprobe_level_path(_ranges(parts), len(parts), _tuning(t))


def level_fanout(suspects, t):
    """the fan-out of the level that splits these suspects"""
    return lib().kzgmi_findprobe_level_fanout(_ranges(suspects), len(suspects), _tuning(t))


def group_chunk(ranges, t):
    return lib().kzgmi_findprobe_group_chunk(_ranges(ranges), len(ranges), _tuning(t))
