"""ctypes binding of the test-only probe of the MSM plan (tests/native/plan_probe.hip, built by the
package Makefile into kzgmi/libkzgmi_planprobe.so): plan_msm, plan_reserve, batch_terms and call_wbits of
csrc/msm_plan.hpp.  Host code only: no GPU, no HIP call.

Term classes are lists [count, pt_base, scal_words, nwin, set_base, scal_stride, scal, win_off]
with scal = [buffer name, word offset], the form of tests/golden/msm_plan_parent.json."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGMI_PLANPROBE_LIB") or os.path.join(
    ROOT, "kzg-batch-verification-scheme_amd", "kzgmi", "libkzgmi_planprobe.so")
MAX_CLASSES = 16
TUNING = ["ncu", "acc_threads_env", "acc_queue", "acc_queue_min", "acc_queue_from", "sort_split", "sort_full_bins",
          "wbits_env", "small_terms", "split_acc", "split_low_prio", "split_side_fix", "split_side_prio", "split_rev",
          "seg4_waves"]
SCALARS = ["scal_r", "scal_s", "scal_t", "glv_r", "glv_s", "glv_t", "cell_coef"]
BYTES = ["small_nodes", "small_flags", "digits", "cnt", "off", "cntb", "offb", "coarse", "ent", "total", "accq", "crowd",
         "sval", "skey", "acc29", "acc29b", "R", "U", "scratch", "winsum", "res"]
COUNTS = ["ndig", "own_npts", "nbuckets", "bins", "rb_parts", "NB", "nchunks", "acc_threads", "can_split", "split",
          "split_set", "pieces", "crowd_words", "second"]
_CLASS_WORDS = 9
_TERM_WORDS = 2 + MAX_CLASSES * _CLASS_WORDS
_BASE_SHIFT = 44  # scalar buffer i stands at address (i + 1) << 44: no term reaches the next one
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libkzgmi_planprobe.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        L.kzgmi_planprobe_plan.argtypes = [ctypes.c_int, u64p, u64p, ctypes.c_uint32, ctypes.c_uint64, u32p] + \
            [ctypes.c_int] * 5 + [u64p]
        L.kzgmi_planprobe_plan.restype = ctypes.c_char_p
        L.kzgmi_planprobe_reserve.argtypes = [ctypes.c_int, u64p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int,
                                              u64p, u64p]
        L.kzgmi_planprobe_reserve.restype = None
        L.kzgmi_planprobe_batch_terms.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_uint32] * 3 + \
            [ctypes.c_uint64] * 4 + [ctypes.c_int, u64p, u64p]
        L.kzgmi_planprobe_batch_terms.restype = None
        L.kzgmi_planprobe_wbits.argtypes = [u64p, ctypes.c_uint64, ctypes.c_uint64]
        L.kzgmi_planprobe_wbits.restype = ctypes.c_int
        L.kzgmi_planprobe_windows.argtypes = [ctypes.c_int, ctypes.c_int]
        L.kzgmi_planprobe_windows.restype = ctypes.c_uint32
        _lib = L
    return _lib


def _tuning(t):
    return (ctypes.c_uint64 * len(TUNING))(*[int(t[k]) & (2**64 - 1) for k in TUNING])


def _addr(scal):
    return ((SCALARS.index(scal[0]) + 1) << _BASE_SHIFT) + 4 * scal[1]


def _scal(addr):
    return [SCALARS[(addr >> _BASE_SHIFT) - 1], (addr & ((1 << _BASE_SHIFT) - 1)) // 4] if addr else None


def _pack_terms(tl):
    w = [tl["nclass"], tl["total"]]
    for c in tl["c"]:
        w += c[:6] + [_addr(c[6]), c[7], 0]
    w += [0] * (_TERM_WORDS - len(w))
    return (ctypes.c_uint64 * _TERM_WORDS)(*w)


def _unpack_terms(w):
    """-> (term list in the golden form, the classes' dig_base)"""
    cls = [list(w[2 + k * _CLASS_WORDS: 2 + (k + 1) * _CLASS_WORDS]) for k in range(MAX_CLASSES)]
    assert all(not any(c) for c in cls[w[0]:]), "classes past nclass are not zero"
    cls = cls[:w[0]]
    return ({"nclass": w[0], "total": w[1], "c": [c[:6] + [_scal(c[6]), c[7]] for c in cls]}, [c[8] for c in cls])


_PLAN_WORDS = 2 + 2 + 3 * MAX_CLASSES + 6 + 3 + _TERM_WORDS + len(COUNTS) + len(BYTES)


def _bases():
    return (ctypes.c_uint64 * len(SCALARS))(*[(i + 1) << _BASE_SHIFT for i in range(len(SCALARS))])


def plan(curve, tuning, tl, nsets, emax, mw, wbits, part, own_pts, alone, sync_call):
    """plan_msm<curve> -> dict: refuse (message or None), small, sp, small_terms / small_nodes /
    small_flags, tl, dig_base, the COUNTS and bytes {buffer: size}."""
    out = (ctypes.c_uint64 * _PLAN_WORDS)()
    msg = lib().kzgmi_planprobe_plan(curve, _tuning(tuning), _pack_terms(tl), nsets, emax, (ctypes.c_uint32 * 5)(*mw), wbits,
                                     part, int(own_pts), int(alone), int(sync_call), out)
    assert bool(out[0]) == (msg is not None)
    return _plan_dict(list(out), msg.decode() if msg else None)


def reserve(curve, tuning, glv, powers, n, own_pts):
    """plan_reserve<curve> -> the same dict"""
    out = (ctypes.c_uint64 * _PLAN_WORDS)()
    lib().kzgmi_planprobe_reserve(curve, _tuning(tuning), int(glv), int(powers), n, int(own_pts), _bases(), out)
    assert not out[0]
    return _plan_dict(list(out), None)


def _plan_dict(w, refuse):
    n_out = _PLAN_WORDS
    p = {"refuse": refuse, "small": w[1]}
    i = 2
    sp = {"nclass": w[i], "nmsm": w[i + 1]}
    i += 2
    for name, cnt in (("term_base", MAX_CLASSES), ("leaf_base", MAX_CLASSES), ("msm", MAX_CLASSES), ("count", 2),
                      ("node_base", 2), ("flag_base", 2)):
        sp[name] = w[i:i + cnt]
        i += cnt
    p["sp"] = sp
    p["small_terms"], p["small_nodes"], p["small_flags"] = w[i:i + 3]
    i += 3
    p["tl"], p["dig_base"] = _unpack_terms(w[i:i + _TERM_WORDS])
    i += _TERM_WORDS
    for name in COUNTS:
        p[name] = w[i]
        i += 1
    p["bytes"] = dict(zip(BYTES, w[i:]))
    assert i + len(BYTES) == n_out
    return p


def batch_terms(glv, powers, cell_terms, H, F, n, m, lo, nj, last):
    """batch_terms -> dict: tl, mw, nsets, emax"""
    out = (ctypes.c_uint64 * (_TERM_WORDS + 7))()
    lib().kzgmi_planprobe_batch_terms(int(glv), int(powers), cell_terms, H, F, n, m, lo, nj, int(last), _bases(), out)
    w = list(out)
    tl, dig = _unpack_terms(w[:_TERM_WORDS])
    assert not any(dig)
    return {"tl": tl, "mw": w[_TERM_WORDS:_TERM_WORDS + 5], "nsets": w[_TERM_WORDS + 5], "emax": w[_TERM_WORDS + 6]}


def call_wbits(tuning, entries16, max13):
    return lib().kzgmi_planprobe_wbits(_tuning(tuning), entries16, max13)


def windows(wb):
    """(windows_half, windows_full) at width wb"""
    return lib().kzgmi_planprobe_windows(wb, 0), lib().kzgmi_planprobe_windows(wb, 1)
