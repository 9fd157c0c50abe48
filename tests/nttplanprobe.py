"""ctypes binding of the test-only probe of the transform plan (tests/native/ntt_plan_probe.hip, built
by the package Makefile into kzgmi/libkzgmi_nttplanprobe.so): ntt_plan of csrc/ntt_plan.hpp and the
shipped constants.  Host code only: no GPU, no HIP call."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGMI_NTTPLANPROBE_LIB") or os.path.join(
    ROOT, "kzg-batch-verification-scheme_amd", "kzgmi", "libkzgmi_nttplanprobe.so")
CONSTANTS = ("max_logn", "tile_bits", "max_bits", "min_pass_bits", "max_passes", "min_tile_bits", "max_tile_bits")
PASS = ("bits", "lstride", "lprev", "tw_step", "flags")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libkzgmi_nttplanprobe.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
        # one HIP runtime per process (kzgmi.lib()): the probe is linked like the library, so torch's
        # copy of the runtime has to be the one that is loaded first
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        L.kzgmi_nttplanprobe_constants.argtypes = [u32p]
        L.kzgmi_nttplanprobe_constants.restype = None
        L.kzgmi_nttplanprobe_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
                                              ctypes.c_int, ctypes.c_int, u32p, u64p]
        L.kzgmi_nttplanprobe_plan.restype = ctypes.c_int
        _lib = L
    return _lib


def constants():
    out = (ctypes.c_uint32 * len(CONSTANTS))()
    lib().kzgmi_nttplanprobe_constants(out)
    return dict(zip(CONSTANTS, list(out)))


def plan(logn, count=1, flags=0, shift=False, bound=None, read_be=True, write_be=True):
    """-> ([pass dict], scratch bytes), or None where the arguments are refused"""
    c = constants()
    if bound is None:
        bound = c["max_bits"]
    passes = (ctypes.c_uint32 * (len(PASS) * c["max_passes"]))()
    out = (ctypes.c_uint64 * 2)()
    if not lib().kzgmi_nttplanprobe_plan(logn, count, flags, int(shift), bound, int(read_be), int(write_be), passes, out):
        return None
    n = len(PASS)
    return [dict(zip(PASS, passes[n * k: n * k + n])) for k in range(out[0])], int(out[1])
