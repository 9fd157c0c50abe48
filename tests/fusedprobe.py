"""ctypes binding of the test-only probe of the fused product-and-subtract forms
(tests/native/field29_fused_probe.hip, built by the package Makefile into
kzgmi/libkzgmi_fusedprobe.so): one kernel per op.  run() takes three operands of N limbs per case
and returns N limbs per case."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGMI_FUSEDPROBE_LIB") or os.path.join(
    ROOT, "kzg-batch-verification-scheme_amd", "kzgmi", "libkzgmi_fusedprobe.so")
CURVE_ID = {"bls12_381": 0, "bn254": 1}
_lib = None
_hip_error = None  # first HIP failure: nothing more is launched in this process after it


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libkzgmi_fusedprobe.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
        try:  # one HIP runtime per process, as kzgmi.lib() and fieldprobe.lib() do
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.kzgmi_fusedprobe_run.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32,
                                           ctypes.c_void_p]
        L.kzgmi_fusedprobe_run.restype = ctypes.c_int
        _lib = L
    return _lib


def run(curve, op, cases, n_limbs):
    """cases: one flat list of 3 n_limbs words per case.  Returns one list of n_limbs words per case."""
    global _hip_error
    if _hip_error:
        raise RuntimeError("probe not run: an earlier launch failed (%s)" % _hip_error)
    n = len(cases)
    assert n > 0 and all(len(c) == 3 * n_limbs for c in cases), (op, {len(c) for c in cases})
    inp = np.ascontiguousarray(np.array(cases, dtype=np.uint64).astype(np.uint32))
    out = np.zeros((n, n_limbs), dtype=np.uint32)
    rc = lib().kzgmi_fusedprobe_run(CURVE_ID[curve], op.encode(), inp.ctypes.data, n, out.ctypes.data)
    if rc >= 1000:
        _hip_error = "%s/%s: HIP error %d" % (curve, op, rc - 1000)
    if rc != 0:
        raise RuntimeError("probe %s/%s failed: rc %d %s" % (curve, op, rc, _hip_error or ""))
    return out.tolist()
