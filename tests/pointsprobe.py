"""ctypes binding of the test-only probe of the G1 point layer (tests/native/points_probe.hip,
built by the package Makefile into kzgmi/libkzgmi_pointsprobe.so).

run(curve, op, cases) calls one device function of csrc/g1.hpp, csrc/points.hpp or csrc/glv.hpp per
kernel, one case per thread, on flat lists of 32-bit words (`words(curve, op)` per case).  The stage
functions call the shipped launchers of csrc/launch_io.hip on caller-supplied inputs: every buffer
has its exact size and a guard behind it, outputs are poisoned first, and `guards` maps the name of
every buffer the stage allocated to True (guard intact) or False.  per_elem=True enqueues the
launcher once per case with n = 1 and that case's own error word; per_elem=False makes one launch
over all cases and returns the one sticky error word.  Arrays come back as numpy."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGMI_POINTSPROBE_LIB") or os.path.join(
    ROOT, "kzg-batch-verification-scheme_amd", "kzgmi", "libkzgmi_pointsprobe.so")
CURVE_ID = {"bls12_381": 0, "bn254": 1}
GUARDS = ["in", "in_inf", "pts", "inf", "img", "img_inf", "err", "out", "h0", "h1"]
POISON = 0xA5
_lib = None
_hip_error = None  # first HIP failure: nothing more is launched in this process after it


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libkzgmi_pointsprobe.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
        try:  # one HIP runtime per process, as kzgmi.lib() does
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        i, u32, vp, cp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p
        for name, args in (("words", [i, cp, ctypes.POINTER(i), ctypes.POINTER(i)]),
                           ("run", [i, cp, vp, u32, vp]),
                           ("sizes", [i, vp]),
                           ("convert_points", [i, i, i, i, vp, u32, vp, vp, vp, vp, vp, vp]),
                           ("decompress_points", [i, i, i, vp, u32, vp, vp, vp, vp]),
                           ("compress_points", [i, i, i, vp, u32, vp, vp]),
                           ("subgroup_check", [i, i, i, vp, vp, u32, vp, vp]),
                           ("glv_split", [i, i, i, vp, u32, u32, vp, vp, vp]),
                           ("endo_points", [i, i, i, i, vp, vp, u32, vp, vp, vp]),
                           ("convert_scalars", [i, i, i, vp, u32, vp, vp, vp]),
                           ("encode_points", [i, i, i, vp, u32, vp, vp])):
            f = getattr(L, "kzgmi_pointsprobe_" + name)
            f.argtypes, f.restype = args, i
        assert L.kzgmi_pointsprobe_guard_words() == len(GUARDS)
        _lib = L
    return _lib


def words(curve, op):
    """(input words, output words) per case of `op`; raises KeyError for an op the probe lacks."""
    i, o = ctypes.c_int(), ctypes.c_int()
    rc = lib().kzgmi_pointsprobe_words(CURVE_ID[curve], op.encode(), ctypes.byref(i), ctypes.byref(o))
    if rc != 0:
        raise KeyError("probe has no op %r for %s (rc %d)" % (op, curve, rc))
    return i.value, o.value


def sizes(curve):
    """Words of an Fp, of an Affine slot and of an Xyzz record (no GPU)."""
    out = np.zeros(3, dtype=np.uint32)
    assert lib().kzgmi_pointsprobe_sizes(CURVE_ID[curve], out.ctypes.data) == 0
    return dict(zip(("fp", "affine", "xyzz"), (int(v) for v in out)))


def _check_alive():
    if _hip_error:
        raise RuntimeError("probe not run: an earlier launch failed (%s)" % _hip_error)


def _done(what, rc, guards=None):
    global _hip_error
    if rc >= 1000:
        _hip_error = "%s: HIP error %d" % (what, rc - 1000)
    if rc != 0:
        raise RuntimeError("probe %s failed: rc %d %s" % (what, rc, _hip_error or ""))
    if guards is not None:
        return {n: bool(v) for n, v in zip(GUARDS, guards.tolist()) if v != 2}


def run(curve, op, cases):
    """cases: one list of 32-bit words per case.  Returns one list of output words per case."""
    _check_alive()
    wi, wo = words(curve, op)
    n = len(cases)
    assert n > 0 and all(len(c) == wi for c in cases), (op, wi, {len(c) for c in cases})
    inp = np.ascontiguousarray(np.array(cases, dtype=np.uint64).astype(np.uint32))
    out = np.zeros((n, wo), dtype=np.uint32)
    rc = lib().kzgmi_pointsprobe_run(CURVE_ID[curve], op.encode(), inp.ctypes.data, n, out.ctypes.data)
    _done("%s/%s" % (curve, op), rc)
    return out.tolist()


def _u8(b):
    return np.ascontiguousarray(np.frombuffer(bytes(b), dtype=np.uint8))


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32))


def _p(a):
    return a.ctypes.data


def _g():
    _check_alive()
    return np.zeros(len(GUARDS), dtype=np.uint32)


def _z32(n):
    return np.zeros(max(int(n), 1), dtype=np.uint32)


def _z8(n):
    return np.zeros(max(int(n), 1), dtype=np.uint8)


def convert_points(curve, form, data, n, per_elem, poison=POISON):
    """form 0: 32-bit Montgomery slots, 1: radix-29 slots, 2: radix-29 slots and GLV images."""
    g, aw, b = _g(), sizes(curve)["affine"], _u8(data)
    assert b.size == n * 8 * sizes(curve)["fp"]
    o = dict(pts=_z32(n * aw), inf=_z8(n), img=_z32(n * aw), img_inf=_z8(n), err=_z32(n if per_elem else 1))
    rc = lib().kzgmi_pointsprobe_convert_points(CURVE_ID[curve], form, int(per_elem), poison, _p(b), n, _p(o["pts"]),
                                                _p(o["inf"]), _p(o["img"]), _p(o["img_inf"]), _p(o["err"]), _p(g))
    o["guards"] = _done("%s convert_points/%d" % (curve, form), rc, g)
    return o


def decompress_points(curve, data, n, per_elem, poison=POISON):
    g, aw, b = _g(), sizes(curve)["affine"], _u8(data)
    assert b.size == n * 4 * sizes(curve)["fp"]
    o = dict(pts=_z32(n * aw), inf=_z8(n), err=_z32(n if per_elem else 1))
    rc = lib().kzgmi_pointsprobe_decompress_points(CURVE_ID[curve], int(per_elem), poison, _p(b), n, _p(o["pts"]),
                                                   _p(o["inf"]), _p(o["err"]), _p(g))
    o["guards"] = _done("%s decompress_points" % curve, rc, g)
    return o


def compress_points(curve, data, n, per_elem, poison=POISON):
    g, fw, b = _g(), sizes(curve)["fp"], _u8(data)
    assert b.size == n * 8 * fw
    o = dict(out=_z8(n * 4 * fw))
    rc = lib().kzgmi_pointsprobe_compress_points(CURVE_ID[curve], int(per_elem), poison, _p(b), n, _p(o["out"]), _p(g))
    o["guards"] = _done("%s compress_points" % curve, rc, g)
    return o


def subgroup_check(curve, pts, inf, per_elem, poison=POISON):
    g, aw, p, f = _g(), sizes(curve)["affine"], _u32(pts), _u8(inf)
    n = f.size
    assert p.size == n * aw
    o = dict(err=_z32(n if per_elem else 1))
    rc = lib().kzgmi_pointsprobe_subgroup_check(CURVE_ID[curve], int(per_elem), poison, _p(p), _p(f), n, _p(o["err"]), _p(g))
    o["guards"] = _done("%s subgroup_check" % curve, rc, g)
    return o


def glv_split(curve, scal, stride, n, per_elem, poison=POISON):
    g, s = _g(), _u32(scal)
    assert s.size == n * stride
    o = dict(h0=_z32(4 * n), h1=_z32(4 * n))
    rc = lib().kzgmi_pointsprobe_glv_split(CURVE_ID[curve], int(per_elem), poison, _p(s), stride, n, _p(o["h0"]),
                                           _p(o["h1"]), _p(g))
    o["guards"] = _done("%s glv_split/%d" % (curve, stride), rc, g)
    return o


def endo_points(curve, in29, src, src_inf, per_elem, poison=POISON):
    g, aw, s, f = _g(), sizes(curve)["affine"], _u32(src), _u8(src_inf)
    n = f.size
    assert s.size == n * aw
    o = dict(dst=_z32(n * aw), dst_inf=_z8(n))
    rc = lib().kzgmi_pointsprobe_endo_points(CURVE_ID[curve], int(in29), int(per_elem), poison, _p(s), _p(f), n,
                                             _p(o["dst"]), _p(o["dst_inf"]), _p(g))
    o["guards"] = _done("%s endo_points/%d" % (curve, in29), rc, g)
    return o


def convert_scalars(curve, data, n, per_elem, poison=POISON):
    g, b = _g(), _u8(data)
    assert b.size == 32 * n
    o = dict(out=_z32(8 * n), err=_z32(n if per_elem else 1))
    rc = lib().kzgmi_pointsprobe_convert_scalars(CURVE_ID[curve], int(per_elem), poison, _p(b), n, _p(o["out"]),
                                                 _p(o["err"]), _p(g))
    o["guards"] = _done("%s convert_scalars" % curve, rc, g)
    return o


def encode_points(curve, res, n, per_elem, poison=POISON):
    g, sz, r = _g(), sizes(curve), _u32(res)
    assert r.size == n * sz["xyzz"]
    o = dict(out=_z8(n * 8 * sz["fp"]))
    rc = lib().kzgmi_pointsprobe_encode_points(CURVE_ID[curve], int(per_elem), poison, _p(r), n, _p(o["out"]), _p(g))
    o["guards"] = _done("%s encode_points" % curve, rc, g)
    return o
