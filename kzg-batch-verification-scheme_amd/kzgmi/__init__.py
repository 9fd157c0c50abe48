"""kzgmi -- MI355X-native KZG batch verifier (Python host side over the C-ABI).

`batch_verify(commitments, zs, ys, proofs, srs)` is the north-star entry point
(BASELINE.json:5).  The reference repository contains no code
(/root/reference/LICENSE:1-201), so its "plugin interface" is the signature named in
BASELINE.json; this module mirrors it and calls libkzgmi.so (hand-written gfx950 HIP
kernels) through ctypes.  There is no CPU fallback: without the built library or without a
HIP device every call raises.

Inputs may be `bytes`/`bytearray`/`memoryview`, numpy uint8 arrays, or torch uint8 tensors.
CUDA(HIP) tensors are passed by device pointer (no PCIe copy: the HBM-resident path);
host buffers go through the host-pointer entry points.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# KZGMI_LIB selects an alternative build (timing experiments); default: the in-tree library
LIB_PATH = os.environ.get("KZGMI_LIB") or os.path.join(_HERE, "libkzgmi.so")

ABI_VERSION = 6  # include/kzgmi.h KZGMI_ABI_VERSION
CURVES = {"bls12_381": 0, "bn254": 1}
FP_BYTES = {"bls12_381": 48, "bn254": 32}
PHASES = ["convert", "scalars", "sort", "accumulate", "reduce", "combine", "pairing", "h2d"]

ERR_NAMES = {-1: "ARG", -2: "ENCODING", -3: "NOT_ON_CURVE", -4: "SCALAR", -5: "DEVICE", -6: "OOM",
             -7: "NOT_IN_SUBGROUP", -8: "SHARD"}


class KzgmiError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("kzgmi error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


_lib = None


def lib():
    """Load libkzgmi.so (fails loudly if the HIP extension was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libkzgmi.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
    # One HIP runtime per process: torch-ROCm ships its own libamdhip64 with the same
    # soname (libamdhip64.so.7).  Loading torch first makes libkzgmi bind to that copy, so
    # device pointers, streams and RCCL all live in one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    c = ctypes
    vp, sz, u8p, ip = c.c_void_p, c.c_size_t, c.c_char_p, c.POINTER(c.c_int)
    sig = {
        "kzgmi_version": ([], c.c_char_p),
        "kzgmi_last_error": ([], c.c_char_p),
        "kzgmi_phase_names": ([], c.c_char_p),
        "kzgmi_ctx_create": ([c.POINTER(vp), c.POINTER(c.c_int), c.c_int, c.c_int], c.c_int),
        "kzgmi_ctx_create_device": ([c.POINTER(vp), c.c_int, c.c_int], c.c_int),
        "kzgmi_ctx_destroy": ([vp], None),
        "kzgmi_srs_load": ([vp, c.c_int, u8p, u8p, u8p, c.POINTER(vp)], c.c_int),
        "kzgmi_ctx_num_devices": ([vp], c.c_int),
        "kzgmi_slot_device": ([vp, c.c_int], c.c_int),
        "kzgmi_abi_version": ([], c.c_int),
        "kzgmi_ctx_reserve": ([vp, c.c_int, sz, c.c_uint32], c.c_int),
        "kzgmi_alloc_count": ([], c.c_uint64),
        "kzgmi_stream_wait": ([vp, c.c_int, vp], c.c_int),
        "kzgmi_slot_signal": ([vp, c.c_int, vp], c.c_int),
        "kzgmi_host_alloc": ([sz, c.POINTER(vp)], c.c_int),
        "kzgmi_host_free": ([vp], None),
        "kzgmi_host_register": ([vp, sz], c.c_int),
        "kzgmi_host_unregister": ([vp], c.c_int),
        "kzgmi_partial_encode_device": ([vp, c.c_int, vp, sz, u8p], c.c_int),
        "kzgmi_batch_verify_multi_device": ([vp, vp, c.POINTER(vp), c.POINTER(vp), c.POINTER(vp), c.POINTER(vp),
                                             c.POINTER(sz), u8p, c.c_uint32, ip], c.c_int),
        "kzgmi_msm_g1_multi_device": ([vp, c.c_int, c.POINTER(vp), c.POINTER(vp), c.POINTER(sz), u8p], c.c_int),
        "kzgmi_srs_free": ([vp], None),
        "kzgmi_batch_verify": ([vp, vp, vp, vp, vp, vp, sz, u8p, ip], c.c_int),
        "kzgmi_batch_verify_device": ([vp, vp, vp, vp, vp, vp, sz, u8p, ip], c.c_int),
        "kzgmi_batch_verify_device_async": ([vp, vp, c.c_int, vp, vp, vp, vp, sz, u8p], c.c_int),
        "kzgmi_batch_verify_ex": ([vp, vp, vp, vp, vp, vp, sz, u8p, c.c_uint32, ip], c.c_int),
        "kzgmi_batch_verify_ex_async": ([vp, vp, c.c_int, vp, vp, vp, vp, sz, u8p, c.c_uint32], c.c_int),
        "kzgmi_batch_verify_device_ex_async": ([vp, vp, c.c_int, vp, vp, vp, vp, sz, u8p, c.c_uint32], c.c_int),
        "kzgmi_g1_validate_device": ([vp, c.c_int, vp, sz, c.c_uint32], c.c_int),
        "kzgmi_g1_compress_device": ([vp, c.c_int, vp, sz, vp], c.c_int),
        "kzgmi_ck_load": ([vp, c.c_int, u8p, sz, c.POINTER(c.c_void_p)], c.c_int),
        "kzgmi_ck_free": ([vp], None),
        "kzgmi_commit": ([vp, vp, u8p, sz, u8p], c.c_int),
        "kzgmi_commit_device": ([vp, vp, vp, sz, u8p], c.c_int),
        "kzgmi_open": ([vp, vp, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_open_device": ([vp, vp, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_open_device_async": ([vp, vp, c.c_int, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_open_quotient_device": ([vp, c.c_int, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_fr_ntt": ([vp, c.c_int, vp, c.c_uint, sz, c.c_uint32, u8p, vp], c.c_int),
        "kzgmi_fr_ntt_device": ([vp, c.c_int, vp, c.c_uint, sz, c.c_uint32, u8p, vp], c.c_int),
        "kzgmi_fr_ntt_device_async": ([vp, c.c_int, c.c_int, vp, c.c_uint, sz, c.c_uint32, u8p, vp], c.c_int),
        "kzgmi_g1_ntt": ([vp, c.c_int, vp, c.c_uint, sz, c.c_uint32, vp], c.c_int),
        "kzgmi_g1_ntt_device": ([vp, c.c_int, vp, c.c_uint, sz, c.c_uint32, vp], c.c_int),
        "kzgmi_g1_ntt_device_async": ([vp, c.c_int, c.c_int, vp, c.c_uint, sz, c.c_uint32, vp], c.c_int),
        "kzgmi_open_all_key_load": ([vp, vp, c.c_uint, c.POINTER(vp)], c.c_int),
        "kzgmi_open_all_key_free": ([vp], None),
        "kzgmi_open_all_key_device_bytes": ([vp], sz),
        "kzgmi_open_all": ([vp, vp, vp, sz, c.c_uint32, vp, vp], c.c_int),
        "kzgmi_open_all_device": ([vp, vp, vp, sz, c.c_uint32, vp, vp], c.c_int),
        "kzgmi_open_all_device_async": ([vp, vp, c.c_int, vp, sz, c.c_uint32, vp, vp], c.c_int),
        "kzgmi_open_cosets_key_load": ([vp, vp, c.c_uint, c.c_uint, c.POINTER(vp)], c.c_int),
        "kzgmi_open_cosets_key_free": ([vp], None),
        "kzgmi_open_cosets_key_device_bytes": ([vp], sz),
        "kzgmi_open_cosets": ([vp, vp, vp, sz, sz, c.c_uint, c.c_uint32, vp, vp], c.c_int),
        "kzgmi_open_cosets_device": ([vp, vp, vp, sz, sz, c.c_uint, c.c_uint32, vp, vp], c.c_int),
        "kzgmi_open_cosets_device_async": ([vp, vp, c.c_int, vp, sz, sz, c.c_uint, c.c_uint32, vp, vp], c.c_int),
        "kzgmi_open_evals": ([vp, vp, vp, c.c_uint, c.c_uint32, vp, sz, vp, vp], c.c_int),
        "kzgmi_open_evals_device": ([vp, vp, vp, c.c_uint, c.c_uint32, vp, sz, vp, vp], c.c_int),
        "kzgmi_open_evals_device_async": ([vp, vp, c.c_int, vp, c.c_uint, c.c_uint32, vp, sz, vp, vp], c.c_int),
        "kzgmi_fs_challenge_device": ([vp, c.c_int, vp, vp, vp, vp, sz, c.c_uint32, u8p], c.c_int),
        "kzgmi_fs_chunk_digests_device": ([vp, c.c_int, vp, vp, vp, vp, sz, c.c_uint64, c.c_uint32, vp], c.c_int),
        "kzgmi_fs_challenge_from_digests_device": ([vp, c.c_int, vp, sz, c.c_uint64, u8p], c.c_int),
        "kzgmi_blob_challenges_device": ([vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_blob_eval_device": ([vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_blob_batch_challenge_device": ([vp, vp, vp, vp, vp, sz, u8p], c.c_int),
        "kzgmi_verify_blob_batch": ([vp, vp, vp, vp, vp, sz, ip], c.c_int),
        "kzgmi_verify_blob_batch_device": ([vp, vp, vp, vp, vp, sz, ip], c.c_int),
        "kzgmi_verify_blob_batch_device_async": ([vp, vp, c.c_int, vp, vp, vp, sz], c.c_int),
        "kzgmi_blob_pk_load": ([vp, u8p, c.POINTER(vp)], c.c_int),
        "kzgmi_blob_pk_free": ([vp], None),
        "kzgmi_blob_pk_device_bytes": ([vp], sz),
        "kzgmi_blob_commit": ([vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_blob_commit_device": ([vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_blob_commit_device_async": ([vp, vp, c.c_int, vp, sz, vp], c.c_int),
        "kzgmi_compute_kzg_proofs": ([vp, vp, vp, vp, sz, vp, vp], c.c_int),
        "kzgmi_compute_kzg_proofs_device": ([vp, vp, vp, vp, sz, vp, vp], c.c_int),
        "kzgmi_compute_kzg_proofs_device_async": ([vp, vp, c.c_int, vp, vp, sz, vp, vp], c.c_int),
        "kzgmi_compute_blob_proofs": ([vp, vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_compute_blob_proofs_device": ([vp, vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_compute_blob_proofs_device_async": ([vp, vp, c.c_int, vp, vp, sz, vp], c.c_int),
        "kzgmi_blob_quotient_device": ([vp, vp, vp, sz, vp, vp], c.c_int),
        "kzgmi_cell_srs_load": ([vp, u8p, u8p, u8p, c.POINTER(vp)], c.c_int),
        "kzgmi_cell_srs_free": ([vp], None),
        "kzgmi_cell_batch_challenge_device": ([vp, vp, sz, vp, vp, vp, vp, sz, u8p], c.c_int),
        "kzgmi_cell_interp_device": ([vp, vp, vp, sz, u8p, vp], c.c_int),
        "kzgmi_verify_cell_batch": ([vp, vp, vp, sz, vp, vp, vp, vp, sz, u8p, ip], c.c_int),
        "kzgmi_verify_cell_batch_device": ([vp, vp, vp, sz, vp, vp, vp, vp, sz, u8p, ip], c.c_int),
        "kzgmi_verify_cell_batch_device_async": ([vp, vp, c.c_int, vp, sz, vp, vp, vp, vp, sz, u8p], c.c_int),
        "kzgmi_compute_cells": ([vp, vp, sz, vp], c.c_int),
        "kzgmi_compute_cells_device": ([vp, vp, sz, vp], c.c_int),
        "kzgmi_compute_cells_device_async": ([vp, c.c_int, vp, sz, vp], c.c_int),
        "kzgmi_recover_cells": ([vp, vp, sz, vp, sz, vp], c.c_int),
        "kzgmi_recover_cells_device": ([vp, vp, sz, vp, sz, vp], c.c_int),
        "kzgmi_recover_cells_device_async": ([vp, c.c_int, vp, sz, vp, sz, vp], c.c_int),
        "kzgmi_cell_pk_load": ([vp, u8p, c.POINTER(vp)], c.c_int),
        "kzgmi_cell_pk_free": ([vp], None),
        "kzgmi_cell_pk_device_bytes": ([vp], sz),
        "kzgmi_compute_cells_and_proofs": ([vp, vp, vp, sz, vp, vp], c.c_int),
        "kzgmi_compute_cells_and_proofs_device": ([vp, vp, vp, sz, vp, vp], c.c_int),
        "kzgmi_compute_cells_and_proofs_device_async": ([vp, vp, c.c_int, vp, sz, vp, vp], c.c_int),
        "kzgmi_recover_cells_and_proofs": ([vp, vp, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_recover_cells_and_proofs_device": ([vp, vp, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_recover_cells_and_proofs_device_async": ([vp, vp, c.c_int, vp, sz, vp, sz, vp, vp], c.c_int),
        "kzgmi_fk20_scalars_device": ([vp, vp, sz, vp], c.c_int),
        "kzgmi_g1_fft128_device": ([vp, vp, sz, c.c_int, vp], c.c_int),
        "kzgmi_slot_wait": ([vp, c.c_int, ip], c.c_int),
        "kzgmi_last_combination": ([vp, u8p, u8p], c.c_int),
        "kzgmi_msm_g1": ([vp, c.c_int, vp, vp, sz, u8p], c.c_int),
        "kzgmi_msm_g1_device": ([vp, c.c_int, vp, vp, sz, u8p], c.c_int),
        "kzgmi_msm_g1_device_async": ([vp, c.c_int, c.c_int, vp, vp, sz], c.c_int),
        "kzgmi_msm_wait": ([vp, c.c_int, u8p], c.c_int),
        "kzgmi_set_glv": ([vp, c.c_int, c.c_int], c.c_int),
        "kzgmi_commit_device_async": ([vp, vp, c.c_int, vp, sz], c.c_int),
        "kzgmi_set_trusted_g1": ([vp, c.c_int], c.c_int),
        "kzgmi_set_split_acc": ([vp, c.c_int], c.c_int),
        "kzgmi_msm_partial_device_async": ([vp, c.c_int, c.c_int, vp, vp, sz, vp], c.c_int),
        "kzgmi_msm_combine_device_async": ([vp, c.c_int, c.c_int, vp, c.c_int], c.c_int),
        "kzgmi_partial_bytes": ([c.c_int], sz),
        "kzgmi_batch_partial_device": ([vp, vp, vp, vp, vp, vp, sz, c.c_uint64, u8p, vp], c.c_int),
        "kzgmi_batch_combine_device": ([vp, vp, vp, c.c_int, ip], c.c_int),
        "kzgmi_batch_partial_device_async": ([vp, vp, c.c_int, vp, vp, vp, vp, sz, c.c_uint64, u8p, c.c_uint32, vp],
                                             c.c_int),
        "kzgmi_batch_combine_device_async": ([vp, vp, c.c_int, vp, c.c_int], c.c_int),
        "kzgmi_msm_partial_device": ([vp, c.c_int, vp, vp, sz, vp], c.c_int),
        "kzgmi_msm_combine_device": ([vp, c.c_int, vp, c.c_int, u8p], c.c_int),
        "kzgmi_pairing": ([vp, c.c_int, u8p, u8p, u8p], c.c_int),
        "kzgmi_gen_g1": ([vp, c.c_int, vp, sz, vp], c.c_int),
        "kzgmi_gen_tuples": ([vp, c.c_int, u8p, u8p, sz, vp, vp, vp, vp], c.c_int),
        "kzgmi_g2_mul": ([vp, c.c_int, u8p, u8p, u8p], c.c_int),
        "kzgmi_probe_fpmul": ([vp, c.c_int, c.POINTER(c.c_double)], c.c_int),
        "kzgmi_set_profiling": ([vp, c.c_int], c.c_int),
        "kzgmi_get_phase_ms": ([vp, c.POINTER(c.c_double), c.c_int], c.c_int),
        "kzgmi_batch_check_partials_device": ([vp, vp, vp, sz, u8p], c.c_int),
        "kzgmi_batch_range_partials_device": ([vp, vp, vp, vp, vp, vp, sz, c.c_uint64, u8p, c.c_uint32,
                                               c.POINTER(c.c_uint64), sz, vp], c.c_int),
        "kzgmi_batch_find_invalid": ([vp, vp, vp, vp, vp, vp, sz, u8p, c.c_uint32, c.POINTER(c.c_uint64), sz,
                                      c.POINTER(sz), ip], c.c_int),
        "kzgmi_batch_find_invalid_device": ([vp, vp, vp, vp, vp, vp, sz, u8p, c.c_uint32, c.POINTER(c.c_uint64), sz,
                                             c.POINTER(sz), ip], c.c_int),
        "kzgmi_verify_blob_batch_find_invalid": ([vp, vp, vp, vp, vp, sz, c.POINTER(c.c_uint64), sz, c.POINTER(sz), ip],
                                                  c.c_int),
        "kzgmi_verify_blob_batch_find_invalid_device": ([vp, vp, vp, vp, vp, sz, c.POINTER(c.c_uint64), sz,
                                                         c.POINTER(sz), ip], c.c_int),
        "kzgmi_find_invalid_stats": ([vp, c.POINTER(c.c_uint64)], c.c_int),
        "kzgmi_cell_coeffs_device": ([vp, vp, vp, sz, vp], c.c_int),
        "kzgmi_cell_range_partials_device": ([vp, vp, vp, sz, vp, vp, vp, vp, sz, c.c_uint64, u8p,
                                              c.POINTER(c.c_uint64), sz, vp], c.c_int),
        "kzgmi_verify_cell_batch_find_invalid": ([vp, vp, vp, sz, vp, vp, vp, vp, sz, u8p, c.POINTER(c.c_uint64), sz,
                                                  c.POINTER(sz), ip], c.c_int),
        "kzgmi_verify_cell_batch_find_invalid_device": ([vp, vp, vp, sz, vp, vp, vp, vp, sz, u8p, c.POINTER(c.c_uint64),
                                                         sz, c.POINTER(sz), ip], c.c_int),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    if L.kzgmi_abi_version() != ABI_VERSION:  # include/kzgmi.h KZGMI_ABI_VERSION
        raise ImportError("libkzgmi.so ABI %d, this binding expects %d (rebuild: __graft_entry__.build())"
                          % (L.kzgmi_abi_version(), ABI_VERSION))
    _lib = L
    return L


def exported_symbols():
    return [
        "kzgmi_version", "kzgmi_last_error", "kzgmi_phase_names", "kzgmi_ctx_create", "kzgmi_ctx_create_device",
        "kzgmi_ctx_destroy", "kzgmi_srs_load", "kzgmi_srs_free", "kzgmi_batch_verify",
        "kzgmi_batch_verify_device", "kzgmi_batch_verify_device_async", "kzgmi_slot_wait",
        "kzgmi_batch_verify_ex", "kzgmi_batch_verify_device_ex_async", "kzgmi_g1_validate_device",
        "kzgmi_g1_compress_device", "kzgmi_ck_load", "kzgmi_ck_free", "kzgmi_commit", "kzgmi_commit_device",
        "kzgmi_fs_challenge_device", "kzgmi_fs_chunk_digests_device",
        "kzgmi_fs_challenge_from_digests_device",
        "kzgmi_last_combination", "kzgmi_msm_g1", "kzgmi_msm_g1_device", "kzgmi_msm_g1_device_async",
        "kzgmi_msm_wait", "kzgmi_set_glv", "kzgmi_commit_device_async", "kzgmi_set_trusted_g1", "kzgmi_set_split_acc", "kzgmi_msm_partial_device_async", "kzgmi_msm_combine_device_async", "kzgmi_partial_bytes",
        "kzgmi_batch_partial_device", "kzgmi_batch_combine_device", "kzgmi_batch_partial_device_async",
        "kzgmi_batch_combine_device_async", "kzgmi_msm_partial_device",
        "kzgmi_msm_combine_device", "kzgmi_pairing", "kzgmi_gen_g1", "kzgmi_gen_tuples",
        "kzgmi_g2_mul", "kzgmi_probe_fpmul", "kzgmi_set_profiling", "kzgmi_get_phase_ms",
        "kzgmi_ctx_num_devices", "kzgmi_slot_device", "kzgmi_stream_wait", "kzgmi_slot_signal", "kzgmi_partial_encode_device",
        "kzgmi_batch_verify_multi_device", "kzgmi_msm_g1_multi_device",
        "kzgmi_abi_version", "kzgmi_ctx_reserve", "kzgmi_alloc_count", "kzgmi_batch_verify_ex_async",
        "kzgmi_host_alloc", "kzgmi_host_free", "kzgmi_host_register", "kzgmi_host_unregister",
        "kzgmi_blob_challenges_device", "kzgmi_blob_eval_device", "kzgmi_blob_batch_challenge_device",
        "kzgmi_verify_blob_batch", "kzgmi_verify_blob_batch_device", "kzgmi_verify_blob_batch_device_async",
        "kzgmi_cell_srs_load", "kzgmi_cell_srs_free", "kzgmi_cell_batch_challenge_device", "kzgmi_cell_interp_device",
        "kzgmi_verify_cell_batch", "kzgmi_verify_cell_batch_device", "kzgmi_verify_cell_batch_device_async",
        "kzgmi_compute_cells", "kzgmi_compute_cells_device", "kzgmi_compute_cells_device_async",
        "kzgmi_recover_cells", "kzgmi_recover_cells_device", "kzgmi_recover_cells_device_async",
        "kzgmi_cell_pk_load", "kzgmi_cell_pk_free", "kzgmi_cell_pk_device_bytes",
        "kzgmi_compute_cells_and_proofs", "kzgmi_compute_cells_and_proofs_device",
        "kzgmi_compute_cells_and_proofs_device_async", "kzgmi_recover_cells_and_proofs",
        "kzgmi_recover_cells_and_proofs_device", "kzgmi_recover_cells_and_proofs_device_async",
        "kzgmi_fk20_scalars_device", "kzgmi_g1_fft128_device",
        "kzgmi_blob_pk_load", "kzgmi_blob_pk_free", "kzgmi_blob_pk_device_bytes",
        "kzgmi_blob_commit", "kzgmi_blob_commit_device", "kzgmi_blob_commit_device_async",
        "kzgmi_compute_kzg_proofs", "kzgmi_compute_kzg_proofs_device", "kzgmi_compute_kzg_proofs_device_async",
        "kzgmi_compute_blob_proofs", "kzgmi_compute_blob_proofs_device", "kzgmi_compute_blob_proofs_device_async",
        "kzgmi_blob_quotient_device",
        "kzgmi_batch_check_partials_device", "kzgmi_batch_range_partials_device", "kzgmi_batch_find_invalid",
        "kzgmi_batch_find_invalid_device", "kzgmi_verify_blob_batch_find_invalid",
        "kzgmi_verify_blob_batch_find_invalid_device", "kzgmi_find_invalid_stats",
        "kzgmi_cell_coeffs_device", "kzgmi_cell_range_partials_device", "kzgmi_verify_cell_batch_find_invalid",
        "kzgmi_verify_cell_batch_find_invalid_device",
        "kzgmi_open", "kzgmi_open_device", "kzgmi_open_device_async", "kzgmi_open_quotient_device",
        "kzgmi_fr_ntt", "kzgmi_fr_ntt_device", "kzgmi_fr_ntt_device_async",
        "kzgmi_open_evals", "kzgmi_open_evals_device", "kzgmi_open_evals_device_async",
        "kzgmi_g1_ntt", "kzgmi_g1_ntt_device", "kzgmi_g1_ntt_device_async",
        "kzgmi_open_all_key_load", "kzgmi_open_all_key_free", "kzgmi_open_all_key_device_bytes",
        "kzgmi_open_all", "kzgmi_open_all_device", "kzgmi_open_all_device_async",
        "kzgmi_open_cosets_key_load", "kzgmi_open_cosets_key_free", "kzgmi_open_cosets_key_device_bytes",
        "kzgmi_open_cosets", "kzgmi_open_cosets_device", "kzgmi_open_cosets_device_async",
    ]


FLAG_COMPRESSED = 1
FLAG_SUBGROUP_CHECK = 2
FLAG_POWERS = 4
FLAG_FIAT_SHAMIR = 8
FLAG_TRUSTED_G1 = 16
NTT_INVERSE = 1  # KZGMI_NTT_INVERSE
NTT_BITREV = 2   # KZGMI_NTT_BITREV: the evaluation side is in bit-reversed order
NTT_MAX_LOGN = 26
ERR_NOT_IN_SUBGROUP = -7
FS_CHUNK = 4096
BLOB_BYTES = 4096 * 32  # an EIP-4844 blob: 4096 big-endian canonical Fr elements
CELL_BYTES = 64 * 32    # an EIP-7594 cell: 64 big-endian canonical Fr elements
EXT_BLOB_BYTES = 128 * CELL_BYTES  # the 128 cells of one blob
CELLS_PER_EXT_BLOB = 128
PROOFS_BYTES = CELLS_PER_EXT_BLOB * 48  # the 128 compressed cell proofs of one blob


def _flags(compressed: bool = False, subgroup_check: bool = False, fiat_shamir: bool = False,
           challenge=None, trusted_g1: bool = False) -> int:
    return ((FLAG_COMPRESSED if compressed else 0) | (FLAG_SUBGROUP_CHECK if subgroup_check else 0)
            | (FLAG_FIAT_SHAMIR if fiat_shamir else 0) | (FLAG_POWERS if challenge is not None else 0)
            | (FLAG_TRUSTED_G1 if trusted_g1 else 0))


def _challenge_seed(seed, challenge):
    """The 32-byte seed argument of the C-ABI (the library reads exactly 32 bytes from it).
    KZGMI_FLAG_POWERS passes r (int < 2^256 or 32 big-endian bytes) in its place."""
    if challenge is None:
        if seed is None:
            return None
        sd = bytes(seed)
        if len(sd) != 32:
            raise ValueError("seed must be 32 bytes, got %d" % len(sd))
        return sd
    if seed is not None:
        raise ValueError("pass either seed or challenge")
    if isinstance(challenge, int):
        if not 0 <= challenge < (1 << 256):
            raise ValueError("challenge must be in [0, 2^256)")
        return challenge.to_bytes(32, "big")
    sd = bytes(challenge)
    if len(sd) != 32:
        raise ValueError("challenge must be 32 bytes, got %d" % len(sd))
    return sd


def _check(rc: int):
    if rc != 0:
        msg = lib().kzgmi_last_error()
        raise KzgmiError(rc, msg.decode() if msg else "")


def _is_device_tensor(x) -> bool:
    return hasattr(x, "is_cuda") and x.is_cuda


def _host_bytes(x) -> bytes:
    if x is None:
        return b""
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    if hasattr(x, "cpu"):  # torch tensor
        return x.detach().cpu().contiguous().numpy().tobytes()
    if hasattr(x, "tobytes"):  # numpy
        return x.tobytes()
    raise TypeError("unsupported buffer type %r" % type(x))


def _host_ptr(x):
    """(address, nbytes, keepalive) of a host buffer, without copying it: bytes, bytearray,
    memoryview, numpy arrays (C-contiguous) and CPU torch tensors.  The keepalive object must
    outlive every use of the address."""
    if x is None:
        return 0, 0, None
    if isinstance(x, bytes):
        cp = ctypes.c_char_p(x)  # points into the bytes object itself
        return ctypes.cast(cp, ctypes.c_void_p).value or 0, len(x), (x, cp)
    if isinstance(x, HostBuffer):
        return x.ptr, x.nbytes, x
    import numpy as np
    if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):  # torch CPU tensor
        t = x.detach()
        if not t.is_contiguous():
            t = t.contiguous()
        return t.data_ptr(), t.numel() * t.element_size(), t
    if isinstance(x, (bytearray, memoryview)):
        x = np.frombuffer(x, dtype=np.uint8)
    if not isinstance(x, np.ndarray):
        try:  # any other buffer-protocol object (array.array, mmap, ...)
            x = np.frombuffer(memoryview(x).cast("B"), dtype=np.uint8)
        except TypeError:
            raise TypeError("unsupported buffer type %r" % type(x)) from None
    if not x.flags["C_CONTIGUOUS"]:
        x = np.ascontiguousarray(x)
    return x.ctypes.data, x.nbytes, x


class HostBuffer:
    """Page-locked host memory from kzgmi_host_alloc: host-buffer batch_verify calls whose arrays
    live here are DMA'd to HBM at PCIe rate, asynchronously (no staging copy).  `array` is a
    writable numpy uint8 view; free() (or garbage collection) releases it -- only when no job
    reading it is in flight."""

    def __init__(self, nbytes: int):
        import numpy as np
        p = ctypes.c_void_p()
        _check(lib().kzgmi_host_alloc(int(nbytes), ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, int(nbytes)
        raw = (ctypes.c_uint8 * self.nbytes).from_address(self.ptr)
        raw._kzgmi_owner = self  # every numpy view's base chain ends here: the block outlives its views
        self.array = np.ctypeslib.as_array(raw)

    def view(self, offset: int, nbytes: int):
        """numpy view of [offset, offset + nbytes) (also accepted by the host entry points)."""
        return self.array[offset:offset + nbytes]

    def free(self):
        """Release the block now (the caller guarantees no view is used afterwards and no job
        reading it is in flight); otherwise it is released when the last view goes away."""
        if getattr(self, "ptr", None):
            self.array = None
            lib().kzgmi_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def register_host(arr) -> None:
    """Pin an existing C-contiguous numpy array in place (kzgmi_host_register) so host-buffer
    calls DMA from it directly; unregister_host(arr) before freeing it."""
    _check(lib().kzgmi_host_register(arr.ctypes.data, arr.nbytes))


def unregister_host(arr) -> None:
    _check(lib().kzgmi_host_unregister(arr.ctypes.data))


def _dptr(x, nbytes: Optional[int] = None) -> int:
    """Device pointer of a contiguous tensor holding at least `nbytes` bytes."""
    if not x.is_contiguous():
        raise ValueError("device tensors must be contiguous")
    if nbytes is not None and x.numel() * x.element_size() < nbytes:
        raise ValueError("device tensor holds %d bytes, the call reads %d" % (x.numel() * x.element_size(), nbytes))
    return x.data_ptr()


def _current_stream(device: int):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


@dataclass
class Srs:
    """{G1, [1]_2, [tau]_2} with device-side Miller-loop line tables."""
    ctx: "Context"
    curve: str
    handle: ctypes.c_void_p

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_srs_free(self.handle)
                self.handle = None
        except Exception:
            pass


@dataclass
class CellSrs:
    """EIP-7594 cell SRS: [tau^m]_1 for m < 64, [1]_2, [tau^64]_2 (kzgmi_cell_srs_load)."""
    ctx: "Context"
    handle: ctypes.c_void_p

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_cell_srs_free(self.handle)
                self.handle = None
        except Exception:
            pass


def _u64_bytes(xs) -> bytes:
    """A sequence of indices as uint64 little-endian bytes (bytes-like input is passed through)."""
    if isinstance(xs, (bytes, bytearray, memoryview)):
        return bytes(xs)
    import struct
    xs = [int(x) for x in xs]
    return struct.pack("<%dQ" % len(xs), *xs)


def _r32(r):
    """The optional caller-supplied batch challenge as a 32-byte big-endian buffer (None: derive)."""
    if r is None:
        return None
    return int(r).to_bytes(32, "big") if isinstance(r, int) else bytes(r)


@dataclass
class CellProofKey:
    """EIP-7594 cell proof key: the FK20 transforms of [tau^m]_1, m < 4096, as a fixed-base window
    table on the device (kzgmi_cell_pk_load)."""
    ctx: "Context"
    handle: ctypes.c_void_p

    @property
    def device_bytes(self) -> int:
        return int(lib().kzgmi_cell_pk_device_bytes(self.handle)) if self.handle else 0

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_cell_pk_free(self.handle)
                self.handle = None
        except Exception:
            pass


@dataclass
class BlobProofKey:
    """EIP-4844 blob proof key: the 4096 Lagrange points [l_j(tau)]_1 (bit-reversed order) as a fixed-base
    window table on the device (kzgmi_blob_pk_load)."""
    ctx: "Context"
    handle: ctypes.c_void_p

    @property
    def device_bytes(self) -> int:
        return int(lib().kzgmi_blob_pk_device_bytes(self.handle)) if self.handle else 0

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_blob_pk_free(self.handle)
                self.handle = None
        except Exception:
            pass


class CommitKey:
    """Prover commit key: [tau^i]_1 powers + fixed-base tables on the device."""
    ctx: "Context"
    curve: str
    n: int
    handle: ctypes.c_void_p

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_ck_free(self.handle)
                self.handle = None
        except Exception:
            pass


class OpenAllKey:
    """Key of open_all for one commit key and one domain size 2^logn: the transform of the SRS."""
    ctx: "Context"
    curve: str
    logn: int
    handle: ctypes.c_void_p

    @property
    def device_bytes(self) -> int:
        return int(lib().kzgmi_open_all_key_device_bytes(self.handle))

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_open_all_key_free(self.handle)
                self.handle = None
        except Exception:
            pass


class OpenCosetsKey:
    """Key of open_cosets for one commit key and one shape (2^logN coefficients, cosets of 2^logl points): the
    transforms of the SRS's l strided columns."""
    ctx: "Context"
    curve: str
    logN: int
    logl: int
    handle: ctypes.c_void_p

    @property
    def device_bytes(self) -> int:
        return int(lib().kzgmi_open_cosets_key_device_bytes(self.handle))

    def __del__(self):
        try:
            if self.handle:
                lib().kzgmi_open_cosets_key_free(self.handle)
                self.handle = None
        except Exception:
            pass


class Context:
    """One GPU (device_id) with `slots` independent workspaces/streams; or, with
    devices=[d0, d1, ...], one context over several GPUs (kzgmi_ctx_create's device list: the
    synchronous host-buffer batch_verify / msm_g1 are sharded over them, d0 being the primary
    device; the async entry points run whole batches per device -- slot s on device
    slot_device(s) = devices[s % len(devices)], device tensors passed to it must live there).

    Device-tensor arguments are read on the library's own streams: every call first orders
    the slot's stream after torch's current stream (kzgmi_stream_wait), so tensors written by
    torch just before the call are seen complete."""

    def __init__(self, device: int = 0, slots: int = 1, devices=None):
        h = ctypes.c_void_p()
        devs = [int(d) for d in devices] if devices is not None else [int(device)]
        arr = (ctypes.c_int * len(devs))(*devs)
        _check(lib().kzgmi_ctx_create(ctypes.byref(h), arr, len(devs), int(slots)))
        device = devs[0]
        self.handle = h
        self.device = device
        self.slots = slots
        self.ndev = len(devs)

    def num_devices(self) -> int:
        return int(lib().kzgmi_ctx_num_devices(self.handle))

    def slot_device(self, slot: int) -> int:
        """The device id slot `slot` runs on (kzgmi_slot_device)."""
        d = int(lib().kzgmi_slot_device(self.handle, int(slot)))
        if d < 0:
            _check(d)
        return d

    def reserve(self, curve: str, n: int, compressed: bool = False, subgroup_check: bool = False,
                fiat_shamir: bool = False, powers: bool = False, trusted_g1: bool = False):
        """kzgmi_ctx_reserve: size every slot's workspace for batches of up to n tuples in this
        mode (and create the profiling events) -- later calls of that size allocate nothing."""
        fl = _flags(compressed, subgroup_check, fiat_shamir, 0 if powers else None, trusted_g1)
        _check(lib().kzgmi_ctx_reserve(self.handle, CURVES[curve], int(n), fl))

    def _order(self, slot: int = 0):
        """Order `slot`'s next job after torch's current stream on the slot's device (device
        inputs written by torch)."""
        dev = self.device if self.ndev == 1 else self.slot_device(slot)
        _check(lib().kzgmi_stream_wait(self.handle, int(slot), _current_stream(dev)))

    def signal(self, slot: int, stream=None):
        """kzgmi_slot_signal: order later work on `stream` (a torch.cuda.Stream; default torch's
        current stream) after everything enqueued so far on `slot` -- no host sync."""
        dev = self.device if self.ndev == 1 else self.slot_device(slot)
        st = stream.cuda_stream if stream is not None else _current_stream(dev)
        _check(lib().kzgmi_slot_signal(self.handle, int(slot), st))

    def close(self):
        if getattr(self, "handle", None):
            lib().kzgmi_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ SRS
    def load_srs(self, curve: str, g2: bytes, tau_g2: bytes, g1: Optional[bytes] = None) -> Srs:
        """srs = {G1, [1]_2, [tau]_2}; g1 None = the standard generator."""
        h = ctypes.c_void_p()
        _check(lib().kzgmi_srs_load(self.handle, CURVES[curve], None if g1 is None else bytes(g1), bytes(g2),
                                    bytes(tau_g2), ctypes.byref(h)))
        return Srs(self, curve, h)

    # ------------------------------------------------------------------ batch verify
    def batch_verify(self, srs: Srs, commitments, zs, ys, proofs, seed: Optional[bytes] = None,
                     n: Optional[int] = None, compressed: bool = False, subgroup_check: bool = False,
                     fiat_shamir: bool = False, challenge=None, trusted_g1: bool = False) -> bool:
        """BASELINE.json:5 batch_verify.  compressed: C/pi are compressed G1 encodings;
        subgroup_check: reject points outside G1 (KZGMI_ERR_NOT_IN_SUBGROUP); fiat_shamir:
        randomisers seeded with a challenge hashed from the inputs on the GPU; challenge:
        r_i = r^i for a caller-supplied r (e.g. the EIP-4844 transcript's); trusted_g1: the
        points are known G1 members (enables GLV on BLS12-381)."""
        flags = _flags(compressed, subgroup_check, fiat_shamir, challenge, trusted_g1)
        g1b = (1 if compressed else 2) * FP_BYTES[srs.curve]
        ok = ctypes.c_int(-1)
        sd = _challenge_seed(seed, challenge)
        if seed is not None and len(sd) != 32:
            raise ValueError("seed must be 32 bytes")
        if _is_device_tensor(commitments):
            if n is None:
                n = commitments.numel() // g1b
            ptrs = (_dptr(commitments, n * g1b), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, n * g1b))
            self._order(0)
            if flags:
                _check(lib().kzgmi_batch_verify_device_ex_async(self.handle, srs.handle, 0, *ptrs, n, sd, flags))
                return self.wait(0)
            _check(lib().kzgmi_batch_verify_device(self.handle, srs.handle, *ptrs, n, sd, ctypes.byref(ok)))
        else:
            ptrs, keep = self._host_inputs(commitments, zs, ys, proofs, n, g1b)
            n = ptrs[-1]
            _check(lib().kzgmi_batch_verify_ex(self.handle, srs.handle, *ptrs[:4], n, sd, flags, ctypes.byref(ok)))
            del keep
        return bool(ok.value)

    @staticmethod
    def _host_inputs(commitments, zs, ys, proofs, n, g1b):
        """Addresses of the four host arrays (no copies) in C-ABI order (C, z, y, pi) + n."""
        (pc, lc, kc), (pz, lz, kz), (py, ly, ky), (pp, lp, kp) = (
            _host_ptr(v) for v in (commitments, zs, ys, proofs))
        if n is None:
            n = lc // g1b
        if lc < n * g1b or lp < n * g1b or lz < 32 * n or ly < 32 * n:
            raise ValueError("input buffers shorter than n tuples")
        return (pc, pz, py, pp, n), (kc, kz, ky, kp)

    def batch_verify_host_async(self, srs: Srs, slot: int, commitments, zs, ys, proofs, n: Optional[int] = None,
                                seed: Optional[bytes] = None, compressed: bool = False,
                                subgroup_check: bool = False, fiat_shamir: bool = False, challenge=None,
                                trusted_g1: bool = False):
        """kzgmi_batch_verify_ex_async: host arrays -> HBM on `slot`'s stream ahead of the batch's
        kernels; wait(slot) returns the verdict.  Arrays in a HostBuffer (or register_host'ed) are
        DMA'd asynchronously and must stay untouched until the wait; others are staged through
        the slot's pinned ring before this returns."""
        g1b = (1 if compressed else 2) * FP_BYTES[srs.curve]
        ptrs, keep = self._host_inputs(commitments, zs, ys, proofs, n, g1b)
        _check(lib().kzgmi_batch_verify_ex_async(self.handle, srs.handle, int(slot), *ptrs,
                                                 _challenge_seed(seed, challenge),
                                                 _flags(compressed, subgroup_check, fiat_shamir, challenge,
                                                        trusted_g1)))
        # the DMA may read the arrays until wait(slot); a failed call (e.g. slot busy) keeps the
        # pending job's keepalive
        self._host_keep = getattr(self, "_host_keep", {})
        self._host_keep[slot] = keep

    def batch_verify_async(self, srs: Srs, slot: int, commitments, zs, ys, proofs, n: int,
                           seed: Optional[bytes] = None, compressed: bool = False, subgroup_check: bool = False,
                           fiat_shamir: bool = False, challenge=None, trusted_g1: bool = False):
        g1b = (1 if compressed else 2) * FP_BYTES[srs.curve]
        ptrs = (_dptr(commitments, n * g1b), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, n * g1b))
        sd = _challenge_seed(seed, challenge)
        self._order(slot)
        _check(lib().kzgmi_batch_verify_device_ex_async(self.handle, srs.handle, int(slot), *ptrs, n, sd,
                                                        _flags(compressed, subgroup_check, fiat_shamir, challenge,
                                                               trusted_g1)))

    def batch_verify_multi(self, srs: Srs, shards, seed: Optional[bytes] = None, compressed: bool = False,
                           subgroup_check: bool = False, fiat_shamir: bool = False, challenge=None,
                           trusted_g1: bool = False) -> bool:
        """Multi-device context: shards[d] = (commitments, zs, ys, proofs[, n]) device tensors on
        device d of the context's list (global tuple order = shard order)."""
        g1b = (1 if compressed else 2) * FP_BYTES[srs.curve]
        D = len(shards)
        if D != self.num_devices():
            raise ValueError("need one shard per device (%d), got %d" % (self.num_devices(), D))
        cols = [[], [], [], []]
        ns = []
        for sh in shards:
            C, z, y, P = sh[:4]
            n = sh[4] if len(sh) > 4 else C.numel() // g1b
            ns.append(n)
            for i, (t, nb) in enumerate(((C, n * g1b), (z, 32 * n), (y, 32 * n), (P, n * g1b))):
                cols[i].append(_dptr(t, nb) if n else None)
        import torch
        for sh in shards:  # inputs written by torch on each device's current stream
            torch.cuda.current_stream(sh[0].device).synchronize()
        arr = [(ctypes.c_void_p * D)(*c) for c in cols]
        nn = (ctypes.c_size_t * D)(*ns)
        ok = ctypes.c_int(-1)
        _check(lib().kzgmi_batch_verify_multi_device(self.handle, srs.handle, *arr, nn, _challenge_seed(seed, challenge),
                                                     _flags(compressed, subgroup_check, fiat_shamir, challenge,
                                                            trusted_g1), ctypes.byref(ok)))
        return bool(ok.value)

    def msm_g1_multi(self, curve: str, shards) -> bytes:
        """Multi-device context: shards[d] = (points, scalars[, n]) device tensors on device d."""
        g1b = 2 * FP_BYTES[curve]
        D = len(shards)
        if D != self.num_devices():
            raise ValueError("need one shard per device (%d), got %d" % (self.num_devices(), D))
        pp, ss, ns = [], [], []
        import torch
        for sh in shards:
            n = sh[2] if len(sh) > 2 else sh[0].numel() // g1b
            ns.append(n)
            pp.append(_dptr(sh[0], n * g1b) if n else None)
            ss.append(_dptr(sh[1], 32 * n) if n else None)
            torch.cuda.current_stream(sh[0].device).synchronize()
        out = ctypes.create_string_buffer(g1b)
        _check(lib().kzgmi_msm_g1_multi_device(self.handle, CURVES[curve], (ctypes.c_void_p * D)(*pp),
                                               (ctypes.c_void_p * D)(*ss), (ctypes.c_size_t * D)(*ns), out))
        return out.raw

    # ------------------------------------------------------------------ prover commit
    def load_commit_key(self, curve: str, g1_powers: bytes, n: Optional[int] = None) -> CommitKey:
        """g1_powers: n uncompressed G1 encodings [tau^i]_1 (host bytes)."""
        pb = _host_bytes(g1_powers)
        if n is None:
            n = len(pb) // (2 * FP_BYTES[curve])
        h = ctypes.c_void_p()
        _check(lib().kzgmi_ck_load(self.handle, CURVES[curve], pb, n, ctypes.byref(h)))
        ck = CommitKey()
        ck.ctx, ck.curve, ck.n, ck.handle = self, curve, n, h
        return ck

    def commit(self, ck: CommitKey, coeffs, m: Optional[int] = None) -> bytes:
        """sum_i coeff_i [tau^i]_1 for m <= ck.n coefficients (32 B canonical Fr each)."""
        out = ctypes.create_string_buffer(2 * FP_BYTES[ck.curve])
        if _is_device_tensor(coeffs):
            if m is None:
                m = coeffs.numel() // 32
            p = _dptr(coeffs, 32 * m)
            self._order(0)
            _check(lib().kzgmi_commit_device(self.handle, ck.handle, p, m, out))
        else:
            cb = _host_bytes(coeffs)
            if m is None:
                m = len(cb) // 32
            _check(lib().kzgmi_commit(self.handle, ck.handle, cb, m, out))
        return out.raw

    # ------------------------------------------------------------------ prover openings
    def open(self, ck: CommitKey, coeffs, zs, m: Optional[int] = None, k: Optional[int] = None, ys_out=None, out=None):
        """KZG openings of p = sum_i coeff_i X^i (m <= ck.n coefficients, 32 B canonical Fr each) at the
        k points zs (32 B each): (proofs, ys) -- k uncompressed G1 encodings [q_j(tau)]_1 of
        q_j = (p - y_j) / (X - z_j), and k x 32 B evaluations y_j = p(z_j).  Device tensors in: device
        tensors out (`out`, `ys_out` where given); host buffers in: bytes out."""
        gb = 2 * FP_BYTES[ck.curve]
        if _is_device_tensor(zs):
            import torch
            if m is None:
                m = coeffs.numel() * coeffs.element_size() // 32
            if k is None:
                k = zs.numel() * zs.element_size() // 32
            if out is None:
                out = torch.empty(max(1, k) * gb, dtype=torch.uint8, device=zs.device)[:k * gb]
            if ys_out is None:
                ys_out = torch.empty(max(1, k) * 32, dtype=torch.uint8, device=zs.device)[:k * 32]
            pc = _dptr(coeffs, 32 * m) if m else None
            ptrs = (pc, int(m), _dptr(zs, 32 * k), int(k), _dptr(ys_out, 32 * k), _dptr(out, gb * k))
            self._order(0)
            _check(lib().kzgmi_open_device(self.handle, ck.handle, *ptrs))
            return out, ys_out
        hc, hz = _host_ptr(coeffs), _host_ptr(zs)
        if m is None:
            m = hc[1] // 32
        if k is None:
            k = hz[1] // 32
        if hc[1] < 32 * m or hz[1] < 32 * k:
            raise ValueError("input buffers shorter than m coefficients / k points")
        pb, yb = ctypes.create_string_buffer(max(1, k * gb)), ctypes.create_string_buffer(max(1, k * 32))
        _check(lib().kzgmi_open(self.handle, ck.handle, hc[0] or None, int(m), hz[0] or None, int(k),
                                ctypes.addressof(yb), ctypes.addressof(pb)))
        del hc, hz
        return pb.raw[:k * gb], yb.raw[:k * 32]

    def open_async(self, ck: CommitKey, slot: int, coeffs, zs, m: int, k: int, ys_out, out):
        """Enqueue open() of device tensors on `slot`; wait(slot) completes it (and raises its
        device-side errors)."""
        gb = 2 * FP_BYTES[ck.curve]
        ptrs = (_dptr(coeffs, 32 * m) if m else None, int(m), _dptr(zs, 32 * k), int(k), _dptr(ys_out, 32 * k),
                _dptr(out, gb * k))
        self._order(slot)
        _check(lib().kzgmi_open_device_async(self.handle, ck.handle, int(slot), *ptrs))

    def open_quotient(self, curve: str, coeffs, m: int, zs, k: int, ys_out=None, out=None):
        """Diagnostic: (ys, q) of m device-resident coefficients at k device-resident points: y_j = p(z_j)
        (k x 32 B) and the m - 1 coefficients of (p - y_j) / (X - z_j), lowest first (k x (m - 1) x 32 B)."""
        import torch
        nq = max(m - 1, 0)
        if ys_out is None:
            ys_out = torch.empty(max(1, k) * 32, dtype=torch.uint8, device=zs.device)[:32 * k]
        if out is None:
            out = torch.empty(max(1, k * nq) * 32, dtype=torch.uint8, device=zs.device)[:32 * k * nq]
        ptrs = (_dptr(coeffs, 32 * m) if m else None, int(m), _dptr(zs, 32 * k), int(k), _dptr(ys_out, 32 * k),
                _dptr(out, 32 * k * nq))
        self._order(0)
        _check(lib().kzgmi_open_quotient_device(self.handle, CURVES[curve], *ptrs))
        return ys_out, out

    # ------------------------------------------------------------------ transforms over Fr
    @staticmethod
    def _ntt_args(values, logn, count, inverse, bitrev, shift, nbytes):
        if logn is None:
            per = nbytes // 32 // max(1, count)
            logn = max(per, 1).bit_length() - 1
            if count < 1 or (32 << logn) * count != nbytes:
                raise ValueError("values are not count transforms of 2^logn x 32 B: pass logn")
        flags = (NTT_INVERSE if inverse else 0) | (NTT_BITREV if bitrev else 0)
        if isinstance(shift, int):
            if not 0 <= shift < (1 << 256):
                raise ValueError("shift must be in [0, 2^256)")
            shift = shift.to_bytes(32, "big")
        elif shift is not None:
            shift = bytes(shift)
            if len(shift) != 32:
                raise ValueError("shift must be 32 bytes, got %d" % len(shift))
        return int(logn), flags, shift

    def fr_ntt(self, curve: str, values, logn: Optional[int] = None, count: int = 1, inverse: bool = False,
               bitrev: bool = False, shift=None, out=None):
        """`count` transforms of n = 2^logn values of Fr (32 B big-endian canonical each, transform t at byte
        32 n t): forward, out[j] = sum_i in[i] (s w_n^j)^i; inverse=True, the n coefficients from the values
        on the coset s <w_n>; bitrev=True, the evaluation side in bit-reversed order.  shift: s as an int or
        32 big-endian bytes (None: 1).  A device tensor in gives a device tensor out (`out` where given; the
        input itself transforms in place); host bytes in give bytes out."""
        if _is_device_tensor(values):
            import torch
            nbytes = values.numel() * values.element_size()
            logn, flags, sh = self._ntt_args(values, logn, count, inverse, bitrev, shift, nbytes)
            total = (32 << logn) * count
            if out is None:
                out = torch.empty(max(1, total), dtype=torch.uint8, device=values.device)[:total]
            self._order(0)
            _check(lib().kzgmi_fr_ntt_device(self.handle, CURVES[curve], _dptr(values, total) if count else None, logn,
                                             int(count), flags, sh, _dptr(out, total) if count else None))
            return out
        hv = _host_ptr(values)
        logn, flags, sh = self._ntt_args(values, logn, count, inverse, bitrev, shift, hv[1])
        total = (32 << logn) * count
        if hv[1] < total:
            raise ValueError("input buffer shorter than count transforms of 2^logn values")
        ob = ctypes.create_string_buffer(max(1, total))
        _check(lib().kzgmi_fr_ntt(self.handle, CURVES[curve], hv[0] or None, logn, int(count), flags, sh,
                                  ctypes.addressof(ob)))
        del hv
        return ob.raw[:total]

    def fr_ntt_async(self, slot: int, curve: str, values, logn: int, count: int = 1, inverse: bool = False,
                     bitrev: bool = False, shift=None, out=None):
        """Enqueue fr_ntt() of device tensors on `slot` (out None: in place); wait(slot) completes it and
        raises its device-side errors.  Returns the output tensor."""
        logn, flags, sh = self._ntt_args(values, logn, count, inverse, bitrev, shift, 0)
        total = (32 << logn) * count
        if out is None:
            out = values
        self._order(slot)
        _check(lib().kzgmi_fr_ntt_device_async(self.handle, CURVES[curve], int(slot), _dptr(values, total) if count else None,
                                               logn, int(count), flags, sh, _dptr(out, total) if count else None))
        return out

    def open_evals(self, ck: CommitKey, evals, zs, logn: Optional[int] = None, k: Optional[int] = None,
                   bitrev: bool = False, ys_out=None, out=None):
        """open() of the polynomial given by its n = 2^logn <= ck.n values on the n-th roots of unity (32 B
        each; bitrev=True: in bit-reversed order): (proofs, ys) as open() returns them.  The inverse
        transform and the opening run as one job on the device."""
        gb = 2 * FP_BYTES[ck.curve]
        flags = NTT_BITREV if bitrev else 0
        if _is_device_tensor(zs):
            import torch
            if logn is None:
                logn = max(evals.numel() * evals.element_size() // 32, 1).bit_length() - 1
            if k is None:
                k = zs.numel() * zs.element_size() // 32
            if out is None:
                out = torch.empty(max(1, k) * gb, dtype=torch.uint8, device=zs.device)[:k * gb]
            if ys_out is None:
                ys_out = torch.empty(max(1, k) * 32, dtype=torch.uint8, device=zs.device)[:k * 32]
            ptrs = (_dptr(evals, 32 << logn), int(logn), flags, _dptr(zs, 32 * k), int(k), _dptr(ys_out, 32 * k),
                    _dptr(out, gb * k))
            self._order(0)
            _check(lib().kzgmi_open_evals_device(self.handle, ck.handle, *ptrs))
            return out, ys_out
        he, hz = _host_ptr(evals), _host_ptr(zs)
        if logn is None:
            logn = max(he[1] // 32, 1).bit_length() - 1
        if k is None:
            k = hz[1] // 32
        if he[1] < (32 << logn) or hz[1] < 32 * k:
            raise ValueError("input buffers shorter than 2^logn evaluations / k points")
        pb, yb = ctypes.create_string_buffer(max(1, k * gb)), ctypes.create_string_buffer(max(1, k * 32))
        _check(lib().kzgmi_open_evals(self.handle, ck.handle, he[0] or None, int(logn), flags, hz[0] or None, int(k),
                                      ctypes.addressof(yb), ctypes.addressof(pb)))
        del he, hz
        return pb.raw[:k * gb], yb.raw[:k * 32]

    def open_evals_async(self, ck: CommitKey, slot: int, evals, zs, logn: int, k: int, ys_out, out, bitrev: bool = False):
        """Enqueue open_evals() of device tensors on `slot`; wait(slot) completes it (and raises its
        device-side errors)."""
        gb = 2 * FP_BYTES[ck.curve]
        ptrs = (_dptr(evals, 32 << logn), int(logn), NTT_BITREV if bitrev else 0, _dptr(zs, 32 * k), int(k),
                _dptr(ys_out, 32 * k), _dptr(out, gb * k))
        self._order(slot)
        _check(lib().kzgmi_open_evals_device_async(self.handle, ck.handle, int(slot), *ptrs))

    # ------------------------------------------------------------------ transforms over G1, openings on a whole domain
    def g1_ntt(self, curve: str, points, logn: Optional[int] = None, count: int = 1, inverse: bool = False,
               bitrev: bool = False, out=None):
        """`count` transforms of n = 2^logn points of G1 (uncompressed encodings, transform t at byte
        96 | 64 times n t): forward, out[j] = sum_i [w_n^(i j)] in[i]; inverse=True, the inverse map;
        bitrev=True, the evaluation side in bit-reversed order.  A device tensor in gives a device tensor
        out (`out` where given; the input itself transforms in place); host bytes in give bytes out."""
        gb = 2 * FP_BYTES[curve]
        flags = (NTT_INVERSE if inverse else 0) | (NTT_BITREV if bitrev else 0)
        dev = _is_device_tensor(points)
        hv = None if dev else _host_ptr(points)
        nbytes = points.numel() * points.element_size() if dev else hv[1]
        if logn is None:
            per = nbytes // gb // max(1, count)
            logn = max(per, 1).bit_length() - 1
            if count < 1 or (gb << logn) * count != nbytes:
                raise ValueError("points are not count transforms of 2^logn encodings: pass logn")
        logn = int(logn)
        total = (gb << logn) * count
        if dev:
            import torch
            if out is None:
                out = torch.empty(max(1, total), dtype=torch.uint8, device=points.device)[:total]
            self._order(0)
            _check(lib().kzgmi_g1_ntt_device(self.handle, CURVES[curve], _dptr(points, total) if count else None, logn,
                                             int(count), flags, _dptr(out, total) if count else None))
            return out
        if hv[1] < total:
            raise ValueError("input buffer shorter than count transforms of 2^logn points")
        ob = ctypes.create_string_buffer(max(1, total))
        _check(lib().kzgmi_g1_ntt(self.handle, CURVES[curve], hv[0] or None, logn, int(count), flags, ctypes.addressof(ob)))
        del hv
        return ob.raw[:total]

    def g1_ntt_async(self, slot: int, curve: str, points, logn: int, count: int = 1, inverse: bool = False,
                     bitrev: bool = False, out=None):
        """Enqueue g1_ntt() of device tensors on `slot` (out None: in place); wait(slot) completes it and
        raises its device-side errors.  Returns the output tensor."""
        flags = (NTT_INVERSE if inverse else 0) | (NTT_BITREV if bitrev else 0)
        total = ((2 * FP_BYTES[curve]) << int(logn)) * count
        if out is None:
            out = points
        self._order(slot)
        _check(lib().kzgmi_g1_ntt_device_async(self.handle, CURVES[curve], int(slot), _dptr(points, total) if count else None,
                                               int(logn), int(count), flags, _dptr(out, total) if count else None))
        return out

    def load_open_all_key(self, ck: CommitKey, logn: int) -> OpenAllKey:
        """The key of open_all on the 2^logn-th roots of unity, derived on the device from `ck`."""
        h = ctypes.c_void_p()
        self._order(0)
        _check(lib().kzgmi_open_all_key_load(self.handle, ck.handle, int(logn), ctypes.byref(h)))
        key = OpenAllKey()
        key.ctx, key.curve, key.logn, key.handle = self, ck.curve, int(logn), h
        return key

    def open_all(self, key: OpenAllKey, coeffs, m: Optional[int] = None, bitrev: bool = False, want_ys: bool = True,
                 ys_out=None, out=None):
        """KZG openings of p = sum_i coeff_i X^i (m <= n = 2^key.logn coefficients, 32 B each) at all n
        points w_n^e: (proofs, ys) -- entry e is open()'s result for z = w_n^e (bitrev=True: at index
        rev(e)); ys is None with want_ys=False.  Device tensors in: device tensors out; host bytes in:
        bytes out."""
        gb, n = 2 * FP_BYTES[key.curve], 1 << key.logn
        flags = NTT_BITREV if bitrev else 0
        if _is_device_tensor(coeffs):
            import torch
            if m is None:
                m = coeffs.numel() * coeffs.element_size() // 32
            if out is None:
                out = torch.empty(n * gb, dtype=torch.uint8, device=coeffs.device)
            if ys_out is None and want_ys:
                ys_out = torch.empty(n * 32, dtype=torch.uint8, device=coeffs.device)
            self._order(0)
            _check(lib().kzgmi_open_all_device(self.handle, key.handle, _dptr(coeffs, 32 * m) if m else None, int(m), flags,
                                               _dptr(ys_out, 32 * n) if ys_out is not None else None, _dptr(out, gb * n)))
            return out, ys_out
        hc = _host_ptr(coeffs)
        if m is None:
            m = hc[1] // 32
        if hc[1] < 32 * m:
            raise ValueError("input buffer shorter than m coefficients")
        pb = ctypes.create_string_buffer(n * gb)
        yb = ctypes.create_string_buffer(n * 32) if want_ys else None
        _check(lib().kzgmi_open_all(self.handle, key.handle, hc[0] or None, int(m), flags,
                                    ctypes.addressof(yb) if want_ys else None, ctypes.addressof(pb)))
        del hc
        return pb.raw, (yb.raw if want_ys else None)

    def open_all_async(self, key: OpenAllKey, slot: int, coeffs, m: int, ys_out, out, bitrev: bool = False):
        """Enqueue open_all() of device tensors on `slot` (ys_out may be None); wait(slot) completes it
        (and raises its device-side errors)."""
        gb, n = 2 * FP_BYTES[key.curve], 1 << key.logn
        self._order(slot)
        _check(lib().kzgmi_open_all_device_async(self.handle, key.handle, int(slot), _dptr(coeffs, 32 * m) if m else None,
                                                 int(m), NTT_BITREV if bitrev else 0,
                                                 _dptr(ys_out, 32 * n) if ys_out is not None else None, _dptr(out, gb * n)))

    def load_open_cosets_key(self, ck: CommitKey, logN: int, logl: int) -> OpenCosetsKey:
        """The key of open_cosets for polynomials of up to 2^logN coefficients opened on cosets of 2^logl
        points, derived on the device from `ck` (which must hold 2^logN - 2^logl powers)."""
        h = ctypes.c_void_p()
        self._order(0)
        _check(lib().kzgmi_open_cosets_key_load(self.handle, ck.handle, int(logN), int(logl), ctypes.byref(h)))
        key = OpenCosetsKey()
        key.ctx, key.curve, key.logN, key.logl, key.handle = self, ck.curve, int(logN), int(logl), h
        return key

    def open_cosets(self, key: OpenCosetsKey, coeffs, logk: int, m: Optional[int] = None, count: int = 1,
                    bitrev: bool = False, want_ys: bool = True, ys_out=None, out=None):
        """FK20 multi-proofs of `count` polynomials of m <= 2^key.logN coefficients each (32 B each, one
        polynomial after the other) on the K = 2^logk cosets of l = 2^key.logl points of the K l-th roots of
        unity: (proofs, ys) -- count x K encodings and count x K l evaluations, coset-major (bitrev=True: both
        in bit-reversed order, EIP-7594's at (12, 6, 7)); ys is None with want_ys=False.  m defaults to the
        input's length / count.  Device tensors in: device tensors out; host bytes in: bytes out."""
        gb, logk, count = 2 * FP_BYTES[key.curve], int(logk), int(count)
        flags = NTT_BITREV if bitrev else 0
        pb, yb = (gb * count) << logk, (32 * count) << (logk + key.logl)
        if _is_device_tensor(coeffs):
            import torch
            if m is None:
                m = coeffs.numel() * coeffs.element_size() // 32 // max(1, count)
            if out is None:
                out = torch.empty(max(1, pb), dtype=torch.uint8, device=coeffs.device)[:pb]
            if ys_out is None and want_ys:
                ys_out = torch.empty(max(1, yb), dtype=torch.uint8, device=coeffs.device)[:yb]
            self._order(0)
            _check(lib().kzgmi_open_cosets_device(
                self.handle, key.handle, _dptr(coeffs, 32 * m * count) if m * count else None, int(m), count, logk, flags,
                _dptr(ys_out, yb) if ys_out is not None and count else None, _dptr(out, pb) if count else None))
            return out, ys_out
        hc = _host_ptr(coeffs)
        if m is None:
            m = hc[1] // 32 // max(1, count)
        if hc[1] < 32 * m * count:
            raise ValueError("input buffer shorter than count polynomials of m coefficients")
        pbuf = ctypes.create_string_buffer(max(1, pb))
        ybuf = ctypes.create_string_buffer(max(1, yb)) if want_ys else None
        _check(lib().kzgmi_open_cosets(self.handle, key.handle, hc[0] or None, int(m), count, logk, flags,
                                       ctypes.addressof(ybuf) if want_ys else None, ctypes.addressof(pbuf)))
        del hc
        return pbuf.raw[:pb], (ybuf.raw[:yb] if want_ys else None)

    def open_cosets_async(self, key: OpenCosetsKey, slot: int, coeffs, m: int, logk: int, ys_out, out, count: int = 1,
                          bitrev: bool = False):
        """Enqueue open_cosets() of device tensors on `slot` (ys_out may be None); wait(slot) completes it
        (and raises its device-side errors)."""
        gb, logk, count = 2 * FP_BYTES[key.curve], int(logk), int(count)
        pb, yb = (gb * count) << logk, (32 * count) << (logk + key.logl)
        self._order(slot)
        _check(lib().kzgmi_open_cosets_device_async(
            self.handle, key.handle, int(slot), _dptr(coeffs, 32 * m * count) if m * count else None, int(m), count, logk,
            NTT_BITREV if bitrev else 0, _dptr(ys_out, yb) if ys_out is not None and count else None,
            _dptr(out, pb) if count else None))

    # ------------------------------------------------------------------ Fiat-Shamir
    def commit_async(self, ck: CommitKey, slot: int, coeffs, m: int):
        """Enqueue a fixed-base commitment of m device-resident coefficients on `slot`;
        msm_wait(slot) returns it."""
        self._msm_curve = getattr(self, "_msm_curve", {})
        self._msm_curve[slot] = ck.curve
        p = _dptr(coeffs, 32 * m)
        self._order(slot)
        _check(lib().kzgmi_commit_device_async(self.handle, ck.handle, int(slot), p, int(m)))

    def fs_challenge(self, curve: str, commitments, zs, ys, proofs, n: int, compressed: bool = False) -> int:
        """r of KZGMI_FLAG_FIAT_SHAMIR for device-resident inputs."""
        out = ctypes.create_string_buffer(32)
        g1b = (1 if compressed else 2) * FP_BYTES[curve]
        ptrs = (_dptr(commitments, n * g1b), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, n * g1b))
        self._order(0)
        _check(lib().kzgmi_fs_challenge_device(self.handle, CURVES[curve], *ptrs, n, _flags(compressed), out))
        return int.from_bytes(out.raw, "big")

    def fs_chunk_digests(self, curve: str, commitments, zs, ys, proofs, n: int, index_offset: int, out,
                         compressed: bool = False):
        """Shard's 4096-leaf subtree roots (ceil(n / 4096) x 32 B) into device tensor `out`."""
        g1b = (1 if compressed else 2) * FP_BYTES[curve]
        ptrs = (_dptr(commitments, n * g1b), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, n * g1b))
        po = _dptr(out, 32 * ((n + FS_CHUNK - 1) // FS_CHUNK))
        self._order(0)
        _check(lib().kzgmi_fs_chunk_digests_device(self.handle, CURVES[curve], *ptrs, n, int(index_offset),
                                                   _flags(compressed), po))

    def fs_challenge_from_digests(self, curve: str, digests, nchunks: int, n_total: int) -> int:
        out = ctypes.create_string_buffer(32)
        p = _dptr(digests, 32 * nchunks)
        self._order(0)
        _check(lib().kzgmi_fs_challenge_from_digests_device(self.handle, CURVES[curve], p, nchunks,
                                                            int(n_total), out))
        return int.from_bytes(out.raw, "big")

    def g1_validate(self, curve: str, points, n: int, compressed: bool = False, subgroup_check: bool = False):
        """Raise KzgmiError unless all n device-resident G1 encodings are valid."""
        p = _dptr(points, n * (1 if compressed else 2) * FP_BYTES[curve])
        self._order(0)
        _check(lib().kzgmi_g1_validate_device(self.handle, CURVES[curve], p, n, _flags(compressed, subgroup_check)))

    def g1_compress(self, curve: str, points, n: int, out):
        """Device utility: uncompressed G1 encodings -> compressed (no validation)."""
        pi, po = _dptr(points, 2 * n * FP_BYTES[curve]), _dptr(out, n * FP_BYTES[curve])
        self._order(0)
        _check(lib().kzgmi_g1_compress_device(self.handle, CURVES[curve], pi, n, po))

    # ------------------------------------------------------------------ EIP-4844 blobs
    def blob_challenges(self, blobs, commitments, n: int, out=None):
        """z_i = H("FSBLOBVERIFY_V1_" || be128(4096) || blob_i || C_i) mod r for n device-resident
        blobs (n x 128 KiB) and compressed commitments (n x 48 B): a device tensor of n x 32 B."""
        import torch
        if out is None:
            out = torch.empty(32 * n, dtype=torch.uint8, device=blobs.device)
        pb, pc, po = _dptr(blobs, n * BLOB_BYTES), _dptr(commitments, 48 * n), _dptr(out, 32 * n)
        self._order(0)
        _check(lib().kzgmi_blob_challenges_device(self.handle, pb, pc, int(n), po))
        return out

    def blob_eval(self, blobs, zs, n: int, out=None):
        """y_i = p_i(z_i) for the blob polynomials in evaluation form over the bit-reversed 4096th
        roots of unity (any z < r, points of the domain included): a device tensor of n x 32 B."""
        import torch
        if out is None:
            out = torch.empty(32 * n, dtype=torch.uint8, device=blobs.device)
        pb, pz, po = _dptr(blobs, n * BLOB_BYTES), _dptr(zs, 32 * n), _dptr(out, 32 * n)
        self._order(0)
        _check(lib().kzgmi_blob_eval_device(self.handle, pb, pz, int(n), po))
        return out

    def blob_batch_challenge(self, commitments, zs, ys, proofs, n: int) -> int:
        """r = H("RCKZGBATCH___V1_" || be64(4096) || be64(n) || (C_i || z_i || y_i || pi_i)_i) mod r
        for device-resident arrays."""
        out = ctypes.create_string_buffer(32)
        ptrs = (_dptr(commitments, 48 * n), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, 48 * n))
        self._order(0)
        _check(lib().kzgmi_blob_batch_challenge_device(self.handle, *ptrs, int(n), out))
        return int.from_bytes(out.raw, "big")

    def verify_blob_batch(self, srs: Srs, blobs, commitments, proofs, n: Optional[int] = None) -> bool:
        """verify_blob_kzg_proof_batch: blobs (n x 128 KiB), compressed commitments and proofs
        (n x 48 B each) as host buffers or device tensors; challenges, evaluations and the
        powers-of-r batch check all run on the GPU."""
        ok = ctypes.c_int(-1)
        if _is_device_tensor(blobs):
            if n is None:
                n = commitments.numel() // 48
            ptrs = (_dptr(blobs, n * BLOB_BYTES), _dptr(commitments, 48 * n), _dptr(proofs, 48 * n))
            self._order(0)
            _check(lib().kzgmi_verify_blob_batch_device(self.handle, srs.handle, *ptrs, int(n), ctypes.byref(ok)))
        else:
            (pb, lb, kb), (pc, lc, kc), (pp, lp, kp) = (_host_ptr(v) for v in (blobs, commitments, proofs))
            if n is None:
                n = lc // 48
            if lb < n * BLOB_BYTES or lc < 48 * n or lp < 48 * n:
                raise ValueError("input buffers shorter than n blobs")
            _check(lib().kzgmi_verify_blob_batch(self.handle, srs.handle, pb, pc, pp, int(n), ctypes.byref(ok)))
            del kb, kc, kp
        return bool(ok.value)

    def verify_blob_batch_async(self, srs: Srs, slot: int, blobs, commitments, proofs, n: int):
        """Enqueue verify_blob_batch of device tensors on `slot`; wait(slot) returns the verdict."""
        ptrs = (_dptr(blobs, n * BLOB_BYTES), _dptr(commitments, 48 * n), _dptr(proofs, 48 * n))
        self._order(slot)
        _check(lib().kzgmi_verify_blob_batch_device_async(self.handle, srs.handle, int(slot), *ptrs, int(n)))

    # ------------------------------------------------------------------ EIP-4844 commitments and proofs
    def load_blob_proof_key(self, g1_lagrange: bytes) -> BlobProofKey:
        """The blob proof key of g1_lagrange = [l_j(tau)]_1 for the Lagrange polynomial of dom[j], j < 4096
        (4096 x 96 B: the trusted setup's Lagrange points in bit-reversed order)."""
        if len(g1_lagrange) != 4096 * 96:
            raise ValueError("g1_lagrange must hold 4096 uncompressed G1 points (393216 bytes)")
        h = ctypes.c_void_p()
        _check(lib().kzgmi_blob_pk_load(self.handle, bytes(g1_lagrange), ctypes.byref(h)))
        return BlobProofKey(self, h)

    @staticmethod
    def _blob_pk_handle(pk):
        if not isinstance(pk, BlobProofKey):
            raise KzgmiError(-1, "not a blob proof key (Context.load_blob_proof_key)")
        return pk.handle

    def _blob_job(self, name, pk, blobs, second, second_bytes, n, outs, out_bytes):
        """One of the three producer calls: `second` (zs or commitments, second_bytes each; None for a
        commitment), outputs of out_bytes[i] per blob.  Device tensors in: device tensors out (`outs[i]`
        where given); host buffers in: bytes out."""
        h = self._blob_pk_handle(pk)
        ins = [blobs] + ([second] if second_bytes else [])
        in_bytes = [BLOB_BYTES] + ([second_bytes] if second_bytes else [])
        if _is_device_tensor(blobs):
            import torch
            if n is None:
                n = blobs.numel() * blobs.element_size() // BLOB_BYTES
            outs = [torch.empty(n * b, dtype=torch.uint8, device=blobs.device) if o is None else o
                    for o, b in zip(outs, out_bytes)]
            ptrs = [_dptr(x, n * b) for x, b in zip(ins, in_bytes)]
            optrs = [_dptr(o, n * b) for o, b in zip(outs, out_bytes)]
            self._order(0)
            _check(getattr(lib(), name + "_device")(self.handle, h, *ptrs, int(n), *optrs))
            return outs
        held = [_host_ptr(x) for x in ins]
        if n is None:
            n = held[0][1] // BLOB_BYTES
        if any(l < n * b for (_, l, _), b in zip(held, in_bytes)):
            raise ValueError("input buffers shorter than n blobs")
        bufs = [ctypes.create_string_buffer(max(1, n * b)) for b in out_bytes]
        _check(getattr(lib(), name)(self.handle, h, *[p for p, _, _ in held], int(n),
                                    *[ctypes.addressof(b) for b in bufs]))
        del held
        return [buf.raw[:n * b] for buf, b in zip(bufs, out_bytes)]

    def _blob_job_async(self, name, pk, slot, blobs, second, second_bytes, n, outs, out_bytes):
        h = self._blob_pk_handle(pk)
        ptrs = [_dptr(blobs, n * BLOB_BYTES)] + ([_dptr(second, n * second_bytes)] if second_bytes else [])
        optrs = [_dptr(o, n * b) for o, b in zip(outs, out_bytes)]
        self._order(slot)
        _check(getattr(lib(), name + "_device_async")(self.handle, h, int(slot), *ptrs, int(n), *optrs))

    def blob_commit(self, pk: BlobProofKey, blobs, n: Optional[int] = None, out=None):
        """blob_to_kzg_commitment for n blobs (n x 128 KiB): n x 48 B compressed commitments.  Device
        tensor in: a device tensor out (`out` if given); host buffer in: bytes out."""
        return self._blob_job("kzgmi_blob_commit", pk, blobs, None, 0, n, [out], [48])[0]

    def blob_commit_async(self, pk: BlobProofKey, slot: int, blobs, n: int, out):
        """Enqueue blob_commit of device tensors on `slot`; wait(slot) completes it (and raises its
        device-side errors)."""
        self._blob_job_async("kzgmi_blob_commit", pk, slot, blobs, None, 0, n, [out], [48])

    def compute_kzg_proofs(self, pk: BlobProofKey, blobs, zs, n: Optional[int] = None, out=None, ys_out=None):
        """compute_kzg_proof for n blobs at zs (n x 32 B big-endian, any z < r): (proofs, ys), n x 48 B
        compressed proofs and n x 32 B evaluations y_i = p_i(z_i)."""
        return tuple(self._blob_job("kzgmi_compute_kzg_proofs", pk, blobs, zs, 32, n, [out, ys_out], [48, 32]))

    def compute_kzg_proofs_async(self, pk: BlobProofKey, slot: int, blobs, zs, n: int, out, ys_out):
        """Enqueue compute_kzg_proofs of device tensors on `slot`; wait(slot) completes it."""
        self._blob_job_async("kzgmi_compute_kzg_proofs", pk, slot, blobs, zs, 32, n, [out, ys_out], [48, 32])

    def compute_blob_proofs(self, pk: BlobProofKey, blobs, commitments, n: Optional[int] = None, out=None):
        """compute_blob_kzg_proof for n blobs and their compressed commitments (n x 48 B, validated): the
        n x 48 B proofs at each blob's own challenge, as verify_blob_batch checks them."""
        return self._blob_job("kzgmi_compute_blob_proofs", pk, blobs, commitments, 48, n, [out], [48])[0]

    def compute_blob_proofs_async(self, pk: BlobProofKey, slot: int, blobs, commitments, n: int, out):
        """Enqueue compute_blob_proofs of device tensors on `slot`; wait(slot) completes it."""
        self._blob_job_async("kzgmi_compute_blob_proofs", pk, slot, blobs, commitments, 48, n, [out], [48])

    def blob_quotient(self, blobs, zs, n: int, ys_out=None, out=None):
        """Diagnostic: (ys, q) of n device-resident blobs at zs: y_i = p_i(z_i) (n x 32 B) and the
        evaluations of (p_i - y_i) / (X - z_i) on the domain (n x 128 KiB, blob layout)."""
        import torch
        if ys_out is None:
            ys_out = torch.empty(32 * n, dtype=torch.uint8, device=blobs.device)
        if out is None:
            out = torch.empty(n * BLOB_BYTES, dtype=torch.uint8, device=blobs.device)
        ptrs = (_dptr(blobs, n * BLOB_BYTES), _dptr(zs, 32 * n))
        py, pq = _dptr(ys_out, 32 * n), _dptr(out, n * BLOB_BYTES)
        self._order(0)
        _check(lib().kzgmi_blob_quotient_device(self.handle, *ptrs, int(n), py, pq))
        return ys_out, out

    # ------------------------------------------------------------------ EIP-7594 cells
    def load_cell_srs(self, g1_monomial: bytes, g2: bytes, tau64_g2: bytes) -> CellSrs:
        """The cell SRS: g1_monomial = [tau^m]_1 for m < 64 (64 x 96 B), [1]_2, [tau^64]_2."""
        if len(g1_monomial) != 64 * 96:
            raise ValueError("g1_monomial must hold 64 uncompressed G1 points (6144 bytes)")
        h = ctypes.c_void_p()
        _check(lib().kzgmi_cell_srs_load(self.handle, bytes(g1_monomial), bytes(g2), bytes(tau64_g2), ctypes.byref(h)))
        return CellSrs(self, h)

    @staticmethod
    def _cell_srs_handle(srs):
        if not isinstance(srs, CellSrs):
            raise KzgmiError(-1, "not a cell SRS (Context.load_cell_srs)")
        return srs.handle

    def cell_batch_challenge(self, commitments, commitment_indices, cell_indices, cells, proofs, m: int, n: int) -> int:
        """r of verify_cell_kzg_proof_batch's transcript for device-resident arrays: m unique 48-byte
        commitments, n uint64 commitment indices and cell indices, n cells (2048 B), n 48-byte proofs."""
        out = ctypes.create_string_buffer(32)
        ptrs = (_dptr(commitments, 48 * m), int(m), _dptr(commitment_indices, 8 * n), _dptr(cell_indices, 8 * n),
                _dptr(cells, CELL_BYTES * n), _dptr(proofs, 48 * n))
        self._order(0)
        _check(lib().kzgmi_cell_batch_challenge_device(self.handle, *ptrs, int(n), out))
        return int.from_bytes(out.raw, "big")

    def cell_interp(self, cell_indices, cells, n: int, r, out=None):
        """The 64 coefficients c_m of sum_k r^k I_k (I_k: cell k's interpolation polynomial on its
        coset) for device-resident uint64 cell indices and cells: a device tensor of 64 x 32 B."""
        import torch
        if out is None:
            out = torch.empty(32 * 64, dtype=torch.uint8, device=cells.device)
        pi, pc, po = _dptr(cell_indices, 8 * n), _dptr(cells, CELL_BYTES * n), _dptr(out, 32 * 64)
        self._order(0)
        _check(lib().kzgmi_cell_interp_device(self.handle, pi, pc, int(n), _r32(r), po))
        return out

    def verify_cell_batch(self, srs: CellSrs, commitments, commitment_indices, cell_indices, cells, proofs,
                          m: Optional[int] = None, n: Optional[int] = None, r=None) -> bool:
        """verify_cell_kzg_proof_batch in its deduplicated form: m unique compressed commitments, n
        uint64 commitment indices and cell indices, n cells and n compressed proofs, as host buffers
        or device tensors (indices on the host may be Python sequences).  r: the batch challenge
        if the caller hashed the transcript itself; None derives it on the GPU."""
        ok = ctypes.c_int(-1)
        h = self._cell_srs_handle(srs)
        if _is_device_tensor(cells):
            if n is None:
                n = proofs.numel() // 48
            if m is None:
                m = commitments.numel() // 48
            ptrs = (_dptr(commitments, 48 * m), int(m), _dptr(commitment_indices, 8 * n), _dptr(cell_indices, 8 * n),
                    _dptr(cells, CELL_BYTES * n), _dptr(proofs, 48 * n))
            self._order(0)
            _check(lib().kzgmi_verify_cell_batch_device(self.handle, h, *ptrs, int(n), _r32(r), ctypes.byref(ok)))
        else:
            ci, ce = _u64_bytes(commitment_indices), _u64_bytes(cell_indices)
            (pc, lc, kc), (pi, li, ki), (pe, le, ke), (pl, ll, kl), (pp, lp, kp) = (
                _host_ptr(v) for v in (commitments, ci, ce, cells, proofs))
            if n is None:
                n = lp // 48
            if m is None:
                m = lc // 48
            if lc < 48 * m or li < 8 * n or le < 8 * n or ll < CELL_BYTES * n or lp < 48 * n:
                raise ValueError("input buffers shorter than n cells")
            _check(lib().kzgmi_verify_cell_batch(self.handle, h, pc, int(m), pi, pe, pl, pp, int(n), _r32(r),
                                                 ctypes.byref(ok)))
            del kc, ki, ke, kl, kp
        return bool(ok.value)

    def verify_cell_batch_async(self, srs: CellSrs, slot: int, commitments, commitment_indices, cell_indices, cells,
                                proofs, m: int, n: int, r=None):
        """Enqueue verify_cell_batch of device tensors on `slot`; wait(slot) returns the verdict."""
        h = self._cell_srs_handle(srs)
        ptrs = (_dptr(commitments, 48 * m), int(m), _dptr(commitment_indices, 8 * n), _dptr(cell_indices, 8 * n),
                _dptr(cells, CELL_BYTES * n), _dptr(proofs, 48 * n))
        self._order(slot)
        _check(lib().kzgmi_verify_cell_batch_device_async(self.handle, h, int(slot), *ptrs, int(n), _r32(r)))

    # ------------------------------------------------------------------ EIP-7594 cell extension / recovery
    @staticmethod
    def _device_indices(cell_indices, like):
        """(tensor, k): the uint64 cell indices on `like`'s device (a device tensor is taken as it is)."""
        if _is_device_tensor(cell_indices):
            return cell_indices, cell_indices.numel() * cell_indices.element_size() // 8
        import torch
        raw = _u64_bytes(cell_indices)
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(like.device), len(raw) // 8

    def compute_cells(self, blobs, n: Optional[int] = None, out=None):
        """compute_cells (the cells only, no proofs): n blobs (n x 128 KiB) -> their 128 cells each
        (n x 256 KiB, cell i of blob b at byte 262144 b + 2048 i).  Device tensor in: a device tensor
        out (`out` if given); host buffer in: bytes out."""
        if _is_device_tensor(blobs):
            import torch
            if n is None:
                n = blobs.numel() * blobs.element_size() // BLOB_BYTES
            if out is None:
                out = torch.empty(n * EXT_BLOB_BYTES, dtype=torch.uint8, device=blobs.device)
            pb, po = _dptr(blobs, n * BLOB_BYTES), _dptr(out, n * EXT_BLOB_BYTES)
            self._order(0)
            _check(lib().kzgmi_compute_cells_device(self.handle, pb, int(n), po))
            return out
        pb, lb, kb = _host_ptr(blobs)
        if n is None:
            n = lb // BLOB_BYTES
        if lb < n * BLOB_BYTES:
            raise ValueError("input buffer shorter than n blobs")
        buf = ctypes.create_string_buffer(max(1, n * EXT_BLOB_BYTES))
        _check(lib().kzgmi_compute_cells(self.handle, pb, int(n), ctypes.addressof(buf)))
        del kb
        return buf.raw[:n * EXT_BLOB_BYTES]

    def compute_cells_async(self, slot: int, blobs, n: int, out):
        """Enqueue compute_cells of device tensors on `slot`; wait(slot) completes it (and raises
        its device-side errors)."""
        pb, po = _dptr(blobs, n * BLOB_BYTES), _dptr(out, n * EXT_BLOB_BYTES)
        self._order(slot)
        _check(lib().kzgmi_compute_cells_device_async(self.handle, int(slot), pb, int(n), po))

    def recover_cells(self, cell_indices, cells, n_blobs: Optional[int] = None, out=None):
        """The cells of recover_cells_and_kzg_proofs for n_blobs blobs that share their k cell indices
        (64 <= k <= 128, distinct, any order): cells holds n_blobs x k cells, blob after blob, each
        blob's in the order of the indices.  Returns all 128 cells of every blob (n_blobs x 256 KiB).
        Inconsistent cells (no polynomial of degree < 4096 takes them all) raise KzgmiError
        (KZGMI_ERR_ARG).  Device tensor in: a device tensor out; host buffer in: bytes out."""
        if _is_device_tensor(cells):
            import torch
            idx, k = self._device_indices(cell_indices, cells)
            if n_blobs is None:
                n_blobs = cells.numel() * cells.element_size() // (CELL_BYTES * k) if k else 0
            if out is None:
                out = torch.empty(n_blobs * EXT_BLOB_BYTES, dtype=torch.uint8, device=cells.device)
            pi, pc = _dptr(idx, 8 * k), _dptr(cells, n_blobs * k * CELL_BYTES)
            po = _dptr(out, n_blobs * EXT_BLOB_BYTES)
            self._order(0)
            _check(lib().kzgmi_recover_cells_device(self.handle, pi, int(k), pc, int(n_blobs), po))
            return out
        raw = _u64_bytes(cell_indices)
        k = len(raw) // 8
        (pi, li, ki), (pc, lc, kc) = _host_ptr(raw), _host_ptr(cells)
        if n_blobs is None:
            n_blobs = lc // (CELL_BYTES * k) if k else 0
        if lc < n_blobs * k * CELL_BYTES:
            raise ValueError("input buffer shorter than n_blobs x k cells")
        buf = ctypes.create_string_buffer(max(1, n_blobs * EXT_BLOB_BYTES))
        _check(lib().kzgmi_recover_cells(self.handle, pi, int(k), pc, int(n_blobs), ctypes.addressof(buf)))
        del ki, kc
        return buf.raw[:n_blobs * EXT_BLOB_BYTES]

    def recover_cells_async(self, slot: int, cell_indices, cells, n_blobs: int, out):
        """Enqueue recover_cells of device tensors on `slot` (cell_indices: a device tensor of k
        uint64, kept alive by the caller until wait(slot)); wait(slot) completes it."""
        k = cell_indices.numel() * cell_indices.element_size() // 8
        pi, pc = _dptr(cell_indices, 8 * k), _dptr(cells, n_blobs * k * CELL_BYTES)
        po = _dptr(out, n_blobs * EXT_BLOB_BYTES)
        self._order(slot)
        _check(lib().kzgmi_recover_cells_device_async(self.handle, int(slot), pi, int(k), pc, int(n_blobs), po))

    # ------------------------------------------------------------------ EIP-7594 cell proofs (FK20)
    def load_cell_proof_key(self, g1_monomial: bytes) -> CellProofKey:
        """The cell proof key of g1_monomial = [tau^m]_1 for m < 4096 (4096 x 96 B)."""
        if len(g1_monomial) != 4096 * 96:
            raise ValueError("g1_monomial must hold 4096 uncompressed G1 points (393216 bytes)")
        h = ctypes.c_void_p()
        _check(lib().kzgmi_cell_pk_load(self.handle, bytes(g1_monomial), ctypes.byref(h)))
        return CellProofKey(self, h)

    @staticmethod
    def _cell_pk_handle(pk):
        if not isinstance(pk, CellProofKey):
            raise KzgmiError(-1, "not a cell proof key (Context.load_cell_proof_key)")
        return pk.handle

    def compute_cells_and_proofs(self, pk: CellProofKey, blobs, n: Optional[int] = None, cells=True, out=None,
                                 proofs_out=None):
        """compute_cells_and_kzg_proofs: n blobs -> (cells, proofs): the cells of compute_cells (None
        with cells=False) and the 128 compressed proofs of every blob (n x 6144 B, proof i of blob b at
        byte 48 (128 b + i)).  Device tensor in: device tensors out (`out`, `proofs_out` if given);
        host buffer in: bytes out."""
        h = self._cell_pk_handle(pk)
        if _is_device_tensor(blobs):
            import torch
            if n is None:
                n = blobs.numel() * blobs.element_size() // BLOB_BYTES
            if cells and out is None:
                out = torch.empty(n * EXT_BLOB_BYTES, dtype=torch.uint8, device=blobs.device)
            if proofs_out is None:
                proofs_out = torch.empty(n * PROOFS_BYTES, dtype=torch.uint8, device=blobs.device)
            pc = _dptr(out, n * EXT_BLOB_BYTES) if cells else None
            pb, pp = _dptr(blobs, n * BLOB_BYTES), _dptr(proofs_out, n * PROOFS_BYTES)
            self._order(0)
            _check(lib().kzgmi_compute_cells_and_proofs_device(self.handle, h, pb, int(n), pc, pp))
            return (out if cells else None), proofs_out
        pb, lb, kb = _host_ptr(blobs)
        if n is None:
            n = lb // BLOB_BYTES
        if lb < n * BLOB_BYTES:
            raise ValueError("input buffer shorter than n blobs")
        cbuf = ctypes.create_string_buffer(max(1, n * EXT_BLOB_BYTES)) if cells else None
        pbuf = ctypes.create_string_buffer(max(1, n * PROOFS_BYTES))
        _check(lib().kzgmi_compute_cells_and_proofs(self.handle, h, pb, int(n),
                                                    ctypes.addressof(cbuf) if cells else None, ctypes.addressof(pbuf)))
        del kb
        return (cbuf.raw[:n * EXT_BLOB_BYTES] if cells else None), pbuf.raw[:n * PROOFS_BYTES]

    def compute_cells_and_proofs_async(self, pk: CellProofKey, slot: int, blobs, n: int, out, proofs_out):
        """Enqueue compute_cells_and_proofs of device tensors on `slot` (out None: proofs only);
        wait(slot) completes it (and raises its device-side errors)."""
        h = self._cell_pk_handle(pk)
        pc = _dptr(out, n * EXT_BLOB_BYTES) if out is not None else None
        pb, pp = _dptr(blobs, n * BLOB_BYTES), _dptr(proofs_out, n * PROOFS_BYTES)
        self._order(slot)
        _check(lib().kzgmi_compute_cells_and_proofs_device_async(self.handle, h, int(slot), pb, int(n), pc, pp))

    def recover_cells_and_proofs(self, pk: CellProofKey, cell_indices, cells, n_blobs: Optional[int] = None, out=None,
                                 proofs_out=None):
        """recover_cells_and_kzg_proofs: recover_cells, then the 128 proofs of every recovered blob ->
        (cells, proofs).  Inconsistent cells raise KzgmiError (KZGMI_ERR_ARG) as recover_cells does.
        Device tensor in: device tensors out; host buffer in: bytes out."""
        h = self._cell_pk_handle(pk)
        if _is_device_tensor(cells):
            import torch
            idx, k = self._device_indices(cell_indices, cells)
            if n_blobs is None:
                n_blobs = cells.numel() * cells.element_size() // (CELL_BYTES * k) if k else 0
            if out is None:
                out = torch.empty(n_blobs * EXT_BLOB_BYTES, dtype=torch.uint8, device=cells.device)
            if proofs_out is None:
                proofs_out = torch.empty(n_blobs * PROOFS_BYTES, dtype=torch.uint8, device=cells.device)
            pi, pc = _dptr(idx, 8 * k), _dptr(cells, n_blobs * k * CELL_BYTES)
            po, pp = _dptr(out, n_blobs * EXT_BLOB_BYTES), _dptr(proofs_out, n_blobs * PROOFS_BYTES)
            self._order(0)
            _check(lib().kzgmi_recover_cells_and_proofs_device(self.handle, h, pi, int(k), pc, int(n_blobs), po, pp))
            return out, proofs_out
        raw = _u64_bytes(cell_indices)
        k = len(raw) // 8
        (pi, li, ki), (pc, lc, kc) = _host_ptr(raw), _host_ptr(cells)
        if n_blobs is None:
            n_blobs = lc // (CELL_BYTES * k) if k else 0
        if lc < n_blobs * k * CELL_BYTES:
            raise ValueError("input buffer shorter than n_blobs x k cells")
        cbuf = ctypes.create_string_buffer(max(1, n_blobs * EXT_BLOB_BYTES))
        pbuf = ctypes.create_string_buffer(max(1, n_blobs * PROOFS_BYTES))
        _check(lib().kzgmi_recover_cells_and_proofs(self.handle, h, pi, int(k), pc, int(n_blobs),
                                                    ctypes.addressof(cbuf), ctypes.addressof(pbuf)))
        del ki, kc
        return cbuf.raw[:n_blobs * EXT_BLOB_BYTES], pbuf.raw[:n_blobs * PROOFS_BYTES]

    def recover_cells_and_proofs_async(self, pk: CellProofKey, slot: int, cell_indices, cells, n_blobs: int, out,
                                       proofs_out):
        """Enqueue recover_cells_and_proofs of device tensors on `slot` (cell_indices: a device tensor
        of k uint64, kept alive by the caller until wait(slot)); wait(slot) completes it."""
        h = self._cell_pk_handle(pk)
        k = cell_indices.numel() * cell_indices.element_size() // 8
        pi, pc = _dptr(cell_indices, 8 * k), _dptr(cells, n_blobs * k * CELL_BYTES)
        po, pp = _dptr(out, n_blobs * EXT_BLOB_BYTES), _dptr(proofs_out, n_blobs * PROOFS_BYTES)
        self._order(slot)
        _check(lib().kzgmi_recover_cells_and_proofs_device_async(self.handle, h, int(slot), pi, int(k), pc,
                                                                 int(n_blobs), po, pp))

    def fk20_scalars(self, blobs, n: int, out=None):
        """Diagnostic: the Fr stage of the proof pipeline for n device-resident blobs: DFT(a^(b))[pos]
        as 32 B big-endian at 32 ((128 blob + pos) 64 + b) of a device tensor of n x 256 KiB."""
        import torch
        if out is None:
            out = torch.empty(n * EXT_BLOB_BYTES, dtype=torch.uint8, device=blobs.device)
        pb, po = _dptr(blobs, n * BLOB_BYTES), _dptr(out, n * EXT_BLOB_BYTES)
        self._order(0)
        _check(lib().kzgmi_fk20_scalars_device(self.handle, pb, int(n), po))
        return out

    def g1_fft128(self, points, count: int, inverse: bool = False, out=None):
        """Diagnostic: `count` independent size-128 DFTs over G1 of device-resident uncompressed points
        (96 B each), natural order in and out, root w^64 (inverse: its inverse and 1 / 128)."""
        import torch
        if out is None:
            out = torch.empty(count * 128 * 96, dtype=torch.uint8, device=points.device)
        pi, po = _dptr(points, count * 128 * 96), _dptr(out, count * 128 * 96)
        self._order(0)
        _check(lib().kzgmi_g1_fft128_device(self.handle, pi, int(count), 1 if inverse else 0, po))
        return out

    def wait(self, slot: int) -> bool:
        ok = ctypes.c_int(-1)
        try:
            _check(lib().kzgmi_slot_wait(self.handle, int(slot), ctypes.byref(ok)))
        finally:
            getattr(self, "_host_keep", {}).pop(slot, None)
        return bool(ok.value)

    def last_combination(self, curve: str):
        g1b = 2 * FP_BYTES[curve]
        a = ctypes.create_string_buffer(g1b)
        b = ctypes.create_string_buffer(g1b)
        _check(lib().kzgmi_last_combination(self.handle, a, b))
        return a.raw, b.raw

    # ------------------------------------------------------------------ MSM
    def msm_g1(self, curve: str, points, scalars, n: Optional[int] = None) -> bytes:
        g1b = 2 * FP_BYTES[curve]
        out = ctypes.create_string_buffer(g1b)
        if _is_device_tensor(points):
            if n is None:
                n = points.numel() // g1b
            pp, ps = _dptr(points, n * g1b), _dptr(scalars, 32 * n)
            self._order(0)
            _check(lib().kzgmi_msm_g1_device(self.handle, CURVES[curve], pp, ps, n, out))
        else:
            (pp, lp, kp), (ps, ls, ks) = _host_ptr(points), _host_ptr(scalars)
            if n is None:
                n = lp // g1b
            if lp < n * g1b or ls < 32 * n:
                raise ValueError("input buffers shorter than n points")
            _check(lib().kzgmi_msm_g1(self.handle, CURVES[curve], pp, ps, n, out))
            del kp, ks
        return out.raw

    def msm_g1_async(self, curve: str, slot: int, points, scalars, n: int):
        """Enqueue sum k_i P_i (device tensors) on workspace `slot`; msm_wait(slot) returns it."""
        self._msm_curve = getattr(self, "_msm_curve", {})
        self._msm_curve[slot] = curve
        pp, ps = _dptr(points, n * 2 * FP_BYTES[curve]), _dptr(scalars, 32 * n)
        self._order(slot)
        _check(lib().kzgmi_msm_g1_device_async(self.handle, CURVES[curve], int(slot), pp, ps, int(n)))

    def msm_wait(self, slot: int) -> bytes:
        g1b = 2 * FP_BYTES[self._msm_curve[slot]]
        out = ctypes.create_string_buffer(g1b)
        _check(lib().kzgmi_msm_wait(self.handle, int(slot), out))
        return out.raw

    # ------------------------------------------------------------------ multi-GPU pieces
    def tensor_device(self):
        import torch
        return torch.device("cuda", self.device)

    def partial_bytes(self, curve: str) -> int:
        return int(lib().kzgmi_partial_bytes(CURVES[curve]))

    def _batch_ptrs(self, curve, commitments, zs, ys, proofs, n, compressed=False):
        g1b = (1 if compressed else 2) * FP_BYTES[curve]
        return (_dptr(commitments, n * g1b), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, n * g1b))

    def batch_partial(self, srs: Srs, commitments, zs, ys, proofs, n: int, index_offset: int, seed: bytes, out):
        ptrs = self._batch_ptrs(srs.curve, commitments, zs, ys, proofs, n)
        po = _dptr(out, 2 * self.partial_bytes(srs.curve))
        sd = _challenge_seed(seed, None)
        self._order(0)
        _check(lib().kzgmi_batch_partial_device(self.handle, srs.handle, *ptrs, n, int(index_offset), sd, po))

    def batch_combine(self, srs: Srs, partials, n_parts: int) -> bool:
        ok = ctypes.c_int(-1)
        p = _dptr(partials, 2 * n_parts * self.partial_bytes(srs.curve))
        self._order(0)
        _check(lib().kzgmi_batch_combine_device(self.handle, srs.handle, p, int(n_parts), ctypes.byref(ok)))
        return bool(ok.value)

    def partial_encode(self, curve: str, records, count: int) -> list:
        """G1 encodings of `count` device-resident partial records (e.g. a shard's [A_k, B_k])."""
        g1b = 2 * FP_BYTES[curve]
        p = _dptr(records, count * self.partial_bytes(curve))
        out = ctypes.create_string_buffer(count * g1b)
        self._order(0)
        _check(lib().kzgmi_partial_encode_device(self.handle, CURVES[curve], p, int(count), out))
        return [out.raw[i * g1b:(i + 1) * g1b] for i in range(count)]

    # ------------------------------------------------------------------ locating invalid tuples
    def batch_check_partials(self, srs: Srs, partials, n_groups: int) -> list:
        """The verdict of each of n_groups device-resident record pairs (A_g, B_g): a sharded caller
        names its failing shard with it.  A marked record raises its own error."""
        p = _dptr(partials, 2 * n_groups * self.partial_bytes(srs.curve))
        out = ctypes.create_string_buffer(max(1, n_groups))
        self._order(0)
        _check(lib().kzgmi_batch_check_partials_device(self.handle, srs.handle, p, int(n_groups), out))
        return [b != 0 for b in out.raw[:n_groups]]

    def batch_range_partials(self, srs: Srs, commitments, zs, ys, proofs, n: int, index_offset: int, seed, ranges,
                             out, compressed: bool = False, subgroup_check: bool = False, trusted_g1: bool = False):
        """(A_g, B_g) of the index ranges [(lo, hi), ...] of a device-resident batch whose first tuple
        has global index index_offset: 2 partial records per range into the device tensor `out`."""
        flags = _flags(compressed, subgroup_check, trusted_g1=trusted_g1)
        ptrs = self._batch_ptrs(srs.curve, commitments, zs, ys, proofs, n, compressed)
        flat = [int(v) for r in ranges for v in r]
        arr = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        po = _dptr(out, 2 * len(ranges) * self.partial_bytes(srs.curve))
        self._order(0)
        _check(lib().kzgmi_batch_range_partials_device(self.handle, srs.handle, *ptrs, int(n), int(index_offset),
                                                       _challenge_seed(seed, None), flags, arr, len(ranges), po))

    @staticmethod
    def _find_outputs(max_bad: int):
        # (a max_bad outside 1 .. 4096 is the library's to refuse: it writes nothing then)
        return (ctypes.c_uint64 * max(1, min(int(max_bad), 4096)))(), ctypes.c_size_t(0), ctypes.c_int(0)

    def batch_find_invalid(self, srs: Srs, commitments, zs, ys, proofs, seed: Optional[bytes] = None,
                           n: Optional[int] = None, max_bad: int = 64, compressed: bool = False,
                           subgroup_check: bool = False, trusted_g1: bool = False, flags: Optional[int] = None):
        """The invalid tuples of a batch, found on the GPU by group testing over index ranges:
        -> (the lowest min(max_bad, #invalid) invalid indices ascending, more) with more True iff a
        further invalid tuple exists.  Host buffers or device tensors, as batch_verify takes them.
        The search uses counter-mode randomisers (seed, or the OS CSPRNG), whatever mode rejected
        the batch.  flags: raw KZGMI_FLAG_* bits instead of the keywords."""
        if flags is None:
            flags = _flags(compressed, subgroup_check, trusted_g1=trusted_g1)
        g1b = (1 if flags & FLAG_COMPRESSED else 2) * FP_BYTES[srs.curve]
        bad, nb, more = self._find_outputs(max_bad)
        sd = _challenge_seed(seed, None)
        if _is_device_tensor(commitments):
            if n is None:
                n = commitments.numel() // g1b
            ptrs = (_dptr(commitments, n * g1b), _dptr(zs, 32 * n), _dptr(ys, 32 * n), _dptr(proofs, n * g1b))
            self._order(0)
            _check(lib().kzgmi_batch_find_invalid_device(self.handle, srs.handle, *ptrs, int(n), sd, flags, bad,
                                                         max_bad, ctypes.byref(nb), ctypes.byref(more)))
        else:
            ptrs, keep = self._host_inputs(commitments, zs, ys, proofs, n, g1b)
            _check(lib().kzgmi_batch_find_invalid(self.handle, srs.handle, *ptrs[:4], int(ptrs[-1]), sd, flags, bad,
                                                  max_bad, ctypes.byref(nb), ctypes.byref(more)))
            del keep
        return list(bad[:nb.value]), bool(more.value)

    def blob_batch_find_invalid(self, srs: Srs, blobs, commitments, proofs, n: Optional[int] = None,
                                max_bad: int = 64):
        """The blobs verify_blob_batch rejects a batch for: -> (indices ascending, more).  Host buffers
        or device tensors, as verify_blob_batch takes them."""
        bad, nb, more = self._find_outputs(max_bad)
        if _is_device_tensor(blobs):
            if n is None:
                n = commitments.numel() // 48
            ptrs = (_dptr(blobs, n * BLOB_BYTES), _dptr(commitments, 48 * n), _dptr(proofs, 48 * n))
            self._order(0)
            _check(lib().kzgmi_verify_blob_batch_find_invalid_device(self.handle, srs.handle, *ptrs, int(n), bad,
                                                                     max_bad, ctypes.byref(nb), ctypes.byref(more)))
        else:
            (pb, lb, kb), (pc, lc, kc), (pp, lp, kp) = (_host_ptr(v) for v in (blobs, commitments, proofs))
            if n is None:
                n = lc // 48
            if lb < n * BLOB_BYTES or lc < 48 * n or lp < 48 * n:
                raise ValueError("input buffers shorter than n blobs")
            _check(lib().kzgmi_verify_blob_batch_find_invalid(self.handle, srs.handle, pb, pc, pp, int(n), bad, max_bad,
                                                              ctypes.byref(nb), ctypes.byref(more)))
            del kb, kc, kp
        return list(bad[:nb.value]), bool(more.value)

    def cell_coeffs(self, cell_indices, cells, n: int, out=None):
        """The 64 coefficients of every cell's own interpolation polynomial I_k, for device-resident
        uint64 cell indices and cells: a device tensor of n x 64 x 32 B big-endian (diagnostic)."""
        import torch
        if out is None:
            out = torch.empty(max(16, CELL_BYTES * n), dtype=torch.uint8, device=cells.device)[:CELL_BYTES * n]
        pi, pc, po = _dptr(cell_indices, 8 * n), _dptr(cells, CELL_BYTES * n), _dptr(out, CELL_BYTES * n)
        self._order(0)
        _check(lib().kzgmi_cell_coeffs_device(self.handle, pi, pc, int(n), po))
        return out

    def cell_range_partials(self, srs: CellSrs, commitments, commitment_indices, cell_indices, cells, proofs, m: int,
                            n: int, index_offset: int, seed, ranges, out):
        """(A_g, B_g) of the index ranges [(lo, hi), ...] of a device-resident cell batch whose first
        cell has global index index_offset: 2 partial records per range into the device tensor `out`."""
        h = self._cell_srs_handle(srs)
        ptrs = (_dptr(commitments, 48 * m), int(m), _dptr(commitment_indices, 8 * n), _dptr(cell_indices, 8 * n),
                _dptr(cells, CELL_BYTES * n), _dptr(proofs, 48 * n))
        flat = [int(v) for r in ranges for v in r]
        arr = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        po = _dptr(out, 2 * len(ranges) * self.partial_bytes("bls12_381"))
        self._order(0)
        _check(lib().kzgmi_cell_range_partials_device(self.handle, h, *ptrs, int(n), int(index_offset),
                                                      _challenge_seed(seed, None), arr, len(ranges), po))

    def cell_batch_find_invalid(self, srs: CellSrs, commitments, commitment_indices, cell_indices, cells, proofs,
                                m: Optional[int] = None, n: Optional[int] = None, seed: Optional[bytes] = None,
                                max_bad: int = 64):
        """The cells verify_cell_batch rejects a batch for, found on the GPU by group testing over
        index ranges: -> (the lowest min(max_bad, #invalid) invalid indices ascending, more).  Host
        buffers or device tensors, as verify_cell_batch takes them; at most 65536 cells per call.
        seed: the 32-byte seed of the counter-mode randomisers (None: the OS CSPRNG)."""
        bad, nb, more = self._find_outputs(max_bad)
        h = self._cell_srs_handle(srs)
        sd = _challenge_seed(seed, None)
        if _is_device_tensor(cells):
            if n is None:
                n = proofs.numel() // 48
            if m is None:
                m = commitments.numel() // 48
            ptrs = (_dptr(commitments, 48 * m), int(m), _dptr(commitment_indices, 8 * n), _dptr(cell_indices, 8 * n),
                    _dptr(cells, CELL_BYTES * n), _dptr(proofs, 48 * n))
            self._order(0)
            _check(lib().kzgmi_verify_cell_batch_find_invalid_device(self.handle, h, *ptrs, int(n), sd, bad, max_bad,
                                                                     ctypes.byref(nb), ctypes.byref(more)))
        else:
            ci, ce = _u64_bytes(commitment_indices), _u64_bytes(cell_indices)
            (pc, lc, kc), (pi, li, ki), (pe, le, ke), (pl, ll, kl), (pp, lp, kp) = (
                _host_ptr(v) for v in (commitments, ci, ce, cells, proofs))
            if n is None:
                n = lp // 48
            if m is None:
                m = lc // 48
            if lc < 48 * m or li < 8 * n or le < 8 * n or ll < CELL_BYTES * n or lp < 48 * n:
                raise ValueError("input buffers shorter than n cells")
            _check(lib().kzgmi_verify_cell_batch_find_invalid(self.handle, h, pc, int(m), pi, pe, pl, pp, int(n), sd, bad,
                                                              max_bad, ctypes.byref(nb), ctypes.byref(more)))
            del kc, ki, ke, kl, kp
        return list(bad[:nb.value]), bool(more.value)

    def find_invalid_stats(self) -> dict:
        """Of the last search on this context: levels, bucket_jobs, wave_terms (grouped kernel), pairings."""
        out = (ctypes.c_uint64 * 4)()
        _check(lib().kzgmi_find_invalid_stats(self.handle, out))
        return dict(zip(("levels", "bucket_jobs", "wave_terms", "pairings"), list(out)))

    def batch_partial_async(self, srs: Srs, slot: int, commitments, zs, ys, proofs, n: int, index_offset: int,
                            seed, out, compressed: bool = False, subgroup_check: bool = False, challenge=None,
                            trusted_g1: bool = False):
        """Enqueue this shard's partial (A_k, B_k) on `slot`; complete with wait(slot).
        challenge: r_i = r^(index_offset + i) (pass seed=None)."""
        ptrs = self._batch_ptrs(srs.curve, commitments, zs, ys, proofs, n, compressed)
        po = _dptr(out, 2 * self.partial_bytes(srs.curve))
        sd = _challenge_seed(seed, challenge)
        self._order(slot)
        _check(lib().kzgmi_batch_partial_device_async(self.handle, srs.handle, int(slot), *ptrs, n, int(index_offset),
                                                      sd, _flags(compressed, subgroup_check, False, challenge,
                                                                 trusted_g1), po))

    def batch_combine_async(self, srs: Srs, slot: int, partials, n_parts: int):
        """Enqueue sum-of-partials + pairing check on `slot`; wait(slot) returns the verdict."""
        p = _dptr(partials, 2 * n_parts * self.partial_bytes(srs.curve))
        self._order(slot)
        _check(lib().kzgmi_batch_combine_device_async(self.handle, srs.handle, int(slot), p, int(n_parts)))

    def msm_partial(self, curve: str, points, scalars, n: int, out):
        pp, ps = _dptr(points, n * 2 * FP_BYTES[curve]), _dptr(scalars, 32 * n)
        po = _dptr(out, self.partial_bytes(curve))
        self._order(0)
        _check(lib().kzgmi_msm_partial_device(self.handle, CURVES[curve], pp, ps, n, po))

    def msm_partial_async(self, curve: str, slot: int, points, scalars, n: int, out):
        pp, ps = _dptr(points, n * 2 * FP_BYTES[curve]), _dptr(scalars, 32 * n)
        po = _dptr(out, self.partial_bytes(curve))
        self._order(slot)
        _check(lib().kzgmi_msm_partial_device_async(self.handle, CURVES[curve], int(slot), pp, ps, int(n), po))

    def msm_combine_async(self, curve: str, slot: int, partials, n_parts: int):
        self._msm_curve = getattr(self, "_msm_curve", {})
        self._msm_curve[slot] = curve
        p = _dptr(partials, n_parts * self.partial_bytes(curve))
        self._order(slot)
        _check(lib().kzgmi_msm_combine_device_async(self.handle, CURVES[curve], int(slot), p, int(n_parts)))

    def msm_combine(self, curve: str, partials, n_parts: int) -> bytes:
        out = ctypes.create_string_buffer(2 * FP_BYTES[curve])
        p = _dptr(partials, n_parts * self.partial_bytes(curve))
        self._order(0)
        _check(lib().kzgmi_msm_combine_device(self.handle, CURVES[curve], p, int(n_parts), out))
        return out.raw

    # ------------------------------------------------------------------ utilities
    def pairing(self, curve: str, g1: bytes, g2: bytes) -> bytes:
        out = ctypes.create_string_buffer(12 * FP_BYTES[curve])
        _check(lib().kzgmi_pairing(self.handle, CURVES[curve], bytes(g1), bytes(g2), out))
        return out.raw

    def gen_g1(self, curve: str, scalars_dev, n: int, out_dev):
        ps, po = _dptr(scalars_dev, 32 * n), _dptr(out_dev, n * 2 * FP_BYTES[curve])
        self._order(0)
        _check(lib().kzgmi_gen_g1(self.handle, CURVES[curve], ps, n, po))

    def gen_tuples(self, curve: str, tau: int, seed: bytes, n: int, C, z, y, pi):
        ptrs = self._batch_ptrs(curve, C, z, y, pi, n)
        sd = _challenge_seed(seed, None)
        self._order(0)
        _check(lib().kzgmi_gen_tuples(self.handle, CURVES[curve], int(tau).to_bytes(32, "big"), sd, n, *ptrs))

    def g2_mul(self, curve: str, g2: bytes, k: int) -> bytes:
        out = ctypes.create_string_buffer(4 * FP_BYTES[curve])
        _check(lib().kzgmi_g2_mul(self.handle, CURVES[curve], bytes(g2), int(k).to_bytes(32, "big"), out))
        return out.raw

    def toy_srs(self, curve: str, tau: int):
        """(G2 generator, [tau]_2) encodings computed on the GPU (test/bench SRS)."""
        g2 = G2_GENERATOR[curve]
        return g2, self.g2_mul(curve, g2, tau)

    def probe_fpmul(self, curve: str) -> float:
        v = ctypes.c_double()
        _check(lib().kzgmi_probe_fpmul(self.handle, CURVES[curve], ctypes.byref(v)))
        return v.value

    def set_glv(self, msm: bool = True, batch: bool = True):
        """GLV split of full Fr scalars for MSMs / batch verification."""
        _check(lib().kzgmi_set_glv(self.handle, int(bool(msm)), int(bool(batch))))

    def set_trusted_g1(self, on: bool = True):
        """MSM inputs on this context are known G1 members (BLS12-381 MSMs may then use GLV)."""
        _check(lib().kzgmi_set_trusted_g1(self.handle, int(bool(on))))

    def set_split_acc(self, mode: int = -1):
        """Split accumulation of a batch's two MSMs: -1 auto (large synchronous calls), 0 never, 1 always."""
        _check(lib().kzgmi_set_split_acc(self.handle, int(mode)))

    def set_profiling(self, on: bool):
        _check(lib().kzgmi_set_profiling(self.handle, 1 if on else 0))

    def phase_ms(self) -> dict:
        arr = (ctypes.c_double * len(PHASES))()
        lib().kzgmi_get_phase_ms(self.handle, arr, len(PHASES))
        return dict(zip(PHASES, list(arr)))


# ---------------------------------------------------------------------- north-star API
# Standard G2 generators (ZCash / EIP-197 encodings, imaginary part first)
G2_GENERATOR = {
    "bls12_381": bytes.fromhex(
        "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
        "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
        "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be"
        "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"),
    "bn254": b"".join(v.to_bytes(32, "big") for v in (
        11559732032986387107991004021392285783925812861821192530917403151452391805634,
        10857046999023057135944570762232829481370756359578518086990519993285655852781,
        4082367875863433681332203403145435568316851327593401208105741076214120093531,
        8495653923123431417604973247489272438418190587263600148770280649306958101930)),
}

_default_ctx: Optional[Context] = None


def alloc_count() -> int:
    """Process-wide number of device workspace allocations made by the library so far."""
    return int(lib().kzgmi_alloc_count())


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0, 1)
    return _default_ctx


def load_srs(curve: str, g2: bytes, tau_g2: bytes, ctx: Optional[Context] = None, g1: Optional[bytes] = None) -> Srs:
    return (ctx or default_context()).load_srs(curve, g2, tau_g2, g1=g1)


def batch_verify(commitments, zs, ys, proofs, srs: Srs, seed: Optional[bytes] = None, compressed: bool = False,
                 subgroup_check: bool = False, fiat_shamir: bool = False, challenge=None,
                 trusted_g1: bool = False) -> bool:
    """BASELINE.json:5 batch_verify(commitments, zs, ys, proofs, srs) on the GPU."""
    return srs.ctx.batch_verify(srs, commitments, zs, ys, proofs, seed=seed, compressed=compressed,
                                subgroup_check=subgroup_check, fiat_shamir=fiat_shamir, challenge=challenge,
                                trusted_g1=trusted_g1)


def verify_blob_batch(blobs, commitments, proofs, srs: Srs, n: Optional[int] = None) -> bool:
    """EIP-4844 verify_blob_kzg_proof_batch(blobs, commitments, proofs) on the GPU (BLS12-381)."""
    return srs.ctx.verify_blob_batch(srs, blobs, commitments, proofs, n=n)


def batch_find_invalid(commitments, zs, ys, proofs, srs: Srs, seed: Optional[bytes] = None, max_bad: int = 64,
                       compressed: bool = False, subgroup_check: bool = False, trusted_g1: bool = False):
    """The invalid tuples of a rejected batch, found on the GPU: -> (indices ascending, more)."""
    return srs.ctx.batch_find_invalid(srs, commitments, zs, ys, proofs, seed=seed, max_bad=max_bad,
                                      compressed=compressed, subgroup_check=subgroup_check, trusted_g1=trusted_g1)


def blob_batch_find_invalid(blobs, commitments, proofs, srs: Srs, n: Optional[int] = None, max_bad: int = 64):
    """The blobs a rejected EIP-4844 blob batch is rejected for: -> (indices ascending, more)."""
    return srs.ctx.blob_batch_find_invalid(srs, blobs, commitments, proofs, n=n, max_bad=max_bad)


def _dedup_cell_batch(commitments_bytes, cell_indices, cells, proofs_bytes, srs):
    """The specification's per-cell lists in the deduplicated form Context.verify_cell_batch takes:
    (unique commitments, commitment indices, cell indices, cells, proofs, m, n); the commitments
    are deduplicated in order of first appearance."""
    n = len(cells)
    if not (len(commitments_bytes) == len(cell_indices) == len(proofs_bytes) == n):
        raise ValueError("commitments, cell indices, cells and proofs must have the same length")
    index, unique, cidx = {}, [], []
    for cm in commitments_bytes:
        cm = bytes(cm)
        if cm not in index:
            index[cm] = len(unique)
            unique.append(cm)
        cidx.append(index[cm])
    if not isinstance(srs, CellSrs):
        raise KzgmiError(-1, "not a cell SRS (Context.load_cell_srs)")
    return (b"".join(unique), cidx, list(cell_indices), b"".join(bytes(x) for x in cells),
            b"".join(bytes(p) for p in proofs_bytes), len(unique), n)


def verify_cell_batch(commitments_bytes, cell_indices, cells, proofs_bytes, srs: CellSrs, r=None) -> bool:
    """EIP-7594 verify_cell_kzg_proof_batch(commitments_bytes, cell_indices, cells, proofs_bytes) on
    the GPU (BLS12-381): lists of 48-byte commitments (one per cell, repeats allowed), cell
    indices, 2048-byte cells and 48-byte proofs.  Commitments are deduplicated here, in order of
    first appearance."""
    *args, m, n = _dedup_cell_batch(commitments_bytes, cell_indices, cells, proofs_bytes, srs)
    return srs.ctx.verify_cell_batch(srs, *args, m=m, n=n, r=r)


def cell_batch_find_invalid(commitments_bytes, cell_indices, cells, proofs_bytes, srs: CellSrs,
                            seed: Optional[bytes] = None, max_bad: int = 64):
    """The cells verify_cell_batch (same arguments) rejects a batch for: -> (indices ascending, more)."""
    *args, m, n = _dedup_cell_batch(commitments_bytes, cell_indices, cells, proofs_bytes, srs)
    return srs.ctx.cell_batch_find_invalid(srs, *args, m=m, n=n, seed=seed, max_bad=max_bad)


def compute_cells(blobs, n: Optional[int] = None, ctx: Optional[Context] = None):
    """EIP-7594 compute_cells on the GPU: the 128 cells of every blob (Context.compute_cells)."""
    return (ctx or default_context()).compute_cells(blobs, n)


def recover_cells(cell_indices, cells, n_blobs: Optional[int] = None, ctx: Optional[Context] = None):
    """The cells of EIP-7594 recover_cells_and_kzg_proofs on the GPU for blobs that share their cell
    indices (Context.recover_cells)."""
    return (ctx or default_context()).recover_cells(cell_indices, cells, n_blobs)


def blob_commit(pk: BlobProofKey, blobs, n: Optional[int] = None):
    """Context.blob_commit on the key's context."""
    return pk.ctx.blob_commit(pk, blobs, n)


def compute_kzg_proofs(pk: BlobProofKey, blobs, zs, n: Optional[int] = None):
    """Context.compute_kzg_proofs on the key's context."""
    return pk.ctx.compute_kzg_proofs(pk, blobs, zs, n)


def compute_blob_proofs(pk: BlobProofKey, blobs, commitments, n: Optional[int] = None):
    """Context.compute_blob_proofs on the key's context."""
    return pk.ctx.compute_blob_proofs(pk, blobs, commitments, n)


def compute_cells_and_proofs(pk: CellProofKey, blobs, n: Optional[int] = None, cells=True):
    """Context.compute_cells_and_proofs on the key's context."""
    return pk.ctx.compute_cells_and_proofs(pk, blobs, n, cells)


def recover_cells_and_proofs(pk: CellProofKey, cell_indices, cells, n_blobs: Optional[int] = None):
    """Context.recover_cells_and_proofs on the key's context."""
    return pk.ctx.recover_cells_and_proofs(pk, cell_indices, cells, n_blobs)


def fr_ntt(curve: str, values, logn: Optional[int] = None, count: int = 1, inverse: bool = False, bitrev: bool = False,
           shift=None, out=None, ctx: Optional[Context] = None):
    """Power-of-two transforms over Fr on the GPU (Context.fr_ntt)."""
    return (ctx or default_context()).fr_ntt(curve, values, logn, count, inverse, bitrev, shift, out)


def open_evals(ck: CommitKey, evals, zs, logn: Optional[int] = None, k: Optional[int] = None, bitrev: bool = False):
    """Context.open_evals on the key's context."""
    return ck.ctx.open_evals(ck, evals, zs, logn, k, bitrev)


def g1_ntt(curve: str, points, logn: Optional[int] = None, count: int = 1, inverse: bool = False, bitrev: bool = False,
           out=None, ctx: Optional[Context] = None):
    """Power-of-two transforms over G1 on the GPU (Context.g1_ntt)."""
    return (ctx or default_context()).g1_ntt(curve, points, logn, count, inverse, bitrev, out)


def open_all(key: OpenAllKey, coeffs, m: Optional[int] = None, bitrev: bool = False, want_ys: bool = True):
    """Context.open_all on the key's context."""
    return key.ctx.open_all(key, coeffs, m, bitrev, want_ys)


def open_cosets(key: OpenCosetsKey, coeffs, logk: int, m: Optional[int] = None, count: int = 1, bitrev: bool = False,
                want_ys: bool = True):
    """Context.open_cosets on the key's context."""
    return key.ctx.open_cosets(key, coeffs, logk, m, count, bitrev, want_ys)


def msm_g1(curve: str, points, scalars, ctx: Optional[Context] = None) -> bytes:
    return (ctx or default_context()).msm_g1(curve, points, scalars)


def tuple_scalars_host(seed: bytes, i: int, tag: str) -> int:
    """The 253-bit synthetic scalar kzgmi_gen_tuples derives (for host-side checks)."""
    import hashlib
    h = hashlib.sha256(bytes(seed) + int(i).to_bytes(8, "little") + tag.encode()).digest()
    return int.from_bytes(h, "big") & ((1 << 253) - 1)
