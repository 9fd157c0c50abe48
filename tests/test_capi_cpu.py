"""CPU-only checks of the drop-in boundary: libkzgmi.so loads, exports every symbol declared
in include/kzgmi.h, and fails loudly (KZGMI_ERR_DEVICE) without a GPU -- no CPU fallback."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    with open(os.path.join(ROOT, "include", "kzgmi.h")) as f:
        src = f.read()
    return sorted(set(re.findall(r"\b(kzgmi_[a-z0-9_]+)\s*\(", src)))


def test_header_matches_python_binding():
    import kzgmi
    assert header_symbols() == sorted(kzgmi.exported_symbols())


def test_library_exports_every_header_symbol():
    import kzgmi
    lib = kzgmi.lib()
    for s in header_symbols():
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.kzgmi_version()
    # the version string reports the header's ABI revision (it is built from KZGMI_ABI_VERSION)
    assert ("abi %d" % lib.kzgmi_abi_version()).encode() in lib.kzgmi_version()
    assert lib.kzgmi_abi_version() == kzgmi.ABI_VERSION


def test_library_contains_gfx950_code_object():
    import kzgmi
    with open(kzgmi.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob or b"gfx950" in blob


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import kzgmi
    with pytest.raises(kzgmi.KzgmiError) as e:
        kzgmi.Context(0)
    assert e.value.code == -5


# one entry point per host unit (csrc/api.hip, host_batch, host_msm, host_eip, host_multi; host_core
# defines none) and per feature family; each checks its context before anything else
NULL_CTX_CALLS = ["kzgmi_ctx_reserve", "kzgmi_batch_verify_device", "kzgmi_msm_g1_device",
                  "kzgmi_verify_blob_batch_device", "kzgmi_verify_cell_batch_device", "kzgmi_recover_cells_device",
                  "kzgmi_compute_cells_and_proofs_device", "kzgmi_batch_verify_multi_device",
                  "kzgmi_msm_g1_multi_device"]


@pytest.mark.parametrize("name", NULL_CTX_CALLS)
def test_null_context_error_is_shared_across_units(name):
    """The host units share one last-error string: a null context is refused with KZGMI_ERR_ARG by
    an entry point of every unit, and kzgmi_last_error(), which lives in api.hip, reports it.  A
    unit with a last-error string of its own would leave the earlier message standing."""
    import ctypes
    import kzgmi
    lib = kzgmi.lib()
    # an earlier, different message (set by api.hip itself)
    assert lib.kzgmi_host_alloc(0, None) == -1 and lib.kzgmi_last_error() == b"bad argument"
    f = getattr(lib, name)
    args = [None if issubclass(t, (ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer)) else 0 for t in f.argtypes]
    assert f(*args) == -1  # KZGMI_ERR_ARG
    assert lib.kzgmi_last_error() == b"null context"


def test_shard_range():
    from kzgmi.distributed import shard_range
    for n in [0, 1, 7, 1 << 20, (1 << 20) + 3]:
        for w in [1, 2, 3, 8]:
            parts = [shard_range(n, w, r) for r in range(w)]
            assert sum(c for _, c in parts) == n
            off = 0
            for o, c in parts:
                assert o == off
                off += c
            assert max(c for _, c in parts) - min(c for _, c in parts) <= 1
            aligned = [shard_range(n, w, r, align=4096) for r in range(w)]
            assert sum(c for _, c in aligned) == n
            assert all(o % 4096 == 0 or c == 0 for o, c in aligned)
            assert [o for o, c in aligned if c] == sorted(o for o, c in aligned if c)
