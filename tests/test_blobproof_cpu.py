"""CPU checks of the EIP-4844 producer model (tests/blobproofref.py) against the closed form that
tests/blobref.py's open_blob uses, and of the C ABI's new entry points."""
import random

import pytest

import blobproofref as P
import blobref as B

TAU = 0x4844_0000_1234_5678_9ABC_DEF1


@pytest.fixture(scope="module")
def model():
    rng = random.Random(0x4844_B10B)
    vals = [rng.randrange(B.R) for _ in range(B.N)]
    lag = P.lagrange_scalars(TAU)
    return {"vals": vals, "lag": lag, "ptau": B.evaluate(vals, TAU), "z": rng.randrange(B.R)}


def test_lagrange_scalars_sum_to_one(model):
    assert sum(model["lag"]) % B.R == 1
    # l_j(dom[i]) would be the unit vectors; at tau the commitment of e_j is l_j itself
    e = [0] * B.N
    e[77] = 1
    assert P.commit_scalar(e, model["lag"]) == model["lag"][77] == B.evaluate(e, TAU)


def test_commit_scalar_is_the_evaluation_at_tau(model):
    assert P.commit_scalar(model["vals"], model["lag"]) == model["ptau"]


def _points(model):
    return [("random", model["z"]), ("0", 0), ("r-1", B.R - 1), ("dom[0]", B.DOM[0]), ("dom[513]", B.DOM[513]),
            ("dom[4095]", B.DOM[4095])]


@pytest.mark.parametrize("which", range(6))
def test_proof_scalar_equals_the_closed_form(model, which):
    """sum_j q_j l_j == (p(tau) - y) / (tau - z): the right side shares no code with the quotient."""
    name, z = _points(model)[which]
    y, s = P.proof_scalar(model["vals"], z, model["lag"])
    assert y == B.evaluate(model["vals"], z), name
    assert s == (model["ptau"] - y) * pow((TAU - z) % B.R, -1, B.R) % B.R, name


def test_quotient_shapes(model):
    assert B.DOM[0] == 1 and B.DOM[1] == B.R - 1  # z = r - 1 is on the domain too
    y, q = P.quotient([5] * B.N, model["z"])
    assert y == 5 and q == [0] * B.N
    y, q = P.quotient([5] * B.N, B.DOM[513])
    assert y == 5 and q == [0] * B.N
    y, q = P.quotient(model["vals"], B.DOM[513])
    assert y == model["vals"][513] and q[513] != 0


def test_symbols_and_methods():
    import kzgmi
    new = ["kzgmi_blob_pk_load", "kzgmi_blob_pk_free", "kzgmi_blob_pk_device_bytes",
           "kzgmi_blob_commit", "kzgmi_blob_commit_device", "kzgmi_blob_commit_device_async",
           "kzgmi_compute_kzg_proofs", "kzgmi_compute_kzg_proofs_device", "kzgmi_compute_kzg_proofs_device_async",
           "kzgmi_compute_blob_proofs", "kzgmi_compute_blob_proofs_device", "kzgmi_compute_blob_proofs_device_async",
           "kzgmi_blob_quotient_device"]
    lib = kzgmi.lib()
    for s in new:
        assert s in kzgmi.exported_symbols(), s
        assert hasattr(lib, s), s
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzgmi.h")) as f:
        header = set(re.findall(r"\b(kzgmi_[a-z0-9_]+)\s*\(", f.read()))
    assert set(new) <= header and header == set(kzgmi.exported_symbols())
    assert kzgmi.ABI_VERSION == 6 and lib.kzgmi_abi_version() == 6
    for m in ("load_blob_proof_key", "blob_commit", "blob_commit_async", "compute_kzg_proofs",
              "compute_kzg_proofs_async", "compute_blob_proofs", "compute_blob_proofs_async", "blob_quotient"):
        assert callable(getattr(kzgmi.Context, m)), m
    assert callable(kzgmi.blob_commit) and callable(kzgmi.compute_kzg_proofs) and callable(kzgmi.compute_blob_proofs)
    assert kzgmi.BlobProofKey.__name__ == "BlobProofKey"
    assert lib.kzgmi_blob_pk_device_bytes(None) == 0
    # a null context is refused before anything else
    assert lib.kzgmi_blob_commit_device(None, None, None, 0, None) == -1
    assert lib.kzgmi_last_error() == b"null context"
