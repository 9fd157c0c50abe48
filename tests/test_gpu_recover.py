"""EIP-7594 compute_cells and recover_cells on the GPU (csrc/recover.hpp) vs the pure-Python
reference of tests/recoverref.py.  Everything is compared bit-exactly.

The transform sizes are fixed (4096 points, one workgroup per blob), so the shapes are small blob
counts; the index sets put the missing cells in the first half, the second half, every other cell,
one end and the other, and nowhere.
"""
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

import cellref as K  # noqa: E402
import recoverref as RR  # noqa: E402

TAU = 0x7594_0000_1234_5678_9ABC_DEF1
ERR_ARG, ERR_SCALAR = -1, -4
EXT = K.NUM_CELLS * K.CELL_BYTES   # bytes of one extended blob
BLOB = K.BLOB_N * 32


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=torch.uint8).cuda()[:len(b)]


def _u64(xs):
    return struct.pack("<%dQ" % len(xs), *xs)


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def data():
    """Three different random blobs and their reference cells (lists of 128 lists of 64 ints)."""
    rng = random.Random(0x7594_E)
    blobs = [[rng.randrange(K.R) for _ in range(K.BLOB_N)] for _ in range(3)]
    return {"blobs": blobs, "cells": [RR.compute_cells(b) for b in blobs]}


def _given(cells_of_blobs, idx):
    """The input of recover_cells: for every blob its cells idx, in that order."""
    return b"".join(K.cell_from_ints(cells[i]) for cells in cells_of_blobs for i in idx)


def _index_sets():
    rng = random.Random(0x1DC5)
    shuffled = rng.sample(range(128), 64)
    assert shuffled != sorted(shuffled)
    s65 = rng.sample(range(128), 65)
    return {"first-half": list(range(64)), "second-half": list(range(64, 128)), "even": list(range(0, 128, 2)),
            "shuffled-64": shuffled, "65": s65, "no-0": list(range(1, 128)), "no-127": list(range(127)),
            "all": list(range(128))}


# ------------------------------------------------------------------------------ compute_cells
def _special_blobs(kind, nb, data):
    if kind == "zero":
        return [[0] * K.BLOB_N] * nb
    if kind == "constant":
        return [[(0x1234567 << 200) + 5 + b] * K.BLOB_N for b in range(nb)]
    if kind == "top":
        return [[K.R - 1] * K.BLOB_N] * nb
    return data["blobs"][:nb]


_COMPUTE_REF = {}


def _compute_ref(blob):
    key = hash(tuple(blob))
    if key not in _COMPUTE_REF:
        _COMPUTE_REF[key] = RR.cells_to_bytes(RR.compute_cells(blob))
    return _COMPUTE_REF[key]


@pytest.mark.parametrize("kind", ["zero", "constant", "top", "random"])
@pytest.mark.parametrize("nb", [1, 3])
def test_compute(ctx, data, nb, kind):
    blobs = _special_blobs(kind, nb, data)
    raw = b"".join(RR.blob_to_bytes(b) for b in blobs)
    got = _host(ctx.compute_cells(_dev(raw), nb))
    assert len(got) == nb * EXT
    for b, blob in enumerate(blobs):
        ext = got[b * EXT:(b + 1) * EXT]
        assert ext[:BLOB] == raw[b * BLOB:(b + 1) * BLOB]  # cells 0..63 are the blob's bytes
        assert ext == _compute_ref(blob)
        if kind != "random":  # a constant polynomial: all 128 cells hold the constant
            assert ext == blob[0].to_bytes(32, "big") * (2 * K.BLOB_N)


def test_compute_element_out_of_range(ctx, data):
    import kzgmi
    nb = 2
    raw = b"".join(RR.blob_to_bytes(b) for b in data["blobs"][:nb])
    for pos in (0, nb * BLOB - 32):  # element 0 of blob 0, element 4095 of the last blob
        bad = bytearray(raw)
        bad[pos:pos + 32] = K.R.to_bytes(32, "big")
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.compute_cells(_dev(bytes(bad)), nb)
        assert e.value.code == ERR_SCALAR
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.compute_cells(bytes(bad), nb)
        assert e.value.code == ERR_SCALAR
    assert _host(ctx.compute_cells(_dev(raw), nb))[:EXT] == _compute_ref(data["blobs"][0])


# ------------------------------------------------------------------------------ recover_cells
@pytest.mark.parametrize("name", list(_index_sets()))
@pytest.mark.parametrize("nb", [1, 2])
def test_recover(ctx, data, nb, name):
    idx = _index_sets()[name]
    cells = data["cells"][:nb]
    want = b"".join(RR.cells_to_bytes(c) for c in cells)
    got = _host(ctx.recover_cells(_dev(_u64(idx)), _dev(_given(cells, idx)), nb))
    assert got == want
    if name == "first-half":  # recover from the blob itself is compute
        raw = b"".join(RR.blob_to_bytes(b) for b in data["blobs"][:nb])
        assert _given(cells, idx) == raw
        assert _host(ctx.compute_cells(_dev(raw), nb)) == got


def test_recover_argument_errors(ctx, data):
    import kzgmi
    cells = data["cells"][:1]
    cases = {"k=63": list(range(63)), "k=129": list(range(128)) + [0], "duplicate": list(range(63)) + [5],
             "index-128": list(range(63)) + [128], "index-2^40": list(range(64)) + [1 << 40]}
    for name, idx in cases.items():
        given = _given(cells, [i if i < 128 else 0 for i in idx])
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.recover_cells(_dev(_u64(idx)), _dev(given), 1)
        assert e.value.code == ERR_ARG, name
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.recover_cells(idx, given, 1)
        assert e.value.code == ERR_ARG, name
    # too many blobs, checked before anything is read
    with pytest.raises(kzgmi.KzgmiError) as e:
        kzgmi._check(kzgmi.lib().kzgmi_recover_cells_device(ctx.handle, 16, 64, 16, 4097, 16))
    assert e.value.code == ERR_ARG
    # nb = 0 succeeds and writes nothing
    assert ctx.recover_cells(list(range(64)), b"", 0) == b""
    assert ctx.compute_cells(b"", 0) == b""
    idx = list(range(64, 128))
    assert _host(ctx.recover_cells(_dev(_u64(idx)), _dev(_given(cells, idx)), 1)) == RR.cells_to_bytes(cells[0])


@pytest.mark.parametrize("k", [64, 65])
def test_recover_element_out_of_range(ctx, data, k):
    """An element equal to r is KZGMI_ERR_SCALAR, also where the zero that replaces it makes the
    other 64 cells disagree with the result (k = 65)."""
    import kzgmi
    idx = _index_sets()["65"][:k]
    cells = data["cells"][:2]
    for pos in (0, 2 * k * K.CELL_BYTES - 32):
        bad = bytearray(_given(cells, idx))
        bad[pos:pos + 32] = K.R.to_bytes(32, "big")
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.recover_cells(_dev(_u64(idx)), _dev(bytes(bad)), 2)
        assert e.value.code == ERR_SCALAR


def _altered(cells_of_blobs, idx, blob, place, elem):
    out = bytearray(_given(cells_of_blobs, idx))
    o = (blob * len(idx) + place) * K.CELL_BYTES + 32 * elem
    v = (int.from_bytes(out[o:o + 32], "big") + 1) % K.R
    out[o:o + 32] = v.to_bytes(32, "big")
    return bytes(out)


@pytest.mark.parametrize("blob", [0, 1])
def test_recover_inconsistent(ctx, data, blob):
    """One altered element (kept in range) among 65 cells: no polynomial of degree < 4096 fits."""
    import kzgmi
    idx = _index_sets()["65"]
    cells = data["cells"][:2]
    bad = _altered(cells, idx, blob, 17, 41)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.recover_cells(_dev(_u64(idx)), _dev(bad), 2)
    assert e.value.code == ERR_ARG
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.recover_cells(idx, bad, 2)
    assert e.value.code == ERR_ARG
    # the slot is usable afterwards
    good = _given(cells, idx)
    assert _host(ctx.recover_cells(_dev(_u64(idx)), _dev(good), 2)) == b"".join(RR.cells_to_bytes(c) for c in cells)


def test_recover_altered_with_64_cells_is_another_polynomial(ctx, data):
    idx = _index_sets()["65"][:64]
    cells = data["cells"][:2]
    bad = _altered(cells, idx, 1, 17, 41)
    got = _host(ctx.recover_cells(_dev(_u64(idx)), _dev(bad), 2))
    altered = [K.cell_to_ints(bad[(64 + p) * K.CELL_BYTES:(65 + p) * K.CELL_BYTES]) for p in range(64)]
    assert RR.consistent(idx, altered)
    assert got[:EXT] == RR.cells_to_bytes(cells[0])
    assert got[EXT:] == RR.cells_to_bytes(RR.recover_cells(idx, altered))
    assert got[EXT:] != RR.cells_to_bytes(cells[1])


# ------------------------------------------------------------------------------ plumbing
def test_host_forms_equal_device_forms(ctx, data):
    import kzgmi
    nb = 2
    cells = data["cells"][:nb]
    want = b"".join(RR.cells_to_bytes(c) for c in cells)
    raw = b"".join(RR.blob_to_bytes(b) for b in data["blobs"][:nb])
    assert ctx.compute_cells(raw) == want
    assert ctx.compute_cells(bytearray(raw), nb) == want
    idx = _index_sets()["shuffled-64"]
    given = _given(cells, idx)
    assert ctx.recover_cells(idx, given) == want
    assert ctx.recover_cells(_u64(idx), given, nb) == want
    assert _host(ctx.recover_cells(idx, _dev(given))) == want   # host indices with device cells
    import torch
    out = torch.zeros(nb * EXT, dtype=torch.uint8, device="cuda")
    assert ctx.recover_cells(_dev(_u64(idx)), _dev(given), nb, out=out) is out
    assert _host(out) == want


def test_second_call_allocates_nothing(ctx, data):
    import kzgmi
    cells = data["cells"][:2]
    idx = _index_sets()["even"]
    d_idx, d_in = _dev(_u64(idx)), _dev(_given(cells, idx))
    d_blobs = _dev(b"".join(RR.blob_to_bytes(b) for b in data["blobs"][:2]))
    ctx.recover_cells(d_idx, d_in, 2)
    ctx.compute_cells(d_blobs, 2)
    ctx.recover_cells(idx, _given(cells, idx), 2)
    before = kzgmi.alloc_count()
    ctx.recover_cells(d_idx, d_in, 2)
    ctx.compute_cells(d_blobs, 2)
    ctx.recover_cells(idx, _given(cells, idx), 2)
    assert kzgmi.alloc_count() == before


@pytest.fixture(scope="module")
def opened():
    """One polynomial of degree 4095 under the toy tau: its cells, its commitment, and three opened
    cells (with proofs) that recovery below has to rebuild."""
    rng = random.Random(0xE2E)
    coeffs = [rng.randrange(K.R) for _ in range(K.BLOB_N)]
    cells = RR.coeffs_to_cells(coeffs)
    have = rng.sample(range(128), 64)
    missing = [i for i in range(128) if i not in have]
    check = [missing[0], missing[31], missing[63]]
    proofs = []
    for i in check:
        cell, proof = K.open_cell(coeffs, i, TAU)
        assert K.cell_to_ints(cell) == cells[i]
        proofs.append(proof)
    return {"cells": cells, "C": K.commit(coeffs, TAU), "have": have, "check": check, "proofs": proofs}


def test_recovered_cells_verify(ctx, opened):
    srs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
    have, check = opened["have"], opened["check"]
    got = ctx.recover_cells(_dev(_u64(have)), _dev(_given([opened["cells"]], have)), 1)
    assert _host(got) == RR.cells_to_bytes(opened["cells"])
    import torch
    rec = torch.cat([got[i * K.CELL_BYTES:(i + 1) * K.CELL_BYTES] for i in check])
    args = (_dev(opened["C"]), _dev(_u64([0, 0, 0])), _dev(_u64(check)), rec, _dev(b"".join(opened["proofs"])))
    assert ctx.verify_cell_batch(srs, *args, m=1, n=3) is True
    wrong = [check[1], check[0], check[2]]
    assert ctx.verify_cell_batch(srs, args[0], args[1], _dev(_u64(wrong)), rec, args[4], m=1, n=3) is False


def test_async_forms_beside_a_verification(ctx, data, opened):
    """recover and compute on slot 1 while a cell verification runs on slot 0; a failed job leaves
    its slot usable."""
    import kzgmi
    import torch
    srs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
    check = opened["check"]
    vcells = _dev(b"".join(K.cell_from_ints(opened["cells"][i]) for i in check))
    vargs = (_dev(opened["C"]), _dev(_u64([0, 0, 0])), _dev(_u64(check)), vcells, _dev(b"".join(opened["proofs"])))
    cells = data["cells"][:2]
    want = b"".join(RR.cells_to_bytes(c) for c in cells)
    idx = _index_sets()["65"]
    d_idx, d_in = _dev(_u64(idx)), _dev(_given(cells, idx))
    sync = _host(ctx.recover_cells(d_idx, d_in, 2))
    out = torch.zeros(2 * EXT, dtype=torch.uint8, device="cuda")
    ctx.verify_cell_batch_async(srs, 0, *vargs, 1, 3)
    ctx.recover_cells_async(1, d_idx, d_in, 2, out)
    assert ctx.wait(1) is True
    assert ctx.wait(0) is True
    assert _host(out) == sync == want
    # a failing job on slot 1 (reported by the wait), then a good one on the same slot
    d_bad = _dev(_altered(cells, idx, 0, 3, 0))
    ctx.verify_cell_batch_async(srs, 0, *vargs, 1, 3)
    ctx.recover_cells_async(1, d_idx, d_bad, 2, out)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.wait(1)
    assert e.value.code == ERR_ARG
    assert ctx.wait(0) is True
    out2 = torch.zeros(2 * EXT, dtype=torch.uint8, device="cuda")
    d_blobs = _dev(b"".join(RR.blob_to_bytes(b) for b in data["blobs"][:2]))
    ctx.compute_cells_async(1, d_blobs, 2, out2)
    assert ctx.wait(1) is True
    assert _host(out2) == want
    # a busy slot refuses a second job
    ctx.compute_cells_async(1, d_blobs, 2, out2)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.recover_cells_async(1, d_idx, d_in, 2, out)
    assert e.value.code == ERR_ARG
    assert ctx.wait(1) is True
