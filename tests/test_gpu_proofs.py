"""EIP-7594 cell proof generation on the GPU (csrc/fk20.hpp) vs the quotient definition of
tests/cellref.py (open_cell) and the stage-by-stage reference of tests/fk20ref.py.  Everything is
compared as exact bytes.

The shapes are fixed by the protocol (4096-element blobs, 128 proofs each), so the shapes are small
blob counts.
"""
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

import cellref as K  # noqa: E402
import fk20ref as F  # noqa: E402
import recoverref as RR  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

TAU = 0x7594_0000_1234_5678_9ABC_DEF1
ERR_ARG, ERR_NOT_ON_CURVE, ERR_SCALAR, ERR_NOT_IN_SUBGROUP = -1, -3, -4, -7
EXT = K.NUM_CELLS * K.CELL_BYTES
BLOB = K.BLOB_N * 32
PROOFS = K.NUM_CELLS * 48
INF48 = b"\xc0" + bytes(47)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=torch.uint8).cuda()[:len(b)]


def _u64(xs):
    return struct.pack("<%dQ" % len(xs), *xs)


def _host(t):
    return t.cpu().numpy().tobytes()


def _be(xs):
    return b"".join((x % K.R).to_bytes(32, "big") for x in xs)


def _g1(xs):
    """[x]_1 for every x: 96-byte encodings, one oracle call."""
    return O.g1_mul_gen(K.CURVE, _be(xs), len(xs))


def _g1c(xs):
    return O.g1_compress(K.CURVE, _g1(xs), len(xs))


def toy_srs(tau):
    return _g1(F.srs_scalars(tau))


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    return ctx.load_cell_proof_key(toy_srs(TAU))


_EXPECT = {}


def expected_proofs(coeffs, tau=TAU):
    """The 128 proofs of open_cell, p(tau) computed once per polynomial."""
    k = (hash(tuple(coeffs)), tau)
    if k not in _EXPECT:
        p_tau = K.horner(coeffs, tau)
        _EXPECT[k] = _g1c([F.quotient_scalar(coeffs, i, tau, p_tau) for i in range(K.NUM_CELLS)])
    return _EXPECT[k]


def blob_of(coeffs):
    """The blob (bytes) of a polynomial: its first 64 cells."""
    return RR.cells_to_bytes(RR.coeffs_to_cells(coeffs)[:64])


@pytest.fixture(scope="module")
def data():
    """Three random polynomials of degree 4095: coefficients, blob bytes, cells."""
    rng = random.Random(0xF20_7594)
    out = []
    for _ in range(3):
        coeffs = [rng.randrange(K.R) for _ in range(K.BLOB_N)]
        cells = RR.coeffs_to_cells(coeffs)
        out.append({"coeffs": coeffs, "cells": cells, "blob": RR.cells_to_bytes(cells[:64])})
    return out


# ------------------------------------------------------------------------------ the stages
def test_fk20_scalars(ctx, data):
    nb = 2
    got = _host(ctx.fk20_scalars(_dev(b"".join(d["blob"] for d in data[:nb])), nb))
    assert len(got) == nb * EXT
    for b in range(nb):
        assert RR.blob_to_coeffs([int.from_bytes(data[b]["blob"][32 * k:32 * k + 32], "big")
                                  for k in range(K.BLOB_N)]) == data[b]["coeffs"]
        want = b"".join(_be(row) for row in F.scalars(data[b]["coeffs"]))
        assert got[b * EXT:(b + 1) * EXT] == want


def _fft_inputs():
    rng = random.Random(0x128)
    a = [rng.randrange(K.R) for _ in range(F.N)]
    a[3] = a[77] = 0                       # infinities
    a[10] = a[74]                          # two equal points, partners of the first stage
    a[20], a[84] = 5, K.R - 5              # P and -P, partners of the first stage
    a[40] = a[41]                          # equal points that meet in the last stage
    b = [0] * F.N                          # mostly infinity: one point, and a pair P, -P
    b[1] = rng.randrange(K.R)
    b[64], b[96] = 9, K.R - 9
    return [a, b]


@pytest.mark.parametrize("inverse", [False, True])
def test_g1_fft128(ctx, inverse):
    vecs = _fft_inputs()
    got = _host(ctx.g1_fft128(_dev(b"".join(_g1(v) for v in vecs)), len(vecs), inverse=inverse))
    want = b"".join(_g1(F.dft(v, inverse=inverse)) for v in vecs)
    assert got == want


# ------------------------------------------------------------------------------ proofs
@pytest.mark.parametrize("nb", [1, 3])
def test_all_proofs_of_random_blobs(ctx, key, data, nb):
    cells, proofs = ctx.compute_cells_and_proofs(key, _dev(b"".join(d["blob"] for d in data[:nb])), nb)
    got = _host(proofs)
    assert len(got) == nb * PROOFS
    for b in range(nb):
        assert got[b * PROOFS:(b + 1) * PROOFS] == expected_proofs(data[b]["coeffs"])
    # the definition itself, once: open_cell's proof of one cell
    assert K.open_cell(data[0]["coeffs"], 77, TAU)[1] == got[77 * 48:78 * 48]


def _special(kind):
    c = [0] * K.BLOB_N
    if kind == "constant":
        c[0] = (0x1234567 << 200) + 5
    elif kind == "degree-63":
        rng = random.Random(63)
        c[:64] = [rng.randrange(K.R) for _ in range(64)]
    elif kind == "x^64":
        c[64] = 1
    elif kind == "top-coefficient":
        c[4095] = 0x7594_F20
    return c


@pytest.mark.parametrize("kind", ["zero", "constant", "degree-63", "x^64", "top-coefficient", "all-r-1"])
def test_special_polynomials(ctx, key, kind):
    if kind == "all-r-1":  # the constant polynomial r - 1: every element of the blob is r - 1
        coeffs = [K.R - 1] + [0] * (K.BLOB_N - 1)
        blob = (K.R - 1).to_bytes(32, "big") * K.BLOB_N
        assert blob_of(coeffs) == blob
    else:
        coeffs = _special(kind)
        blob = blob_of(coeffs)
    got = _host(ctx.compute_cells_and_proofs(key, _dev(blob), 1, cells=False)[1])
    if kind in ("zero", "constant", "degree-63", "all-r-1"):
        assert got == INF48 * 128
    elif kind == "x^64":
        assert got == K.g1_of(1) * 128
    assert got == expected_proofs(coeffs)


def test_degenerate_srs(ctx):
    """tau a primitive cube root of unity: [tau^m]_1 takes three values, so equal points, opposite
    points and infinities meet all through the transforms and the sums.  tau^64 = tau is no 128th
    root of unity, so every quotient is defined."""
    tau = pow(7, (K.R - 1) // 3, K.R)
    assert tau != 1 and pow(tau, 3, K.R) == 1 and pow(tau, 64, K.R) == tau and pow(tau, 128, K.R) != 1
    pkey = ctx.load_cell_proof_key(toy_srs(tau))
    rng = random.Random(3)
    g = {(a, m): rng.randrange(K.R) for a in range(64) for m in range(3)}
    coeffs = [g[(j // 64, (j % 64) % 3)] for j in range(K.BLOB_N)]
    got = _host(ctx.compute_cells_and_proofs(pkey, _dev(blob_of(coeffs)), 1, cells=False)[1])
    assert got == expected_proofs(coeffs, tau)
    assert K.open_cell(coeffs, 5, tau)[1] == got[5 * 48:6 * 48]


def test_cells_output_equals_compute_cells(ctx, key, data):
    nb = 2
    d_blobs = _dev(b"".join(d["blob"] for d in data[:nb]))
    cells, proofs = ctx.compute_cells_and_proofs(key, d_blobs, nb)
    assert _host(cells) == _host(ctx.compute_cells(d_blobs, nb))
    assert _host(cells) == b"".join(RR.cells_to_bytes(d["cells"]) for d in data[:nb])
    none, proofs_only = ctx.compute_cells_and_proofs(key, d_blobs, nb, cells=False)
    assert none is None
    assert _host(proofs_only) == _host(proofs)


def test_proofs_verify(ctx, key, data):
    import torch
    srs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
    d = data[0]
    cells, proofs = ctx.compute_cells_and_proofs(key, _dev(d["blob"]), 1)
    C = K.commit(d["coeffs"], TAU)
    idx = list(range(128))
    cell_list = [K.cell_from_ints(c) for c in d["cells"]]
    pf = _host(proofs)
    proof_list = [pf[48 * i:48 * i + 48] for i in idx]
    r = K.challenge([C], [0] * 128, idx, cell_list, proof_list)
    args = (_dev(C), _dev(_u64([0] * 128)), _dev(_u64(idx)), cells)
    assert ctx.verify_cell_batch(srs, *args, proofs, m=1, n=128, r=r) is True
    swapped = torch.cat([proofs[48:96], proofs[:48], proofs[96:]])
    r2 = K.challenge([C], [0] * 128, idx, cell_list, [proof_list[1], proof_list[0]] + proof_list[2:])
    assert ctx.verify_cell_batch(srs, *args, swapped, m=1, n=128, r=r2) is False


def _given(cells_of_blobs, idx):
    return b"".join(K.cell_from_ints(cells[i]) for cells in cells_of_blobs for i in idx)


def test_recover_cells_and_proofs(ctx, key, data):
    import kzgmi
    import torch
    nb = 2
    rng = random.Random(0x1DC5)
    idx = rng.sample(range(128), 64)
    assert idx != sorted(idx)
    cells_of = [d["cells"] for d in data[:nb]]
    want_cells, want_proofs = ctx.compute_cells_and_proofs(key, _dev(b"".join(d["blob"] for d in data[:nb])), nb)
    cells, proofs = ctx.recover_cells_and_proofs(key, _dev(_u64(idx)), _dev(_given(cells_of, idx)), nb)
    assert _host(cells) == _host(want_cells)
    assert _host(proofs) == _host(want_proofs) == b"".join(expected_proofs(d["coeffs"]) for d in data[:nb])
    # one altered element (kept in range) among 65 cells: no polynomial of degree < 4096 fits
    idx65 = rng.sample(range(128), 65)
    bad = bytearray(_given(cells_of, idx65))
    o = (1 * 65 + 17) * K.CELL_BYTES + 32 * 41
    bad[o:o + 32] = ((int.from_bytes(bad[o:o + 32], "big") + 1) % K.R).to_bytes(32, "big")
    untouched = torch.full((nb * PROOFS,), 0xAA, dtype=torch.uint8, device="cuda")
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.recover_cells_and_proofs(key, _dev(_u64(idx65)), _dev(bytes(bad)), nb, proofs_out=untouched)
    assert e.value.code == ERR_ARG
    assert _host(untouched) == b"\xaa" * (nb * PROOFS)  # no proofs
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.recover_cells_and_proofs(key, idx65, bytes(bad), nb)
    assert e.value.code == ERR_ARG
    # the slot is usable afterwards
    cells, proofs = ctx.recover_cells_and_proofs(key, _dev(_u64(idx65)), _dev(_given(cells_of, idx65)), nb)
    assert _host(cells) == _host(want_cells) and _host(proofs) == _host(want_proofs)


# ------------------------------------------------------------------------------ errors and plumbing
def test_element_out_of_range(ctx, key, data):
    import kzgmi
    nb = 2
    raw = b"".join(d["blob"] for d in data[:nb])
    for pos in (0, nb * BLOB - 32):  # element 0 of blob 0, element 4095 of the last blob
        bad = bytearray(raw)
        bad[pos:pos + 32] = K.R.to_bytes(32, "big")
        for cells in (True, False):
            with pytest.raises(kzgmi.KzgmiError) as e:
                ctx.compute_cells_and_proofs(key, _dev(bytes(bad)), nb, cells=cells)
            assert e.value.code == ERR_SCALAR
            with pytest.raises(kzgmi.KzgmiError) as e:
                ctx.compute_cells_and_proofs(key, bytes(bad), nb, cells=cells)
            assert e.value.code == ERR_SCALAR
    assert _host(ctx.compute_cells_and_proofs(key, _dev(raw), nb)[1])[:PROOFS] == expected_proofs(data[0]["coeffs"])


def test_key_and_argument_errors(ctx, key, data):
    import kzgmi
    from pointcases import non_subgroup_points
    C = pc.BLS12_381
    good = toy_srs(TAU)
    off = bytearray(good)
    off[96 * 4000 + 95] ^= 1  # y + 1: off the curve
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.load_cell_proof_key(bytes(off))
    assert e.value.code == ERR_NOT_ON_CURVE
    out = bytearray(good)
    out[96 * 4095:96 * 4096] = pk.g1_to_bytes(non_subgroup_points(1, seed=7)[0], C)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.load_cell_proof_key(bytes(out))
    assert e.value.code == ERR_NOT_IN_SUBGROUP
    inf = bytearray(good)
    inf[96 * 7:96 * 8] = b"\x40" + bytes(95)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.load_cell_proof_key(bytes(inf))
    assert e.value.code == ERR_ARG
    # a key of another context
    other = kzgmi.Context(0, 1)
    try:
        with pytest.raises(kzgmi.KzgmiError) as e:
            other.compute_cells_and_proofs(key, _dev(data[0]["blob"]), 1)
        assert e.value.code == ERR_ARG
    finally:
        other.close()
    # too many blobs, checked before anything is read
    L = kzgmi.lib()
    with pytest.raises(kzgmi.KzgmiError) as e:
        kzgmi._check(L.kzgmi_compute_cells_and_proofs_device(ctx.handle, key.handle, 16, 4097, 16, 32))
    assert e.value.code == ERR_ARG
    with pytest.raises(kzgmi.KzgmiError) as e:
        kzgmi._check(L.kzgmi_recover_cells_and_proofs_device(ctx.handle, key.handle, 16, 64, 32, 4097, 48, 64))
    assert e.value.code == ERR_ARG
    # nb = 0 succeeds and writes nothing
    assert ctx.compute_cells_and_proofs(key, b"", 0) == (b"", b"")
    assert ctx.recover_cells_and_proofs(key, list(range(64)), b"", 0) == (b"", b"")
    assert key.device_bytes >= 8192 * 64 * 8 * 96
    assert _host(ctx.compute_cells_and_proofs(key, _dev(data[0]["blob"]), 1)[1]) == expected_proofs(data[0]["coeffs"])


def test_host_forms_equal_device_forms(ctx, key, data):
    import kzgmi
    import torch
    nb = 2
    raw = b"".join(d["blob"] for d in data[:nb])
    want_cells = b"".join(RR.cells_to_bytes(d["cells"]) for d in data[:nb])
    want_proofs = b"".join(expected_proofs(d["coeffs"]) for d in data[:nb])
    assert ctx.compute_cells_and_proofs(key, raw) == (want_cells, want_proofs)
    assert ctx.compute_cells_and_proofs(key, bytearray(raw), nb, cells=False) == (None, want_proofs)
    assert kzgmi.compute_cells_and_proofs(key, raw) == (want_cells, want_proofs)
    idx = list(range(1, 128, 2))
    given = _given([d["cells"] for d in data[:nb]], idx)
    assert ctx.recover_cells_and_proofs(key, idx, given) == (want_cells, want_proofs)
    assert kzgmi.recover_cells_and_proofs(key, _u64(idx), given, nb) == (want_cells, want_proofs)
    out = torch.zeros(nb * EXT, dtype=torch.uint8, device="cuda")
    pout = torch.zeros(nb * PROOFS, dtype=torch.uint8, device="cuda")
    c, p = ctx.compute_cells_and_proofs(key, _dev(raw), nb, out=out, proofs_out=pout)
    assert c is out and p is pout
    assert _host(out) == want_cells and _host(pout) == want_proofs
    out.zero_()
    pout.zero_()
    c, p = ctx.recover_cells_and_proofs(key, idx, _dev(given), nb, out=out, proofs_out=pout)  # host indices
    assert c is out and p is pout
    assert _host(out) == want_cells and _host(pout) == want_proofs


def test_second_call_allocates_nothing(ctx, key, data):
    import kzgmi
    nb = 2
    raw = b"".join(d["blob"] for d in data[:nb])
    idx = list(range(0, 128, 2))
    d_blobs, d_idx = _dev(raw), _dev(_u64(idx))
    d_in = _dev(_given([d["cells"] for d in data[:nb]], idx))

    def calls():
        ctx.compute_cells_and_proofs(key, d_blobs, nb)
        ctx.recover_cells_and_proofs(key, d_idx, d_in, nb)
        ctx.compute_cells_and_proofs(key, raw, nb)
        ctx.fk20_scalars(d_blobs, nb)

    calls()
    before = kzgmi.alloc_count()
    calls()
    assert kzgmi.alloc_count() == before


def test_async_beside_a_verification(ctx, key, data):
    """Proofs on slot 1 while a cell verification runs on slot 0; a busy slot refuses a second job."""
    import kzgmi
    import torch
    srs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
    d = data[0]
    check = [3, 64, 127]
    want = expected_proofs(d["coeffs"])
    vargs = (_dev(K.commit(d["coeffs"], TAU)), _dev(_u64([0, 0, 0])), _dev(_u64(check)),
             _dev(b"".join(K.cell_from_ints(d["cells"][i]) for i in check)),
             _dev(b"".join(want[48 * i:48 * i + 48] for i in check)))
    nb = 2
    raw = b"".join(x["blob"] for x in data[:nb])
    d_blobs = _dev(raw)
    out = torch.zeros(nb * EXT, dtype=torch.uint8, device="cuda")
    pout = torch.zeros(nb * PROOFS, dtype=torch.uint8, device="cuda")
    ctx.verify_cell_batch_async(srs, 0, *vargs, 1, 3)
    ctx.compute_cells_and_proofs_async(key, 1, d_blobs, nb, out, pout)
    with pytest.raises(kzgmi.KzgmiError) as e:  # slot 1 is busy
        ctx.compute_cells_and_proofs_async(key, 1, d_blobs, nb, None, pout)
    assert e.value.code == ERR_ARG
    assert ctx.wait(1) is True
    assert ctx.wait(0) is True
    want_all = b"".join(expected_proofs(x["coeffs"]) for x in data[:nb])
    assert _host(pout) == want_all
    assert _host(out) == b"".join(RR.cells_to_bytes(x["cells"]) for x in data[:nb])
    idx = list(range(64, 128))
    d_idx, d_in = _dev(_u64(idx)), _dev(_given([x["cells"] for x in data[:nb]], idx))
    pout.zero_()
    ctx.verify_cell_batch_async(srs, 0, *vargs, 1, 3)
    ctx.recover_cells_and_proofs_async(key, 1, d_idx, d_in, nb, out, pout)
    assert ctx.wait(1) is True
    assert ctx.wait(0) is True
    assert _host(pout) == want_all
