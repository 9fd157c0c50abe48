"""EIP-7594 cell batch verification on the GPU (csrc/cell.hpp) vs the pure-Python reference of
tests/cellref.py and the C oracle's MSM.  Everything is compared bit-exactly.

The fold kernel gives coset c to workgroup c and cell element j to thread j; the transcript hash
fetches 16 words per block on lanes 0-15, a cell record being 528 words = 33 blocks.  The batch
sizes put the MSM's 64-term tail class behind 3n (6n with GLV) other terms on both MSM paths.
"""
import os
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

import cellref as K  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402
from pointcases import non_subgroup_points  # noqa: E402

CURVE = K.CURVE
TAU = 0x7594_0000_1234_5678_9ABC_DEF1
NMAX = 65
E2E_SIZES = [1, 2, 7, 65]


def _context_with_env(slots=2, **env):
    """A kzgmi.Context created with the given environment overrides (read at creation)."""
    import kzgmi
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzgmi.Context(0, slots)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def toy():
    return K.toy_cell_srs(TAU)


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs(ctx, toy):
    return ctx.load_cell_srs(*toy)


@pytest.fixture(scope="module")
def bucket(toy):
    """A context whose MSMs never take the one-wave-per-term path (the bucket method), with its SRS."""
    c = _context_with_env(KZGMI_SMALL_TERMS="0")
    yield c, c.load_cell_srs(*toy)
    c.close()


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=torch.uint8).cuda()[:len(b)]


def _u64(xs):
    return struct.pack("<%dQ" % len(xs), *xs)


def _host(t):
    return t.cpu().numpy().tobytes()


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(len(b) // 32)]


@pytest.fixture(scope="module")
def batch():
    """NMAX valid openings, every prefix a valid batch: five polynomials (two of degree 4095, three
    of degree 100) cycled, so commitments repeat; cell 5 repeats cell 0's (commitment, cell) pair
    (polynomial 0 again, on cell 0's coset) and cell 6 shares cell 2's coset.
    Lists: C (the unique commitments), cidx, cell, cells, pi."""
    rng = random.Random(0x7594)
    polys = [[rng.randrange(K.R) for _ in range(K.BLOB_N)] for _ in range(2)]
    polys += [[rng.randrange(K.R) for _ in range(101)] for _ in range(3)]
    cs = [K.commit(p, TAU) for p in polys]
    assert len(set(cs)) == 5
    cidx = [k % 5 for k in range(NMAX)]
    cell = [rng.randrange(K.NUM_CELLS) for _ in range(NMAX)]
    cell[0], cell[1], cell[2] = 0, 127, 64
    cell[5] = cell[0]  # the duplicate pair
    cell[6] = cell[2]  # same coset as cell 2, another polynomial
    memo = {}
    cells, pi = [], []
    for c, i in zip(cidx, cell):
        if (c, i) not in memo:
            memo[(c, i)] = K.open_cell(polys[c], i, TAU)
        cells.append(memo[(c, i)][0])
        pi.append(memo[(c, i)][1])
    return {"C": cs, "cidx": cidx, "cell": cell, "cells": cells, "pi": pi}


def _prefix(batch, n):
    """The first n cells with the commitments deduplicated in order of first appearance."""
    m = min(n, 5)
    return batch["C"][:m], batch["cidx"][:n], batch["cell"][:n], batch["cells"][:n], batch["pi"][:n]


def _devargs(cs, cidx, cell, cells, pi):
    return (_dev(b"".join(cs)), _dev(_u64(cidx)), _dev(_u64(cell)), _dev(b"".join(cells)), _dev(b"".join(pi)))


_EXPECTED = {}


def _expected(batch, n, toy):
    """(r, A, B) of the first n cells, computed once per n."""
    if n not in _EXPECTED:
        args = _prefix(batch, n)
        r = K.challenge(*args)
        A, Bc = K.expected_combination(*args, r, toy[0])
        assert O.pairing_check(CURVE, A, Bc, toy[1], toy[2]) is True
        _EXPECTED[n] = (r, A, Bc)
    return _EXPECTED[n]


# ------------------------------------------------------------------------------ stage parity
@pytest.mark.parametrize("m,n", [(1, 1), (3, 7), (2, 65)])
def test_batch_challenge(ctx, batch, m, n):
    """48 + 48 m + 2112 n bytes: the cell records start at byte 48 (m + 1), a block boundary only
    for m = 3; n = 65 is 2145 blocks."""
    cs = batch["C"][:m]
    cidx = [k % m for k in range(n)]
    args = (cs, cidx, batch["cell"][:n], batch["cells"][:n], batch["pi"][:n])
    assert (48 * (m + 1) % 64 == 0) == (m == 3)
    assert ctx.cell_batch_challenge(*_devargs(*args), m, n) == K.challenge(*args)


def test_batch_challenge_empty(ctx):
    assert ctx.cell_batch_challenge(*_devargs([], [], [], [], []), 0, 0) == K.challenge([], [], [], [], [])


def _interp(ctx, cell_idx, cells, r):
    out = ctx.cell_interp(_dev(_u64(cell_idx)), _dev(b"".join(cells)), len(cells), r)
    return _ints(_host(out))


def _agg_closed_form(cell_idx, cells, r):
    agg = [0] * K.CELL_N
    for rk, i, cell in zip(K.powers(r, len(cells)), cell_idx, cells):
        for mm, c in enumerate(K.interpolate(i, K.cell_to_ints(cell))):
            agg[mm] = (agg[mm] + rk * c) % K.R
    return agg


@pytest.mark.parametrize("i", [0, 1, 63, 64, 127])
def test_interp_single_cell(ctx, i):
    rng = random.Random(100 + i)
    vals = [rng.randrange(K.R) for _ in range(K.CELL_N)]
    got = _interp(ctx, [i], [K.cell_from_ints(vals)], rng.randrange(K.R))  # r^0 = 1 whatever r is
    assert got == K.interpolate(i, vals)
    assert [K.horner(got, x) for x in K.coset_points(i)] == vals


def test_interp_mix_same_coset(ctx):
    """7 cells, cells 1 and 4 on coset 77: their fold precedes the one transform of that coset."""
    rng = random.Random(7)
    idx = [3, 77, 0, 127, 77, 64, 1]
    cells = [K.cell_from_ints([rng.randrange(K.R) for _ in range(K.CELL_N)]) for _ in idx]
    r = rng.randrange(K.R)
    assert _interp(ctx, idx, cells, r) == _agg_closed_form(idx, cells, r) == K.aggregate(idx, cells, r)


def test_interp_extreme_cells_and_challenges(ctx):
    rng = random.Random(8)
    zero = K.cell_from_ints([0] * K.CELL_N)
    top = K.cell_from_ints([K.R - 1] * K.CELL_N)
    rnd = K.cell_from_ints([rng.randrange(K.R) for _ in range(K.CELL_N)])
    r = rng.randrange(K.R)
    assert _interp(ctx, [5, 9], [zero, zero], r) == [0] * K.CELL_N
    assert _interp(ctx, [5, 9, 5], [top, top, rnd], r) == _agg_closed_form([5, 9, 5], [top, top, rnd], r)
    # a constant cell interpolates to the constant
    assert _interp(ctx, [33], [top], r) == [K.R - 1] + [0] * (K.CELL_N - 1)
    for rr in (0, 1, K.R - 1):  # r = 0: weights 1, 0, 0
        assert _interp(ctx, [5, 9, 5], [rnd, top, top], rr) == _agg_closed_form([5, 9, 5], [rnd, top, top], rr)
    assert _interp(ctx, [5, 9, 5], [rnd, top, top], 0) == K.interpolate(5, K.cell_to_ints(rnd))
    assert _interp(ctx, [], [], r) == [0] * K.CELL_N


# ------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("glv", [True, False], ids=["glv", "noglv"])
@pytest.mark.parametrize("path", ["default", "buckets"])
@pytest.mark.parametrize("n", E2E_SIZES)
def test_verify_device(ctx, srs, bucket, batch, toy, n, path, glv):
    c, s = (ctx, srs) if path == "default" else bucket
    r, A, Bc = _expected(batch, n, toy)
    args = _prefix(batch, n)
    d = _devargs(*args)
    m = len(args[0])
    c.set_glv(batch=glv)
    try:
        assert c.cell_batch_challenge(*d, m, n) == r
        assert c.verify_cell_batch(s, *d, m=m, n=n) is True
        assert c.last_combination(CURVE) == (A, Bc)
        # the caller-supplied challenge gives the same combination
        assert c.verify_cell_batch(s, *d, m=m, n=n, r=r) is True
        assert c.last_combination(CURVE) == (A, Bc)
        # one flipped cell element (kept in range)
        bad = bytearray(b"".join(args[3]))
        o = (n - 1) * K.CELL_BYTES + 32 * 41
        bad[o:o + 32] = ((int.from_bytes(bad[o:o + 32], "big") + 1) % K.R).to_bytes(32, "big")
        assert c.verify_cell_batch(s, d[0], d[1], d[2], _dev(bytes(bad)), d[4], m=m, n=n) is False
    finally:
        c.set_glv(batch=True)


def test_verify_forms_agree(ctx, srs, batch, toy):
    """Host buffers, the module-level specification form and the async form against the device form."""
    import kzgmi
    n = 7
    r, A, Bc = _expected(batch, n, toy)
    cs, cidx, cell, cells, pi = _prefix(batch, n)
    m = len(cs)
    assert ctx.verify_cell_batch(srs, b"".join(cs), cidx, cell, b"".join(cells), b"".join(pi)) is True
    assert ctx.last_combination(CURVE) == (A, Bc)
    assert ctx.verify_cell_batch(srs, b"".join(cs), _u64(cidx), _u64(cell), b"".join(cells), b"".join(pi), r=r) is True
    assert ctx.last_combination(CURVE) == (A, Bc)
    per_cell = [cs[i] for i in cidx]
    assert kzgmi.verify_cell_batch(per_cell, cell, cells, pi, srs) is True
    assert ctx.last_combination(CURVE) == (A, Bc)
    assert kzgmi.verify_cell_batch(per_cell, cell, cells, pi, srs, r=r) is True
    bad = bytearray(b"".join(cells))
    bad[3 * K.CELL_BYTES + 31] ^= 1
    assert ctx.verify_cell_batch(srs, b"".join(cs), cidx, cell, bytes(bad), b"".join(pi)) is False
    d = _devargs(cs, cidx, cell, cells, pi)
    dbad = _dev(bytes(bad))
    ctx.verify_cell_batch_async(srs, 0, *d, m, n)
    ctx.verify_cell_batch_async(srs, 1, d[0], d[1], d[2], dbad, d[4], m, n)
    assert ctx.wait(1) is False
    assert ctx.wait(0) is True
    ctx.verify_cell_batch_async(srs, 0, d[0], d[1], d[2], dbad, d[4], m, n, r=r)
    ctx.verify_cell_batch_async(srs, 1, *d, m, n, r=r)
    assert ctx.wait(0) is False
    assert ctx.wait(1) is True


def test_rejections(ctx, srs, batch):
    n = 7
    cs, cidx, cell, cells, pi = _prefix(batch, n)
    m = len(cs)
    d = _devargs(cs, cidx, cell, cells, pi)
    assert ctx.verify_cell_batch(srs, *d, m=m, n=n) is True
    # a wrong cell_index: cell 3 claimed on another coset
    wrong = list(cell)
    wrong[3] = (wrong[3] + 1) % K.NUM_CELLS
    assert ctx.verify_cell_batch(srs, d[0], d[1], _dev(_u64(wrong)), d[3], d[4], m=m, n=n) is False
    # swapped proofs (of different openings)
    assert pi[0] != pi[1]
    sw = [pi[1], pi[0]] + pi[2:]
    assert ctx.verify_cell_batch(srs, d[0], d[1], d[2], d[3], _dev(b"".join(sw)), m=m, n=n) is False
    # a commitment index pointing at another blob
    other = list(cidx)
    other[2] = (other[2] + 1) % m
    assert ctx.verify_cell_batch(srs, d[0], _dev(_u64(other)), d[2], d[3], d[4], m=m, n=n) is False
    # a wrong caller-supplied challenge still verifies a valid batch (any weights do), a corrupted one not
    assert ctx.verify_cell_batch(srs, *d, m=m, n=n, r=12345) is True
    assert ctx.verify_cell_batch(srs, d[0], d[1], _dev(_u64(wrong)), d[3], d[4], m=m, n=n, r=12345) is False


@pytest.mark.parametrize("pos", [0, 63])
def test_element_out_of_range(ctx, srs, batch, pos):
    """An element equal to r: KZGMI_ERR_SCALAR from every entry point that reads cells' values."""
    import kzgmi
    n = 3
    cs, cidx, cell, cells, pi = _prefix(batch, n)
    bad = bytearray(b"".join(cells))
    o = 2 * K.CELL_BYTES + 32 * pos
    bad[o:o + 32] = K.R.to_bytes(32, "big")
    bad = bytes(bad)
    d = _devargs(cs, cidx, cell, cells, pi)
    dbad = _dev(bad)
    calls = [lambda: ctx.cell_interp(d[2], dbad, n, 5),
             lambda: ctx.verify_cell_batch(srs, d[0], d[1], d[2], dbad, d[4], m=n, n=n),
             lambda: ctx.verify_cell_batch(srs, d[0], d[1], d[2], dbad, d[4], m=n, n=n, r=5),
             lambda: ctx.verify_cell_batch(srs, b"".join(cs), cidx, cell, bad, b"".join(pi)),
             lambda: (ctx.verify_cell_batch_async(srs, 1, d[0], d[1], d[2], dbad, d[4], n, n), ctx.wait(1))]
    for call in calls:
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == -4
    assert ctx.verify_cell_batch(srs, *d, m=n, n=n) is True  # the context still works


def test_index_and_point_errors(ctx, srs, batch, toy):
    import kzgmi
    n = 3
    cs, cidx, cell, cells, pi = _prefix(batch, n)
    d = _devargs(cs, cidx, cell, cells, pi)
    for idx in ([cell[0], 128, cell[2]], [cell[0], cell[1], 1 << 40]):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.verify_cell_batch(srs, d[0], d[1], _dev(_u64(idx)), d[3], d[4], m=n, n=n)
        assert e.value.code == -1
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.cell_interp(_dev(_u64(idx)), d[3], n, 5)
        assert e.value.code == -1
    with pytest.raises(kzgmi.KzgmiError) as e:  # commitment_index = m
        ctx.verify_cell_batch(srs, d[0], _dev(_u64([0, n, 2])), d[2], d[3], d[4], m=n, n=n)
    assert e.value.code == -1
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.verify_cell_batch(srs, b"".join(cs), [0, n, 2], cell, b"".join(cells), b"".join(pi), r=7)
    assert e.value.code == -1
    off = pk.g1_to_bytes_compressed(non_subgroup_points(1)[0], pc.BLS12_381)
    with pytest.raises(kzgmi.KzgmiError) as e:  # a proof outside the subgroup
        ctx.verify_cell_batch(srs, d[0], d[1], d[2], d[3], _dev(pi[0] + off + pi[2]), m=n, n=n)
    assert e.value.code == -7
    with pytest.raises(kzgmi.KzgmiError) as e:  # a commitment outside the subgroup
        ctx.verify_cell_batch(srs, _dev(off + cs[1] + cs[2]), d[1], d[2], d[3], d[4], m=n, n=n)
    assert e.value.code == -7
    # an SRS of the wrong kind
    plain = ctx.load_srs(CURVE, toy[1], toy[2])
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.verify_cell_batch(plain, *d, m=n, n=n)
    assert e.value.code == -1
    rc = kzgmi.lib().kzgmi_verify_cell_batch_device_async(ctx.handle, plain.handle, 0, d[0].data_ptr(), n, d[1].data_ptr(),
                                                          d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), n, None)
    assert rc == -1
    # n = 0 accepts
    e0 = _devargs([], [], [], [], [])
    assert ctx.verify_cell_batch(srs, *e0, m=0, n=0) is True
    assert ctx.verify_cell_batch(srs, b"", [], [], b"", b"") is True
    assert kzgmi.verify_cell_batch([], [], [], [], srs) is True
    assert ctx.verify_cell_batch(srs, *d, m=n, n=n) is True
