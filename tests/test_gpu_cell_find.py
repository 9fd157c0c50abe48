"""Locating the invalid cells of a rejected EIP-7594 cell batch on the GPU (csrc/host_find.hip over
csrc/cell.hpp k_cell_coeffs and csrc/msm_group.hpp k_cell_range_fold / the 64-term tail of k_group_msm)
against the pure-Python reference of tests/cellref.py and tests/cellfindref.py and the C oracle: a cell's
coefficients from cellref.interpolate (the closed form), a range's (A, B) from the oracle's MSM with the
counter-mode weights, a record pair's verdict and a cell's validity from oracle.pairing_check.  Nothing
is compared with the code under test.

Shapes: 1, 5 and 65 cells for the coefficient kernel (a wave per cell, four cells per workgroup: one
past a wave's 64 lanes and no multiple of 4), ranges of 1, 2, 3, 5, 64, 65 and 70 cells (odd, even and
single trees behind the 64 tail leaves), batches of 1, 2, 17 and 4099 cells (one level, a level-0
boundary, four levels at fan-out 16).
"""
import ctypes
import hashlib
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

import cellfindref as F  # noqa: E402
import cellref as K  # noqa: E402
import findprobe  # noqa: E402
import findref  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

CURVE = K.CURVE
TAU = 0x7594_F1ED_0000_1234_5678_9ABC_DEF1
NMAX = 4099
SIZES = [1, 2, 17, 4099]
ERR_ARG, ERR_SCALAR = -1, -4
SEED = hashlib.sha256(b"cell-find-invalid").digest()
INF48 = b"\xc0" + bytes(47)
INF96 = b"\x40" + bytes(95)
COSETS = [0, 1, 63, 64, 127, 2, 5, 9, 17, 31, 32, 33, 40, 62, 65, 77, 90, 96, 100, 111, 120, 125, 126, 3]
SENTINEL = 0xAAAAAAAAAAAAAAAA


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
def batch():
    """NMAX valid openings, every prefix a valid batch (never changed): five polynomials (two of degree
    4095, three of degree 100) cycled over 24 cosets, openings memoised per (polynomial, coset), so
    (commitment, cell) pairs repeat; polynomial 5 has degree 40 < 64, so I = p and its proofs are the
    point at infinity (cells 0 and 23).  Cell 6 shares cell 2's coset under another polynomial, cell 10
    repeats cell 5's pair.  Lists: C (the 6 unique commitments), cidx, cell, cells, pi."""
    rng = random.Random(0x7594F1)
    polys = [[rng.randrange(K.R) for _ in range(K.BLOB_N)] for _ in range(2)]
    polys += [[rng.randrange(K.R) for _ in range(101)] for _ in range(3)]
    polys += [[rng.randrange(K.R) for _ in range(41)]]
    cs = [K.commit(p, TAU) for p in polys]
    assert len(set(cs)) == 6
    cidx = [k % 5 for k in range(NMAX)]
    cell = [rng.choice(COSETS) for _ in range(NMAX)]
    cidx[0] = cidx[23] = 5
    cell[0], cell[1], cell[2] = 0, 127, 64
    cell[6] = cell[2]
    cell[10] = cell[5]
    assert cidx[10] == cidx[5] and cidx[6] != cidx[2]
    memo = {}
    cells, pi = [], []
    for c, i in zip(cidx, cell):
        if (c, i) not in memo:
            memo[(c, i)] = K.open_cell(polys[c], i, TAU)
        cells.append(memo[(c, i)][0])
        pi.append(memo[(c, i)][1])
    assert pi[0] == pi[23] == INF48 and pi[1] != INF48
    return {"C": cs, "cidx": cidx, "cell": cell, "cells": cells, "pi": pi}


def _prefix(batch, n):
    return list(batch["C"]), batch["cidx"][:n], batch["cell"][:n], batch["cells"][:n], batch["pi"][:n]


def _devargs(cs, cidx, cell, cells, pi):
    return (_dev(b"".join(cs)), _dev(_u64(cidx)), _dev(_u64(cell)), _dev(b"".join(cells)), _dev(b"".join(pi)))


def _plus_1(cell_bytes, j):
    v = (int.from_bytes(cell_bytes[32 * j:32 * j + 32], "big") + 1) % K.R
    return cell_bytes[:32 * j] + v.to_bytes(32, "big") + cell_bytes[32 * j + 32:]


def corrupt(batch, n, bad):
    """Make exactly the cells of `bad` invalid, in five ways by turns: a cell element + 1, the proof
    replaced by an untouched cell's other proof, the commitment index pointing at another commitment,
    the cell index moved to another coset with the bytes unchanged, and the proofs of two cells of
    `bad` swapped (both become invalid; their unrandomised sum would still pass).  A way that does
    not apply (no untouched cell, equal proofs) falls back to the first."""
    cs, cidx, cell, cells, pi = _prefix(batch, n)
    bad = sorted(bad)
    other = [i for i in range(n) if i not in set(bad)]
    k = 0
    while k < len(bad):
        i, kind = bad[k], k % 5
        if kind == 4 and k + 1 < len(bad) and pi[i] != pi[bad[k + 1]]:
            j = bad[k + 1]
            pi[i], pi[j] = pi[j], pi[i]
            k += 2
            continue
        donors = [o for o in other if batch["pi"][o] != pi[i]]
        if kind == 1 and donors:
            pi[i] = batch["pi"][donors[k % len(donors)]]
        elif kind == 2:
            cidx[i] = (cidx[i] + 1 + k % 4) % 5 if cidx[i] < 5 else k % 5
        elif kind == 3:
            cell[i] = (cell[i] + 1 + 7 * k) % K.NUM_CELLS
        else:
            cells[i] = _plus_1(cells[i], (11 * k + 41) % K.CELL_N)
        k += 1
    return cs, cidx, cell, cells, pi


def _valid(t, i, toy):
    cs, cidx, cell, cells, pi = t
    return F.cell_valid(cs[cidx[i]], cell[i], cells[i], pi[i], toy)


# ------------------------------------------------------------------------------ coefficients
@pytest.fixture(scope="module")
def coeff_cells():
    """65 cells: cosets 0, 1, 63, 64 and 127 first, then others; random elements, cell 5 alternating
    0 and r - 1; with cellref.interpolate of each, computed once."""
    rng = random.Random(65)
    idx = [0, 1, 63, 64, 127] + [rng.randrange(K.NUM_CELLS) for _ in range(60)]
    vals = [[rng.randrange(K.R) for _ in range(K.CELL_N)] for _ in idx]
    vals[5] = [0 if j % 2 == 0 else K.R - 1 for j in range(K.CELL_N)]
    want = [K.interpolate(i, v) for i, v in zip(idx, vals)]
    return idx, [K.cell_from_ints(v) for v in vals], want


@pytest.mark.parametrize("n", [1, 5, 65])
def test_coefficients(ctx, coeff_cells, n):
    idx, cells, want = coeff_cells
    if n == 5:  # the cell of extreme elements among the five
        idx, cells, want = ([x[k] for k in (0, 1, 5, 3, 4)] for x in (idx, cells, want))
    out = ctx.cell_coeffs(_dev(_u64(idx[:n])), _dev(b"".join(cells[:n])), n)
    got = _ints(_host(out))
    assert len(got) == 64 * n
    for k in range(n):
        assert got[64 * k:64 * k + 64] == want[k], k
    k = n - 1  # the coefficients interpolate the cell
    assert [K.horner(got[64 * k:64 * k + 64], x) for x in K.coset_points(idx[k])] == K.cell_to_ints(cells[k])


def test_coefficients_errors(ctx, coeff_cells):
    import kzgmi
    idx, cells, want = coeff_cells
    n = 6
    over = list(cells[:n])
    over[4] = over[4][:32 * 63] + K.R.to_bytes(32, "big")
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.cell_coeffs(_dev(_u64(idx[:n])), _dev(b"".join(over)), n)
    assert e.value.code == ERR_SCALAR
    for bad_idx in (128, 1 << 40):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.cell_coeffs(_dev(_u64(idx[:n - 1] + [bad_idx])), _dev(b"".join(cells[:n])), n)
        assert e.value.code == ERR_ARG
    # more cells than one call takes: refused before anything is read (these buffers hold 6 cells)
    di, dc = _dev(_u64(idx[:n])), _dev(b"".join(cells[:n]))
    assert kzgmi.lib().kzgmi_cell_coeffs_device(ctx.handle, di.data_ptr(), dc.data_ptr(), 65537, dc.data_ptr()) == ERR_ARG
    out = ctx.cell_coeffs(_dev(_u64(idx[:n])), _dev(b"".join(cells[:n])), n)  # the context still works
    assert _ints(_host(out))[64 * (n - 1):] == want[n - 1]
    assert ctx.cell_coeffs(_dev(b""), _dev(b""), 0).numel() == 0


# ------------------------------------------------------------------------------ range partials
RANGES = [(0, 1), (1, 3), (3, 6), (6, 11), (0, 64), (5, 70)]
RANGES2 = [(2, 5), (0, 70), (69, 70), (0, 1)]
_WANT = {}


def _want(batch, toy, offset):
    """every range's (A, B) at this offset, with the oracle's verdict on it; computed once"""
    if offset not in _WANT:
        args = _prefix(batch, 70)
        _WANT[offset] = {r: F.range_combination(SEED, offset, r[0], r[1], *args, toy[0]) for r in set(RANGES + RANGES2)}
        for r, (A, B) in _WANT[offset].items():
            assert O.pairing_check(CURVE, A, B, toy[1], toy[2]) is True, r
        assert _WANT[offset][(0, 1)] == (INF96, INF96)  # pi = inf and C = [I(tau)]_1
    return _WANT[offset]


@pytest.mark.parametrize("offset", [0, (1 << 33) + 5])
def test_range_partials_match_the_reference(ctx, srs, batch, toy, offset):
    """n = 70: every range's record pair, encoded, equals the reference's (A, B) of that range with
    the randomisers of the global indices index_offset + k; the second call, with other ranges on the
    same context, reuses the arrival counters."""
    import torch
    n = 70
    want = _want(batch, toy, offset)
    d = _devargs(*_prefix(batch, n))
    pb = ctx.partial_bytes(CURVE)
    for ranges in (RANGES, RANGES2):
        out = torch.full((2 * len(ranges) * pb,), 0xAA, dtype=torch.uint8, device="cuda")
        ctx.cell_range_partials(srs, *d, 6, n, offset, SEED, ranges, out)
        enc = ctx.partial_encode(CURVE, out, 2 * len(ranges))
        for g, r in enumerate(ranges):
            assert (enc[2 * g], enc[2 * g + 1]) == want[r], (r, offset)
        # (the batched pairing on the same [1]_2, [tau^64]_2 agrees with the oracle's verdicts in _want)
        assert ctx.batch_check_partials(_plain(ctx, toy), out, len(ranges)) == [True] * len(ranges)


_PLAIN = {}


def _plain(ctx, toy):
    """the ordinary SRS ([1]_2, [tau^64]_2) on this context"""
    if id(ctx) not in _PLAIN:
        _PLAIN[id(ctx)] = ctx.load_srs(CURVE, toy[1], toy[2])
    return _PLAIN[id(ctx)]


def test_range_partials_arguments(ctx, srs, batch, toy):
    import kzgmi
    import torch
    n = 70
    d = _devargs(*_prefix(batch, n))
    out = torch.empty(2 * 4 * ctx.partial_bytes(CURVE), dtype=torch.uint8, device="cuda")
    for ranges in ([(3, 3)], [(5, 4)], [(0, 71)]):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.cell_range_partials(srs, *d, 6, n, 0, SEED, ranges, out)
        assert e.value.code == ERR_ARG
    L = kzgmi.lib()
    ptrs = [d[0].data_ptr(), 6] + [x.data_ptr() for x in d[1:]]
    one = (ctypes.c_uint64 * 2)(0, 1)
    assert L.kzgmi_cell_range_partials_device(ctx.handle, srs.handle, *ptrs, n, 0, SEED, one, 65537, out.data_ptr()) == ERR_ARG
    assert L.kzgmi_cell_range_partials_device(ctx.handle, _plain(ctx, toy).handle, *ptrs, n, 0, SEED, one, 1,
                                              out.data_ptr()) == ERR_ARG
    assert L.kzgmi_cell_range_partials_device(ctx.handle, srs.handle, *ptrs, 65537, 0, SEED, one, 1, out.data_ptr()) == ERR_ARG
    assert L.kzgmi_cell_range_partials_device(ctx.handle, srs.handle, *ptrs, n, 0, SEED, one, 1, out.data_ptr()) == 0


# ------------------------------------------------------------------------------ the search
def _bad_sets(n, rng):
    fan = findprobe.tuning()["fanout"]
    sets = [[], [0], [n - 1]]
    if n > 1:
        b = findprobe.split(0, n, fan)[0][1]  # the first level-0 boundary
        sets.append([b - 1, b])
    if n >= 17:
        sets.append(sorted(rng.sample(range(n), 12)))
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


def _planned_stats(n, bad, max_bad):
    """levels, wave-terms and pairings of the search for `bad`, from the model of tests/findref.py over
    the plan's own split and next_level: every level is grouped at the shipped fan-out, and a part
    of len cells has 3 len + 64 wave-terms."""
    fan = findprobe.tuning()["fanout"]
    tally = {"wave_terms": 0, "pairings": 0}

    def split(lo, hi, f):
        parts = findprobe.split(lo, hi, f)
        tally["wave_terms"] += sum(3 * (b - a) + 64 for a, b in parts)
        tally["pairings"] += len(parts)
        return parts
    got, more, levels = findref.search(n, fan, max_bad, findref.contains(bad), split, findprobe.next_level)
    assert (got, more) == (bad[:max_bad], len(bad) > max_bad)
    return dict(tally, levels=levels, bucket_jobs=0)


@pytest.mark.parametrize("n", SIZES)
def test_search_finds_exactly_the_corrupted_cells(ctx, srs, batch, toy, n):
    import kzgmi
    rng = random.Random(n)
    for k, bad in enumerate(_bad_sets(n, rng)):
        t = corrupt(batch, n, bad)
        # the reference's word on every corrupted cell and on three untouched ones
        for i in bad:
            assert _valid(t, i, toy) is False, i
        for i in [i for i in (0, n // 2, n - 1) if i not in bad][:3]:
            assert _valid(t, i, toy) is True, i
        d = _devargs(*t)
        for seed in (SEED, None):
            got, more = ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=seed, max_bad=16)
            assert (got, more) == (bad, False), (n, bad, seed)
            assert ctx.find_invalid_stats() == _planned_stats(n, bad, 16)
        # the host-buffer form, staged by the library, and the specification's per-cell lists
        cs, cidx, cell, cells, pi = t
        got, more = ctx.cell_batch_find_invalid(srs, b"".join(cs), cidx, cell, b"".join(cells), b"".join(pi), seed=SEED,
                                                max_bad=16)
        assert (got, more) == (bad, False)
        if k == 1:
            got, more = kzgmi.cell_batch_find_invalid([cs[i] for i in cidx], cell, cells, pi, srs, seed=None, max_bad=16)
            assert (got, more) == (bad, False)
        assert ctx.verify_cell_batch(srs, *d, m=6, n=n) is (not bad)
    assert ctx.cell_batch_find_invalid(srs, *_devargs(*_prefix(batch, 1)), m=6, n=0) == ([], False)
    assert ctx.cell_batch_find_invalid(srs, b"", [], [], b"", b"") == ([], False)


def test_truncation(ctx, srs, batch, toy):
    import kzgmi
    n = 40
    t = corrupt(batch, n, range(n))
    for i in (0, 1, 2, 3, 4, 5, n - 1):  # each way of corrupt() once (the oracle's pairing takes ~0.2 s)
        assert _valid(t, i, toy) is False, i
    d = _devargs(*t)
    assert ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=SEED, max_bad=8) == (list(range(8)), True)
    assert ctx.find_invalid_stats() == _planned_stats(n, list(range(n)), 8)
    assert ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=SEED, max_bad=40) == (list(range(40)), False)
    assert ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=SEED, max_bad=39) == (list(range(39)), True)
    for max_bad in (0, 4097):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=SEED, max_bad=max_bad)
        assert e.value.code == ERR_ARG


def test_errors_leave_the_outputs_and_the_context_alone(ctx, srs, batch, toy):
    import kzgmi
    L = kzgmi.lib()
    n = 17
    t = corrupt(batch, n, [3])
    assert _valid(t, 3, toy) is False
    d = _devargs(*t)
    over = list(t[3])
    over[9] = over[9][:32 * 7] + K.R.to_bytes(32, "big") + over[9][32 * 8:]  # an element = r
    d_over = (d[0], d[1], d[2], _dev(b"".join(over)), d[4])
    bad = (ctypes.c_uint64 * 4)(*[SENTINEL] * 4)
    nb, more = ctypes.c_size_t(77), ctypes.c_int(77)

    def call(dd, handle=srs.handle, nn=n, m=6):
        return L.kzgmi_verify_cell_batch_find_invalid_device(ctx.handle, handle, dd[0].data_ptr(), m,
                                                             *[x.data_ptr() for x in dd[1:]], nn, SEED, bad, 4,
                                                             ctypes.byref(nb), ctypes.byref(more))

    def untouched():
        return list(bad) == [SENTINEL] * 4 and nb.value == 77 and more.value == 77

    def works():
        return ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=SEED) == ([3], False)

    assert call(d_over) == ERR_SCALAR and untouched() and works()
    # index errors found on the device: a cell index of 128, a commitment index of m
    d_cell = (d[0], d[1], _dev(_u64(t[2][:5] + [128] + t[2][6:])), d[3], d[4])
    assert call(d_cell) == ERR_ARG and untouched() and works()
    d_cidx = (d[0], _dev(_u64(t[1][:5] + [6] + t[1][6:])), d[2], d[3], d[4])
    assert call(d_cidx) == ERR_ARG and untouched() and works()
    # an SRS of the wrong kind
    assert call(d, handle=_plain(ctx, toy).handle) == ERR_ARG and untouched() and works()
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.cell_batch_find_invalid(_plain(ctx, toy), *d, m=6, n=n)
    assert e.value.code == ERR_ARG
    # more cells than one search takes: refused before any buffer is read (these hold 17 cells)
    assert call(d, nn=65537) == ERR_ARG and untouched() and b"65536" in L.kzgmi_last_error() and works()
    assert call(d, m=0) == ERR_ARG and untouched()
    # a job pending on slot 0: the error every synchronous slot-0 call gives
    gd = _devargs(*_prefix(batch, n))
    ctx.verify_cell_batch_async(srs, 0, *gd, 6, n)
    assert call(d) == ERR_ARG and untouched() and b"slot 0 busy" in L.kzgmi_last_error()
    assert ctx.wait(0) is True
    assert works()
    assert call(d) == 0 and list(bad) == [3] + [SENTINEL] * 3 and nb.value == 1 and more.value == 0


def test_search_leaves_no_state_behind(ctx, srs, batch):
    n = 300
    d = _devargs(*corrupt(batch, n, [17, 250]))
    before = (ctx.verify_cell_batch(srs, *d, m=6, n=n), ctx.last_combination(CURVE))
    assert ctx.cell_batch_find_invalid(srs, *d, m=6, n=n, seed=None) == ([17, 250], False)
    after = (ctx.verify_cell_batch(srs, *d, m=6, n=n), ctx.last_combination(CURVE))
    assert before == after and before[0] is False
