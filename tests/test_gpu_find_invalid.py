"""Locating the invalid tuples of a rejected batch on the GPU (csrc/host_find.hip): the batched pairing
check, the grouped small MSMs and the search over index ranges, all against the C oracle: a range's
(A, B) from oracle.batch_verify_g1(.., offset, pairing=False), a record pair's verdict from
oracle.pairing_check, a tuple's validity from oracle.batch_verify_g1 at n = 1.  Nothing is compared
with the code under test.

Shapes: the smallest at which each path can go wrong -- group lengths 1, 2, 3, 5, 64 and 65 (odd, even
and single trees, one past a wave's 64 lanes), 257 pairing workgroups (more than the 256 CUs), batches
of 1, 2, 17 and 4099 tuples (one level, a level-0 boundary, three levels), and the smallest batch whose
level-0 parts pass the shipped crossover into bucket jobs (read through the plan probe).
"""
import ctypes
import hashlib
import random

import pytest

pytestmark = pytest.mark.gpu

import blobproofref as BP  # noqa: E402
import blobref as BR  # noqa: E402
import findprobe  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402

CURVES = ["bls12_381", "bn254"]
TAU = 0x5EA2_C4F0_0D15_EA5E
BLOB_TAU = 0x4844_0000_1234_5678_9ABC_DEF1
ERR_ARG, ERR_SCALAR, ERR_SHARD = -1, -4, -8
FLAG_COMPRESSED, FLAG_SUBGROUP_CHECK, FLAG_POWERS, FLAG_TRUSTED_G1 = 1, 2, 4, 16
SEED = hashlib.sha256(b"find-invalid").digest()


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=torch.uint8).cuda()[:len(b)]


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


class Env:
    """A curve's SRS under TAU and batches of valid tuples made on the device."""

    def __init__(self, ctx, curve):
        self.ctx, self.curve = ctx, curve
        self.C = pc.CURVES[curve]
        self.r = self.C.r
        self.g1b = 2 * self.C.fp_bytes
        self.g2 = pk.g2_to_bytes(self.C.g2, self.C)
        self.tg2 = O.g2_mul(curve, self.g2, TAU)
        self.srs = ctx.load_srs(curve, self.g2, self.tg2)
        self.pb = ctx.partial_bytes(curve)
        self.inf = (b"\x40" if curve == "bls12_381" else b"\x00") + bytes(self.g1b - 1)
        self._batches = {}

    def batch(self, n):
        """n valid tuples as host lists [C_i], [z_i], [y_i], [pi_i] (made once per n, never changed)"""
        if n not in self._batches:
            import torch
            t = [torch.empty(n * s, dtype=torch.uint8, device="cuda") for s in (self.g1b, 32, 32, self.g1b)]
            self.ctx.gen_tuples(self.curve, TAU, hashlib.sha256(b"find-tuples-%d" % n).digest(), n, *t)
            self._batches[n] = tuple([b[i:i + s] for i in range(0, len(b), s)]
                                     for b, s in zip(map(_host, t), (self.g1b, 32, 32, self.g1b)))
        return tuple(list(x) for x in self._batches[n])

    def valid(self, C, z, y, pi):
        """one tuple's validity, by the oracle at n = 1"""
        return O.batch_verify_g1(self.curve, C, z, y, pi, 1, None, self.g2, self.tg2, SEED)[0]

    def combination(self, t, lo, hi, offset):
        Cs, zs, ys, ps = (b"".join(x[lo:hi]) for x in t)
        _, A, B = O.batch_verify_g1(self.curve, Cs, zs, ys, ps, hi - lo, None, self.g2, self.tg2, SEED,
                                    offset=offset + lo, pairing=False)
        return A, B


_envs = {}


@pytest.fixture
def env(ctx, request):
    curve = request.param
    if curve not in _envs:
        _envs[curve] = Env(ctx, curve)
    return _envs[curve]


def _y_plus_1(env, y):
    return ((int.from_bytes(y, "big") + 1) % env.r).to_bytes(32, "big")


def corrupt(env, t, bad):
    """Make exactly the tuples of `bad` invalid, in four ways by turns: y + 1, pi replaced by another
    tuple's proof, C replaced by another's, and the proofs of two tuples of `bad` swapped (both become
    invalid; their unrandomised sum would still pass)."""
    Cs, zs, ys, ps = (list(x) for x in t)
    bad = sorted(bad)
    other = [i for i in range(len(zs)) if i not in set(bad)]  # the replacements come from untouched tuples
    k = 0
    while k < len(bad):
        i, kind = bad[k], k % 4
        if kind == 3 and k + 1 < len(bad):
            j = bad[k + 1]
            ps[i], ps[j] = ps[j], ps[i]
            k += 2
            continue
        if kind == 1 and other:
            ps[i] = t[3][other[k % len(other)]]
        elif kind == 2 and other:
            Cs[i] = t[0][other[(k + 1) % len(other)]]
        else:
            ys[i] = _y_plus_1(env, ys[i])
        k += 1
    return Cs, zs, ys, ps


def device(t):
    return tuple(_dev(b"".join(x)) for x in t)


# ------------------------------------------------------------------------------ batched pairing
@pytest.mark.parametrize("env", CURVES, indirect=True)
def test_batched_pairing_matches_the_oracle(ctx, env):
    """G in {1, 2, 5, 257} record pairs from kzgmi_batch_partial_device, passing and failing entries in
    fixed places, with (inf, inf), which accepts, and (inf, finite), which rejects, among them."""
    import kzgmi
    import torch
    curve = env.curve
    base = env.batch(4)
    y0 = int.from_bytes(base[2][0], "big")
    yG = O.g1_mul_gen(curve, base[2][0], 1)
    kinds = [
        base,                                                                  # valid
        corrupt(env, env.batch(4), [2]),                                       # corrupted
        ([yG], [base[1][0]], [base[2][0]], [env.inf]),                         # pi = inf, C = y G1: A = B = inf
        ([base[0][1]], [base[1][0]], [base[2][0]], [env.inf]),                 # pi = inf, C != y G1: A = inf, B finite
    ]
    assert y0 != 0
    pool, want = [], []
    for t in kinds:
        rec = torch.empty(2 * env.pb, dtype=torch.uint8, device="cuda")
        ctx.batch_partial(env.srs, *[_dev(b"".join(x)) for x in t], len(t[1]), 7, SEED, rec)
        A, B = ctx.partial_encode(curve, rec, 2)
        pool.append(rec)
        want.append(O.pairing_check(curve, A, B, env.g2, env.tg2))
        if len(pool) >= 3:
            assert A == env.inf and (B == env.inf) == (len(pool) == 3)
    assert want == [True, False, True, False]
    for G in (1, 2, 5, 257):
        pattern = [1] if G == 1 else [(3 * g + g // 7) % 4 for g in range(G)]
        recs = torch.cat([pool[k] for k in pattern])
        assert ctx.batch_check_partials(env.srs, recs, G) == [want[k] for k in pattern], G
    assert ctx.batch_check_partials(env.srs, pool[0], 1) == [True]
    # a record marked by its caller fails the call
    recs = torch.cat([pool[0], torch.full((2 * env.pb,), 0xFF, dtype=torch.uint8, device="cuda"), pool[1]])
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.batch_check_partials(env.srs, recs, 3)
    assert e.value.code == ERR_SHARD
    assert ctx.batch_check_partials(env.srs, torch.cat([pool[1], pool[0]]), 2) == [False, True]


# ------------------------------------------------------------------------------ grouped partials
RANGES = [(0, 1), (1, 3), (3, 6), (6, 11), (0, 64), (5, 70)]


@pytest.mark.parametrize("env", CURVES, indirect=True)
@pytest.mark.parametrize("offset", [0, (1 << 33) + 5])
def test_grouped_partials_match_the_oracle(ctx, env, offset):
    """n = 70: every range's record pair, encoded, equals the oracle's (A, B) of that range at
    index_offset + lo, plain and compressed + subgroup-checked; a second call on the same context
    with other ranges reuses the arrival counters."""
    import torch
    curve, n = env.curve, 70
    t = env.batch(n)
    # tuple 0: pi = inf and C = y G1, so A of the singleton range [0, 1) is the point at infinity
    t[3][0] = env.inf
    t[0][0] = O.g1_mul_gen(curve, t[2][0], 1)
    want = {r: env.combination(t, r[0], r[1], offset) for r in RANGES + [(69, 70), (0, 70), (2, 5)]}
    assert want[(0, 1)] == (env.inf, env.inf)
    plain = device(t)
    comp = (_dev(O.g1_compress(curve, b"".join(t[0]), n)), plain[1], plain[2], _dev(O.g1_compress(curve, b"".join(t[3]), n)))
    for d, kw in ((plain, {}), (comp, {"compressed": True, "subgroup_check": True})):
        for ranges in (RANGES, [(2, 5), (0, 70), (69, 70), (0, 1)]):
            out = torch.full((2 * len(ranges) * env.pb,), 0xAA, dtype=torch.uint8, device="cuda")
            ctx.batch_range_partials(env.srs, *d, n, offset, SEED, ranges, out, **kw)
            enc = ctx.partial_encode(curve, out, 2 * len(ranges))
            for g, r in enumerate(ranges):
                assert (enc[2 * g], enc[2 * g + 1]) == want[r], (r, kw)


@pytest.mark.parametrize("env", ["bls12_381"], indirect=True)
def test_grouped_partials_arguments(ctx, env):
    import kzgmi
    import torch
    n = 70
    d = device(env.batch(n))
    out = torch.empty(2 * 4 * env.pb, dtype=torch.uint8, device="cuda")
    for ranges in ([(3, 3)], [(5, 4)], [(0, 71)]):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.batch_range_partials(env.srs, *d, n, 0, SEED, ranges, out)
        assert e.value.code == ERR_ARG
    L = kzgmi.lib()
    ptrs = [x.data_ptr() for x in d]
    one = (ctypes.c_uint64 * 2)(0, 1)
    rc = L.kzgmi_batch_range_partials_device(ctx.handle, env.srs.handle, *ptrs, n, 0, SEED, FLAG_POWERS, one, 1, out.data_ptr())
    assert rc == ERR_ARG
    rc = L.kzgmi_batch_range_partials_device(ctx.handle, env.srs.handle, *ptrs, n, 0, SEED, 0, one, 65537, out.data_ptr())
    assert rc == ERR_ARG


def test_grouped_partials_workspace_bound(ctx):
    """Ranges whose trees would pass the shipped bound are refused before anything runs."""
    import kzgmi
    import torch
    env = _envs.get("bls12_381") or Env(ctx, "bls12_381")
    t = findprobe.tuning()
    n = 1 << 12
    reps = 1
    while findprobe.group_plan([(0, n)] * reps)[0]["bytes"] <= t["group_bytes"]:
        reps *= 2
    assert reps <= t["max_ranges"]
    d = [torch.zeros(n * s, dtype=torch.uint8, device="cuda") for s in (env.g1b, 32, 32, env.g1b)]
    out = torch.empty(16, dtype=torch.uint8, device="cuda")
    flat = (ctypes.c_uint64 * (2 * reps))(*([0, n] * reps))
    rc = kzgmi.lib().kzgmi_batch_range_partials_device(ctx.handle, env.srs.handle, *[x.data_ptr() for x in d], n, 0, SEED,
                                                       0, flat, reps, out.data_ptr())
    assert rc == ERR_ARG and b"bound" in kzgmi.lib().kzgmi_last_error()


# ------------------------------------------------------------------------------ the search
def _bad_sets(n, rng):
    F = findprobe.level_fanout([(0, n)], findprobe.tuning())
    sets = [[], [0], [n - 1]]
    if n > 1:
        b = findprobe.split(0, n, F)[0][1]  # the first level-0 boundary
        sets.append([b - 1, b])
    if n >= 17:
        sets.append(sorted(rng.sample(range(n), 12)))
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


@pytest.mark.parametrize("env", CURVES, indirect=True)
@pytest.mark.parametrize("n", [1, 2, 17, 4099])
def test_search_finds_exactly_the_corrupted_tuples(ctx, env, n):
    rng = random.Random(n)
    for k, bad in enumerate(_bad_sets(n, rng)):
        t = corrupt(env, env.batch(n), bad)
        # the oracle's word on every corrupted tuple and on three untouched ones
        for i in bad:
            assert env.valid(*[x[i] for x in t]) is False, i
        for i in [i for i in (0, n // 2, n - 1) if i not in bad][:3]:
            assert env.valid(*[x[i] for x in t]) is True, i
        d = device(t)
        seeds = [SEED, None] if k % 2 == 0 else [SEED]
        for seed in seeds:
            got, more = ctx.batch_find_invalid(env.srs, *d, seed=seed, n=n, max_bad=16)
            assert (got, more) == (bad, False), (n, bad, seed)
        if k == 1:  # the host-buffer form, staged by the library
            got, more = ctx.batch_find_invalid(env.srs, *[b"".join(x) for x in t], seed=SEED, max_bad=16)
            assert (got, more) == (bad, False)
        assert ctx.batch_verify(env.srs, *d, seed=SEED, n=n) is (not bad)
    assert ctx.batch_find_invalid(env.srs, *device(env.batch(1)), n=0) == ([], False)


@pytest.mark.parametrize("env", CURVES, indirect=True)
def test_truncation(ctx, env):
    import kzgmi
    n = 40
    d = device(corrupt(env, env.batch(n), range(n)))
    assert ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n, max_bad=8) == (list(range(8)), True)
    assert ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n, max_bad=40) == (list(range(40)), False)
    assert ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n, max_bad=39) == (list(range(39)), True)
    for max_bad in (0, 4097):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n, max_bad=max_bad)
        assert e.value.code == ERR_ARG


@pytest.mark.parametrize("env", ["bls12_381"], indirect=True)
def test_both_paths_in_one_search(ctx, env):
    """The smallest n whose level-0 parts pass the shipped crossover: level 0 runs as bucket partial
    jobs, the last levels in the grouped kernel; with TRUSTED_G1 the bucket jobs take the GLV form."""
    import torch
    t = findprobe.tuning()
    longest = (t["group_terms"] - 1) // 3  # the longest part the grouped kernel takes
    n = t["bucket_fanout"] * longest + 4
    f0 = findprobe.level_fanout([(0, n)], t)
    parts = findprobe.split(0, n, f0)
    assert f0 == t["bucket_fanout"] and findprobe.level_path(parts, t) == 0
    f1 = findprobe.level_fanout(parts, t)
    assert f1 == t["fanout"] and findprobe.level_path(findprobe.split(*parts[0], f1), t) == 1
    bufs = [torch.empty(n * s, dtype=torch.uint8, device="cuda") for s in (env.g1b, 32, 32, env.g1b)]
    ctx.gen_tuples(env.curve, TAU, hashlib.sha256(b"find-both-paths").digest(), n, *bufs)
    bad = [5, parts[len(parts) // 2][0], n - 1]
    for i in bad:  # another y, on the device: its last byte + 1 (mod 256)
        bufs[2][32 * i + 31] += 1
    for i in bad + [0]:
        tup = [_host(b[i * s:(i + 1) * s]) for b, s in zip(bufs, (env.g1b, 32, 32, env.g1b))]
        assert env.valid(tup[0], tup[1], tup[2], tup[3]) is (i == 0)
    for kw in ({}, {"trusted_g1": True}):
        assert ctx.batch_find_invalid(env.srs, *bufs, seed=SEED, n=n, max_bad=8, **kw) == (bad, False)
        st = ctx.find_invalid_stats()
        assert st["bucket_jobs"] > 0 and st["wave_terms"] > 0 and st["levels"] >= 2 and st["pairings"] >= st["bucket_jobs"]


@pytest.mark.parametrize("env", ["bls12_381"], indirect=True)
def test_errors_leave_the_outputs_and_the_context_alone(ctx, env):
    import kzgmi
    L = kzgmi.lib()
    n = 17
    good = env.batch(n)
    t = corrupt(env, env.batch(n), [3])
    d = device(t)
    over = list(t[1])
    over[9] = env.r.to_bytes(32, "big")  # z >= r
    d_over = (d[0], _dev(b"".join(over)), d[2], d[3])
    bad = (ctypes.c_uint64 * 4)(*[0xAAAAAAAAAAAAAAAA] * 4)
    nb, more = ctypes.c_size_t(77), ctypes.c_int(77)

    def call(dd, flags=0):
        return L.kzgmi_batch_find_invalid_device(ctx.handle, env.srs.handle, *[x.data_ptr() for x in dd], n, SEED, flags,
                                                 bad, 4, ctypes.byref(nb), ctypes.byref(more))

    def untouched():
        return list(bad) == [0xAAAAAAAAAAAAAAAA] * 4 and nb.value == 77 and more.value == 77

    assert call(d_over) == ERR_SCALAR and untouched()
    assert ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n) == ([3], False)
    assert call(d, FLAG_POWERS) == ERR_ARG and untouched()
    assert ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n) == ([3], False)
    # a job pending on slot 0: the error every synchronous slot-0 call gives
    gd = device(good)
    ctx.batch_verify_async(env.srs, 0, *gd, n, seed=SEED)
    assert call(d) == ERR_ARG and untouched() and b"slot 0 busy" in L.kzgmi_last_error()
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.last_combination(env.curve)
    assert e.value.code == ERR_ARG and "slot 0 busy" in str(e.value)
    assert ctx.wait(0) is True
    assert ctx.batch_find_invalid(env.srs, *d, seed=SEED, n=n) == ([3], False)
    assert call(d) == 0 and list(bad)[:1] == [3] and nb.value == 1 and more.value == 0


@pytest.mark.parametrize("env", CURVES, indirect=True)
def test_search_leaves_no_state_behind(ctx, env):
    n = 300
    d = device(corrupt(env, env.batch(n), [17, 250]))
    before = (ctx.batch_verify(env.srs, *d, seed=SEED, n=n), ctx.last_combination(env.curve))
    assert ctx.batch_find_invalid(env.srs, *d, seed=None, n=n) == ([17, 250], False)
    after = (ctx.batch_verify(env.srs, *d, seed=SEED, n=n), ctx.last_combination(env.curve))
    assert before == after and before[0] is False


# ------------------------------------------------------------------------------ blobs
@pytest.fixture(scope="module")
def blob_key(ctx):
    lag = BP.lagrange_scalars(BLOB_TAU)
    return ctx.load_blob_proof_key(O.g1_mul_gen(BR.CURVE, BP.be(lag), len(lag)))


@pytest.mark.parametrize("n,which", [(3, 1), (6, 5)])
def test_blob_search_names_the_changed_blob(ctx, blob_key, n, which):
    C = pc.CURVES[BR.CURVE]
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(BR.CURVE, g2, O.g2_mul(BR.CURVE, g2, BLOB_TAU))
    rng = random.Random(4844 + n)
    blobs = b"".join(BR.blob_from_ints([rng.randrange(BR.R) for _ in range(BR.N)]) for _ in range(n))
    d_blobs = _dev(blobs)
    cs = ctx.blob_commit(blob_key, d_blobs, n)
    pis = ctx.compute_blob_proofs(blob_key, d_blobs, cs, n)
    assert ctx.verify_blob_batch(srs, d_blobs, cs, pis, n) is True
    assert ctx.blob_batch_find_invalid(srs, d_blobs, cs, pis, n) == ([], False)
    # one element of one blob changed after proving
    changed = bytearray(blobs)
    o = which * BR.BLOB_BYTES + 32 * 1234
    changed[o:o + 32] = ((int.from_bytes(changed[o:o + 32], "big") + 1) % BR.R).to_bytes(32, "big")
    d_changed = _dev(bytes(changed))
    assert ctx.verify_blob_batch(srs, d_changed, cs, pis, n) is False
    assert ctx.blob_batch_find_invalid(srs, d_changed, cs, pis, n) == ([which], False)
    assert ctx.blob_batch_find_invalid(srs, bytes(changed), _host(cs), _host(pis)) == ([which], False)
    assert ctx.verify_blob_batch(srs, d_blobs, cs, pis, n) is True
