"""EIP-4844 commitments and proofs on the GPU (csrc/blobproof.hpp) vs the pure-Python model of
tests/blobproofref.py, in the exponent under a toy tau, and vs tests/blobref.py's open_blob.
Everything is compared as exact bytes.

The shapes are fixed by the protocol (4096-element blobs), so the shapes are small blob counts.  The
quotient kernel gives element j to thread j % 512 (pass j // 512); the MSM gives base j to block
j // 64, thread j % 64 (+ 64 part): the domain points and indices below sit on those boundaries.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

import blobproofref as P  # noqa: E402
import blobref as B  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.pyspec import curves as pc  # noqa: E402
from oracle.pyspec import kzg as pk  # noqa: E402
from pointcases import non_subgroup_points  # noqa: E402

CURVE = B.CURVE
R = B.R
TAU = 0x4844_0000_1234_5678_9ABC_DEF1
ERR_ARG, ERR_ENCODING, ERR_NOT_ON_CURVE, ERR_SCALAR, ERR_NOT_IN_SUBGROUP = -1, -2, -3, -4, -7
BLOB = B.BLOB_BYTES
INF48 = b"\xc0" + bytes(47)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=torch.uint8).cuda()[:len(b)]


def _host(t):
    return t.cpu().numpy().tobytes()


def _be(xs):
    return P.be(xs)


def _g1(xs):
    """[x]_1 for every x: 96-byte encodings, one oracle call."""
    return O.g1_mul_gen(CURVE, _be(xs), len(xs))


def _g1c(xs):
    return O.g1_compress(CURVE, _g1(xs), len(xs))


def _split(b, size):
    return [b[i:i + size] for i in range(0, len(b), size)]


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lag():
    return P.lagrange_scalars(TAU)


@pytest.fixture(scope="module")
def key(ctx, lag):
    return ctx.load_blob_proof_key(_g1(lag))


@pytest.fixture(scope="module")
def key_g(ctx):
    """Every point the generator."""
    return ctx.load_blob_proof_key(_g1([1]) * B.N)


@pytest.fixture(scope="module")
def key_alt(ctx):
    """G, -G, G, -G, ..."""
    return ctx.load_blob_proof_key(_g1([1, R - 1]) * (B.N // 2))


@pytest.fixture(scope="module")
def data(lag):
    """Three random blobs, opened as blobref does: vals, blob, C, z, y, pi."""
    rng = random.Random(0x4844_9207)
    out = []
    for _ in range(3):
        vals = [rng.randrange(R) for _ in range(B.N)]
        blob, c48, z, y, pi = B.open_blob(vals, TAU)
        out.append({"vals": vals, "blob": blob, "C": c48, "z": z, "y": y, "pi": pi})
    return out


# the z set of the issue: off the domain, on it at thread/pass boundaries of the quotient kernel
# (513 = thread 1, pass 1), and the ends of the field
Z_FIRST = [0x1234_5678_9ABC_DEF0_4844 << 100, B.DOM[0], B.DOM[4095]]
Z_SECOND = [B.DOM[513], 0, R - 1]


# ------------------------------------------------------------------------------ stage: the quotient
@pytest.mark.parametrize("zs", [Z_FIRST, Z_SECOND], ids=["off-dom0-dom4095", "dom513-0-rm1"])
def test_quotient_against_the_model(ctx, data, zs):
    """Blobs on and off the domain in one launch."""
    assert B.DOM[1] == R - 1  # r - 1 is a domain point as well
    blobs = [data[i]["blob"] for i in range(3)]
    ys, q = ctx.blob_quotient(_dev(b"".join(blobs)), _dev(_be(zs)), 3)
    got_y, got_q = _split(_host(ys), 32), _split(_host(q), BLOB)
    for i, z in enumerate(zs):
        y, want = P.quotient(data[i]["vals"], z)
        assert got_y[i] == y.to_bytes(32, "big"), i
        assert got_q[i] == _be(want), i


def test_quotient_of_constant_and_maximal_blobs(ctx):
    c = 0x0123_4567_89AB_CDEF << 180
    kinds = [[c] * B.N, [R - 1] * B.N]
    zs = [Z_FIRST[0], B.DOM[64], Z_FIRST[0], B.DOM[64]]
    vals = [kinds[0], kinds[0], kinds[1], kinds[1]]
    ys, q = ctx.blob_quotient(_dev(b"".join(B.blob_from_ints(v) for v in vals)), _dev(_be(zs)), 4)
    assert _host(ys) == _be([c, c, R - 1, R - 1])
    assert _host(q) == bytes(4 * BLOB)  # q = 0 everywhere
    for v, z in zip(vals[1:3], zs[1:3]):
        assert P.quotient(v, z) == (v[0], [0] * B.N)


# ------------------------------------------------------------------------------ stage: the bare MSM
def test_msm_every_join_doubles(ctx, key_g):
    """All points G, all scalars 1: every tree join, in the block and across blocks, is P + P."""
    got = ctx.blob_commit(key_g, _dev(B.blob_from_ints([1] * B.N)), 1)
    assert _host(got) == B.g1_of(4096)


def test_msm_every_first_join_cancels(ctx, key_alt):
    """Points G, -G alternating, all scalars 7: every first join is P + (-P)."""
    got = ctx.blob_commit(key_alt, _dev(B.blob_from_ints([7] * B.N)), 1)
    assert _host(got) == INF48


DIGIT_VALUES = [1, 8, 9, int("8" * 63, 16), 1 << 252, R - 1]
DIGIT_INDICES = [0, 63, 64, 4095]  # first and last base of a chunk, first and last chunk


@pytest.mark.parametrize("v", DIGIT_VALUES, ids=["1", "8", "9", "0x88..8", "2^252", "r-1"])
def test_msm_digit_recoding(ctx, key_g, v):
    assert v < R
    blobs = []
    for j in DIGIT_INDICES:
        vals = [0] * B.N
        vals[j] = v
        blobs.append(B.blob_from_ints(vals))
    got = _host(ctx.blob_commit(key_g, _dev(b"".join(blobs)), len(blobs)))
    assert got == B.g1_of(v) * len(blobs)


# ------------------------------------------------------------------------------ stage: commitments
def test_commit_unit_vectors_give_the_key_points(ctx, key, lag):
    idx = [0, 1, 2049, 4095]
    blobs = []
    for j in idx:
        vals = [0] * B.N
        vals[j] = 1
        blobs.append(B.blob_from_ints(vals))
    got = _host(ctx.blob_commit(key, _dev(b"".join(blobs)), len(idx)))
    assert got == _g1c([lag[j] for j in idx])  # table row 0 of every base asked


def test_commit_ones_and_zero(ctx, key):
    raw = B.blob_from_ints([1] * B.N) + bytes(BLOB)
    assert _host(ctx.blob_commit(key, _dev(raw), 2)) == B.g1_of(1) + INF48


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_commit_random_blobs(ctx, key, lag, data, nb):
    got = _host(ctx.blob_commit(key, _dev(b"".join(d["blob"] for d in data[:nb])), nb))
    assert got == _g1c([P.commit_scalar(d["vals"], lag) for d in data[:nb]])
    assert got == b"".join(d["C"] for d in data[:nb])  # blobref's p(tau) G


# ------------------------------------------------------------------------------ end to end
def test_compute_kzg_proofs(ctx, key, lag, data):
    zs = Z_FIRST + Z_SECOND
    vals = [data[i % 3]["vals"] for i in range(len(zs))]
    raw = b"".join(data[i % 3]["blob"] for i in range(len(zs)))
    want = [P.proof_scalar(v, z, lag) for v, z in zip(vals, zs)]
    proofs, ys = ctx.compute_kzg_proofs(key, _dev(raw), _dev(_be(zs)), len(zs))
    assert _host(ys) == _be([y for y, _ in want])
    assert _host(proofs) == _g1c([s for _, s in want])


@pytest.mark.parametrize("nb", [1, 3])
def test_compute_blob_proofs(ctx, key, data, nb):
    raw, cs = b"".join(d["blob"] for d in data[:nb]), b"".join(d["C"] for d in data[:nb])
    got = _host(ctx.compute_blob_proofs(key, _dev(raw), _dev(cs), nb))
    assert got == b"".join(d["pi"] for d in data[:nb])


def test_round_trip_through_the_verifier(ctx, key, data):
    C = pc.CURVES[CURVE]
    g2 = pk.g2_to_bytes(C.g2, C)
    srs = ctx.load_srs(CURVE, g2, O.g2_mul(CURVE, g2, TAU))
    nb = 3
    raw = b"".join(d["blob"] for d in data[:nb])
    d_blobs = _dev(raw)
    cs = ctx.blob_commit(key, d_blobs, nb)
    proofs = ctx.compute_blob_proofs(key, d_blobs, cs, nb)
    assert ctx.verify_blob_batch(srs, d_blobs, cs, proofs, nb) is True
    bad = bytearray(raw)
    o = BLOB + 32 * 2049
    bad[o:o + 32] = ((int.from_bytes(bad[o:o + 32], "big") + 1) % R).to_bytes(32, "big")
    assert ctx.verify_blob_batch(srs, _dev(bytes(bad)), cs, proofs, nb) is False


# ------------------------------------------------------------------------------ forms
def test_host_device_and_async_forms_agree(ctx, key, data):
    import kzgmi
    import torch
    nb = 2
    raw, cs = b"".join(d["blob"] for d in data[:nb]), b"".join(d["C"] for d in data[:nb])
    zs = _be([Z_FIRST[0], B.DOM[513]])
    d_blobs, d_cs, d_zs = _dev(raw), _dev(cs), _dev(zs)
    want_c = _host(ctx.blob_commit(key, d_blobs, nb))
    want_p, want_y = (_host(t) for t in ctx.compute_kzg_proofs(key, d_blobs, d_zs, nb))
    want_b = _host(ctx.compute_blob_proofs(key, d_blobs, d_cs, nb))
    assert want_c == cs and want_b == b"".join(d["pi"] for d in data[:nb])
    # host forms: bytes in, bytes out
    assert ctx.blob_commit(key, raw) == want_c
    assert ctx.compute_kzg_proofs(key, bytearray(raw), zs, nb) == (want_p, want_y)
    assert ctx.compute_blob_proofs(key, raw, cs) == want_b
    assert kzgmi.blob_commit(key, raw) == want_c
    assert kzgmi.compute_kzg_proofs(key, raw, zs) == (want_p, want_y)
    assert kzgmi.compute_blob_proofs(key, raw, cs) == want_b
    # async on slot 1, into the caller's tensors
    out = torch.zeros(48 * nb, dtype=torch.uint8, device="cuda")
    ys = torch.zeros(32 * nb, dtype=torch.uint8, device="cuda")
    ctx.blob_commit_async(key, 1, d_blobs, nb, out)
    with pytest.raises(kzgmi.KzgmiError) as e:  # slot 1 is busy
        ctx.blob_commit_async(key, 1, d_blobs, nb, out)
    assert e.value.code == ERR_ARG
    assert ctx.wait(1) is True
    assert _host(out) == want_c
    ctx.compute_kzg_proofs_async(key, 1, d_blobs, d_zs, nb, out, ys)
    assert ctx.wait(1) is True
    assert (_host(out), _host(ys)) == (want_p, want_y)
    ctx.compute_blob_proofs_async(key, 1, d_blobs, d_cs, nb, out)
    assert ctx.wait(1) is True
    assert _host(out) == want_b
    same = ctx.blob_commit(key, d_blobs, nb, out=out)
    assert same is out and _host(out) == want_c


def test_two_jobs_in_flight(ctx, key, data):
    import torch
    nb = 3
    raw, cs = b"".join(d["blob"] for d in data[:nb]), b"".join(d["C"] for d in data[:nb])
    d_blobs, d_cs = _dev(raw), _dev(cs)
    out0 = torch.zeros(48 * nb, dtype=torch.uint8, device="cuda")
    out1 = torch.zeros(48 * nb, dtype=torch.uint8, device="cuda")
    ctx.compute_blob_proofs_async(key, 0, d_blobs, d_cs, nb, out0)
    ctx.blob_commit_async(key, 1, d_blobs, nb, out1)
    assert ctx.wait(1) is True
    assert ctx.wait(0) is True
    assert _host(out0) == b"".join(d["pi"] for d in data[:nb])
    assert _host(out1) == cs


def test_second_call_allocates_nothing(ctx, key, data):
    import kzgmi
    nb = 2
    raw, cs = b"".join(d["blob"] for d in data[:nb]), b"".join(d["C"] for d in data[:nb])
    d_blobs, d_cs, d_zs = _dev(raw), _dev(cs), _dev(_be([5, B.DOM[0]]))

    def calls():
        ctx.blob_commit(key, d_blobs, nb)
        ctx.compute_kzg_proofs(key, d_blobs, d_zs, nb)
        ctx.compute_blob_proofs(key, d_blobs, d_cs, nb)
        ctx.compute_blob_proofs(key, raw, cs, nb)
        ctx.blob_quotient(d_blobs, d_zs, nb)

    calls()
    before = kzgmi.alloc_count()
    calls()
    assert kzgmi.alloc_count() == before


# ------------------------------------------------------------------------------ errors
def _calls(ctx, key, d_blobs, d_zs, d_cs, nb, out, ys):
    """The three device forms, writing into out (and ys)."""
    return [lambda: ctx.blob_commit(key, d_blobs, nb, out=out),
            lambda: ctx.compute_kzg_proofs(key, d_blobs, d_zs, nb, out=out, ys_out=ys),
            lambda: ctx.compute_blob_proofs(key, d_blobs, d_cs, nb, out=out)]


def _pattern(nb):
    import torch
    return (torch.full((48 * nb,), 0xAA, dtype=torch.uint8, device="cuda"),
            torch.full((32 * nb,), 0xAA, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("which,index", [(0, 0), (1, 4095)])
def test_element_out_of_range(ctx, key, data, which, index):
    """A blob element equal to r: KZGMI_ERR_SCALAR from all three calls, in the device, host and async
    forms; nothing is written, and the slot works afterwards."""
    import kzgmi
    nb = 2
    raw, cs = b"".join(d["blob"] for d in data[:nb]), b"".join(d["C"] for d in data[:nb])
    zs = _be([Z_FIRST[0], B.DOM[0]])
    bad = bytearray(raw)
    o = which * BLOB + 32 * index
    bad[o:o + 32] = R.to_bytes(32, "big")
    bad = bytes(bad)
    out, ys = _pattern(nb)
    d_bad, d_zs, d_cs = _dev(bad), _dev(zs), _dev(cs)
    host = [lambda: ctx.blob_commit(key, bad), lambda: ctx.compute_kzg_proofs(key, bad, zs),
            lambda: ctx.compute_blob_proofs(key, bad, cs)]
    for call in _calls(ctx, key, d_bad, d_zs, d_cs, nb, out, ys) + host:
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == ERR_SCALAR
    ctx.blob_commit_async(key, 1, d_bad, nb, out)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.wait(1)
    assert e.value.code == ERR_SCALAR
    assert _host(out) == b"\xaa" * (48 * nb) and _host(ys) == b"\xaa" * (32 * nb)
    assert _host(ctx.blob_commit(key, _dev(raw), nb)) == cs
    ctx.blob_commit_async(key, 1, _dev(raw), nb, out)
    assert ctx.wait(1) is True and _host(out) == cs


def test_z_out_of_range(ctx, key, data):
    import kzgmi
    nb = 2
    raw = b"".join(d["blob"] for d in data[:nb])
    zs = _be([5]) + R.to_bytes(32, "big")
    out, ys = _pattern(nb)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.compute_kzg_proofs(key, _dev(raw), _dev(zs), nb, out=out, ys_out=ys)
    assert e.value.code == ERR_SCALAR
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.compute_kzg_proofs(key, raw, zs, nb)
    assert e.value.code == ERR_SCALAR
    assert _host(out) == b"\xaa" * (48 * nb) and _host(ys) == b"\xaa" * (32 * nb)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.blob_quotient(_dev(raw), _dev(zs), nb)
    assert e.value.code == ERR_SCALAR


def _x_off_curve():
    """A compressed encoding whose x has no y on the curve."""
    p = pc.CURVES[CURVE].p
    x = 1
    while pow((x * x * x + 4) % p, (p - 1) // 2, p) == 1:
        x += 1
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    return bytes(b)


def test_bad_commitments(ctx, key, data):
    import kzgmi
    nb = 2
    raw, cs = b"".join(d["blob"] for d in data[:nb]), b"".join(d["C"] for d in data[:nb])
    noflag = bytearray(cs)
    noflag[48] &= 0x7F  # compression bit missing
    outside = pk.g1_to_bytes_compressed(non_subgroup_points(1)[0], pc.BLS12_381)
    cases = [(bytes(noflag), ERR_ENCODING), (cs[:48] + _x_off_curve(), ERR_NOT_ON_CURVE),
             (outside + cs[48:], ERR_NOT_IN_SUBGROUP)]
    out, _ = _pattern(nb)
    d_blobs = _dev(raw)
    for bad, code in cases:
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.compute_blob_proofs(key, d_blobs, _dev(bad), nb, out=out)
        assert e.value.code == code
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.compute_blob_proofs(key, raw, bad, nb)
        assert e.value.code == code
    assert _host(out) == b"\xaa" * (48 * nb)
    assert _host(ctx.compute_blob_proofs(key, d_blobs, _dev(cs), nb)) == b"".join(d["pi"] for d in data[:nb])


def test_key_errors(ctx, key, data):
    import kzgmi
    good = _g1([1, 2, 3, 4]) * (B.N // 4)
    inf = bytearray(good)
    inf[96 * 7:96 * 8] = b"\x40" + bytes(95)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.load_blob_proof_key(bytes(inf))
    assert e.value.code == ERR_ARG
    out = bytearray(good)
    out[96 * 4095:96 * 4096] = pk.g1_to_bytes(non_subgroup_points(1, seed=7)[0], pc.BLS12_381)
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.load_blob_proof_key(bytes(out))
    assert e.value.code == ERR_NOT_IN_SUBGROUP
    off = bytearray(good)
    off[96 * 4000 + 95] ^= 1  # y + 1: off the curve
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.load_blob_proof_key(bytes(off))
    assert e.value.code == ERR_NOT_ON_CURVE
    with pytest.raises(ValueError):
        ctx.load_blob_proof_key(good[:-96])
    # a key of another context
    other = kzgmi.Context(0, 1)
    try:
        with pytest.raises(kzgmi.KzgmiError) as e:
            other.blob_commit(key, _dev(data[0]["blob"]), 1)
        assert e.value.code == ERR_ARG
        with pytest.raises(kzgmi.KzgmiError) as e:
            other.blob_commit(key, data[0]["blob"], 1)
        assert e.value.code == ERR_ARG
    finally:
        other.close()
    # 64 windows x 8 multiples per point, affine rows of 96 B in 128 B slots, and one flag byte per point
    assert key.device_bytes == 4096 * 64 * 8 * 128 + 4096
    assert _host(ctx.blob_commit(key, _dev(data[0]["blob"]), 1)) == data[0]["C"]


def test_argument_errors(ctx, key, data):
    import kzgmi
    import torch
    L = kzgmi.lib()
    # too many blobs, checked before anything is read
    for rc in (L.kzgmi_blob_commit_device(ctx.handle, key.handle, 16, 4097, 1 << 30),
               L.kzgmi_compute_kzg_proofs_device(ctx.handle, key.handle, 16, 1 << 29, 4097, 1 << 30, 1 << 31),
               L.kzgmi_compute_blob_proofs_device(ctx.handle, key.handle, 16, 1 << 29, 4097, 1 << 30),
               L.kzgmi_blob_quotient_device(ctx.handle, 16, 1 << 29, 4097, 1 << 30, 1 << 31)):
        with pytest.raises(kzgmi.KzgmiError) as e:
            kzgmi._check(rc)
        assert e.value.code == ERR_ARG
    nb = 1
    raw, cs = data[0]["blob"], data[0]["C"]
    zs = _be([5])
    out, ys = _pattern(nb)
    # a misaligned device pointer, input or output
    shifted = _dev(bytes(1) + raw)[1:]
    assert shifted.data_ptr() % 16 == 1
    wide = torch.full((64,), 0xAA, dtype=torch.uint8, device="cuda")
    for call in _calls(ctx, key, shifted, _dev(zs), _dev(cs), nb, out, ys) + \
            _calls(ctx, key, _dev(raw), _dev(zs), _dev(cs), nb, wide[8:56], ys):
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == ERR_ARG
    # an output that overlaps an input, or the other output
    d_blobs = _dev(raw)
    both = torch.full((96,), 0xAA, dtype=torch.uint8, device="cuda")
    for call in _calls(ctx, key, d_blobs, _dev(zs), _dev(cs), nb, d_blobs[BLOB - 48:], ys) + \
            [lambda: ctx.compute_kzg_proofs(key, d_blobs, _dev(zs), nb, out=both[:48], ys_out=both[32:64]),
             lambda: ctx.compute_kzg_proofs(key, d_blobs, both[:32], nb, out=both[:48], ys_out=both[64:])]:
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == ERR_ARG
    assert _host(d_blobs) == raw
    assert _host(out) == b"\xaa" * 48 and _host(ys) == b"\xaa" * 32 and _host(wide) == b"\xaa" * 64
    # nb = 0 succeeds and writes nothing
    assert ctx.blob_commit(key, b"", 0) == b""
    assert ctx.compute_kzg_proofs(key, b"", b"", 0) == (b"", b"")
    assert ctx.compute_blob_proofs(key, b"", b"", 0) == b""
    ctx.blob_commit_async(key, 1, d_blobs, 0, out)
    assert ctx.wait(1) is True
    assert _host(out) == b"\xaa" * 48
    # not a blob proof key
    with pytest.raises(kzgmi.KzgmiError) as e:
        ctx.blob_commit("key", raw, 1)
    assert e.value.code == ERR_ARG
    assert _host(ctx.blob_commit(key, d_blobs, nb, out=out)) == cs
