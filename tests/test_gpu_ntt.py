"""Power-of-two transforms over Fr on the GPU (kzgmi_fr_ntt*) against the big-integer model
(tests/nttref.py), bit for bit: every size across the one-pass / two-pass boundary, plans of many passes
at small sizes (KZGMI_NTT_PASS_BITS), batches, in place, the three forms, errors, a closed-form input at
2^20, the full size 2^26 and the tie to the shipped EIP-7594 transforms.
"""
import ctypes
import itertools
import random

import pytest

pytestmark = pytest.mark.gpu

import nttplanprobe as P  # noqa: E402
import nttref as N  # noqa: E402

CURVES = ["bls12_381", "bn254"]
B = P.constants()["max_bits"]  # the shipped most bits of one pass
COMBOS = list(itertools.product((False, True), (False, True)))  # (inverse, bitrev)


@pytest.fixture(scope="module")
def ctx():
    import kzgmi
    c = kzgmi.Context(0, 2)
    yield c
    c.close()


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b or bytes(32)), dtype=torch.uint8).cuda()[:len(b)]


def _host(t):
    return t.cpu().numpy().tobytes()


def _model(curve, vals, logn, inverse, bitrev, shift):
    return N.dft(vals, logn, N.MODULUS[curve], N.GENERATOR[curve], inverse=inverse, bitrev=bitrev, shift=shift or 1)


def _raw(ctx, curve, d_in, logn, count, flags, shift, d_out, slot=None):
    """the C entry point itself (device form, or the async form on `slot`): its return code"""
    import kzgmi
    ctx._order(slot or 0)
    if slot is None:
        return kzgmi.lib().kzgmi_fr_ntt_device(ctx.handle, kzgmi.CURVES[curve], d_in, logn, count, flags, shift, d_out)
    return kzgmi.lib().kzgmi_fr_ntt_device_async(ctx.handle, kzgmi.CURVES[curve], slot, d_in, logn, count, flags, shift, d_out)


def _special_inputs(r, n):
    yield [0] * n
    yield [r - 1] * n
    for at in sorted({0, n // 2, n - 1}):
        v = [0] * n
        v[at] = 0x1234567 % r or 1
        yield v


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", range(0, B + 3))
def test_sizes_against_the_model(ctx, curve, logn):
    r = N.MODULUS[curve]
    n = 1 << logn
    rng = random.Random(1000 + logn)
    inputs = [[rng.randrange(r) for _ in range(n)]]
    if logn in (0, 1, B, B + 1):
        inputs += list(_special_inputs(r, n))
    shift = rng.randrange(1, r)
    for vals in inputs:
        d_in = _dev(N.to_bytes(vals))
        for (inverse, bitrev), s in itertools.product(COMBOS, (None, shift)):
            got = ctx.fr_ntt(curve, d_in, logn, inverse=inverse, bitrev=bitrev, shift=s)
            assert _host(got) == N.to_bytes(_model(curve, vals, logn, inverse, bitrev, s)), (logn, inverse, bitrev, s)


@pytest.mark.parametrize("bits", [2, 3, 5])
def test_many_passes_at_small_sizes(ctx, bits, monkeypatch):
    """KZGMI_NTT_PASS_BITS bounds a pass: up to six passes and uneven widths below 2^12 points"""
    import kzgmi
    for name, value in {"KZGMI_NTT_PASS_BITS": str(bits)}.items():  # read when the context is created
        monkeypatch.setenv(name, value)
    c = kzgmi.Context(0, 1)
    try:
        for curve, logn in itertools.product(CURVES, range(1, 12)):
            r = N.MODULUS[curve]
            rng = random.Random(2000 + 16 * bits + logn)
            vals = [rng.randrange(r) for _ in range(1 << logn)]
            d_in = _dev(N.to_bytes(vals))
            for (inverse, bitrev), s in itertools.product(COMBOS, (None, rng.randrange(1, r))):
                got = _host(c.fr_ntt(curve, d_in, logn, inverse=inverse, bitrev=bitrev, shift=s))
                assert got == N.to_bytes(_model(curve, vals, logn, inverse, bitrev, s)), (curve, logn, inverse, bitrev)
                assert got == _host(ctx.fr_ntt(curve, d_in, logn, inverse=inverse, bitrev=bitrev, shift=s))
    finally:
        c.close()


@pytest.mark.parametrize("tile", [10, 11, 12])
def test_every_tile_size(ctx, tile, monkeypatch):
    """KZGMI_NTT_TILE_BITS selects a workgroup's tile (2^tile elements, passes of at most tile - 2 bits):
    each of the three built sizes against the model across its own one-pass / two-pass boundary"""
    import kzgmi
    for name, value in {"KZGMI_NTT_TILE_BITS": str(tile)}.items():  # read when the context is created
        monkeypatch.setenv(name, value)
    c = kzgmi.Context(0, 1)
    try:
        for curve, (logn, count) in itertools.product(CURVES, ((3, 5), (tile - 2, 3), (tile - 1, 2), (tile, 1), (tile + 1, 1))):
            r = N.MODULUS[curve]
            rng = random.Random(2500 + 16 * tile + logn)
            vals = [rng.randrange(r) for _ in range(count << logn)]
            d_in = _dev(N.to_bytes(vals))
            for (inverse, bitrev), s in itertools.product(COMBOS, (None, rng.randrange(1, r))):
                got = _host(c.fr_ntt(curve, d_in, logn, count=count, inverse=inverse, bitrev=bitrev, shift=s))
                want = b"".join(N.to_bytes(_model(curve, vals[t << logn:(t + 1) << logn], logn, inverse, bitrev, s))
                                for t in range(count))
                assert got == want, (curve, logn, inverse, bitrev)
    finally:
        c.close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [0, 1, 5, B, B + 1])
def test_batches(ctx, curve, logn):
    """transform t of a batch equals the single transform of its slice"""
    import torch
    r = N.MODULUS[curve]
    n = 1 << logn
    rng = random.Random(3000 + logn)
    torch.manual_seed(3000 + logn)
    data = torch.randint(0, 256, (65 * n, 32), dtype=torch.uint8, device="cuda")
    data[:, 0] &= 0x1F  # below 2^253 < r on both curves
    data = data.reshape(-1)
    shift = rng.randrange(1, r)
    singles = {}
    for count in (1, 2, 3, 65):
        for (inverse, bitrev), s in itertools.product(COMBOS, (None, shift)):
            got = ctx.fr_ntt(curve, data[:32 * n * count], logn, count=count, inverse=inverse, bitrev=bitrev, shift=s)
            for t in range(count):
                key = (t, inverse, bitrev, s)
                if key not in singles:
                    singles[key] = ctx.fr_ntt(curve, data[32 * n * t:32 * n * (t + 1)], logn, inverse=inverse, bitrev=bitrev,
                                              shift=s)
                assert torch.equal(got[32 * n * t:32 * n * (t + 1)], singles[key]), (count, t, inverse, bitrev)
    # and a slice of the batch against the model (the slices differ)
    vals = N.from_bytes(_host(data[32 * n * 64:32 * n * 65]))
    assert _host(singles[(64, False, True, shift)]) == N.to_bytes(_model(curve, vals, logn, False, True, shift))
    assert not torch.equal(singles[(0, False, False, None)], singles[(1, False, False, None)])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("logn", [3, B, B + 1, B + 2])
def test_in_place(ctx, curve, logn):
    import torch
    import kzgmi
    r = N.MODULUS[curve]
    n = 1 << logn
    rng = random.Random(4000 + logn)
    vals = [rng.randrange(r) for _ in range(2 * n)]
    shift = rng.randrange(1, r)
    for inverse, bitrev in COMBOS:
        src = _dev(N.to_bytes(vals))
        want = ctx.fr_ntt(curve, src, logn, count=2, inverse=inverse, bitrev=bitrev, shift=shift)
        assert _host(src) == N.to_bytes(vals)
        same = ctx.fr_ntt(curve, src, logn, count=2, inverse=inverse, bitrev=bitrev, shift=shift, out=src)
        assert same.data_ptr() == src.data_ptr() and torch.equal(src, want)
    # a partial overlap is refused
    buf = torch.zeros(32 * (2 * n + 1), dtype=torch.uint8, device="cuda")
    for a, b in ((buf[:64 * n], buf[32:]), (buf[32:], buf[:64 * n])):
        with pytest.raises(kzgmi.KzgmiError) as e:
            ctx.fr_ntt(curve, a, logn, count=2, out=b)
        assert e.value.code == -1


@pytest.mark.parametrize("curve", CURVES)
def test_forms_agree(ctx, curve):
    import torch
    import kzgmi
    r = N.MODULUS[curve]
    rng = random.Random(5000)
    for logn, count in ((4, 3), (B + 1, 2)):
        vals = [rng.randrange(r) for _ in range(count << logn)]
        shift = rng.randrange(1, r)
        for inverse, bitrev in COMBOS:
            host = ctx.fr_ntt(curve, N.to_bytes(vals), logn, count=count, inverse=inverse, bitrev=bitrev, shift=shift)
            assert isinstance(host, bytes)
            want = b"".join(N.to_bytes(_model(curve, vals[t << logn:(t + 1) << logn], logn, inverse, bitrev, shift))
                            for t in range(count))
            assert host == want
            d_in = _dev(N.to_bytes(vals))
            assert _host(ctx.fr_ntt(curve, d_in, logn, count=count, inverse=inverse, bitrev=bitrev, shift=shift)) == want
            out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
            ctx.fr_ntt_async(1, curve, d_in, logn, count=count, inverse=inverse, bitrev=bitrev, shift=shift, out=out)
            assert ctx.wait(1) is True
            assert _host(out) == want
    # a repeat of a call allocates nothing
    d_in = _dev(N.to_bytes(vals))
    ctx.fr_ntt(curve, d_in, B + 1, count=2, inverse=True, shift=shift)
    before = kzgmi.alloc_count()
    ctx.fr_ntt(curve, d_in, B + 1, count=2, inverse=True, shift=shift, out=out)
    assert kzgmi.alloc_count() == before


def test_two_async_jobs_in_flight(ctx):
    """two curves and sizes on two slots, both enqueued before either wait"""
    import torch
    rng = random.Random(5100)
    jobs = []
    for slot, (curve, logn, inverse, bitrev) in enumerate([("bls12_381", B + 2, False, True), ("bn254", 7, True, False)]):
        r = N.MODULUS[curve]
        vals = [rng.randrange(r) for _ in range(1 << logn)]
        shift = rng.randrange(1, r)
        jobs.append((curve, logn, inverse, bitrev, shift, _dev(N.to_bytes(vals)),
                     torch.zeros(32 << logn, dtype=torch.uint8, device="cuda"),
                     N.to_bytes(_model(curve, vals, logn, inverse, bitrev, shift))))
    for slot, (curve, logn, inverse, bitrev, shift, d_in, out, _) in enumerate(jobs):
        ctx.fr_ntt_async(slot, curve, d_in, logn, inverse=inverse, bitrev=bitrev, shift=shift, out=out)
    for slot in (1, 0):
        assert ctx.wait(slot) is True
        assert _host(jobs[slot][6]) == jobs[slot][7]


@pytest.mark.parametrize("curve", CURVES)
def test_errors(ctx, curve):
    import torch
    import kzgmi
    r = N.MODULUS[curve]
    rng = random.Random(6000)
    logn, count = 5, 3
    n = 1 << logn
    vals = [rng.randrange(r) for _ in range(count * n)]
    good = _dev(N.to_bytes(vals))
    want = b"".join(N.to_bytes(_model(curve, vals[t * n:(t + 1) * n], logn, False, False, None)) for t in range(count))
    out = torch.zeros(32 * count * n, dtype=torch.uint8, device="cuda")

    def still_works(slot=0):
        ctx.fr_ntt_async(slot, curve, good, logn, count=count, out=out)
        assert ctx.wait(slot) is True
        assert _host(out) == want

    def refused(code, call, slot=0):
        with pytest.raises(kzgmi.KzgmiError) as e:
            call()
        assert e.value.code == code
        still_works(slot)

    # a value >= r: at the first, a middle and the last place of the batch's last transform, one pass and two
    for ln, bad in itertools.product((logn, B + 1), (r, (1 << 256) - 1)):
        m = 1 << ln
        v = [rng.randrange(r) for _ in range(count * m)]
        for at in (2 * m, 2 * m + m // 2, 3 * m - 1):
            w = list(v)
            w[at] = bad
            d_bad = _dev(N.to_bytes(w))
            for inverse, bitrev in ((False, False), (True, True)):
                refused(-4, lambda: ctx.fr_ntt(curve, d_bad, ln, count=count, inverse=inverse, bitrev=bitrev))
    refused(-4, lambda: ctx.fr_ntt(curve, N.to_bytes(vals[:n - 1] + [r]), logn))  # host form
    ctx.fr_ntt_async(1, curve, _dev(N.to_bytes([r] + vals[1:])), logn, count=count, out=torch.zeros_like(out))
    with pytest.raises(kzgmi.KzgmiError) as e:  # the async form reports it at the wait
        ctx.wait(1)
    assert e.value.code == -4
    still_works(1)
    # the shift
    refused(-4, lambda: ctx.fr_ntt(curve, good, logn, count=count, shift=r))
    refused(-4, lambda: ctx.fr_ntt(curve, good, logn, count=count, shift=(1 << 256) - 1))
    refused(-1, lambda: ctx.fr_ntt(curve, good, logn, count=count, shift=0))
    # arguments (checked before anything is read: the arrays need not have the size asked for)
    p_in, p_out = good.data_ptr(), out.data_ptr()
    assert _raw(ctx, curve, p_in, 27, 1, 0, None, p_out) == -1
    assert _raw(ctx, curve, p_in, 10, (1 << 16) + 1, 0, None, p_out) == -1  # count n = 2^26 + n
    assert _raw(ctx, curve, p_in, logn, count, 4, None, p_out) == -1       # an unknown flag bit
    assert _raw(ctx, curve, p_in + 8, logn, count - 1, 0, None, p_out) == -1  # misaligned
    assert _raw(ctx, curve, p_in, logn, count, 0, None, p_out + 4) == -1
    assert _raw(ctx, curve, None, logn, count, 0, None, p_out) == -1
    assert _raw(ctx, curve, p_in, logn, count, 0, None, None) == -1
    assert _raw(ctx, curve, p_in, logn, count, 0, None, p_out, slot=1) == 0 and ctx.wait(1) is True
    assert _host(out) == want
    still_works()
    # count = 0 succeeds and writes nothing
    out.fill_(0xA5)
    assert _raw(ctx, curve, p_in, logn, 0, 0, None, p_out) == 0
    assert _raw(ctx, curve, p_in, logn, 0, 0, None, p_out, slot=1) == 0 and ctx.wait(1) is True
    assert ctx.fr_ntt(curve, b"", logn, count=0) == b""
    torch.cuda.synchronize()
    assert _host(out) == b"\xa5" * len(want)
    still_works()


def test_closed_form_at_2_20(ctx):
    """c_i = a^i + b^i plus three single coefficients e X^t: p(w^j) = (a^n - 1) / (a w^j - 1) + (b^n - 1) /
    (b w^j - 1) + sum e w^(t j), every j by one batch inversion.  Forward, natural order; the inverse
    returns the input."""
    curve, logn = "bls12_381", 20
    r, n = N.MODULUS[curve], 1 << 20
    rng = random.Random(7000)
    a, b = rng.randrange(2, r), rng.randrange(2, r)
    extra = [(rng.randrange(n), rng.randrange(1, r)) for _ in range(3)]
    coeffs, x, y = [], 1, 1
    for _ in range(n):
        coeffs.append((x + y) % r)
        x, y = x * a % r, y * b % r
    an, bn = (x - 1) % r, (y - 1) % r  # a^n - 1, b^n - 1
    for t, e in extra:
        coeffs[t] = (coeffs[t] + e) % r
    w = N.root(r, N.GENERATOR[curve], logn)
    wj, x = [], 1
    for _ in range(n):
        wj.append(x)
        x = x * w % r
    den = [(a * u - 1) % r for u in wj] + [(b * u - 1) % r for u in wj]
    assert all(den)
    pre, acc = [], 1
    for d in den:
        pre.append(acc)
        acc = acc * d % r
    inv = pow(acc, r - 2, r)
    for i in range(2 * n - 1, -1, -1):
        den[i], inv = inv * pre[i] % r, inv * den[i] % r
    want = bytearray(32 * n)
    for j in range(n):
        v = an * den[j] + bn * den[n + j]
        for t, e in extra:
            v += e * wj[t * j & (n - 1)]
        want[32 * j:32 * j + 32] = (v % r).to_bytes(32, "big")
    d_in = _dev(N.to_bytes(coeffs))
    got = ctx.fr_ntt(curve, d_in, logn)
    assert _host(got) == bytes(want)
    import torch
    assert torch.equal(ctx.fr_ntt(curve, got, logn, inverse=True), d_in)


def test_full_size_2_26(ctx):
    """count n = 2^26 on BN254 (the smaller 2-adicity): 2 GiB arrays, byte offsets above 2^31.  Forward
    then inverse is the identity, and one output above index 2^25 equals p(w^j) from the opening scan."""
    import torch
    curve, logn = "bn254", 26
    r, n = N.MODULUS[curve], 1 << 26
    torch.manual_seed(8000)
    data = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda")
    data[:, 0] &= 0x1F  # below 2^253 < r
    data = data.reshape(-1)
    ev = ctx.fr_ntt(curve, data, logn)
    j = (1 << 25) + 12345
    z = pow(N.root(r, N.GENERATOR[curve], logn), j, r)
    ys, q = ctx.open_quotient(curve, data, n, _dev(z.to_bytes(32, "big")), 1)
    assert torch.equal(ev[32 * j:32 * j + 32], ys)
    del q
    back = ctx.fr_ntt(curve, ev, logn, inverse=True, out=ev)
    assert torch.equal(back, data)


def test_tie_to_the_cell_transforms(ctx):
    """the blob's coefficients, their extension and its coset half against compute_cells"""
    curve = "bls12_381"
    r = N.MODULUS[curve]
    rng = random.Random(9000)
    blob = N.to_bytes([rng.randrange(r) for _ in range(4096)])
    cells = ctx.compute_cells(blob)
    coeffs = ctx.fr_ntt(curve, blob, 12, inverse=True, bitrev=True)
    assert ctx.fr_ntt(curve, coeffs + bytes(32 * 4096), 13, bitrev=True) == cells
    assert ctx.fr_ntt(curve, coeffs, 12, bitrev=True, shift=N.root(r, 7, 13)) == cells[131072:]
    assert cells[:131072] == blob
