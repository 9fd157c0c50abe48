"""The rules a slot's pending job imposes on what may follow it (csrc/host.hpp JobKind): who may
chain behind whom, which wait collects which job, what an empty call leaves behind.

One context with two slots; slot 1 is walked through every job kind in sequence on the n = 16
golden batch (the smallest that takes the real path), and every verdict, point and combination is
the C oracle's.
"""
import struct

import pytest

pytestmark = pytest.mark.gpu

import cellref as K  # noqa: E402
import fk20ref as F  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

CURVE = "bls12_381"
TAU = 0x7594_0000_1234_5678_9ABC_DEF1


def h(x):
    return bytes.fromhex(x)


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b) if len(b) else bytearray(16), dtype=torch.uint8).cuda()[:len(b)]


def _arg_error(kzgmi, text, call, *args, **kw):
    with pytest.raises(kzgmi.KzgmiError) as e:
        call(*args, **kw)
    assert e.value.code == -1 and text in str(e.value), str(e.value)


def test_slot_walks_every_job_kind(golden):
    import kzgmi
    g = golden("bls12_381_batch_n16.json")
    n, seed = g["n"], h(g["seed"])
    raw = {k: h(g[k]) for k in ("commitments", "zs", "ys", "proofs")}
    bad_ys = h(g["neg_flip_y"]["ys"])
    ok_o, A_o, B_o = O.batch_verify(CURVE, raw["commitments"], raw["zs"], raw["ys"], raw["proofs"], n, h(g["g2"]),
                                    h(g["tau_g2"]), seed, want_ab=True)
    bad_o, bA_o, bB_o = O.batch_verify(CURVE, raw["commitments"], raw["zs"], bad_ys, raw["proofs"], n, h(g["g2"]),
                                       h(g["tau_g2"]), seed, want_ab=True)
    assert ok_o is True and bad_o is False
    msm_o = O.msm_g1(CURVE, raw["commitments"], raw["zs"], n)  # the commitments weighted by the z_i
    inf_o = O.msm_g1(CURVE, b"", b"", 0)

    ctx = kzgmi.Context(0, 2)
    try:
        srs = ctx.load_srs(CURVE, h(g["g2"]), h(g["tau_g2"]))
        C, z, y, P = (_dev(raw[k]) for k in ("commitments", "zs", "ys", "proofs"))
        ybad, none = _dev(bad_ys), _dev(b"")
        rec = ctx.partial_bytes(CURVE)
        part, mpart = _dev(bytes(2 * rec)), _dev(bytes(rec))

        def verify(slot, ys=y):
            ctx.batch_verify_async(srs, slot, C, z, ys, P, n, seed=seed)

        # a batch partial, a batch combine chained behind it, one wait: the oracle's verdict (and the
        # partial records are the oracle's combination)
        ctx.batch_partial_async(srs, 1, C, z, y, P, n, 0, seed, part)
        ctx.batch_combine_async(srs, 1, part, 1)
        assert ctx.wait(1) is ok_o
        assert ctx.partial_encode(CURVE, part, 2) == [A_o, B_o]

        # an MSM partial, an MSM combine chained behind it: msm_wait gives the oracle's point
        ctx.msm_partial_async(CURVE, 1, C, z, n, mpart)
        ctx.msm_combine_async(CURVE, 1, mpart, 1)
        assert ctx.msm_wait(1) == msm_o

        # a combine chains only behind a partial of its own family; the refused call leaves the
        # partial pending and collectable
        ctx.batch_partial_async(srs, 1, C, z, y, P, n, 0, seed, part)
        _arg_error(kzgmi, "slot busy", ctx.msm_combine_async, CURVE, 1, mpart, 1)
        assert ctx.wait(1) is True
        ctx.msm_partial_async(CURVE, 1, C, z, n, mpart)
        _arg_error(kzgmi, "slot busy", ctx.batch_combine_async, srs, 1, part, 1)
        assert ctx.wait(1) is True
        assert ctx.batch_combine(srs, part, 1) is ok_o  # both records are intact
        assert ctx.msm_combine(CURVE, mpart, 1) == msm_o

        # msm_wait takes MSM results only: a pending verify stays collectable by wait
        verify(1)
        _arg_error(kzgmi, "slot has no pending MSM", ctx.msm_wait, 1)
        # ... and a second enqueue on the pending slot is refused
        _arg_error(kzgmi, "slot busy", verify, 1)
        _arg_error(kzgmi, "slot busy", ctx.msm_g1_async, CURVE, 1, C, z, n)
        assert ctx.wait(1) is ok_o
        _arg_error(kzgmi, "slot has no pending batch", ctx.wait, 1)

        # an empty call of each family accepts, and the next real job on the slot is still right
        csrs = ctx.load_cell_srs(*K.toy_cell_srs(TAU))
        key = ctx.load_cell_proof_key(O.g1_mul_gen(CURVE, b"".join((x % K.R).to_bytes(32, "big")
                                                                   for x in F.srs_scalars(TAU)), 4096))
        idx64 = _dev(struct.pack("<64Q", *range(64)))
        empties = [
            lambda: ctx.batch_verify_async(srs, 1, none, none, none, none, 0, seed=seed),
            lambda: ctx.batch_partial_async(srs, 1, none, none, none, none, 0, 0, seed, part),
            lambda: ctx.msm_partial_async(CURVE, 1, none, none, 0, mpart),
            lambda: ctx.verify_blob_batch_async(srs, 1, none, none, none, 0),
            lambda: ctx.verify_cell_batch_async(csrs, 1, none, none, none, none, none, 0, 0),
            lambda: ctx.compute_cells_async(1, none, 0, none),
            lambda: ctx.recover_cells_async(1, idx64, none, 0, none),
            lambda: ctx.compute_cells_and_proofs_async(key, 1, none, 0, none, none),
        ]
        for k, empty in enumerate(empties):
            empty()
            assert ctx.wait(1) is True, k
            verify(1, ybad if k % 2 else y)
            assert ctx.wait(1) is (bad_o if k % 2 else ok_o), k
        ctx.msm_g1_async(CURVE, 1, none, none, 0)
        assert ctx.msm_wait(1) == inf_o
        ctx.msm_g1_async(CURVE, 1, C, z, n)
        assert ctx.msm_wait(1) == msm_o

        # a slot-0 utility call between two verifies on slot 0 leaves the second one's verdict and
        # combination the oracle's
        blob, z1 = _dev(bytes(4096 * 32)), _dev((5).to_bytes(32, "big"))
        cidx, cell = _dev(struct.pack("<Q", 3)), _dev(bytes(2048))
        utilities = [lambda: ctx.blob_eval(blob, z1, 1), lambda: ctx.cell_interp(cidx, cell, 1, 7)]
        for utility in utilities:
            verify(0, ybad)
            assert ctx.wait(0) is bad_o
            utility()
            verify(0)
            assert ctx.wait(0) is ok_o
            assert ctx.last_combination(CURVE) == (A_o, B_o)

        # after all of that, a corrupted batch is still rejected, with the oracle's combination
        verify(1, ybad)
        assert ctx.wait(1) is bad_o
        verify(0, ybad)
        assert ctx.wait(0) is bad_o
        assert ctx.last_combination(CURVE) == (bA_o, bB_o)
    finally:
        ctx.close()
