"""Pure-Python restatement of the EIP-4844 blob transcript (Deneb polynomial-commitments,
verify_blob_kzg_proof_batch) that csrc/blob.hpp implements: hashlib, Python ints, Montgomery
batch inversion; G1 points from the C oracle.  Test infrastructure only.

  z_i = int_be(SHA256("FSBLOBVERIFY_V1_" || be128(4096) || blob_i || C_i)) mod r
  dom[i] = w^rev12(i), w = 7^((r-1)/4096)
  y_i = blob_i[j] if z_i == dom[j] else (z_i^4096 - 1)/4096 * sum_j blob_i[j] dom[j] / (z_i - dom[j])
  r = int_be(SHA256("RCKZGBATCH___V1_" || be64(4096) || be64(n) || (C_i || z_i || y_i || pi_i)_i)) mod r
"""
import hashlib

from oracle import oracle as O
from oracle.pyspec import curves as pc

CURVE = "bls12_381"
R = pc.CURVES[CURVE].r
N = 4096
BLOB_BYTES = 32 * N
BLOB_TAG = b"FSBLOBVERIFY_V1_"
BATCH_TAG = b"RCKZGBATCH___V1_"


def rev12(i):
    return int(format(i, "012b")[::-1], 2)


OMEGA = pow(7, (R - 1) // N, R)
DOM = [pow(OMEGA, rev12(i), R) for i in range(N)]
DOM_INDEX = {d: i for i, d in enumerate(DOM)}
INV_N = pow(N, -1, R)


def batch_inverse(xs):
    """Inverses of nonzero xs mod R with one modular inversion."""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for k in range(len(xs) - 1, -1, -1):
        out[k] = inv * pre[k] % R
        inv = inv * xs[k] % R
    return out


def blob_from_ints(vals):
    assert len(vals) == N
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def blob_to_ints(blob):
    assert len(blob) == BLOB_BYTES
    return [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(N)]


def evaluate(vals, z):
    """p(z) for p given by its values vals[j] = p(dom[j])."""
    j = DOM_INDEX.get(z % R)
    if j is not None:
        return vals[j]
    inv = batch_inverse([(z - d) % R for d in DOM])
    s = sum(v * d % R * i for v, d, i in zip(vals, DOM, inv)) % R
    return (pow(z, N, R) - 1) * INV_N % R * s % R


def blob_challenge(blob, c48):
    msg = BLOB_TAG + N.to_bytes(16, "big") + blob + c48
    assert len(msg) == 131152
    return int.from_bytes(hashlib.sha256(msg).digest(), "big") % R


def batch_challenge(cs, zs, ys, ps):
    """cs, ps: lists of 48-byte encodings; zs, ys: lists of ints."""
    n = len(cs)
    msg = BATCH_TAG + N.to_bytes(8, "big") + n.to_bytes(8, "big")
    for c, z, y, p in zip(cs, zs, ys, ps):
        msg += c + z.to_bytes(32, "big") + y.to_bytes(32, "big") + p
    assert len(msg) == 32 + 160 * n
    return int.from_bytes(hashlib.sha256(msg).digest(), "big") % R


def g1_of(k):
    """compress(k G1), 48 bytes."""
    return O.g1_compress(CURVE, O.g1_mul_gen(CURVE, (k % R).to_bytes(32, "big"), 1), 1)


def open_blob(vals, tau):
    """(blob, C, z, y, pi) of a valid opening under the toy secret tau (not a domain point):
    C = p(tau) G1, z the blob's challenge, y = p(z), pi = ((p(tau) - y)/(tau - z)) G1."""
    blob = blob_from_ints(vals)
    ptau = evaluate(vals, tau)
    c48 = g1_of(ptau)
    z = blob_challenge(blob, c48)
    y = evaluate(vals, z)
    q = (ptau - y) * pow((tau - z) % R, -1, R) % R
    return blob, c48, z, y, g1_of(q)


def decompress(points48):
    """Uncompressed encodings of a list of valid 48-byte encodings."""
    rc, out = O.g1_decompress(CURVE, b"".join(points48), len(points48))
    assert rc == 0
    return out
