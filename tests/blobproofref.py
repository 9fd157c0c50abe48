"""Pure-Python model of the EIP-4844 producer side that csrc/blobproof.hpp implements (Deneb
polynomial-commitments blob_to_kzg_commitment, compute_kzg_proof, compute_blob_kzg_proof), in the
exponent under a toy secret tau: Python ints and the helpers of tests/blobref.py.  Test
infrastructure only.

  l_j = l_j(tau) = (tau^4096 - 1)/4096 * dom[j] / (tau - dom[j])      (the Lagrange key's scalars)
  commitment = sum_j v_j l_j                                          (v_j = p(dom[j]))
  y = p(z),  q_j = (v_j - y) / (dom[j] - z),  proof = sum_j q_j l_j
  z = dom[m]:  y = v_m,  q_m = sum_{i != m} (v_i - y) dom[i] / (z (z - dom[i]))
"""
import blobref as B

R, N, DOM = B.R, B.N, B.DOM


def lagrange_scalars(tau):
    """l_j(tau) for every j; tau is no domain point."""
    tau %= R
    assert tau not in B.DOM_INDEX
    fac = (pow(tau, N, R) - 1) * B.INV_N % R
    inv = B.batch_inverse([(tau - d) % R for d in DOM])
    return [fac * d % R * i % R for d, i in zip(DOM, inv)]


def quotient(vals, z):
    """(y, q): y = p(z) and the evaluations on the domain of (p - y) / (X - z), as the specification's
    compute_kzg_proof_impl reads, with compute_quotient_eval_within_domain for z on the domain."""
    z %= R
    y = B.evaluate(vals, z)
    shifted = [(v - y) % R for v in vals]
    denom = [(d - z) % R for d in DOM]
    q = [0] * N
    m = B.DOM_INDEX.get(z)
    for j in range(N):
        if j == m:
            continue
        q[j] = shifted[j] * pow(denom[j], -1, R) % R
    if m is not None:
        acc = 0
        for i in range(N):
            if i == m:
                continue
            f_i = (vals[i] - y) % R
            numerator = f_i * DOM[i] % R
            denominator = z * ((z - DOM[i]) % R) % R
            acc = (acc + numerator * pow(denominator, -1, R)) % R
        q[m] = acc
    return y, q


def commit_scalar(vals, lag):
    """p(tau) = sum_j v_j l_j for lag = lagrange_scalars(tau)."""
    return sum(v * l for v, l in zip(vals, lag)) % R


def proof_scalar(vals, z, lag):
    """(y, sum_j q_j l_j)."""
    y, q = quotient(vals, z)
    return y, sum(a * l for a, l in zip(q, lag)) % R


def be(xs):
    return b"".join((x % R).to_bytes(32, "big") for x in xs)
