// EIP-7594 (PeerDAS) cell extension and recovery (compute_cells, recover_cells: the cells, not
// their proofs): a 4096-point number-theoretic transform over Fr with one workgroup per blob and
// the whole vector in LDS.  BLS12-381 only.  Reference: none (LICENSE only); the definitions are
// restated in include/kzgmi.h and tests/recoverref.py.
//
//   w = 7^((r-1)/8192), w2 = w^2; blob[k] = p(w2^rev12(k)); the extended blob, in cell order, is
//   ext[q] = p(w^rev13(q)), q < 8192: ext[k] = blob[k] and ext[4096 + k] = p(w w2^rev12(k)), k < 4096
//
// Two in-place transforms (radix-2 stages, two to a pass), both without a permutation pass:
//   ntt_dit_inv: x[k] in bit-reversed order -> X[m] = sum_k x[k] w2^(-rev12(k) m), natural order
//   ntt_dif_fwd: X[m] in natural order      -> x[k] = sum_m X[m] w2^(rev12(k) m), bit-reversed order
// compute_cells: c = dit_inv(blob); ext[4096 + .] = dif_fwd(c[m] w^m / 4096).
//
// recover_cells (the given cell indices are shared by every blob of the call).  Z(X) = prod over the
// missing cells i of (X^64 - h_i^64) depends on X^64 only: Zc[c] on cell c's points, and Zq[u] on
// the points 7 w2^e with e mod 64 = u.  D = p Z has degree < 8192 and D = E Z on the whole domain
// (E: the given cells, the missing ones zero).  With A = dit_inv(E Z on the even points) and
// B = dit_inv(E Z on the odd points), D's coefficients are d[m] = (A[m] + w^-m B[m]) / 8192 and
// d[m + 4096] = (A[m] - w^-m B[m]) / 8192.  p has degree < 4096, so the quotient is needed on 4096
// points only, the coset 7 w2^e:  D(7X) mod (X^4096 - 1) has coefficients
//   g[m] = 7^m (d[m] + 7^4096 d[m + 4096]) = GA[m] A[m] + GB[m] B[m]
// and dif_fwd(g)[k] = D(7 w2^rev12(k)); times Zq[rev6(k >> 6)]^-1 it is p there; dit_inv of that is
// 4096 7^m p[m].  Then p is extended as compute_cells does.  Six transforms per blob; HBM holds the
// input, the output, and A and later p parked in the output's second half until it is final (the
// registers of a 1024-thread workgroup are short).  The result always has degree < 4096, so the input is
// consistent exactly when the result's cells equal the given ones: compared as they are written.
//
// Elements stay in standard form throughout: every product is (standard) x (Montgomery table).
// LDS layout: limb-planar, limb q of element i at word 4096 q + i, so in the passes with a span of
// 64 or more a wave's 64 threads read 64 consecutive words.
#pragma once
#include "cell.hpp"

namespace kzgmi {

constexpr uint32_t NTT_N = BLOB_N;             // 4096
constexpr uint32_t NTT_EXT = 2 * NTT_N;        // 8192 elements of an extended blob
constexpr int NTT_THREADS = 1024;              // one workgroup per blob; thread t owns elements t + 1024 q
constexpr int NTT_PER = NTT_N / NTT_THREADS;   // elements per thread
constexpr int NTT_GROUPS = NTT_PER / 4;        // radix-4 groups per thread and pass
// the transform table (Montgomery), once per context:
//   w^e, e < 8192 | GA[m] = 7^m (1 + 7^4096) / 8192 | GB[m] = 7^m (1 - 7^4096) w^-m / 8192 |
//   PI[m] = 7^-m / 4096 | CW[m] = w^m / 4096          (m < 4096)
constexpr uint32_t NTT_T_TW = 0, NTT_T_GA = NTT_EXT, NTT_T_GB = NTT_T_GA + NTT_N, NTT_T_PI = NTT_T_GB + NTT_N,
                   NTT_T_CW = NTT_T_PI + NTT_N, NTT_TABLE = NTT_T_CW + NTT_N;
// the per-call table of recover_cells: Zc[c], c < 128 | Zq[u]^-1, u < 64 (Montgomery), then
// pos[c], c < 128 (int32): cell c's place among the given cells, -1 if missing
constexpr uint32_t REC_Z_C = 0, REC_Z_Q = CELL_COSETS, REC_Z_F = CELL_COSETS + CELL_N;
constexpr size_t REC_Z_BYTES = REC_Z_F * sizeof(BlobF) + CELL_COSETS * sizeof(int32_t);

KZ_DEV BlobF ntt_pow(BlobF x, uint32_t e, int bits) {
  BlobF acc = BlobF::one();
  for (int k = 0; k < bits; ++k) {
    if ((e >> k) & 1) acc = fp_mul(acc, x);
    x = fp_sqr(x);
  }
  return acc;
}

KZ_DEV BlobF ntt_small(uint32_t v) {  // the small integer v, Montgomery
  BlobF x = BlobF::zero();
  x.v[0] = v;
  return fp_to_mont(x);
}

// the transform table: NTT_TABLE threads
static __global__ void __launch_bounds__(256) k_ntt_table(BlobF* __restrict__ table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NTT_TABLE) return;
  if (i < NTT_T_GA) {
    table[i] = cell_root_pow(i);
    return;
  }
  const uint32_t m = (i - NTT_T_GA) & (NTT_N - 1), reg = (i - NTT_T_GA) / NTT_N;
  const BlobF seven = ntt_small(7);
  BlobF v;
  if (reg <= 1) {
    const BlobF s = ntt_pow(seven, NTT_N, 13);  // 7^4096
    v = fp_mul(ntt_pow(seven, m, 12), fp_inv_c(ntt_small(NTT_EXT)));
    if (reg == 0) v = fp_mul(v, fp_add(BlobF::one(), s));
    else v = fp_mul(fp_mul(v, fp_sub(BlobF::one(), s)), cell_root_pow((NTT_EXT - m) & (NTT_EXT - 1)));
  } else if (reg == 2) {
    v = fp_inv_c(fp_mul(ntt_pow(seven, m, 12), ntt_small(NTT_N)));
  } else {
    v = fp_mul(cell_root_pow(m), fp_inv_c(ntt_small(NTT_N)));
  }
  table[i] = v;
}

KZ_DEV BlobF ntt_ld(const uint32_t* x, uint32_t i) {
  BlobF r;
#pragma unroll
  for (int q = 0; q < 8; ++q) r.v[q] = x[NTT_N * q + i];
  return r;
}
KZ_DEV void ntt_st(uint32_t* x, uint32_t i, const BlobF& a) {
#pragma unroll
  for (int q = 0; q < 8; ++q) x[NTT_N * q + i] = a.v[q];
}

// Every thread of the workgroup calls these.  A pass is two radix-2 stages (spans h and 2h) on the
// four elements base + {0, h, 2h, 3h} in registers: a group belongs to one thread, so a pass costs
// one barrier, and 12 stages are six passes over LDS.  Both begin and end with a barrier.
KZ_DEV void ntt_dit_inv(uint32_t* x, const BlobF* __restrict__ tw) {
  const uint32_t t = threadIdx.x;
#pragma unroll 1
  for (uint32_t h = 1, sh = 12; h < NTT_N; h <<= 2, sh -= 2) {  // span h: w2^-(k N / 2h) = w^-(k << sh)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NTT_GROUPS; ++q) {
      const uint32_t g = t + NTT_THREADS * q, k = g & (h - 1), e0 = ((g - k) << 2) | k;
      const BlobF w1 = tw[(NTT_EXT - (k << sh)) & (NTT_EXT - 1)];
      const BlobF w2 = tw[(NTT_EXT - (k << (sh - 1))) & (NTT_EXT - 1)];
      const BlobF w3 = tw[(NTT_EXT - ((k + h) << (sh - 1))) & (NTT_EXT - 1)];
      const BlobF x0 = ntt_ld(x, e0), x2 = ntt_ld(x, e0 + 2 * h);
      const BlobF c1 = fp_mul(w1, ntt_ld(x, e0 + h)), c3 = fp_mul(w1, ntt_ld(x, e0 + 3 * h));
      const BlobF a0 = fp_add(x0, c1), a1 = fp_sub(x0, c1);
      const BlobF c2 = fp_mul(w2, fp_add(x2, c3)), d3 = fp_mul(w3, fp_sub(x2, c3));
      ntt_st(x, e0, fp_add(a0, c2));
      ntt_st(x, e0 + 2 * h, fp_sub(a0, c2));
      ntt_st(x, e0 + h, fp_add(a1, d3));
      ntt_st(x, e0 + 3 * h, fp_sub(a1, d3));
    }
  }
  __syncthreads();
}

KZ_DEV void ntt_dif_fwd(uint32_t* x, const BlobF* __restrict__ tw) {
  const uint32_t t = threadIdx.x;
#pragma unroll 1
  for (uint32_t h = NTT_N / 4, sh = 2; h >= 1; h >>= 2, sh += 2) {  // span h: w2^(k N / 2h) = w^(k << sh)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NTT_GROUPS; ++q) {
      const uint32_t g = t + NTT_THREADS * q, k = g & (h - 1), e0 = ((g - k) << 2) | k;
      const BlobF w1 = tw[k << sh], w2 = tw[k << (sh - 1)], w3 = tw[(k + h) << (sh - 1)];
      const BlobF x0 = ntt_ld(x, e0), x1 = ntt_ld(x, e0 + h), x2 = ntt_ld(x, e0 + 2 * h), x3 = ntt_ld(x, e0 + 3 * h);
      const BlobF a0 = fp_add(x0, x2), a1 = fp_add(x1, x3);
      const BlobF a2 = fp_mul(w2, fp_sub(x0, x2)), a3 = fp_mul(w3, fp_sub(x1, x3));
      ntt_st(x, e0, fp_add(a0, a1));
      ntt_st(x, e0 + h, fp_mul(w1, fp_sub(a0, a1)));
      ntt_st(x, e0 + 2 * h, fp_add(a2, a3));
      ntt_st(x, e0 + 3 * h, fp_mul(w1, fp_sub(a2, a3)));
    }
  }
  __syncthreads();
}

// compute_cells: workgroup b extends blob b.  out: 8192 x 32 B per blob, cell order; the first half
// is the blob itself.  Every element is range-checked at the load (DERR_SCALAR).
static __global__ void __launch_bounds__(NTT_THREADS) k_compute_cells(const uint8_t* __restrict__ blobs,
                                                                      const BlobF* __restrict__ table,
                                                                      uint8_t* __restrict__ out,
                                                                      uint32_t* __restrict__ err) {
  __shared__ uint32_t x[8 * NTT_N];
  const uint32_t t = threadIdx.x;
  const uint8_t* blob = blobs + (size_t)blockIdx.x * BLOB_BYTES;
  uint8_t* o = out + (size_t)blockIdx.x * 2 * BLOB_BYTES;
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t k = t + NTT_THREADS * q;
    uint32_t we[8];
    load_words(blob + (size_t)k * 32, we);
    BlobF e = fp_from_be_words<BlobR>(we, 0);
    if (!fp_raw_lt_mod(e)) {
      raise_err(err, DERR_SCALAR);
      e = BlobF::zero();
    }
    store_words(o + (size_t)k * 32, we);
    ntt_st(x, k, e);
  }
  ntt_dit_inv(x, table + NTT_T_TW);
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t m = t + NTT_THREADS * q;
    ntt_st(x, m, fp_mul(table[NTT_T_CW + m], ntt_ld(x, m)));
  }
  ntt_dif_fwd(x, table + NTT_T_TW);
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t k = t + NTT_THREADS * q;
    uint32_t wo[8];
    fp_to_be_words(ntt_ld(x, k), wo, 0);
    store_words(o + (size_t)(NTT_N + k) * 32, wo);
  }
}

// The per-call table of recover_cells, one workgroup: the place of every cell among the k given
// indices (an index >= 128 or a duplicate raises DERR_ARG), Zc and Zq^-1.  Each of the 192 values
// is a product over the missing cells; four threads take 32 candidate cells each (thread t: value
// t mod 192, part t / 192, so a wave has one part and skips the given cells together), which
// shortens the chain of dependent products from 64 to 32 + 2.  cell_table: cell.hpp's coset table
// (h_i^64); tw: w^e.
constexpr uint32_t REC_Z_PARTS = 4, REC_Z_THREADS = REC_Z_F * REC_Z_PARTS;  // 768
static __global__ void __launch_bounds__(REC_Z_THREADS) k_recover_z(const uint64_t* __restrict__ cell_indices,
                                                                    uint32_t k, const BlobF* __restrict__ cell_table,
                                                                    const BlobF* __restrict__ tw, BlobF* __restrict__ z,
                                                                    int32_t* __restrict__ pos,
                                                                    uint32_t* __restrict__ err) {
  __shared__ int32_t sp[CELL_COSETS];
  __shared__ BlobF part[REC_Z_THREADS];
  const uint32_t t = threadIdx.x;
  if (t < CELL_COSETS) sp[t] = -1;
  __syncthreads();
  for (uint32_t n = t; n < k; n += REC_Z_THREADS) {
    const uint64_t ci = cell_indices[n];
    if (ci >= CELL_COSETS) {
      raise_err(err, DERR_ARG);
    } else if (atomicExch(&sp[(uint32_t)ci], (int32_t)n) != -1) {
      raise_err(err, DERR_ARG);
    }
  }
  __syncthreads();
  if (t < CELL_COSETS) pos[t] = sp[t];
  const uint32_t v = t % REC_Z_F, pt = t / REC_Z_F;
  // X^64 at the value's points: h_v^64 on cell v, 7^64 w^(128 u) on the coset points with e mod 64 = u
  const BlobF x64 = v < REC_Z_Q ? cell_table[CELL_T_H64 + v]
                                : fp_mul(ntt_pow(ntt_small(7), CELL_N, 7), tw[2 * CELL_N * (v - REC_Z_Q)]);
  BlobF acc = BlobF::one();
  constexpr uint32_t PER = CELL_COSETS / REC_Z_PARTS;
  for (uint32_t i = PER * pt; i < PER * (pt + 1); ++i) {
    if (sp[i] >= 0) continue;  // wave-uniform
    acc = fp_mul(acc, fp_sub(x64, cell_table[CELL_T_H64 + i]));
  }
  part[t] = acc;
  __syncthreads();
  if (pt != 0) return;
  acc = fp_mul(fp_mul(acc, part[v + REC_Z_F]), fp_mul(part[v + 2 * REC_Z_F], part[v + 3 * REC_Z_F]));
  z[v] = v < REC_Z_Q ? acc : fp_inv_c(acc);  // Zq is never zero: 7^64 is no 128th root of unity
}

// One half of the extended blob out of LDS: element k of half h to out, compared with the given
// cell it belongs to (a difference raises DERR_ARG unless this blob had a range error).
KZ_DEV void recover_store(const uint32_t* x, uint32_t h, const uint8_t* __restrict__ in, const int32_t* __restrict__ pos,
                          uint8_t* __restrict__ o, bool skip_compare, uint32_t* __restrict__ err) {
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t k = t + NTT_THREADS * q, c = CELL_N * h + (k >> 6);
    uint32_t wo[8];
    fp_to_be_words(ntt_ld(x, k), wo, 0);
    store_words(o + (size_t)(NTT_N * h + k) * 32, wo);
    const int32_t p = pos[c];
    if (p >= 0 && !skip_compare) {
      uint32_t wi[8], d = 0;
      load_words(in + (size_t)p * CELL_BYTES + 32 * (k & (CELL_N - 1)), wi);
#pragma unroll
      for (int l = 0; l < 8; ++l) d |= wi[l] ^ wo[l];
      if (d) raise_err(err, DERR_ARG);
    }
  }
}

// recover_cells: workgroup b rebuilds blob b from its k given cells (cells: nb x k x 2048 B, in the
// order of the index array).  Every given element is range-checked at the load (DERR_SCALAR).
static __global__ void __launch_bounds__(NTT_THREADS) k_recover_cells(const uint8_t* __restrict__ cells, uint32_t k,
                                                                      const BlobF* __restrict__ table,
                                                                      const BlobF* __restrict__ z,
                                                                      const int32_t* __restrict__ pos,
                                                                      uint8_t* __restrict__ out,
                                                                      uint32_t* __restrict__ err) {
  __shared__ uint32_t x[8 * NTT_N];
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x;
  const uint8_t* in = cells + (size_t)blockIdx.x * k * CELL_BYTES;
  uint8_t* o = out + (size_t)blockIdx.x * 2 * BLOB_BYTES;
  const BlobF* tw = table + NTT_T_TW;
  if (t == 0) bad = 0;
  __syncthreads();
  // A, later p, wait in the second half of this blob's output (elements t + 1024 q, written and
  // read back by the same thread) until that half gets its final values: registers are short
  uint8_t* keep = o + (size_t)NTT_N * 32;
#pragma unroll 1
  for (uint32_t h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < NTT_PER; ++q) {
      const uint32_t kk = t + NTT_THREADS * q, c = CELL_N * h + (kk >> 6);
      const int32_t p = pos[c];
      BlobF e = BlobF::zero();
      if (p >= 0) {
        uint32_t we[8];
        load_words(in + (size_t)p * CELL_BYTES + 32 * (kk & (CELL_N - 1)), we);
        e = fp_from_be_words<BlobR>(we, 0);
        if (!fp_raw_lt_mod(e)) {
          raise_err(err, DERR_SCALAR);
          bad = 1;
          e = BlobF::zero();
        }
        e = fp_mul(z[REC_Z_C + c], e);
      }
      ntt_st(x, kk, e);
    }
    ntt_dit_inv(x, tw);
    if (h == 0) {
#pragma unroll
      for (int q = 0; q < NTT_PER; ++q) {
        const uint32_t m = t + NTT_THREADS * q;
        store_words(keep + (size_t)m * 32, ntt_ld(x, m).v);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t m = t + NTT_THREADS * q;
    BlobF a;
    load_words(keep + (size_t)m * 32, a.v);
    ntt_st(x, m, fp_add(fp_mul(table[NTT_T_GA + m], a), fp_mul(table[NTT_T_GB + m], ntt_ld(x, m))));
  }
  ntt_dif_fwd(x, tw);
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t kk = t + NTT_THREADS * q;
    ntt_st(x, kk, fp_mul(z[REC_Z_Q + (__brev(kk >> 6) >> 26)], ntt_ld(x, kk)));
  }
  ntt_dit_inv(x, tw);
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t m = t + NTT_THREADS * q;
    const BlobF pm = fp_mul(table[NTT_T_PI + m], ntt_ld(x, m));
    store_words(keep + (size_t)m * 32, pm.v);
    ntt_st(x, m, pm);
  }
  ntt_dif_fwd(x, tw);
  const bool skip = bad != 0;
  recover_store(x, 0, in, pos, o, skip, err);
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t m = t + NTT_THREADS * q;
    BlobF pm;
    load_words(keep + (size_t)m * 32, pm.v);
    ntt_st(x, m, fp_mul(tw[m], pm));
  }
  ntt_dif_fwd(x, tw);
  recover_store(x, 1, in, pos, o, skip, err);
}

}  // namespace kzgmi
