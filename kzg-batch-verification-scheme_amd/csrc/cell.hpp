// EIP-7594 (PeerDAS) cell front end of batch verification (verify_cell_kzg_proof_batch): coset
// tables, the r-weighted fold of the cells per coset, a size-64 inverse NTT per coset, the
// transcript hash.  BLS12-381 only.  Reference: none (LICENSE only); the definitions are restated
// in include/kzgmi.h and tests/cellref.py.
//
//   w = 7^((r-1)/8192); cell i (i < 128), element j (j < 64) is p(w^rev13(64 i + j)) =
//   p(h_i w64^rev6(j)), h_i = w^rev7(i), w64 = w^128; h_i^64 = (w^64)^rev7(i)
//   I_k = p_k mod (X^64 - h^64):  c_m = h^-m / 64 * sum_j e_j w64^(-rev6(j) m)
//   e(sum r^k pi_k, [tau^64]_2) = e(sum r^k C_k + sum r^k h_k^64 pi_k - [sum r^k I_k(tau)]_1, [1]_2)
//
// The interpolation is linear in the cell, so the cells of one coset are folded first
// (E_c = sum r^k cells[k] over the k on coset c) and each of the at most 128 cosets is
// transformed once, whatever n is.  Field sums are exact: any summation order is bit-exact.
#pragma once
#include "blob.hpp"

namespace kzgmi {

constexpr uint32_t CELL_N = 64;                  // field elements per cell
constexpr uint32_t CELL_BYTES = 32 * CELL_N;     // 2048
constexpr uint32_t CELL_COSETS = 128;            // cells per extended blob
// the coset table (Montgomery): h_i^64, i < 128 | h_i^-1, i < 128 | w64^-t, t < 64 | 64^-1
constexpr uint32_t CELL_T_H64 = 0, CELL_T_HINV = 128, CELL_T_TW = 256, CELL_T_INV64 = 320, CELL_TABLE = 321;

// "RCKZGCBATCH__V1_" as big-endian words
__constant__ static const uint32_t kCellBatchTag[4] = {0x52434b5au, 0x47434241u, 0x5443485fu, 0x5f56315fu};

// w^e for e < 8192 from the one generated constant
KZ_DEV BlobF cell_root_pow(uint32_t e) {
  BlobF x = BlobF::from_const(BlobR::ROOT8192_M), acc = BlobF::one();
  for (int k = 0; k < 13; ++k) {
    if ((e >> k) & 1) acc = fp_mul(acc, x);
    x = fp_sqr(x);
  }
  return acc;
}

// the coset table, once per context: CELL_TABLE threads
static __global__ void __launch_bounds__(64) k_cell_table(BlobF* __restrict__ table) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= CELL_TABLE) return;
  BlobF v;
  if (t < CELL_T_HINV) {
    v = cell_root_pow((64u * (__brev(t) >> 25)) & 8191u);                  // (w^64)^rev7(i)
  } else if (t < CELL_T_TW) {
    v = cell_root_pow((8192u - (__brev(t - CELL_T_HINV) >> 25)) & 8191u);  // w^-rev7(i)
  } else if (t < CELL_T_INV64) {
    v = cell_root_pow((8192u - 128u * (t - CELL_T_TW)) & 8191u);           // w64^-t
  } else {
    BlobF nn = BlobF::zero();
    nn.v[0] = CELL_N;
    v = fp_inv_c(fp_to_mont(nn));
  }
  table[t] = v;
}

// z_k = h_{cell_index[k]}^64 (32 B big-endian, where k_scalar_prep_pow reads z) and y_k = 0; an index
// out of range raises DERR_ARG (and reads coset / commitment 0).  Indices: uint64, little-endian.
static __global__ void __launch_bounds__(256) k_cell_z(const uint64_t* __restrict__ cell_indices,
                                                       const uint64_t* __restrict__ commitment_indices, uint32_t n,
                                                       uint32_t m, const BlobF* __restrict__ table,
                                                       uint8_t* __restrict__ zs, uint8_t* __restrict__ ys,
                                                       uint32_t* __restrict__ err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint64_t ci = cell_indices[k];
  if (ci >= CELL_COSETS) {
    raise_err(err, DERR_ARG);
    ci = 0;
  }
  if (commitment_indices && commitment_indices[k] >= m) raise_err(err, DERR_ARG);
  uint32_t w[8], zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  fp_to_be_words(fp_from_mont(table[CELL_T_H64 + (uint32_t)ci]), w, 0);
  store_words(zs + (size_t)k * 32, w);
  store_words(ys + (size_t)k * 32, zero);
}

// pts[dst + k] = pts[src + commitment_indices[k]]: the n gathered commitments of MSM#1's r^k C_k
// class from the m decoded unique ones (an index out of range was raised by k_cell_z: reads 0)
template <class Cv>
__global__ void __launch_bounds__(256) k_cell_gather(const uint64_t* __restrict__ commitment_indices, uint32_t n,
                                                     uint32_t m, Affine<Cv>* __restrict__ pts, uint8_t* __restrict__ inf,
                                                     uint32_t src, uint32_t dst) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint64_t ci = commitment_indices[k];
  if (ci >= m) ci = 0;
  pts[dst + k] = pts[src + (uint32_t)ci];
  inf[dst + k] = inf[src + (uint32_t)ci];
}

// Fold and transform: workgroup c (one wave) owns coset c, thread j element j.
//   E[j] = sum over the k with cell_index[k] = c of r^k cells[k][j]   (rk: r^k, 8 LE words, standard)
// Every cell belongs to exactly one coset, so every element is range-checked here, once
// (DERR_SCALAR); the index array is scanned by every workgroup (wave-uniform loads).
// Then the inverse NTT: the cell's element order is the bit-reversed one a decimation-in-time
// transform takes as input, so six radix-2 stages (root w64^-1) run on E as it is; output m is
// scaled by 64^-1 h_c^-m.  part[c][m]: standard form, zero for an empty coset.
static __global__ void __launch_bounds__(64) k_cell_fold_intt(const uint64_t* __restrict__ cell_indices,
                                                              const uint8_t* __restrict__ cells,
                                                              const uint32_t* __restrict__ rk, uint32_t n,
                                                              const BlobF* __restrict__ table,
                                                              BlobF* __restrict__ part, uint32_t* __restrict__ err) {
  __shared__ BlobF x[CELL_N];
  const uint32_t c = blockIdx.x, j = threadIdx.x;
  BlobF acc = BlobF::zero();
  uint32_t hits = 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (cell_indices[k] != c) continue;
    hits += 1;
    uint32_t we[8], wr[8];
    load_words(cells + (size_t)k * CELL_BYTES + 32 * j, we);
    load_words(reinterpret_cast<const uint8_t*>(rk + 8 * (size_t)k), wr);
    BlobF e = fp_from_be_words<BlobR>(we, 0);
    if (!fp_raw_lt_mod(e)) {
      raise_err(err, DERR_SCALAR);
      e = BlobF::zero();
    }
    BlobF r;
#pragma unroll
    for (int q = 0; q < 8; ++q) r.v[q] = wr[q];
    // standard-form e times the Montgomery r^k stays in standard form
    acc = fp_add(acc, fp_mul(e, fp_to_mont(r)));
  }
  if (hits == 0) {  // wave-uniform: every thread scanned the same indices
    part[c * CELL_N + j] = BlobF::zero();
    return;
  }
  x[j] = acc;
  __syncthreads();
#pragma unroll 1
  for (uint32_t half = 1; half < CELL_N; half <<= 1) {
    const BlobF w = table[CELL_T_TW + (j & (half - 1)) * (CELL_N / (2 * half))];
    const bool up = (j & half) != 0;
    const BlobF a = x[up ? j - half : j];
    const BlobF b = fp_mul(w, x[up ? j : j + half]);
    const BlobF y = up ? fp_sub(a, b) : fp_add(a, b);
    __syncthreads();
    x[j] = y;
    __syncthreads();
  }
  // 64^-1 h_c^-m, m = j (6 bits)
  BlobF hp = table[CELL_T_HINV + c], s = table[CELL_T_INV64];
  for (int q = 0; q < 6; ++q) {
    if ((j >> q) & 1) s = fp_mul(s, hp);
    hp = fp_sqr(hp);
  }
  part[c * CELL_N + j] = fp_mul(s, x[j]);
}

// The 64 coefficients of every cell's own interpolation polynomial I_k, unfolded (the search for a
// rejected batch's invalid cells weights them per index range: msm_group.hpp k_cell_range_fold):
// one wave per cell, lane j element j, four cells per workgroup; the same six stages and scale as
// k_cell_fold_intt.  coef_le[(64 k + m) 8 ..]: c_m as 8 LE words in standard form; coeffs_be (may
// be null): c_m as 32 B big-endian at 32 (64 k + m).  Every element is range-checked here, once
// (DERR_SCALAR, counts as 0); a cell index out of range reads coset 0 (k_cell_z raises it).
constexpr uint32_t CELL_COEFF_PACK = 4;  // cells per workgroup
static __global__ void __launch_bounds__(64 * CELL_COEFF_PACK) k_cell_coeffs(
    const uint64_t* __restrict__ cell_indices, const uint8_t* __restrict__ cells, uint32_t n,
    const BlobF* __restrict__ table, uint32_t* __restrict__ coef_le, uint8_t* __restrict__ coeffs_be,
    uint32_t* __restrict__ err) {
  __shared__ BlobF xs[CELL_COEFF_PACK][CELL_N];
  const uint32_t wv = threadIdx.x >> 6, j = threadIdx.x & 63u;
  const uint32_t k = blockIdx.x * CELL_COEFF_PACK + wv;
  const bool live = k < n;  // wave-uniform; the waves past the last cell keep the barriers
  BlobF* x = xs[wv];
  BlobF e = BlobF::zero();
  uint32_t c = 0;
  if (live) {
    const uint64_t ci = cell_indices[k];
    c = ci < CELL_COSETS ? (uint32_t)ci : 0u;
    uint32_t we[8];
    load_words(cells + (size_t)k * CELL_BYTES + 32 * j, we);
    e = fp_from_be_words<BlobR>(we, 0);
    if (!fp_raw_lt_mod(e)) {
      raise_err(err, DERR_SCALAR);
      e = BlobF::zero();
    }
  }
  x[j] = e;
  __syncthreads();
#pragma unroll 1
  for (uint32_t half = 1; half < CELL_N; half <<= 1) {
    const BlobF w = table[CELL_T_TW + (j & (half - 1)) * (CELL_N / (2 * half))];
    const bool up = (j & half) != 0;
    const BlobF a = x[up ? j - half : j];
    const BlobF b = fp_mul(w, x[up ? j : j + half]);
    const BlobF y = up ? fp_sub(a, b) : fp_add(a, b);
    __syncthreads();
    x[j] = y;
    __syncthreads();
  }
  if (!live) return;
  // 64^-1 h_c^-m, m = j (6 bits)
  BlobF hp = table[CELL_T_HINV + c], s = table[CELL_T_INV64];
  for (int q = 0; q < 6; ++q) {
    if ((j >> q) & 1) s = fp_mul(s, hp);
    hp = fp_sqr(hp);
  }
  const BlobF cm = fp_mul(s, x[j]);  // the Montgomery scale times the standard-form sum: standard form
  const size_t o = (size_t)k * CELL_N + j;
  store_words(reinterpret_cast<uint8_t*>(coef_le + 8 * o), cm.v);
  if (coeffs_be) {
    uint32_t w[8];
    fp_to_be_words(cm, w, 0);
    store_words(coeffs_be + 32 * o, w);
  }
}

// c_m = sum over the cosets of part[c][m].  neg_le: -c_m as 8 LE words in standard form (the
// scalars of MSM#1's [tau^m]_1 class); coeffs_be (may be null): c_m as 32 B big-endian.
static __global__ void __launch_bounds__(64) k_cell_sum(const BlobF* __restrict__ part, uint32_t* __restrict__ neg_le,
                                                        uint8_t* __restrict__ coeffs_be) {
  const uint32_t m = threadIdx.x;
  BlobF acc = BlobF::zero();
  for (uint32_t c = 0; c < CELL_COSETS; ++c) acc = fp_add(acc, part[c * CELL_N + m]);
  const BlobF neg = fp_neg(acc);
  store_words(reinterpret_cast<uint8_t*>(neg_le + 8 * m), neg.v);
  if (coeffs_be) {
    uint32_t w[8];
    fp_to_be_words(acc, w, 0);
    store_words(coeffs_be + 32 * m, w);
  }
}

// ---------------------------------------------------------------------------- batch challenge
// r of the whole batch: one sequential SHA-256 over 48 + 48 m + 2112 n bytes on one wave, in the
// style of k_blob_batch_challenge (lanes 0-15 fetch the next block's words while every lane
// compresses the current one in vector registers); 33 compressions per cell.  Writes r (8
// big-endian words) and the power table r^(2^k); r = 0 stays 0 (powers 1, 0, 0, ...).
static __global__ void __launch_bounds__(64) k_cell_batch_challenge(const uint8_t* __restrict__ commitments, uint32_t m,
                                                                    const uint64_t* __restrict__ commitment_indices,
                                                                    const uint64_t* __restrict__ cell_indices,
                                                                    const uint8_t* __restrict__ cells,
                                                                    const uint8_t* __restrict__ proofs, uint32_t n,
                                                                    BlobF* __restrict__ pow,
                                                                    uint32_t* __restrict__ chal_out) {
  const uint32_t lane = threadIdx.x;
  const uint32_t* cw = reinterpret_cast<const uint32_t*>(commitments);
  const uint32_t* ciw = reinterpret_cast<const uint32_t*>(commitment_indices);  // [lo, hi] pairs
  const uint32_t* cew = reinterpret_cast<const uint32_t*>(cell_indices);
  const uint32_t* clw = reinterpret_cast<const uint32_t*>(cells);
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(proofs);
  constexpr uint32_t PER = 4 + CELL_BYTES / 4 + 12;          // words per cell record: 528
  const uint64_t head = 12 + 12 * (uint64_t)m;               // tag, four lengths, the commitments
  const uint64_t nwords = head + PER * (uint64_t)n;          // message words
  const uint64_t nblocks = (4 * nwords + 9 + 63) / 64;       // padded blocks
  const uint64_t bits = 32 * nwords;
  // big-endian word w of the padded message
  auto word = [&](uint64_t w) -> uint32_t {
    if (w < 4) return kCellBatchTag[w];
    if (w < 12) return w == 5 ? BLOB_N : w == 7 ? CELL_N : w == 9 ? m : w == 11 ? n : 0u;
    if (w < head) return __builtin_bswap32(cw[w - 12]);
    if (w < nwords) {
      const uint32_t q = (uint32_t)((w - head) / PER), o = (uint32_t)((w - head) % PER);
      if (o < 2) return ciw[2 * (size_t)q + (1 - o)];        // be64: the high word first
      if (o < 4) return cew[2 * (size_t)q + (3 - o)];
      const uint32_t v = o < 4 + CELL_BYTES / 4 ? clw[(CELL_BYTES / 4) * (size_t)q + (o - 4)]
                                                : pw[12 * (size_t)q + (o - 4 - CELL_BYTES / 4)];
      return __builtin_bswap32(v);
    }
    if (w == nwords) return 0x80000000u;
    if (w == 16 * nblocks - 2) return (uint32_t)(bits >> 32);
    if (w == 16 * nblocks - 1) return (uint32_t)bits;
    return 0u;
  };
  uint32_t h[8];
  sha256_init(h);
  uint32_t nxt = lane < 16 ? word(lane) : 0u;
  for (uint64_t b = 0; b < nblocks; ++b) {
    const uint32_t cur = nxt;
    if (b + 1 < nblocks && lane < 16) nxt = word(16 * (b + 1) + lane);
    uint32_t blk[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) blk[k] = (uint32_t)__shfl((int)cur, k);
    sha256_compress(blk, h);
  }
  if (lane != 0) return;
  const BlobF r = blob_hash_to_fr(h);
#pragma unroll
  for (int k = 0; k < 8; ++k) chal_out[k] = r.v[7 - k];
  BlobF x = fp_to_mont(r);
  for (int k = 0; k < FS_POW_BITS; ++k) {
    pow[k] = x;
    x = fp_sqr(x);
  }
}

}  // namespace kzgmi
