// EIP-4844 producer side (Deneb polynomial-commitments: blob_to_kzg_commitment, compute_kzg_proof,
// compute_blob_kzg_proof).  BLS12-381 only, domain size 4096.  Reference: none (LICENSE only); the
// definitions are restated in include/kzgmi.h and tests/blobproofref.py.
//
//   C = sum_j v_j L_j               (v_j = blob element j = p(dom[j]), L_j = [l_j(tau)]_1 the key's point j)
//   y = p(z),  q_j = (v_j - y) / (dom[j] - z),  proof = sum_j q_j L_j
//   z = dom[m]:  y = v_m,  q_m = sum_{i != m} (v_i - y) dom[i] / (z (z - dom[i]))
//
// Both sums are one fixed-base MSM of 4096 terms over the key: the window table of fk20.hpp (signed
// 4-bit digits, no doublings, no buckets), whose scalar format, 32 B big-endian, is a blob's bytes.
//
// Per call, on the slot's stream:
//   k_blob_quotient   one workgroup per blob, k_blob_eval's ownership: the inverses of z - dom[j] by
//                     Montgomery's trick give y, then, still in registers, q
//   k_blob_msm        block (blob, chunk of 64 bases), thread (base, part): the table rows of its 16
//                     windows, then a fixed-order tree in LDS -> one partial per block
//   k_blob_msm_join   one block per blob: a fixed-order tree over its 64 partials
//   encode, compress (kernels.hpp, points.hpp), k_fk20_emit (nothing is written once an error is raised)
#pragma once
#include "fk20.hpp"

#include <type_traits>

namespace kzgmi {

constexpr uint32_t BP_BASES = BLOB_N;                       // the key's points
constexpr uint32_t BP_CHUNKS = BP_BASES / FK_COLS;          // blocks per blob: 64 bases each
constexpr size_t BP_TABLE_POINTS = (size_t)BP_BASES * FK_WINDOWS * FK_MULTS;

// f(integral_constant<int, K>) for K = 0 .. N - 1, in order.  k_blob_quotient's passes index their register
// arrays through it: a `#pragma unroll` loop is unrolled too late for the array to leave the stack (the
// 312 B of k_blob_eval)
template <int K, int N, class F>
KZ_DEV void bp_unrolled(F&& f) {
  if constexpr (K < N) {
    f(std::integral_constant<int, K>{});
    bp_unrolled<K + 1, N>(f);
  }
}

// ------------------------------------------------------------------------------ quotient
// y = p(z) and q of blob blockIdx.x: y as 32 B, q as 4096 x 32 B big-endian in blob layout.  Thread t
// owns elements t + 512 k as in k_blob_eval.  The first pass leaves 1 / (z - dom[j]) of its elements in
// registers (in place of the prefix products); the second turns them into q_j = (y - v_j) / (z - dom[j]).
// z = dom[m] (hit): the inverse of element m is a placeholder, y = v_m, and q_m comes from a second
// tree sum over q_i dom[i] (i != m): q_m = -(sum_i q_i dom[i]) / z, with 1 / z read from the domain
// table.  hit is per block, so blobs on and off the domain mix in one launch.  range_check: the elements
// are checked here (DERR_SCALAR); else k_blob_challenge did.  An element >= r counts as 0 either way,
// also as y on a hit, where k_blob_eval answers the element's raw bytes: under that error (raised by
// both) the two kernels' y differ.
static __global__ void __launch_bounds__(BLOB_EVAL_THREADS) k_blob_quotient(const uint8_t* __restrict__ blobs,
                                                                            const uint8_t* __restrict__ zs,
                                                                            const BlobF* __restrict__ table,
                                                                            int range_check, uint8_t* __restrict__ ys,
                                                                            uint8_t* __restrict__ qs,
                                                                            uint32_t* __restrict__ err) {
  __shared__ BlobF red[BLOB_EVAL_THREADS];
  __shared__ BlobF ysh;
  __shared__ uint32_t hit;
  const uint32_t t = threadIdx.x;
  const uint8_t* blob = blobs + (size_t)blockIdx.x * BLOB_BYTES;
  uint8_t* q_out = qs + (size_t)blockIdx.x * BLOB_BYTES;
  if (t == 0) hit = 0;
  uint32_t wz[8];
  load_words(zs + (size_t)blockIdx.x * 32, wz);
  BlobF zr = fp_from_be_words<BlobR>(wz, 0);
  if (!fp_raw_lt_mod(zr)) {
    if (t == 0) raise_err(err, DERR_SCALAR);
    zr = BlobF::zero();
  }
  const BlobF z = fp_to_mont(zr);
  __syncthreads();
  BlobF dinv[BLOB_EVAL_PER];  // prefix products, then the inverses
  BlobF acc = BlobF::one();
  bp_unrolled<0, BLOB_EVAL_PER>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const uint32_t j = t + BLOB_EVAL_THREADS * k;
    BlobF d = fp_sub(z, table[j]);
    if (d.is_zero()) {
      hit = j + 1;  // at most one j: the domain points are distinct
      d = BlobF::one();
    }
    dinv[k] = acc;
    acc = fp_mul(acc, d);
  });
  BlobF inv = fp_inv(acc);  // inlined: the out-of-line form saves the prefix products on the stack across the call
  BlobF sum = BlobF::zero();
  bp_unrolled<0, BLOB_EVAL_PER>([&](auto kc) {
    constexpr int k = BLOB_EVAL_PER - 1 - decltype(kc)::value;
    const uint32_t j = t + BLOB_EVAL_THREADS * k;
    const BlobF w = table[j];
    BlobF d = fp_sub(z, w);
    if (d.is_zero()) d = BlobF::one();
    dinv[k] = fp_mul(inv, dinv[k]);
    inv = fp_mul(inv, d);
    uint32_t we[8];
    load_words(blob + (size_t)j * 32, we);
    BlobF e = fp_from_be_words<BlobR>(we, 0);  // standard form
    if (!fp_raw_lt_mod(e)) {
      if (range_check) raise_err(err, DERR_SCALAR);
      e = BlobF::zero();
    }
    // standard-form e times two Montgomery factors stays in standard form
    sum = fp_add(sum, fp_mul(fp_mul(e, w), dinv[k]));
  });
  red[t] = sum;
  __syncthreads();
  for (int st = BLOB_EVAL_THREADS / 2; st >= 1; st >>= 1) {
    if ((int)t < st) red[t] = fp_add(red[t], red[t + st]);
    __syncthreads();
  }
  const uint32_t m = hit;  // j + 1 of the element z sits on, or 0
  if (t == 0) {
    BlobF y;
    if (m) {
      uint32_t we[8];
      load_words(blob + (size_t)(m - 1) * 32, we);
      y = fp_from_be_words<BlobR>(we, 0);
      if (!fp_raw_lt_mod(y)) y = BlobF::zero();
    } else {
      BlobF zn = z;
      for (int k = 0; k < 12; ++k) zn = fp_sqr(zn);
      const BlobF fac = fp_mul(fp_sub(zn, BlobF::one()), table[BLOB_N]);
      y = fp_mul(red[0], fac);
    }
    ysh = y;
    uint32_t wy[8];
    fp_to_be_words(y, wy, 0);
    store_words(ys + (size_t)blockIdx.x * 32, wy);
  }
  __syncthreads();
  const BlobF y = ysh;
  BlobF side = BlobF::zero();  // sum of q_j dom[j] over this thread's elements but m
  bp_unrolled<0, BLOB_EVAL_PER>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const uint32_t j = t + BLOB_EVAL_THREADS * k;
    if (j + 1 == m) return;  // written below
    uint32_t we[8];
    load_words(blob + (size_t)j * 32, we);
    BlobF e = fp_from_be_words<BlobR>(we, 0);
    if (!fp_raw_lt_mod(e)) e = BlobF::zero();
    const BlobF q = fp_mul(fp_sub(y, e), dinv[k]);  // standard form
    if (m) side = fp_add(side, fp_mul(q, table[j]));
    uint32_t wq[8];
    fp_to_be_words(q, wq, 0);
    store_words(q_out + (size_t)j * 32, wq);
  });
  if (!m) return;  // the whole block alike
  red[t] = side;
  __syncthreads();
  for (int st = BLOB_EVAL_THREADS / 2; st >= 1; st >>= 1) {
    if ((int)t < st) red[t] = fp_add(red[t], red[t + st]);
    __syncthreads();
  }
  if (t != 0) return;
  // 1 / z is a domain point too: dom[m - 1] = w^e with e = rev12(m - 1), 1 / z = w^(4096 - e)
  const uint32_t e = __brev(m - 1) >> 20;
  const BlobF qm = fp_neg(fp_mul(red[0], table[__brev((BLOB_N - e) & (BLOB_N - 1)) >> 20]));
  uint32_t wq[8];
  fp_to_be_words(qm, wq, 0);
  store_words(q_out + (size_t)(m - 1) * 32, wq);
}

// ------------------------------------------------------------------------------ fixed-base MSM
// part[blob * 64 + c] = sum_{b < 64} k_{64 c + b} L_{64 c + b}: block (blob, c), thread t = b + 64 part.
// scal: 4096 x 32 B big-endian per blob (q, or the blob itself).  The table and the additions are those
// of k_fk20_msm.  range_check: a scalar >= r raises DERR_SCALAR (and adds nothing).
static __global__ void __launch_bounds__(FK_MSM_THREADS) k_blob_msm(const uint8_t* __restrict__ scal,
                                                                    const FkAF* __restrict__ tab,
                                                                    const uint8_t* __restrict__ tab_inf,
                                                                    int range_check, FkXY* __restrict__ out,
                                                                    uint32_t* __restrict__ err) {
  __shared__ __align__(16) FkXY part[FK_MSM_THREADS];
  const uint32_t t = threadIdx.x, b = t & (FK_COLS - 1), pt = t / FK_COLS;
  const uint32_t base = (blockIdx.x & (BP_CHUNKS - 1)) * FK_COLS + b;
  FkXY acc = FkXY::inf();
  uint32_t we[8];
  load_words(scal + ((size_t)blockIdx.x * FK_COLS + b) * 32, we);
  const BlobF kf = fp_from_be_words<BlobR>(we, 0);
  bool use = !tab_inf[base];
  if (range_check && !fp_raw_lt_mod(kf)) {
    if (pt == 0) raise_err(err, DERR_SCALAR);
    use = false;
  }
  if (use) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = kf.v[i];
    constexpr int PER = FK_WINDOWS / FK_PARTS;
    const FkAF* rows = tab + ((size_t)base * FK_WINDOWS + PER * pt) * FK_MULTS;
#pragma unroll 1
    for (int i = 0; i < PER; ++i) {
      const int d = fk_digit(k, PER * (int)pt + i);
      if (d == 0) continue;
      FkAF q = load_affine(rows, (uint32_t)(i * FK_MULTS + (d < 0 ? -d : d) - 1));
      if (d < 0) q.y = fp_neg(q.y);
      acc = xyzz_add_affine(acc, q);
    }
  }
  store_xyzz(&part[t], acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t st = FK_MSM_THREADS / 2; st >= 1; st >>= 1) {  // the same tree for every input
    if (t < st) store_xyzz(&part[t], xyzz_add(load_xyzz(&part[t]), load_xyzz(&part[t + st])));
    __syncthreads();
  }
  if (t == 0) store_xyzz(&out[blockIdx.x], load_xyzz(&part[0]));
}

// out[blob] = the sum of the blob's 64 partials, in a fixed order
static __global__ void __launch_bounds__(BP_CHUNKS) k_blob_msm_join(const FkXY* __restrict__ parts,
                                                                    FkXY* __restrict__ out) {
  __shared__ __align__(16) FkXY part[BP_CHUNKS];
  const uint32_t t = threadIdx.x;
  store_xyzz(&part[t], load_xyzz(&parts[(size_t)blockIdx.x * BP_CHUNKS + t]));
  __syncthreads();
#pragma unroll 1
  for (uint32_t st = BP_CHUNKS / 2; st >= 1; st >>= 1) {
    if (t < st) store_xyzz(&part[t], xyzz_add(load_xyzz(&part[t]), load_xyzz(&part[t + st])));
    __syncthreads();
  }
  if (t == 0) store_xyzz(&out[blockIdx.x], load_xyzz(&part[0]));
}

// ------------------------------------------------------------------------------ the key's table
// rows of the table from the validated points: thread (w, base), a wave shares w (k_fk20_table's rows,
// tab[(base FK_WINDOWS + w) FK_MULTS + m - 1] = m 2^(4 w) L_base)
static __global__ void __launch_bounds__(256) k_blob_table(const FkAF* __restrict__ pts, const uint8_t* __restrict__ inf,
                                                           FkAF* __restrict__ tab, uint8_t* __restrict__ tab_inf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BP_BASES * FK_WINDOWS) return;
  const uint32_t w = i / BP_BASES, base = i & (BP_BASES - 1);
  const bool is_inf = inf[base] != 0;
  if (w == 0) tab_inf[base] = is_inf ? 1 : 0;
  if (is_inf) return;
  FkXY unit = xyzz_from_affine(load_affine(pts, base));
#pragma unroll 1
  for (uint32_t k = 0; k < FK_WBITS * w; ++k) unit = xyzz_dbl_c(unit);
  FkXY m = unit;
  FkAF* rows = tab + ((size_t)base * FK_WINDOWS + w) * FK_MULTS;
#pragma unroll 1
  for (int j = 0; j < FK_MULTS; ++j) {
    FkAF a;
    xyzz_to_affine(m, a);  // never infinity: a multiple below r of a point of order r
    uint32_t o[24];
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      o[q] = a.x.v[q];
      o[12 + q] = a.y.v[q];
    }
    store_words(reinterpret_cast<uint8_t*>(rows + j), o);
    if (j + 1 < FK_MULTS) m = xyzz_add_c(m, unit);
  }
}

}  // namespace kzgmi
