// KZG openings of a coefficient-form polynomial: evaluation and synthetic division as one suffix
// scan over Fr.  For p = sum_{i<m} c_i X^i and a point z
//     Q_m = 0,  Q_i = c_i + z Q_{i+1}:   y = p(z) = Q_0,   (p - y) / (X - z) = sum_{1<=i<m} Q_i X^(i-1)
// so the evaluation and every quotient coefficient are the running values of Horner's rule, i.e. the
// suffix scan of the affine maps x -> c_i + z x.  A run of L maps composes to x -> V + z^L x with V
// the run's Horner value from a zero carry-in.  The coefficient array is read as if it went on with
// zeros above m (Q_i = 0 there), so every run and every tile is full and the multiplier of a run of
// OPEN_RUN maps is z^OPEN_RUN, of a tile z^OPEN_TILE: the scans below are of the recurrence
// S_j = V_j + w S_{j+1} with one multiplier w per level and need the powers w^(2^s) only.
//
// Boundaries (all powers of two, named here; tests/test_gpu_open_quotient.py crosses each):
//   OPEN_RUN   = 16    coefficients one thread runs Horner over
//   OPEN_BLOCK = 256   threads per workgroup = runs per tile = values per workgroup scan
//   OPEN_TILE  = 4096  coefficients per tile (OPEN_RUN x OPEN_BLOCK): one workgroup of pass 1 and 3
//   OPEN_SPAN  = 256   tile aggregates the second-level workgroup scans at once (2^20 coefficients);
//                      beyond that it loops from the top, carrying the value of the step before
//   OPEN_POWERS = 20   z^(2^i), i < 20: runs use i = 4..11, tiles 12..19 (k_open_points, once per point)
//
// Passes, grid (tiles, points of the group) -- a group is the points whose quotients fit the slot's
// scratch (host_open.hip):
//   k_open_tiles     each thread: V of its run; a workgroup scan composes the runs; the run values and
//                    the tile's aggregate are kept
//   k_open_carry     one workgroup per point: scan of the tile aggregates -> the carry into every tile
//                    (Q at the first index above it) and y = Q_0
//   k_open_quotient  the tile's run values scanned again with the tile's carry put into the top run,
//                    which gives every thread its true carry-in; Horner again from it, Q_i written
// Two Fr products per coefficient (one Horner step in pass 1, one in pass 3) plus 8 per run and pass
// for the scans: 3 in all at OPEN_RUN = 16.  No exponentiation per element.
//
// Number forms: coefficients and Q_i are canonical standard-form Fr values as 8 little-endian words
// (what k_convert_scalars writes and the MSM's TermList reads); the powers of z are in Montgomery
// form, so fp_mul(power, value) is the standard-form product with no conversion of the values.
#pragma once
#include "kernels.hpp"

namespace kzgmi {

constexpr uint32_t OPEN_RUN = 16;
constexpr uint32_t OPEN_BLOCK = 256;
constexpr uint32_t OPEN_TILE = OPEN_RUN * OPEN_BLOCK;
constexpr uint32_t OPEN_SPAN = 256;
constexpr uint32_t OPEN_POWERS = 20;
constexpr uint32_t OPEN_LOG_RUN = 4, OPEN_LOG_TILE = 12;
static_assert((1u << OPEN_LOG_RUN) == OPEN_RUN && (1u << OPEN_LOG_TILE) == OPEN_TILE, "powers of two");
static_assert(OPEN_BLOCK == 256 && OPEN_SPAN == OPEN_BLOCK, "the workgroup scan covers 256 values in 8 steps");
static_assert(OPEN_LOG_TILE + 8 == OPEN_POWERS, "the second-level scan's last step reads the top power");

template <class R>
KZ_DEV Fp<R> open_load(const uint32_t* p) {
  uint32_t w[8];
  load_words(reinterpret_cast<const uint8_t*>(p), w);
  Fp<R> r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = w[k];
  return r;
}
template <class R>
KZ_DEV void open_store(uint32_t* p, const Fp<R>& a) {
  store_words(reinterpret_cast<uint8_t*>(p), a.v);
}
template <class R>
KZ_DEV void open_store_be(uint8_t* p, const Fp<R>& a) {
  uint32_t w[8];
  fp_to_be_words(a, w, 0);
  store_words(p, w);
}

// The suffix scan S_t = v_t + w S_{t+1} over the workgroup's OPEN_BLOCK values (S beyond the last
// thread is 0): step s adds w^(2^s) times the value 2^s threads up; zp[s] = w^(2^s), s < 8, the same
// for every thread.  sh: word k of thread t at sh[k][t] (consecutive lanes, consecutive banks).
// Every thread of the workgroup calls it; sh may be reused after it returns.
template <class R>
KZ_DEV Fp<R> open_scan(Fp<R> v, const Fp<R>* __restrict__ zp, uint32_t (*sh)[OPEN_BLOCK], uint32_t t) {
#pragma unroll 1
  for (uint32_t s = 0; s < 8; ++s) {
    const uint32_t d = 1u << s;
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k][t] = v.v[k];
    __syncthreads();
    if (t + d < OPEN_BLOCK) {
      Fp<R> u;
#pragma unroll
      for (int k = 0; k < 8; ++k) u.v[k] = sh[k][t + d];
      v = fp_add(v, fp_mul(zp[s], u));
    }
    __syncthreads();
  }
  return v;
}

// The value thread t + 1 holds (`top` for the last thread) and, in *first, the value of thread 0
template <class R>
KZ_DEV Fp<R> open_next(const Fp<R>& v, const Fp<R>& top, uint32_t (*sh)[OPEN_BLOCK], uint32_t t, Fp<R>* first) {
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[k][t] = v.v[k];
  __syncthreads();
  Fp<R> r = top;
  if (t + 1 < OPEN_BLOCK) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = sh[k][t + 1];
  }
  if (first) {
#pragma unroll
    for (int k = 0; k < 8; ++k) first->v[k] = sh[k][0];
  }
  __syncthreads();
  return r;
}

// z_j (32 B big-endian, canonical: else DERR_SCALAR and z = 0) -> zp[j][i] = z^(2^i) in Montgomery
// form, i < OPEN_POWERS
template <class Cv>
__global__ void __launch_bounds__(64) k_open_points(const uint8_t* __restrict__ zs, uint32_t k, uint32_t* __restrict__ zp,
                                                    uint32_t* __restrict__ err) {
  using R = typename Cv::FrP;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  uint32_t w[8];
  load_words(zs + (size_t)j * 32, w);
  Fp<R> z = fp_from_be_words<R>(w, 0);
  if (!fp_raw_lt_mod(z)) { raise_err(err, DERR_SCALAR); z = Fp<R>::zero(); }
  z = fp_to_mont(z);
  uint32_t* out = zp + (size_t)j * OPEN_POWERS * 8;
#pragma unroll 1
  for (uint32_t i = 0; i < OPEN_POWERS; ++i) {
    open_store<R>(out + 8 * i, z);
    z = fp_sqr(z);
  }
}

// Horner over the run [lo, lo + OPEN_RUN) from the carry-in acc, coefficients at and above m read as
// 0 and left out.  Q: the running values Q_i, 1 <= i < m, are written -- 8 LE words at q + 8 (i - 1),
// or with BE 32 big-endian bytes at q8 + 32 (i - 1).
template <class R, bool Q, bool BE>
KZ_DEV Fp<R> open_horner(const uint32_t* __restrict__ coef, uint32_t m, uint32_t lo, const Fp<R>& z, Fp<R> acc,
                         uint32_t* __restrict__ q) {
#pragma unroll 1
  for (int e = (int)OPEN_RUN - 1; e >= 0; --e) {
    const uint32_t i = lo + (uint32_t)e;
    if (i >= m) continue;
    acc = fp_add(open_load<R>(coef + 8 * (size_t)i), fp_mul(z, acc));
    if constexpr (Q) {
      if (i >= 1) {
        if constexpr (BE) open_store_be<R>(reinterpret_cast<uint8_t*>(q) + 32 * (size_t)(i - 1), acc);
        else open_store<R>(q + 8 * (size_t)(i - 1), acc);
      }
    }
  }
  return acc;
}

// Pass 1.  grid (tiles, points); zp: the group's first point's powers; runv: [point][tile][thread],
// tilev: [point][tile], 8 words each
template <class Cv>
__global__ void __launch_bounds__(OPEN_BLOCK) k_open_tiles(const uint32_t* __restrict__ coef, uint32_t m,
                                                           const uint32_t* __restrict__ zp, uint32_t* __restrict__ runv,
                                                           uint32_t* __restrict__ tilev) {
  using R = typename Cv::FrP;
  __shared__ uint32_t sh[8][OPEN_BLOCK];
  const uint32_t t = threadIdx.x, tile = blockIdx.x, pt = blockIdx.y, tiles = gridDim.x;
  const Fp<R>* zpp = reinterpret_cast<const Fp<R>*>(zp) + (size_t)pt * OPEN_POWERS;
  const uint32_t lo = tile * OPEN_TILE + t * OPEN_RUN;
  const Fp<R> v = open_horner<R, false, false>(coef, m, lo, zpp[0], Fp<R>::zero(), nullptr);
  const size_t run = ((size_t)pt * tiles + tile) * OPEN_BLOCK + t;
  open_store<R>(runv + 8 * run, v);
  const Fp<R> s = open_scan<R>(v, zpp + OPEN_LOG_RUN, sh, t);
  if (t == 0) open_store<R>(tilev + 8 * ((size_t)pt * tiles + tile), s);
}

// Pass 2.  grid (points), one workgroup each: the tile aggregates from the top, OPEN_SPAN at a time;
// tilec[point][tile] = Q at the first index of tile + 1 (0 for the top tile), ys[point] = Q_0
// (32 B big-endian)
template <class Cv>
__global__ void __launch_bounds__(OPEN_BLOCK) k_open_carry(const uint32_t* __restrict__ zp, const uint32_t* __restrict__ tilev,
                                                           uint32_t tiles, uint32_t* __restrict__ tilec,
                                                           uint8_t* __restrict__ ys) {
  using R = typename Cv::FrP;
  __shared__ uint32_t sh[8][OPEN_BLOCK];
  const uint32_t t = threadIdx.x, pt = blockIdx.x;
  const Fp<R>* zpp = reinterpret_cast<const Fp<R>*>(zp) + (size_t)pt * OPEN_POWERS;
  Fp<R> carry = Fp<R>::zero();  // Q at the first index above the span (every thread holds it)
#pragma unroll 1
  for (uint32_t base = (tiles + OPEN_SPAN - 1) / OPEN_SPAN * OPEN_SPAN; base > 0;) {
    base -= OPEN_SPAN;
    const uint32_t tile = base + t;
    Fp<R> v = tile < tiles ? open_load<R>(tilev + 8 * ((size_t)pt * tiles + tile)) : Fp<R>::zero();
    if (t == OPEN_SPAN - 1) v = fp_add(v, fp_mul(zpp[OPEN_LOG_TILE], carry));
    const Fp<R> s = open_scan<R>(v, zpp + OPEN_LOG_TILE, sh, t);
    Fp<R> first;
    const Fp<R> cin = open_next<R>(s, carry, sh, t, &first);
    if (tile < tiles) open_store<R>(tilec + 8 * ((size_t)pt * tiles + tile), cin);
    carry = first;
  }
  if (t == 0) open_store_be<R>(ys + 32 * (size_t)pt, carry);
}

// Pass 3.  grid (tiles, points); q: point p's m - 1 values from q + 8 (m - 1) p (BE: bytes, as 32 (m - 1) p)
template <class Cv, bool BE>
__global__ void __launch_bounds__(OPEN_BLOCK) k_open_quotient(const uint32_t* __restrict__ coef, uint32_t m,
                                                              const uint32_t* __restrict__ zp,
                                                              const uint32_t* __restrict__ runv,
                                                              const uint32_t* __restrict__ tilec, uint32_t* __restrict__ q) {
  using R = typename Cv::FrP;
  __shared__ uint32_t sh[8][OPEN_BLOCK];
  const uint32_t t = threadIdx.x, tile = blockIdx.x, pt = blockIdx.y, tiles = gridDim.x;
  const Fp<R>* zpp = reinterpret_cast<const Fp<R>*>(zp) + (size_t)pt * OPEN_POWERS;
  const Fp<R> tc = open_load<R>(tilec + 8 * ((size_t)pt * tiles + tile));
  Fp<R> v = open_load<R>(runv + 8 * (((size_t)pt * tiles + tile) * OPEN_BLOCK + t));
  if (t == OPEN_BLOCK - 1) v = fp_add(v, fp_mul(zpp[OPEN_LOG_RUN], tc));
  const Fp<R> s = open_scan<R>(v, zpp + OPEN_LOG_RUN, sh, t);
  const Fp<R> cin = open_next<R>(s, tc, sh, t, nullptr);
  const uint32_t lo = tile * OPEN_TILE + t * OPEN_RUN;
  if (lo >= m) return;
  (void)open_horner<R, true, BE>(coef, m, lo, zpp[0], cin, q + 8 * (size_t)(m - 1) * pt);
}

}  // namespace kzgmi
