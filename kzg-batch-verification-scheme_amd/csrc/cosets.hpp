// FK20 multi-proofs on every coset of a domain (kzgmi_open_cosets*), both curves, any power-of-two
// shape: N = 2^logN coefficients, cosets of l = 2^logl points, R = N / l.  DESIGN.md 3j; the
// definitions are restated in include/kzgmi.h and tests/opencosetsref.py.  The Fr passes, the G1
// stages, the bit reversal and the encoding are those of ntt.hpp and g1ntt.hpp; what is here is what
// lies between them:
//
//   hhat[pos] = sum_{b<l} [ahat^(b)[pos]] xhat^(b)[pos],   pos < 2R, per polynomial
//
// and the gathers around it.  A *term* is one scalar multiple; the terms of a call are numbered
//   g = (P l + b),   P = t 2R + pos   (polynomial t, position pos, column b)
// so that the l terms of a position are consecutive and the key, stored [pos][b], is read at
// g mod 2N.  ahat comes out of the batched Fr passes as count * l transforms of 2R values,
// [t][b][pos]; k_cosets_scal puts it in term order, so the lanes of a wave read consecutive scalars
// as they read consecutive key records.
//
// k_cosets_mul is the throughput form: a thread per term with g1ntt_mul as it is, then the wave sums
// its terms in segments of min(l, 64) lanes through the workgroup's table LDS, which the products
// no longer need (cosets_wave_sum).  Where l > 64 the l / 64 sums of a position are records of their
// own and k_cosets_fold, the same sum without the product, brings them together 64 at a time in
// launches of its own: no wave waits for another.  k_cosets_mul_wave is the latency form, a wave
// per term in the lane-parallel arithmetic (k_g1ntt_stage_wave's product); its terms are summed by
// the same fold.  Sums use the complete xyzz_add: a degenerate SRS brings equal points, opposite
// points and infinities.
#pragma once
#include "g1ntt.hpp"

namespace kzgmi {

// the sum of `seg` consecutive lanes' points (seg a power of two <= 64, segments aligned), left in every
// lane of the segment: log2(seg) exchanges through row 0 of the workgroup's table.  Every lane of the
// workgroup (one wave) calls it; idle lanes pass infinity.
template <class Cv>
KZ_DEV Xyzz<Cv> cosets_wave_sum(Xyzz<Cv> acc, uint32_t seg, uint32_t* tab, uint32_t lane) {
#pragma unroll 1
  for (uint32_t d = 1; d < seg; d <<= 1) {
    g1ntt_tab_store<Cv>(tab, 0, lane, acc);
    __syncthreads();
    const Xyzz<Cv> q = g1ntt_tab_load<Cv>(tab, 0, lane ^ d);
    __syncthreads();
    acc = xyzz_add(acc, q);
  }
  return acc;
}

// the scalars in term order: out[(t 2R + pos) l + b] = ahat[(t l + b) 2R + pos] (8 LE words each, ahat != out)
static __global__ void __launch_bounds__(256) k_cosets_scal(const uint32_t* __restrict__ ahat, uint32_t logN, uint32_t logl,
                                                            uint32_t terms, uint32_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= terms) return;
  const uint32_t logr2 = logN - logl + 1;  // log2(2R)
  const uint32_t b = g & ((1u << logl) - 1), P = g >> logl, pos = P & ((1u << logr2) - 1), t = P >> logr2;
  uint32_t w[8];
  load_words(reinterpret_cast<const uint8_t*>(ahat + 8 * ((((size_t)t << logl) + b) << logr2) + 8 * (size_t)pos), w);
  store_words(reinterpret_cast<uint8_t*>(out + 8 * (size_t)g), w);
}

// Thread form.  terms = count 2N; key: [pos][b] records (2N); scal: term order, 8 canonical LE words;
// out[g / seg], seg = min(l, 64): the sum of the segment's products
template <class Cv>
__global__ void __launch_bounds__(G1NTT_THREADS) k_cosets_mul(const Xyzz<Cv>* __restrict__ key, const uint32_t* __restrict__ scal,
                                                              uint32_t logN, uint32_t logl, uint32_t terms,
                                                              Xyzz<Cv>* __restrict__ out) {
  __shared__ uint32_t tab[kG1nttLdsWords<Cv>];
  const uint32_t lane = threadIdx.x, g = blockIdx.x * G1NTT_THREADS + lane;
  Xyzz<Cv> p = Xyzz<Cv>::inf();
  if (g < terms) {
    p = load_xyzz(&key[g & ((2u << logN) - 1)]);
    if (!p.is_inf()) {
      uint32_t k[8];
      load_words(reinterpret_cast<const uint8_t*>(scal + 8 * (size_t)g), k);
      p = g1ntt_mul<Cv>(p, k, tab, lane);
    }
  }
  __syncthreads();  // the products' table rows are free from here on
  const uint32_t lseg = logl < 6 ? logl : 6;
  p = cosets_wave_sum<Cv>(p, 1u << lseg, tab, lane);
  if (g < terms && (lane & ((1u << lseg) - 1)) == 0) store_xyzz(&out[g >> lseg], p);
}

// out[i] = in[i seg] + .. + in[i seg + seg - 1] for i < nout (seg a power of two <= 64)
template <class Cv>
__global__ void __launch_bounds__(G1NTT_THREADS) k_cosets_fold(const Xyzz<Cv>* __restrict__ in, uint32_t lseg, uint32_t nout,
                                                               Xyzz<Cv>* __restrict__ out) {
  __shared__ uint32_t tab[kG1nttPointWords<Cv> * G1NTT_THREADS];
  const uint32_t lane = threadIdx.x, g = blockIdx.x * G1NTT_THREADS + lane;
  const bool live = (g >> lseg) < nout;
  Xyzz<Cv> p = Xyzz<Cv>::inf();
  if (live) p = load_xyzz(&in[g]);
  p = cosets_wave_sum<Cv>(p, 1u << lseg, tab, lane);
  if (live && (lane & ((1u << lseg) - 1)) == 0) store_xyzz(&out[g >> lseg], p);
}

// Wave form: block g is term g; out[g] = [scal] key (no sum: k_cosets_fold follows)
template <class Cv>
__global__ void __launch_bounds__(64) k_cosets_mul_wave(const Xyzz<Cv>* __restrict__ key, const uint32_t* __restrict__ scal,
                                                        uint32_t logN, Xyzz<Cv>* __restrict__ out) {
  const LpCtx<Cv> c = lp_ctx<Cv>();
  const uint32_t g = blockIdx.x;
  LpXyzz<Cv> p = lp_load_xyzz(c, &key[g & ((2u << logN) - 1)]);
  if (!p.inf) {
    const uint32_t* sw = scal + 8 * (size_t)g;
    uint32_t kk[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) kk[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw[q]);
    p = small_mul<Cv, 8>(c, p, kk);  // a zero scalar leaves infinity
  }
  lp_store_xyzz(c, &out[g], p);
}

// The key's l vectors x^(b) of length 2R, [b][i]: x^(b)[0] = S_b, x^(b)[2R - u] = S_{l u + b} (u = 1 .. R - 2),
// infinity elsewhere (k_g1ntt_key_x with a stride); S: the commit key's resident row of powers
template <class Cv>
__global__ void __launch_bounds__(256) k_cosets_key_x(const Affine<Cv>* __restrict__ srs29, const uint8_t* __restrict__ srs_inf,
                                                      uint32_t logN, uint32_t logl, Xyzz<Cv>* __restrict__ x) {
  using Q = Fp29Of<Cv>;
  using P = typename Cv::FpP;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (2u << logN)) return;
  const uint32_t logr2 = logN - logl + 1, r2 = 1u << logr2;
  const uint32_t i = g & (r2 - 1), b = g >> logr2, u = (r2 - i) & (r2 - 1);
  const uint32_t src = (u << logl) + b;  // <= N - l - 1 where it is read
  Xyzz<Cv> p = Xyzz<Cv>::inf();
  if (u + 1 < (r2 >> 1) && !srs_inf[src]) {  // u <= R - 2
    F29<Q> x29, y29;
    load_pt29<Cv>(srs29 + src, x29, y29);
    Affine<Cv> a;
    a.x = fp_from29<Q, P>(x29);
    a.y = fp_from29<Q, P>(y29);
    p = xyzz_from_affine(a);
  }
  store_xyzz(&x[g], p);
}

// the key as the products read it: out[pos l + b] = xs[b 2R + rev(pos)], xs the stages' bit-reversed output
template <class Cv>
__global__ void __launch_bounds__(256) k_cosets_key_gather(const Xyzz<Cv>* __restrict__ xs, uint32_t logN, uint32_t logl,
                                                           Xyzz<Cv>* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (2u << logN)) return;
  const uint32_t logr2 = logN - logl + 1, b = g & ((1u << logl) - 1), pos = g >> logl;
  store_xyzz(&out[g], load_xyzz(&xs[((size_t)b << logr2) + ntt_rev(pos, logr2)]));
}

// a[(t l + b) 2^loglen + u] = c_t[l u + b] for u < ulim and l u + b < m, else 0 (8 LE words each): the strided
// pad of the l convolutions (loglen = log2 2R, ulim = R) and, with logl = 0, the plain pad to 2^loglen
static __global__ void __launch_bounds__(256) k_cosets_pad(const uint32_t* __restrict__ coef, uint32_t m, uint32_t logl,
                                                           uint32_t loglen, uint32_t ulim, uint32_t total,
                                                           uint32_t* __restrict__ a) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint32_t u = g & ((1u << loglen) - 1), tb = g >> loglen, b = tb & ((1u << logl) - 1), t = tb >> logl;
  const uint32_t src = (u << logl) + b;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (u < ulim && src < m) load_words(reinterpret_cast<const uint8_t*>(coef + 8 * ((size_t)t * m + src)), w);
  store_words(reinterpret_cast<uint8_t*>(a + 8 * (size_t)g), w);
}

// d[t K + j] = H_j of polynomial t for j <= R - 2, infinity for R - 1 <= j < K, out of the inverse
// 2R-point transforms' bit-reversed output: H_j = ihat[t 2R + rev(j + 1)]
template <class Cv>
__global__ void __launch_bounds__(256) k_cosets_shift(const Xyzz<Cv>* __restrict__ ihat, uint32_t logr2, uint32_t logk,
                                                      uint32_t total, Xyzz<Cv>* __restrict__ d) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint32_t j = g & ((1u << logk) - 1), t = g >> logk;
  Xyzz<Cv> p = Xyzz<Cv>::inf();
  if (j + 1 < (1u << logr2 >> 1)) p = load_xyzz(&ihat[((size_t)t << logr2) + ntt_rev(j + 1, logr2)]);
  store_xyzz(&d[g], p);
}

// coset-major order: out[t n + e l + j] = y[t n + e + K j] (32-byte values, n = K l)
static __global__ void __launch_bounds__(256) k_cosets_ys(const uint4* __restrict__ y, uint32_t logk, uint32_t logl,
                                                          uint32_t total, uint4* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint32_t n1 = (1u << (logk + logl)) - 1, i = g & n1, e = i >> logl, j = i & ((1u << logl) - 1);
  const size_t src = (size_t)(g & ~n1) + e + ((size_t)j << logk);
  out[2 * (size_t)g] = y[2 * src];
  out[2 * (size_t)g + 1] = y[2 * src + 1];
}

}  // namespace kzgmi
