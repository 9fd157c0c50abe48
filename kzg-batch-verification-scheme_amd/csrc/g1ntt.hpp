// Power-of-two transforms over G1, both curves, n = 2^0 .. 2^20, batched (kzgmi_g1_ntt*), and the
// kernels around them that turn a polynomial into its n openings on <w_n> (kzgmi_open_all*).
// DESIGN.md 3i; the definitions are restated in include/kzgmi.h, tests/g1nttref.py and
// tests/openallref.py.  w_n is the root of ntt.hpp.
//
// A transform is logn radix-2 decimation-in-frequency stages over XYZZ records in HBM, in place:
// the stage of span `half` pairs elements i0 and i0 + half of every transform,
//   (a, b) -> (a + b, [w_{2 half}^(+-k)] (a - b)),   k = i0 mod half,
// and stages half = n/2 .. 1 take natural order to bit-reversed order.  What the call's order flags
// ask beyond that is a gather: on the load from the affine input (k_g1ntt_from_affine) or in one
// permutation before the encoding (k_g1ntt_rev).
//
// k_g1ntt_stage is the throughput form: a thread per butterfly, the points in registers, the complete
// formulas of g1.hpp inlined (butterflies meet P = +-Q and infinity on ordinary inputs).  The sum is
// stored before the product starts; the product is a fixed-window double-and-add over the twiddle's
// canonical bits (g1ntt_mul): the lanes of a wave hold different scalars, so a wave pays for an
// addition in every window whatever the digits are, and G1NTT_WBITS = 2 halves those against
// bit-by-bit.  The window's multiples P, 2P, 3P of each lane sit in LDS, word-planar
// ([multiple][word][lane]: a lane's words are G1NTT_THREADS apart, every access is conflict-free
// whichever multiples the lanes pick).  A butterfly whose twiddle is 1, or whose difference is
// infinity, multiplies nothing.  The twiddle is one product of the two-level root table of ntt.hpp
// and one conversion out of Montgomery form per butterfly.
//
// The factor n^-1 of an inverse transform is one scalar multiplication per point (k_g1ntt_mul with
// no scalar array), run behind the stages; kzgmi_open_all folds its 1 / (2n) into the Fr scalars
// instead and never runs it.  The same kernel with a scalar array is open_all's pointwise product.
#pragma once
#include "msm_small.hpp"
#include "ntt.hpp"

namespace kzgmi {

// (G1NTT_MAX_LOGN and OPEN_ALL_MAX_LOGN, the bounds of a call, are host-side: launch.hpp)
constexpr uint32_t G1NTT_THREADS = 64;    // a workgroup of the multiplying kernels: one wave
constexpr int G1NTT_WBITS = 2;            // window of the double-and-add
constexpr int G1NTT_WINDOWS = 256 / G1NTT_WBITS;  // over all 256 bits of the scalar's 8 words
constexpr int G1NTT_MULTS = (1 << G1NTT_WBITS) - 1;  // multiples 1 .. 3 per lane
static_assert(G1NTT_WINDOWS * G1NTT_WBITS == 256, "the windows tile the scalar's words");

template <class Cv>
constexpr uint32_t kG1nttPointWords = 4 * Cv::FpP::N;
template <class Cv>
constexpr uint32_t kG1nttLdsWords = G1NTT_MULTS * kG1nttPointWords<Cv> * G1NTT_THREADS;  // 36 KiB / 24 KiB

template <class Cv>
KZ_DEV void g1ntt_tab_store(uint32_t* tab, uint32_t m, uint32_t lane, const Xyzz<Cv>& p) {
  constexpr int N = Cv::FpP::N;
  uint32_t* t = tab + m * kG1nttPointWords<Cv> * G1NTT_THREADS + lane;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    t[k * G1NTT_THREADS] = p.x.v[k];
    t[(N + k) * G1NTT_THREADS] = p.y.v[k];
    t[(2 * N + k) * G1NTT_THREADS] = p.zz.v[k];
    t[(3 * N + k) * G1NTT_THREADS] = p.zzz.v[k];
  }
}
template <class Cv>
KZ_DEV Xyzz<Cv> g1ntt_tab_load(const uint32_t* tab, uint32_t m, uint32_t lane) {
  constexpr int N = Cv::FpP::N;
  const uint32_t* t = tab + m * kG1nttPointWords<Cv> * G1NTT_THREADS + lane;
  Xyzz<Cv> p;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    p.x.v[k] = t[k * G1NTT_THREADS];
    p.y.v[k] = t[(N + k) * G1NTT_THREADS];
    p.zz.v[k] = t[(2 * N + k) * G1NTT_THREADS];
    p.zzz.v[k] = t[(3 * N + k) * G1NTT_THREADS];
  }
  return p;
}

// [k] p for the integer k (8 little-endian words, consumed), any p on the curve: the windows from the
// top, two doublings and at most one addition each.  tab: the workgroup's kG1nttLdsWords words; only
// this lane's words of it are touched, so no barrier is needed and lanes may skip the call.
template <class Cv>
KZ_DEV Xyzz<Cv> g1ntt_mul(const Xyzz<Cv>& p, uint32_t (&k)[8], uint32_t* tab, uint32_t lane) {
  g1ntt_tab_store<Cv>(tab, 0, lane, p);
  Xyzz<Cv> q = xyzz_dbl(p);
  g1ntt_tab_store<Cv>(tab, 1, lane, q);
  q = xyzz_add(q, p);
  g1ntt_tab_store<Cv>(tab, 2, lane, q);
  Xyzz<Cv> acc = Xyzz<Cv>::inf();
#pragma unroll 1
  for (int w = 0; w < G1NTT_WINDOWS; ++w) {
#pragma unroll 1
    for (int i = 0; i < G1NTT_WBITS; ++i) acc = xyzz_dbl(acc);  // infinity stays infinity
    const uint32_t d = k[7] >> (32 - G1NTT_WBITS);
#pragma unroll
    for (int i = 7; i > 0; --i) k[i] = (k[i] << G1NTT_WBITS) | (k[i - 1] >> (32 - G1NTT_WBITS));
    k[0] <<= G1NTT_WBITS;
    if (d) acc = xyzz_add(acc, g1ntt_tab_load<Cv>(tab, d - 1, lane));
  }
  return acc;
}

// One stage of span 2^ls over `nbfly` = count * n / 2 butterflies (logn >= 1), a thread each
template <class Cv>
__global__ void __launch_bounds__(G1NTT_THREADS) k_g1ntt_stage(Xyzz<Cv>* __restrict__ data, uint32_t nbfly, uint32_t logn,
                                                               uint32_t ls, uint32_t inverse,
                                                               const uint32_t* __restrict__ roots) {
  using R = typename Cv::FrP;
  __shared__ uint32_t tab[kG1nttLdsWords<Cv>];
  const uint32_t g = blockIdx.x * G1NTT_THREADS + threadIdx.x;
  if (g >= nbfly) return;
  const uint32_t half = 1u << ls;
  const uint32_t j = g & ((1u << (logn - 1)) - 1), k = j & (half - 1), i0 = ((j - k) << 1) | k;
  Xyzz<Cv>* x = data + ((size_t)(g >> (logn - 1)) << logn);
  const Xyzz<Cv> a = load_xyzz(&x[i0]);
  const Xyzz<Cv> b = load_xyzz(&x[i0 + half]);
  store_xyzz(&x[i0], xyzz_add(a, b));
  Xyzz<Cv> d = xyzz_add(a, xyzz_neg(b));
  uint32_t e = k << (NTT_ROOT_BITS - 1 - ls);  // w_{2 half}^k = w_{2^26}^e, e < 2^25
  if (e != 0 && !d.is_inf()) {
    if (inverse) e = (1u << NTT_ROOT_BITS) - e;
    Fp<R> w = fp_from_mont(ntt_two_level<R>(roots, e));
    d = g1ntt_mul<Cv>(d, w.v, tab, threadIdx.x);
  }
  store_xyzz(&x[i0 + half], d);
}

// The latency form of the same stage: a wave per butterfly in the lane-parallel arithmetic of lpfield.hpp
// (k_fk20_bfly of fk20.hpp for any curve, size and root): one scalar multiplication takes a fraction of
// a millisecond instead of several, at about a third of the thread form's throughput.  Stages of at
// most G1NTT_WAVE_MAX_BFLY butterflies take it (launch_g1ntt.hip; DESIGN.md 3i for the measurement).
constexpr uint32_t G1NTT_WAVE_MAX_BFLY = 1u << 14;
template <class Cv>
__global__ void __launch_bounds__(64) k_g1ntt_stage_wave(Xyzz<Cv>* __restrict__ data, uint32_t logn, uint32_t ls,
                                                         uint32_t inverse, const uint32_t* __restrict__ roots) {
  using R = typename Cv::FrP;
  const LpCtx<Cv> c = lp_ctx<Cv>();
  const uint32_t g = blockIdx.x, half = 1u << ls;
  const uint32_t j = g & ((1u << (logn - 1)) - 1), k = j & (half - 1), i0 = ((j - k) << 1) | k;
  Xyzz<Cv>* x = data + ((size_t)(g >> (logn - 1)) << logn);
  const LpXyzz<Cv> a = lp_load_xyzz(c, &x[i0]);
  LpXyzz<Cv> b = lp_load_xyzz(c, &x[i0 + half]);
  const LpXyzz<Cv> s = lp_xyzz_add(c, a, b);
  b.y = lp_sub(c, 0, b.y);
  LpXyzz<Cv> d = lp_xyzz_add(c, a, b);
  uint32_t e = k << (NTT_ROOT_BITS - 1 - ls);
  if (e != 0 && !d.inf) {
    if (inverse) e = (1u << NTT_ROOT_BITS) - e;
    const Fp<R> w = fp_from_mont(ntt_two_level<R>(roots, e));  // the same in every lane
    uint32_t kk[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) kk[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.v[q]);
    d = small_mul<Cv, 8>(c, d, kk);
  }
  lp_store_xyzz(c, &x[i0], s);
  lp_store_xyzz(c, &x[i0 + half], d);
}

// out[i] = [scal[i]] in[i] (scal: 8 canonical little-endian words per point), or with scal == nullptr
// [2^-logn] in[i]: a thread per point.  in == out is allowed.  Infinity is never multiplied.
template <class Cv>
__global__ void __launch_bounds__(G1NTT_THREADS) k_g1ntt_mul(const Xyzz<Cv>* in, const uint32_t* __restrict__ scal,
                                                             uint32_t logn, uint32_t total, Xyzz<Cv>* out) {
  using R = typename Cv::FrP;
  __shared__ uint32_t tab[kG1nttLdsWords<Cv>];
  const uint32_t i = blockIdx.x * G1NTT_THREADS + threadIdx.x;
  if (i >= total) return;
  Xyzz<Cv> p = load_xyzz(&in[i]);
  if (!p.is_inf()) {
    uint32_t k[8];
    if (scal) {
      load_words(reinterpret_cast<const uint8_t*>(scal + 8 * (size_t)i), k);
    } else {  // 1 / n = r - (r - 1) / n; r - 1 and r differ in bit 0 only
      Fp<R> q;
#pragma unroll
      for (int w = 0; w < 8; ++w) q.v[w] = R::MOD[w];
      q.v[0] &= ~1u;
#pragma unroll 1
      for (uint32_t s = 0; s < logn; ++s) {
#pragma unroll
        for (int w = 0; w < 8; ++w) q.v[w] = (q.v[w] >> 1) | (w < 7 ? q.v[w + 1] << 31 : 0u);
      }
      q = fp_neg(q);
#pragma unroll
      for (int w = 0; w < 8; ++w) k[w] = q.v[w];
    }
    p = g1ntt_mul<Cv>(p, k, tab, threadIdx.x);
  }
  store_xyzz(&out[i], p);
}

// validated affine points and their infinity flags -> records; rev: record i of a transform takes
// point rev_logn(i) of it
template <class Cv>
__global__ void __launch_bounds__(256) k_g1ntt_from_affine(const Affine<Cv>* __restrict__ pts, const uint8_t* __restrict__ inf,
                                                           uint32_t total, uint32_t logn, uint32_t rev,
                                                           Xyzz<Cv>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t n1 = (1u << logn) - 1, src = rev ? (i & ~n1) | ntt_rev(i & n1, logn) : i;
  store_xyzz(&out[i], inf[src] ? Xyzz<Cv>::inf() : xyzz_from_affine(load_affine(pts, src)));
}

// out[i] = in[rev_logn(i)] within every transform (in != out)
template <class Cv>
__global__ void __launch_bounds__(256) k_g1ntt_rev(const Xyzz<Cv>* __restrict__ in, uint32_t logn, uint32_t total,
                                                   Xyzz<Cv>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t n1 = (1u << logn) - 1;
  store_xyzz(&out[i], load_xyzz(&in[(i & ~n1) | ntt_rev(i & n1, logn)]));
}

// ------------------------------------------------------------------------------ kzgmi_open_all
// The key's vector x of length 2n = 2^(logn + 1): x[0] = S_0, x[2n - u] = S_u (u = 1 .. n - 2),
// infinity elsewhere; S: the commit key's resident row of powers, in the accumulation's format
template <class Cv>
__global__ void __launch_bounds__(256) k_g1ntt_key_x(const Affine<Cv>* __restrict__ srs29, const uint8_t* __restrict__ srs_inf,
                                                     uint32_t logn, Xyzz<Cv>* __restrict__ x) {
  using Q = Fp29Of<Cv>;
  using P = typename Cv::FpP;
  const uint32_t n = 1u << logn, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n) return;
  const uint32_t u = (2 * n - i) & (2 * n - 1);
  Xyzz<Cv> p = Xyzz<Cv>::inf();
  if (u + 1 < n && !srs_inf[u]) {  // u <= n - 2: below the key's n - 1 points
    F29<Q> x29, y29;
    load_pt29<Cv>(srs29 + u, x29, y29);
    Affine<Cv> a;
    a.x = fp_from29<Q, P>(x29);
    a.y = fp_from29<Q, P>(y29);
    p = xyzz_from_affine(a);
  }
  store_xyzz(&x[i], p);
}

// d = (h_0 .. h_{n-2}, infinity) out of the inverse 2n-point transform's bit-reversed output:
// h_t = ihat[t + 1]
template <class Cv>
__global__ void __launch_bounds__(256) k_g1ntt_shift(const Xyzz<Cv>* __restrict__ ihat, uint32_t logn,
                                                     Xyzz<Cv>* __restrict__ d) {
  const uint32_t n = 1u << logn, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Xyzz<Cv> p = Xyzz<Cv>::inf();
  if (t + 1 < n) p = load_xyzz(&ihat[ntt_rev(t + 1, logn + 1)]);
  store_xyzz(&d[t], p);
}

// a = (c_0 .. c_{m-1}, 0 ..) of 2^lg values, 8 little-endian words each
static __global__ void __launch_bounds__(256) k_g1ntt_pad(const uint32_t* __restrict__ coef, uint32_t m, uint32_t total,
                                                          uint32_t* __restrict__ a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (i < m) load_words(reinterpret_cast<const uint8_t*>(coef + 8 * (size_t)i), w);
  store_words(reinterpret_cast<uint8_t*>(a + 8 * (size_t)i), w);
}

// v[i] <- v[i] / 2^lg mod r in place (standard form, 8 little-endian words): lg halvings
template <class Cv>
__global__ void __launch_bounds__(256) k_g1ntt_halve(uint32_t* __restrict__ v, uint32_t lg, uint32_t total) {
  using R = typename Cv::FrP;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  uint32_t a[8];
  load_words(reinterpret_cast<const uint8_t*>(v + 8 * (size_t)i), a);
#pragma unroll 1
  for (uint32_t h = 0; h < lg; ++h) {
    uint32_t s[9], c = 0;
    const bool odd = (a[0] & 1u) != 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = __builtin_addc(a[q], odd ? R::MOD[q] : 0u, c, &c);
    s[8] = c;
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = (s[q] >> 1) | (s[q + 1] << 31);
  }
  store_words(reinterpret_cast<uint8_t*>(v + 8 * (size_t)i), a);
}

}  // namespace kzgmi
