// EIP-7594 (PeerDAS) cell proof generation, the FK20 way: all 128 proofs of a blob from one
// batched fixed-base MSM and two size-128 transforms over G1.  BLS12-381 only.  Reference: none
// (LICENSE only); the definitions are restated in include/kzgmi.h and tests/fk20ref.py.
//
//   p(X) = sum_{j < 4096} c_j X^j (c = dit_inv(blob) / 4096 as in k_compute_cells), omega = w^64
//   (order 128), S_m = [tau^m]_1:   proof_i = [floor(p / (X^64 - h_i^64))(tau)]_1 = P_{rev7(i)}
//   P_e = sum_{t < 63} omega^(e t) H_t,   H_t = sum_{b < 64} sum_{u <= 62 - t} c_{64 (u + t + 1) + b} S_{64 u + b}
// H is a sum of 64 cyclic convolutions of length 128: with a^(b) = (c_b, c_{64 + b}, .., c_{64 63 + b},
// 0 x 64) and x^(b)[0] = S_b, x^(b)[128 - u] = S_{64 u + b} (u = 1 .. 62), infinity elsewhere,
//   hhat[pos] = sum_b DFT(a^(b))[pos] DFT(x^(b))[pos],   H_t = IDFT(hhat)[t + 1]   (t < 63)
// (the other entries of the inverse transform are discarded).  xhat = DFT(x^(b)) depends on the SRS
// only: the proof key holds its 8192 points as a table of window multiples.
//
// Per call, on the slot's stream:
//   k_fk20_coeffs   one workgroup per blob: range check, dit_inv, scale by 1 / (4096 * 128) (the
//                   inverse transform's 1 / 128 is folded in here: no scalar multiplication for it)
//   k_fk20_dft      ahat: block (b, blob) transforms a^(b) directly (64 products per output; the
//                   8192 outputs of a blob spread over 64 blocks)
//   k_fk20_msm      hhat: one block per output, thread (b, part) adds the table rows of its windows
//                   of ahat^(b)[pos] (signed FK_WBITS-bit digits: no doublings, no buckets), then a
//                   fixed-order tree in LDS joins the 256 partial sums
//   k_fk20_bfly     one radix-2 decimation-in-frequency stage over G1, a wave per butterfly in
//                   lane-parallel arithmetic: 7 launches for the inverse transform (natural order
//                   in, bit-reversed out), k_fk20_shift, 7 for the forward one, whose bit-reversed
//                   output order is the cell order.  A butterfly whose twiddle is 1 multiplies nothing
//   encode, compress (kernels.hpp, points.hpp), k_fk20_emit (nothing is written once an error is raised)
#pragma once
#include "msm_small.hpp"
#include "recover.hpp"

namespace kzgmi {

using FkCv = Bls12_381;
using FkXY = Xyzz<FkCv>;
using FkAF = Affine<FkCv>;

constexpr uint32_t FK_N = 128;                    // transform size (cells per extended blob)
constexpr uint32_t FK_COLS = 64;                  // the b of a^(b), x^(b)
constexpr uint32_t FK_BASES = FK_N * FK_COLS;     // xhat: base pos * 64 + b
constexpr uint32_t FK_H = 63;                     // H_0 .. H_62
constexpr int FK_WBITS = 4;                       // window width of the fixed-base table
constexpr int FK_WINDOWS = (255 + FK_WBITS) / FK_WBITS;  // signed digits of a scalar < 2^255: its top bit is 0, no carry out
constexpr int FK_MULTS = 1 << (FK_WBITS - 1);     // |digit| <= FK_MULTS: multiples 1 .. FK_MULTS per row
constexpr int FK_PARTS = 4;                       // threads per (output, base): FK_WINDOWS / FK_PARTS windows each
constexpr int FK_MSM_THREADS = FK_COLS * FK_PARTS;
constexpr size_t FK_TABLE_POINTS = (size_t)FK_BASES * FK_WINDOWS * FK_MULTS;
static_assert(FK_WINDOWS % FK_PARTS == 0, "every part takes the same number of windows");
static_assert(FK_WINDOWS * FK_WBITS >= 256, "the top window's sign bit is bit 255 or above: zero");

KZ_DEV uint32_t fk_rev7(uint32_t i) { return __brev(i) >> 25; }

KZ_DEV BlobF fk_half(const BlobF& a) {  // a / 2 mod r, in either form
  uint32_t s[9], c = 0;
  const bool odd = (a.v[0] & 1u) != 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = __builtin_addc(a.v[i], odd ? BlobR::MOD[i] : 0u, c, &c);
  s[8] = c;
  BlobF r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (s[i] >> 1) | (s[i + 1] << 31);
  return r;
}

// ------------------------------------------------------------------------------ Fr stage
// c_m * 2^-halvings of blob b -> coef[4096 b + m], standard form (8 LE words); blobs are `stride`
// bytes apart (a recovered blob is the first half of its 256 KiB of cells)
static __global__ void __launch_bounds__(NTT_THREADS) k_fk20_coeffs(const uint8_t* __restrict__ blobs, size_t stride,
                                                                    const BlobF* __restrict__ table, int halvings,
                                                                    BlobF* __restrict__ coef,
                                                                    uint32_t* __restrict__ err) {
  __shared__ uint32_t x[8 * NTT_N];
  const uint32_t t = threadIdx.x;
  const uint8_t* blob = blobs + (size_t)blockIdx.x * stride;
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
    ntt_st(x, k, e);
  }
  ntt_dit_inv(x, table + NTT_T_TW);
  BlobF scale = table[NTT_T_CW];  // 1 / 4096
  for (int h = 0; h < halvings; ++h) scale = fk_half(scale);
#pragma unroll
  for (int q = 0; q < NTT_PER; ++q) {
    const uint32_t m = t + NTT_THREADS * q;
    const BlobF c = fp_mul(scale, ntt_ld(x, m));
    store_words(reinterpret_cast<uint8_t*>(coef + (size_t)blockIdx.x * NTT_N + m), c.v);
  }
}

// ahat^(b)[pos] = sum_{v < 64} c_{64 v + b} omega^(pos v): block (b, blob), thread pos; 32 B
// big-endian at 32 ((128 blob + pos) 64 + b), the 64 scalars of one MSM output side by side
static __global__ void __launch_bounds__(FK_N) k_fk20_dft(const BlobF* __restrict__ coef, const BlobF* __restrict__ tw,
                                                          uint8_t* __restrict__ out) {
  __shared__ BlobF a[FK_COLS];
  const uint32_t b = blockIdx.x, blob = blockIdx.y, pos = threadIdx.x;
  if (pos < FK_COLS) a[pos] = coef[(size_t)blob * NTT_N + FK_COLS * pos + b];
  __syncthreads();
  BlobF acc = a[0];
#pragma unroll 1
  for (uint32_t v = 1; v < FK_COLS; ++v) acc = fp_add(acc, fp_mul(tw[((pos * v) & (FK_N - 1)) << 6], a[v]));
  uint32_t wo[8];
  fp_to_be_words(acc, wo, 0);
  store_words(out + (((size_t)blob * FK_N + pos) * FK_COLS + b) * 32, wo);
}

// ------------------------------------------------------------------------------ fixed-base MSM
// digit w of k (8 LE words, k < 2^255), signed: -2^(c-1) b_{cw+c-1} + (bits cw .. cw+c-2) + b_{cw-1}
KZ_DEV int fk_digit(const uint32_t (&k)[8], int w) {
  const int lo = FK_WBITS * w - 1;
  uint32_t u;
  if (lo < 0) {
    u = (k[0] << 1) & ((2u << FK_WBITS) - 1u);
  } else {
    const int wi = lo >> 5, sh = lo & 31;
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i == wi) v |= (uint64_t)k[i];
      if (i == wi + 1) v |= (uint64_t)k[i] << 32;
    }
    u = (uint32_t)(v >> sh) & ((2u << FK_WBITS) - 1u);
  }
  return (int)((u + 1u) >> 1) - (int)((u >> FK_WBITS) << FK_WBITS);
}

// hhat[blob][pos] = sum_b ahat^(b)[pos] xhat^(b)[pos]: block (blob, pos), thread t = b + 64 part.
// tab[(base FK_WINDOWS + w) FK_MULTS + m - 1] = m 2^(c w) xhat[base], affine; tab_inf[base]: xhat[base]
// is the point at infinity (its rows are not read).  Partial sums may meet as P = +-Q: the complete
// formulas throughout, inlined (the out-of-line forms pass their operands through the stack: 896 B
// of scratch per lane here, against none).
static __global__ void __launch_bounds__(FK_MSM_THREADS) k_fk20_msm(const uint8_t* __restrict__ scal,
                                                                    const FkAF* __restrict__ tab,
                                                                    const uint8_t* __restrict__ tab_inf,
                                                                    FkXY* __restrict__ out) {
  __shared__ __align__(16) FkXY part[FK_MSM_THREADS];
  const uint32_t t = threadIdx.x, b = t & (FK_COLS - 1), pt = t / FK_COLS;
  const uint32_t pos = blockIdx.x & (FK_N - 1), base = pos * FK_COLS + b;
  FkXY acc = FkXY::inf();
  if (!tab_inf[base]) {
    uint32_t we[8], k[8];
    load_words(scal + ((size_t)blockIdx.x * FK_COLS + b) * 32, we);
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = __builtin_bswap32(we[7 - i]);
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

// ------------------------------------------------------------------------------ the key's table
// the monomial SRS -> the 64 vectors x^(b), XYZZ: thread (b, j)
static __global__ void __launch_bounds__(256) k_fk20_xvec(const FkAF* __restrict__ srs, FkXY* __restrict__ x) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= FK_BASES) return;
  const uint32_t b = i / FK_N, j = i & (FK_N - 1), u = (FK_N - j) & (FK_N - 1);
  FkXY p = FkXY::inf();
  if (u < FK_H) p = xyzz_from_affine(load_affine(srs, FK_COLS * u + b));
  store_xyzz(&x[i], p);
}

// rows of the table: thread (w, base), a wave shares w.  xhat: the 64 transforms as the butterflies
// leave them, xhat^(b)[pos] at 128 b + rev7(pos)
static __global__ void __launch_bounds__(256) k_fk20_table(const FkXY* __restrict__ xhat, FkAF* __restrict__ tab,
                                                           uint8_t* __restrict__ tab_inf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= FK_BASES * FK_WINDOWS) return;
  const uint32_t w = i / FK_BASES, base = i & (FK_BASES - 1);
  const uint32_t pos = base / FK_COLS, b = base & (FK_COLS - 1);
  const FkXY p = load_xyzz(&xhat[b * FK_N + fk_rev7(pos)]);
  if (w == 0) tab_inf[base] = p.is_inf() ? 1 : 0;
  if (p.is_inf()) return;
  FkXY unit = p;
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

// ------------------------------------------------------------------------------ G1 transforms
KZ_DEV void fk_uniform_scalar(const BlobF& s, uint32_t (&k)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) k[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.v[q]);
}

// One decimation-in-frequency stage of `count` transforms in place: block = butterfly j of
// transform blockIdx.x / 64, on elements i0 and i0 + half, (a, b) -> (a + b, omega^(+-k 64 / half) (a - b)).
// Stages half = 64, 32, .., 1 take natural order to bit-reversed order.
static __global__ void __launch_bounds__(64) k_fk20_bfly(FkXY* __restrict__ data, uint32_t half,
                                                         const BlobF* __restrict__ tw, int inverse) {
  const LpCtx<FkCv> c = lp_ctx<FkCv>();
  const uint32_t j = blockIdx.x & 63, k = j & (half - 1), i0 = ((j - k) << 1) | k;
  FkXY* x = data + (size_t)(blockIdx.x >> 6) * FK_N;
  const LpXyzz<FkCv> a = lp_load_xyzz(c, &x[i0]);
  LpXyzz<FkCv> b = lp_load_xyzz(c, &x[i0 + half]);
  const LpXyzz<FkCv> s = lp_xyzz_add(c, a, b);
  b.y = lp_sub(c, 0, b.y);
  LpXyzz<FkCv> d = lp_xyzz_add(c, a, b);
  if (k != 0 && !d.inf) {
    const uint32_t e = (k * (FK_COLS / half)) << 6;  // omega^(k 64 / half) = w^e
    uint32_t kk[8];
    fk_uniform_scalar(fp_from_mont(tw[inverse ? (NTT_EXT - e) & (NTT_EXT - 1) : e]), kk);
    d = small_mul<FkCv, 8>(c, d, kk);
  }
  lp_store_xyzz(c, &x[i0], s);
  lp_store_xyzz(c, &x[i0 + half], d);
}

// p <- p / 128, a wave per point (the inverse transform of kzgmi_g1_fft128_device only)
static __global__ void __launch_bounds__(64) k_fk20_scale128(FkXY* __restrict__ data) {
  const LpCtx<FkCv> c = lp_ctx<FkCv>();
  LpXyzz<FkCv> p = lp_load_xyzz(c, &data[blockIdx.x]);
  if (p.inf) return;
  BlobF one = BlobF::zero();
  one.v[0] = 1;
  BlobF q = fp_neg(one);  // r - 1
#pragma unroll
  for (int i = 0; i < 8; ++i) q.v[i] = (q.v[i] >> 7) | (i < 7 ? q.v[i + 1] << 25 : 0u);
  uint32_t kk[8];
  fk_uniform_scalar(fp_neg(q), kk);  // 1 / 128 = r - (r - 1) / 128
  p = small_mul<FkCv, 8>(c, p, kk);
  lp_store_xyzz(c, &data[blockIdx.x], p);
}

// D = (H_0, .., H_62, infinity x 65) out of the inverse transform's bit-reversed output
static __global__ void __launch_bounds__(FK_N) k_fk20_shift(const FkXY* __restrict__ h, FkXY* __restrict__ d) {
  const uint32_t t = threadIdx.x;
  const size_t o = (size_t)blockIdx.x * FK_N;
  FkXY p = FkXY::inf();
  if (t < FK_H) p = load_xyzz(&h[o + fk_rev7(t + 1)]);
  store_xyzz(&d[o + t], p);
}

// bit-reversed order -> natural order (kzgmi_g1_fft128_device)
static __global__ void __launch_bounds__(FK_N) k_fk20_unrev(const FkXY* __restrict__ in, FkXY* __restrict__ out) {
  const size_t o = (size_t)blockIdx.x * FK_N;
  store_xyzz(&out[o + threadIdx.x], load_xyzz(&in[o + fk_rev7(threadIdx.x)]));
}

// validated affine points (and their infinity flags) -> XYZZ
static __global__ void __launch_bounds__(256) k_fk20_from_affine(const FkAF* __restrict__ pts,
                                                                 const uint8_t* __restrict__ inf, uint32_t n,
                                                                 FkXY* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_xyzz(&out[i], inf[i] ? FkXY::inf() : xyzz_from_affine(load_affine(pts, i)));
}

// the call's result leaves the workspace only if no kernel of the job raised an error: n 16-byte granules
static __global__ void __launch_bounds__(256) k_fk20_emit(const uint4* __restrict__ in, size_t n,
                                                          const uint32_t* __restrict__ err, uint4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || *err != 0) return;
  out[i] = in[i];
}

}  // namespace kzgmi
