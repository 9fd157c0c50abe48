// Power-of-two number-theoretic transforms over Fr, both curves, n = 2^0 .. 2^26, batched
// (DESIGN.md 3h).  w_n = g^((r-1)/n), g = 7 (BLS12-381) or 5 (BN254); the definitions are restated
// in include/kzgmi.h and tests/nttref.py.  The passes of one call are planned on the host
// (ntt_plan.hpp); k_ntt_pass below runs one of them.
//
// A pass transforms one digit of the index (ntt_plan.hpp): 2^bits elements, 2^lstride apart, for
// every value of the other digits -- a column.  A workgroup takes a tile of 2^TB elements: C =
// 2^(TB - bits) columns with adjacent low digits, so that a global access of a wave covers runs of
// C >= 4 elements (128 B), or whole columns where those are contiguous (lstride = 0, or a
// bit-reversed side: index k of that side holds point bitrev(k), and the reversal of a first or
// last digit keeps its elements together).  The tile sits in LDS limb-planar (word q of element e
// at [q][e]); 2^bits-point transforms run there as `bits` radix-2 decimation-in-frequency stages,
// which leave digit value k at position bitrev(k): later passes and the last store read the digits
// above theirs through one bit reversal (kappa).  What lies between the sub-transforms is folded
// into the load (big-endian input and its range check, the shift powers s^i, the twiddles
// w^(a kappa step)) or the store (n^-1 s^-i, big-endian output, the output order).
//
// Number forms: data are canonical standard-form values, 8 little-endian words; every table is in
// Montgomery form, so fp_mul(table, value) is the standard-form product and no element is converted.
// Tables, per curve and context (NttTables): w_{2^26}^lo and w_{2^26}^(hi 2^13), lo, hi < 2^13 -- any
// root is one product of the two, the inverse direction takes the negated index -- and
// w_{2^10}^i, i < 2^10, for the stages in LDS.  Per call with a shift or an inverse (NttCallTable):
// b^lo and c b^(hi 2^13) with b = s or s^-1 and c = 1 or n^-1.  No exponentiation per element.
#pragma once
#include "kernels.hpp"
#include "ntt_plan.hpp"

namespace kzgmi {

constexpr uint32_t NTT_TAB = 1u << NTT_TABLE_BITS;          // entries of each level of a two-level table
constexpr uint32_t NTT_SMALL_BITS = NTT_WIDEST_BITS;  // the widest sub-transform: 2^10
constexpr uint32_t NTT_SMALL = 1u << NTT_SMALL_BITS;
// the per-curve table: [lo | hi | small], the per-call table: [lo | hi]
constexpr uint32_t NTT_T_LO = 0, NTT_T_HI = NTT_TAB, NTT_T_SMALL = 2 * NTT_TAB, NTT_T_ENTRIES = 2 * NTT_TAB + NTT_SMALL;
constexpr uint32_t NTT_CALL_ENTRIES = 2 * NTT_TAB;
static_assert(2 * NTT_TABLE_BITS == NTT_ROOT_BITS, "two levels cover every exponent below 2^26");

struct NttPassArgs {
  const void* in;
  void* out;
  uint64_t cols;     // columns of the whole call: count * 2^(logn - bits)
  uint32_t logn, bits, lstride, lprev, tw_step, flags;
};

template <class R>
KZ_DEV Fp<R> ntt_pow(Fp<R> x, uint32_t e) {  // Montgomery x^e
  Fp<R> acc = Fp<R>::one();
#pragma unroll 1
  for (; e; e >>= 1) {
    if (e & 1) acc = fp_mul(acc, x);
    x = fp_sqr(x);
  }
  return acc;
}
template <class R>
KZ_DEV Fp<R> ntt_small_int(uint32_t v) {  // the integer v, Montgomery
  Fp<R> x = Fp<R>::zero();
  x.v[0] = v;
  return fp_to_mont(x);
}

// w_{2^26} = g^((r-1) / 2^26), Montgomery: square-and-multiply over the bits of (r-1) >> 26
template <class Cv>
KZ_DEV Fp<typename Cv::FrP> ntt_root26() {
  using R = typename Cv::FrP;
  const Fp<R> g = ntt_small_int<R>(Cv::ID == 0 ? 7u : 5u);
  Fp<R> acc = Fp<R>::one();
#pragma unroll 1
  for (int bit = 32 * R::N - 1; bit >= (int)NTT_ROOT_BITS; --bit) {  // r - 1 and r differ in bit 0 only
    acc = fp_sqr(acc);
    if ((R::MOD[bit >> 5] >> (bit & 31)) & 1) acc = fp_mul(acc, g);
  }
  return acc;
}

// The per-curve table: NTT_T_ENTRIES threads
template <class Cv>
__global__ void __launch_bounds__(256) k_ntt_roots(uint32_t* __restrict__ table) {
  using R = typename Cv::FrP;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NTT_T_ENTRIES) return;
  const Fp<R> w = ntt_root26<Cv>();
  uint32_t e;
  if (i < NTT_T_HI) e = i;
  else if (i < NTT_T_SMALL) e = (i - NTT_T_HI) << NTT_TABLE_BITS;
  else e = (i - NTT_T_SMALL) << (NTT_ROOT_BITS - NTT_SMALL_BITS);
  store_words(reinterpret_cast<uint8_t*>(table + 8 * (size_t)i), ntt_pow<R>(w, e).v);
}

// The per-call table: tab[lo] = b^lo, tab[2^13 + hi] = c b^(hi 2^13); b = s (8 big-endian words,
// canonical and nonzero: checked on the host; has_shift = 0: b = 1 and one thread writes c alone) or
// its inverse, c = 2^-logn for an inverse transform, else 1.  NTT_CALL_ENTRIES threads.
template <class Cv>
__global__ void __launch_bounds__(256) k_ntt_call_table(Seed shift, uint32_t has_shift, uint32_t inverse, uint32_t logn,
                                                        uint32_t* __restrict__ tab) {
  using R = typename Cv::FrP;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NTT_CALL_ENTRIES || (!has_shift && i != NTT_TAB)) return;
  Fp<R> b = Fp<R>::one();
  if (has_shift) {
#pragma unroll
    for (int k = 0; k < 8; ++k) b.v[k] = shift.w[7 - k];  // Seed: word 0 is the most significant
    b = fp_to_mont(b);
    if (inverse) b = fp_inv(b);
  }
  Fp<R> v;
  if (i < NTT_TAB) {
    v = ntt_pow<R>(b, i);
  } else {
#pragma unroll 1
    for (uint32_t k = 0; k < NTT_TABLE_BITS; ++k) b = fp_sqr(b);
    v = ntt_pow<R>(b, i - NTT_TAB);
    if (inverse) v = fp_mul(v, fp_inv(ntt_small_int<R>(1u << logn)));
  }
  store_words(reinterpret_cast<uint8_t*>(tab + 8 * (size_t)i), v.v);
}

KZ_DEV uint32_t ntt_rev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0; }

template <class R>
KZ_DEV Fp<R> ntt_tab(const uint32_t* __restrict__ t, uint32_t i) {
  Fp<R> r;
  load_words(reinterpret_cast<const uint8_t*>(t + 8 * (size_t)i), r.v);
  return r;
}
// lo[e mod 2^13] hi[e >> 13], Montgomery
template <class R>
KZ_DEV Fp<R> ntt_two_level(const uint32_t* __restrict__ t, uint32_t e) {
  return fp_mul(ntt_tab<R>(t, NTT_T_LO + (e & (NTT_TAB - 1))), ntt_tab<R>(t, NTT_T_HI + (e >> NTT_TABLE_BITS)));
}

// One pass.  TB: log2 of the tile's elements; 2^TB / 4 threads, four elements and two butterflies
// of each stage per thread.  grid: ceil(cols / C) workgroups.  roots: the curve's table; call: the
// call's table (read with NTT_P_SHIFT or NTT_P_SCALE only).
template <class Cv, int TB>
__global__ void __launch_bounds__((1 << TB) / 4) k_ntt_pass(const NttPassArgs a, const uint32_t* __restrict__ roots,
                                                            const uint32_t* __restrict__ call, uint32_t* __restrict__ err) {
  using R = typename Cv::FrP;
  using F = Fp<R>;
  constexpr uint32_t E = 1u << TB, NT = E / 4;
  __shared__ uint32_t sh[8][E];
  const uint32_t t = threadIdx.x;
  const uint32_t b = a.bits, Rn = 1u << b, lc = TB - b, C = 1u << lc;
  const uint32_t lt = a.logn - b;  // columns of one transform: lprev + lstride bits
  const uint32_t fl = a.flags;
  const bool inv = fl & NTT_P_INVERSE, last = fl & NTT_P_LAST;
  const uint64_t g0 = (uint64_t)blockIdx.x << lc;
  // element (row r, column c) of the tile at r C + ((c + r) mod C): a row's columns and a column's
  // rows both fall on consecutive banks
  auto lidx = [&](uint32_t r, uint32_t c) { return (r << lc) | ((c + r) & (C - 1)); };
  // column c of the tile: its transform, the digits above this pass's (h), kappa and the low digits
  auto column = [&](uint32_t c, uint64_t& tr, uint32_t& h, uint32_t& kappa, uint32_t& lo) {
    const uint64_t g = g0 + c;
    tr = g >> lt;
    const uint32_t colw = (uint32_t)(g & ((uint64_t(1) << lt) - 1));
    if (last) {  // lstride = 0: the columns in the order of kappa, so that natural-order stores run along c
      kappa = colw;
      h = ntt_rev(colw, a.lprev);
      lo = 0;
    } else {
      lo = colw & ((1u << a.lstride) - 1);
      h = colw >> a.lstride;
      kappa = ntt_rev(h, a.lprev);
    }
    return g < a.cols;
  };
  // ---- load: lanes along the columns where the digit is strided, along the column where it is contiguous
  const bool row_load = a.lstride == 0 || (fl & NTT_P_BITREV_IN);
#pragma unroll 1
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t u = t + NT * q;
    const uint32_t c = row_load ? u >> b : u & (C - 1);
    const uint32_t rm = row_load ? u & (Rn - 1) : u >> lc;  // the place in memory along the digit
    uint64_t tr;
    uint32_t h, kappa, lo;
    F x = F::zero();
    uint32_t r = rm;
    if (column(c, tr, h, kappa, lo)) {
      uint32_t pos;
      if (fl & NTT_P_BITREV_IN) {  // pass 0: logical index r 2^lstride + lo sits at bitrev of it
        r = ntt_rev(rm, b);
        pos = (ntt_rev(lo, a.lstride) << b) | rm;
      } else {
        pos = (((h << b) | rm) << a.lstride) | lo;
      }
      const uint8_t* src = static_cast<const uint8_t*>(a.in) + 32 * ((tr << a.logn) | pos);
      uint32_t w[8];
      load_words(src, w);
      if (fl & NTT_P_READ_BE) {
        x = fp_from_be_words<R>(w, 0);
        if (!fp_raw_lt_mod(x)) {
          raise_err(err, DERR_SCALAR);
          x = F::zero();
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x.v[k] = w[k];
      }
      // pass 0 of a forward transform: (r, lo) is the coefficient's index
      if ((fl & NTT_P_SHIFT) && !inv) x = fp_mul(ntt_two_level<R>(call, (r << a.lstride) | lo), x);
      if (fl & NTT_P_TWIDDLE) {
        uint32_t e = r * kappa * a.tw_step;  // r kappa < 2^(lprev + bits): below 2^26
        if (inv) e = (0u - e) & ((1u << NTT_ROOT_BITS) - 1);
        if (e) x = fp_mul(ntt_two_level<R>(roots, e), x);
      }
    }
    const uint32_t e = lidx(r, c);
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k][e] = x.v[k];
  }
  __syncthreads();
  // ---- the sub-transforms: stage of span hs pairs rows r and r + hs, root w_{2 hs}^(r mod hs)
#pragma unroll 1
  for (uint32_t ls = b; ls-- > 0;) {
    const uint32_t hs = 1u << ls;
#pragma unroll 1
    for (uint32_t q = 0; q < 2; ++q) {
      const uint32_t w = t + NT * q, c = w & (C - 1), k = w >> lc, kk = k & (hs - 1), r0 = ((k - kk) << 1) | kk;
      const uint32_t e0 = lidx(r0, c), e1 = lidx(r0 + hs, c);
      F x0, x1;
#pragma unroll
      for (int j = 0; j < 8; ++j) { x0.v[j] = sh[j][e0]; x1.v[j] = sh[j][e1]; }
      const F s = fp_add(x0, x1);
      F d = fp_sub(x0, x1);
      uint32_t ti = kk << (NTT_SMALL_BITS - 1 - ls);
      if (inv) ti = (0u - ti) & (NTT_SMALL - 1);
      if (ti) d = fp_mul(ntt_tab<R>(roots, NTT_T_SMALL + ti), d);
#pragma unroll
      for (int j = 0; j < 8; ++j) { sh[j][e0] = s.v[j]; sh[j][e1] = d.v[j]; }
    }
    __syncthreads();
  }
  // ---- store.  Row p of the tile holds digit value bitrev(p).  Every pass but the last writes where
  // it read; the last writes X[kappa + bitrev(p) 2^lt] to its natural place, or to the bit reversal of
  // that: (h 2^bits + p), which again is where it read.
  const bool natural_last = last && !(fl & NTT_P_BITREV_OUT);
  const bool row_store = natural_last ? lt == 0 : a.lstride == 0;
#pragma unroll 1
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t u = t + NT * q;
    const uint32_t c = row_store ? u >> b : u & (C - 1);
    const uint32_t rs = row_store ? u & (Rn - 1) : u >> lc;
    uint64_t tr;
    uint32_t h, kappa, lo;
    if (!column(c, tr, h, kappa, lo)) continue;
    uint32_t p, pos;
    if (natural_last) {
      // one pass: lanes along the output index (row bitrev of it); more: lanes along kappa
      p = lt == 0 ? ntt_rev(rs, b) : rs;
      pos = kappa + ((lt == 0 ? rs : ntt_rev(rs, b)) << lt);
    } else {
      p = rs;
      pos = (((h << b) | p) << a.lstride) | lo;
    }
    const uint32_t e = lidx(p, c);
    F x;
#pragma unroll
    for (int k = 0; k < 8; ++k) x.v[k] = sh[k][e];
    if (last && inv) {  // the coefficient side is in natural order: pos is the coefficient's index
      if (fl & NTT_P_SHIFT) x = fp_mul(ntt_two_level<R>(call, pos), x);
      else if (fl & NTT_P_SCALE) x = fp_mul(ntt_tab<R>(call, NTT_T_HI), x);
    }
    uint8_t* dst = static_cast<uint8_t*>(a.out) + 32 * ((tr << a.logn) | pos);
    if (fl & NTT_P_WRITE_BE) {
      uint32_t w[8];
      fp_to_be_words(x, w, 0);
      store_words(dst, w);
    } else {
      store_words(dst, x.v);
    }
  }
}

}  // namespace kzgmi
