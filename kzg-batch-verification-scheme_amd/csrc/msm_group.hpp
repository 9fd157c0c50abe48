// Grouped small MSMs: the randomised combinations (A_g, B_g) of G index ranges of one resident batch
// in one launch (the search of host_find.hip, kzgmi_batch_range_partials_device).  k_small_msm
// (msm_small.hpp) generalised from at most 2 MSMs to 2 G trees: one wave per term, small_mul, the
// same arrival-counter trees in which no wave ever waits for another; the layout comes from
// find_plan.hpp's find_group_plan as a table in device memory (a SmallPlan passed by value cannot
// hold it).
//
// Group g covers tuples [lo, lo + len) of the batch and has 3 len + 1 waves:
//   r_i pi_i                -> tree A_g, 4-word scalars
//   r_i C_i, s_i pi_i       -> tree B_g, 4- and 8-word scalars (s_i = r_i z_i mod r)
//   (-t_g) G1               -> tree B_g, t_g = sum_{i in g} r_i y_i (k_group_tsum)
// A range of EIP-7594 cells (z_k = h_k^64, y_k = 0) has 3 len + 64 waves: in place of the last term
//   (-c_m(g)) [tau^m]_1     -> tree B_g, m < 64, c_m(g) = sum_{k in g} r_k coef_k[m] (k_cell_range_fold)
// over the points [pi (n) | C (n) | tau^m (64)].
// No GLV split: the sums are the same on G1 and exact off it.  Points: the slot's radix-2^29 slots
// [pi (n) | C (n) | G1], as k_small_msm reads them.  Results: res[2 g] = A_g, res[2 g + 1] = B_g (XYZZ).
// The arrival counters are zeroed by every launch (launch_find.hip).
#pragma once
#include "find_plan.hpp"
#include "kernels.hpp"

namespace kzgmi {

// what every group's terms read: the resident batch of n tuples and its scalars
struct GroupBatch {
  uint32_t n;               // C_i at pts[n + i], G1 at pts[2 n]
  uint32_t ngroups;
  const uint32_t* scal_r;   // r_i: 4 words each
  const uint32_t* scal_s;   // s_i: 8 words each
  const uint32_t* negt;     // -t_g: 8 words each
};

// -t_g = -(sum of r_i y_i over group g's tuples) mod r as 8 LE words, one block per group; r_i is the
// counter-mode randomiser of the global index index_offset + i, as k_scalar_prep derives it (which
// has range-checked y_i: a y_i >= r counts as 0 here too)
template <class Cv>
__global__ void __launch_bounds__(256) k_group_tsum(const FindGroup* __restrict__ groups, Seed seed, uint64_t index_offset,
                                                    const uint8_t* __restrict__ ys, uint32_t* __restrict__ negt) {
  using R = typename Cv::FrP;
  using F = Fp<R>;
  __shared__ F lds[256];
  const FindGroup g = groups[blockIdx.x];
  F acc = F::zero();
  for (uint32_t k = threadIdx.x; k < g.len; k += 256) {
    const uint32_t i = g.lo + k;
    uint32_t wy[8];
    load_words(ys + (size_t)i * 32, wy);
    F y = fp_from_be_words<R>(wy, 0);
    if (!fp_raw_lt_mod(y)) y = F::zero();
    uint32_t r4[4];
    randomizer127(seed.w, index_offset + i, r4);
    F r = F::zero();
#pragma unroll
    for (int q = 0; q < 4; ++q) r.v[q] = r4[q];
    acc = fp_add(acc, fp_mul(fp_to_mont(r), y));  // r y (standard form)
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st) lds[threadIdx.x] = fp_add(lds[threadIdx.x], lds[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const F t = fp_neg(lds[0]);
#pragma unroll
    for (int q = 0; q < 8; ++q) negt[8 * (size_t)blockIdx.x + q] = t.v[q];
  }
}

// -c_m(g) = -(sum of r_k coef_k[m] over group g's cells) mod r, m < 64, as 8 LE words each at
// negt[8 (64 g + m)]: the scalars of a cell range's 64 tail terms, in the place of k_group_tsum's one
// (y_k = 0 for cells).  coef: k_cell_coeffs' table, 64 x 8 LE words per cell in standard form.  One
// block per group: wave s takes the cells lo + s, lo + s + 4, ... (r_k is wave-uniform), lane m
// coefficient m, so consecutive lanes read consecutive 32 B; the four strides meet in LDS.
template <class Cv>
__global__ void __launch_bounds__(256) k_cell_range_fold(const FindGroup* __restrict__ groups, Seed seed,
                                                         uint64_t index_offset, const uint32_t* __restrict__ coef,
                                                         uint32_t* __restrict__ negt) {
  using R = typename Cv::FrP;
  using F = Fp<R>;
  __shared__ F lds[256];
  const FindGroup g = groups[blockIdx.x];
  const uint32_t m = threadIdx.x & 63u;
  F acc = F::zero();
  for (uint32_t k = threadIdx.x >> 6; k < g.len; k += 4) {
    const uint32_t i = g.lo + k;
    uint32_t r4[4];
    randomizer127(seed.w, index_offset + i, r4);
    F r = F::zero();
#pragma unroll
    for (int q = 0; q < 4; ++q) r.v[q] = r4[q];
    F cf;
    load_words(reinterpret_cast<const uint8_t*>(coef + 8 * ((size_t)i * 64 + m)), cf.v);
    acc = fp_add(acc, fp_mul(fp_to_mont(r), cf));  // r c (standard form)
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    const F t = fp_neg(fp_add(fp_add(lds[m], lds[64 + m]), fp_add(lds[128 + m], lds[192 + m])));
    store_words(reinterpret_cast<uint8_t*>(negt + 8 * ((size_t)blockIdx.x * 64 + m)), t.v);
  }
}

// T: the group's tail terms (find_plan.hpp): 1 for opening tuples, 64 for cell ranges, whose tail
// term m reads point pts[2 n + m] and scalar negt[8 (T g + m)] and is leaf 2 len + m of tree B
template <class Cv, uint32_t T = 1>
__global__ void __launch_bounds__(64) k_group_msm(GroupBatch b, const FindGroup* __restrict__ groups,
                                                  const Affine<Cv>* __restrict__ pts, const uint8_t* __restrict__ inf,
                                                  uint32_t* __restrict__ nodes, uint32_t* __restrict__ flags,
                                                  Xyzz<Cv>* __restrict__ res) {
  using Q = Fp29Of<Cv>;
  using LQ = LpQ<Cv>;
  KZ_TAIL_PRIO();
  const LpCtx<Cv> c = lp_ctx<Cv>();
  const uint32_t w = blockIdx.x, j = threadIdx.x & 15;
  // the wave's group: the last one whose first wave is at or below w (wave-uniform search)
  uint32_t lo = 0, hi = b.ngroups;
#pragma unroll 1
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (groups[mid].wave_base <= w) lo = mid;
    else hi = mid;
  }
  const uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
  const FindGroup g = groups[gi];
  const uint32_t t = w - g.wave_base;  // the term within the group
  if (t > 3 * g.len + (T - 1)) return;  // (a wave past the last group's terms: the grid is exact, so none)
  // its point, scalar, tree (0: A, 1: B) and leaf
  const uint32_t cls = t < g.len ? 0u : t < 2 * g.len ? 1u : t < 3 * g.len ? 2u : 3u;
  const uint32_t i = g.lo + (t - cls * g.len);  // the tuple (classes 0 .. 2)
  const uint32_t tm = T == 1 ? 0u : t - 3 * g.len;  // the tail term (class 3)
  const uint32_t pi = cls == 0 || cls == 2 ? i : cls == 1 ? b.n + i : 2 * b.n + tm;
  const uint32_t m = cls == 0 ? 0u : 1u;
  uint32_t v = cls == 0 ? t : t - g.len;
  const uint32_t* sw = cls <= 1 ? b.scal_r + 4 * (size_t)i : cls == 2 ? b.scal_s + 8 * (size_t)i
                                                                     : b.negt + 8 * ((size_t)T * gi + tm);
  const uint32_t* slot = reinterpret_cast<const uint32_t*>(pts + pi);
  int32_t one = 0, from29 = 0;  // per-lane limbs of R mod p and R^2 / R29 mod p
#pragma unroll
  for (int q = 0; q < LQ::N; ++q)
    if (j == (uint32_t)q) {
      one = (int32_t)LQ::ONE[q];
      from29 = (int32_t)LQ::FROM29[q];
    }
  LpXyzz<Cv> P;
  if constexpr (kPackPts<Cv>) {  // BN254: x R29, y R29 as 32-bit words
    lp_step2(c, P.x, lp_raw_from_words<Cv>(slot), from29, P.y, lp_raw_from_words<Cv>(slot + Cv::FpP::N), from29);
  } else {  // BLS12-381: 14 radix-29 limbs of x, then of y
    static_assert(Q::N == LQ::N, "radix-29 slot limbs are the lane-parallel limbs");
    P.x = j < (uint32_t)Q::N ? (int32_t)slot[j] : 0;
    P.y = j < (uint32_t)Q::N ? (int32_t)slot[Q::N + j] : 0;
  }
  P.zz = P.zzz = one;
  P.inf = inf[pi] != 0;
  LpXyzz<Cv> acc;
  if (cls >= 2) {
    uint32_t kk[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) kk[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw[q]);
    acc = small_mul<Cv, 8>(c, P, kk);
  } else {  // r_i < 2^127
    uint32_t kk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) kk[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw[q]);
    acc = small_mul<Cv, 4>(c, P, kk);
  }
  if (P.inf) acc.inf = true;
  // climb tree m of the group (msm_small.hpp)
  uint32_t cnt = m ? 2 * g.len + T : g.len, node = g.node_base[m], flag = g.flag_base[m];
#pragma unroll 1
  while (cnt > 1) {
    const uint32_t partner = v ^ 1u;
    if (partner < cnt) {
      small_store<Cv>(nodes + (size_t)(node + v) * SMALL_NODE_WORDS, acc);
      __threadfence();
      uint32_t old = 0;
      if (threadIdx.x == 0)
        old = __hip_atomic_fetch_add(flags + flag + (v >> 1), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
      if (old == 0) return;  // the sibling's wave carries on
      __threadfence();
      acc = lp_xyzz_add(c, acc, small_load<Cv>(nodes + (size_t)(node + partner) * SMALL_NODE_WORDS));
    }
    node += cnt;
    flag += (cnt + 1) >> 1;
    v >>= 1;
    cnt = (cnt + 1) >> 1;
  }
  lp_store_xyzz(c, &res[2 * (size_t)gi + m], acc);
}

// records[k] (k < count) become marked records (kernels.hpp partial_mark) when *err != 0
template <class Cv>
__global__ void __launch_bounds__(256) k_mark_records(Xyzz<Cv>* __restrict__ recs, uint32_t count,
                                                      const uint32_t* __restrict__ err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t e = *err;
  if (k >= count || !e) return;
  using F = typename Xyzz<Cv>::F;
  Xyzz<Cv> p;
  p.y = F::zero();
  p.zz = F::zero();
  p.zzz = F::zero();
#pragma unroll
  for (int i = 0; i < F::N; ++i) p.x.v[i] = 0xffffffffu;
  p.y.v[0] = e;
  store_xyzz(&recs[k], p);
}

// a marked record among recs[0, count) raises its code into *err
template <class Cv>
__global__ void __launch_bounds__(256) k_check_marks(const Xyzz<Cv>* __restrict__ recs, uint32_t count,
                                                     uint32_t* __restrict__ err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  // the mark is in the top word of x and the low word of y
  Xyzz<Cv> p;
  p.x.v[Cv::FpP::N - 1] = recs[k].x.v[Cv::FpP::N - 1];
  p.y.v[0] = recs[k].y.v[0];
  if (const uint32_t m = partial_mark(p)) raise_err(err, m);
}

}  // namespace kzgmi
