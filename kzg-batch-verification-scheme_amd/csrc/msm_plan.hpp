// What one MSM call decides before anything is enqueued, as plain data: the tuning knobs
// (MsmTuning), the window width of a call (call_wbits), the term lists of a batch (batch_terms)
// and the plan itself (plan_msm -> MsmPlan): small or bucket form, the digit offsets, the
// accumulation grid, whether the call splits, and the byte size of every slot buffer it needs.
// Nothing here allocates, launches or reads the environment: host_core.hip grows the slot's
// buffers to a plan's sizes and launches from its counts, kzgmi_ctx_reserve only does the former,
// and tests/native/plan_probe.hip exposes the functions to a test that needs no GPU.
#pragma once
#include "msm_small.hpp"

#include <algorithm>

namespace kzgmi {

struct MsmTuning {
  // accumulation grid cap: one resident round (CUs x 4 SIMDs x kAccWaves<Cv> waves x 64 lanes)
  // of equal chunks instead of 64-entry chunks in 2-3 partial rounds: 113 -> 116
  // batch-verifies/s pipelined when introduced (tools/ab.py).
  int ncu = 0;                // compute units: the accumulation grid cap (kAccWaves, msm.hpp)
  size_t acc_threads_env = 0;  // KZGMI_ACC_THREADS override of that cap (0 = none)
  int acc_queue = ACC_QUEUE_FACTOR;  // KZGMI_ACC_QUEUE: chunks per capped thread (<= 1: static grid)
  size_t acc_queue_min = ACC_QUEUE_MIN_LEN;  // KZGMI_ACC_QUEUE_MIN: shortest queue chunk (entries)
  size_t acc_queue_from = ACC_QUEUE_FROM;    // KZGMI_ACC_QUEUE_FROM: calls with fewer entries keep the static grid
  bool sort_split = false;     // KZGMI_SORT_SPLIT: split coarse-pass entries at every size (tests)
  bool sort_full_bins = false;  // KZGMI_SORT_FULL_BINS: the set-table-overflow fallback at every size (tests)
  int wbits_env = 0;           // KZGMI_WBITS: 13 or 16 forces the window width (tests, A/B)
  uint32_t small_terms = 4096;  // calls of at most this many terms: msm_small.hpp (KZGMI_SMALL_TERMS; 0: never)
  // Split accumulation of two-MSM calls (run_msm_core): -1 synchronous device calls of at least
  // SPLIT_FROM entries with no other slot in flight (latency-bound), 0 never, 1 always
  // (KZGMI_SPLIT_ACC).  Single 2^20 BLS12-381 batches 8.02 -> 7.95 ms; 2^17 ones lose (2.95 ->
  // 3.01 ms: the side work outlasts the short second launch), so smaller calls keep one launch
  // (profiles/r06/split_accumulation.txt, ab_split_rev.txt)
  static constexpr size_t SPLIT_FROM = size_t(1) << 25;
  int split_acc = -1;
  bool split_low_prio = true;    // KZGMI_SPLIT_LOWPRIO: the side stream's kernels without the tail's raised issue priority
  bool split_side_fix = true;    // KZGMI_SPLIT_SIDEFIX: the first launch's piece joins on the side stream
  bool split_side_prio = true;   // KZGMI_SPLIT_SIDEPRIO: the side stream at the device's greatest priority
  // KZGMI_SPLIT_REV: MSM#0's sets (8 windows) in the first launch, its short tail on the side
  // stream, hidden behind MSM#1's 3x longer launch; MSM#1's tail after it on an idle chip.  0:
  // MSM#1's first, whose side tail outlasts the short second launch.  2^20: 7.95 vs 7.98 ms
  // (one launch 8.02; profiles/r06/ab_split_rev.txt)
  bool split_rev = true;
  // reduction segments on 4 threads instead of 2 while that grid stays within seg4_waves waves per
  // SIMD (Launch::reduce; KZGMI_SEG4_WAVES, 0: always 2)
  int seg4_waves = 1;
  // Row accumulation (msm.hpp k_accumulate_rows) instead of the equal-chunk kernel: -1 the
  // asynchronous BLS12-381 batches of at least ROWS_FROM entries, whose uneven queue tail the next
  // batch's accumulation fills; 0 never; 1 every unsplit single-store call (KZGMI_ACC_ROWS; tests, A/B)
  static constexpr size_t ROWS_FROM = size_t(1) << 23;
  int acc_rows = -1;
  uint32_t row_len = ROW_LEN_MAX;  // L: the longest item, a longer bucket is cut (no knob: the stage tests set 8)
};

// Window width of a call from its entry count at c = 16 (msm.hpp Win): c = 13 for mid-size calls,
// 2^20 < entries <= max13 (batches: 2^15 < n <= 2^17, max13 = 2^22; MSMs: 2^16 < n <= 2^17,
// max13 = 2^21) -- 8x fewer buckets for 5/4 the terms, where the bucket-sum reduction is a large
// share of the pipelined work (2^17-tuple batches 875 -> 1024/s, 2^17-point MSMs 193 -> 224 M
// pts/s; profiles/r03/misc_ab_r03.txt).  Not for larger calls (a 2^18-point MSM: 270 -> 242)
// nor tiny ones, whose latency it raises: the top window of a 10 x 13-bit split of a 128-bit
// magnitude holds 11 bits (of a 20 x 13 split of 256 bits, 9), so its terms crowd into a few
// hundred buckets whose pieces k_fixup joins serially (n = 256: 3.0 -> 3.3 ms).  At 14 bits the
// top windows keep 2 and 4 bits: a 2^17 batch took 19 ms.  KZGMI_WBITS=13/16 forces one.
inline int call_wbits(const MsmTuning& t, size_t entries16, size_t max13) {
  if (t.wbits_env == 13 || t.wbits_env == WBITS) return t.wbits_env;
  return entries16 > (size_t(1) << 20) && entries16 <= max13 ? 13 : WBITS;
}
// windows of a 127-bit magnitude (randomisers, GLV halves) and of a full 255-bit scalar at width c
// (signed digits: the top window takes the last carry)
inline uint32_t windows_half(int wb) { return (uint32_t)((128 + wb - 1) / wb); }
inline uint32_t windows_full(int wb) { return (uint32_t)((256 + wb - 1) / wb); }

// ... of a batch of n tuples: 32 entries per tuple with 127-bit r_i, 48 with full ones
inline int batch_wbits(const MsmTuning& t, bool powers, size_t n) {
  return call_wbits(t, (size_t)(powers ? 48 : 32) * n, size_t(1) << 22);
}

// ------------------------------------------------------------------------------ batch terms
// The scalar arrays a batch's terms read (slot buffers): r_i, s_i, -t; their GLV halves
// ([h0 x n | h1 x n]; glv_t: [h0 x tail | h1 x tail]); a cell batch's 64 coefficients -c_m
struct BatchScalars {
  const uint32_t *scal_r, *scal_s, *scal_t, *glv_r, *glv_s, *glv_t, *cell_coef;
};
struct BatchTerms {
  TermList tl;
  MsmWindows mw;
  uint32_t nsets;
  size_t emax;  // bound on the window entries (+ 16 of slack)
};
// Tuples [lo, lo + nj) of a batch of n (a whole batch: lo = 0, nj = n, last) as the terms of
// MSM#0 = sum r_i pi_i and MSM#1 = sum r_i C_i + s_i pi_i - t G1, at H windows per 127-bit
// magnitude and F per full scalar.  Points: [pi (n) | m unique commitments of a cell batch |
// C (n) | tail], with GLV their images behind them; the tail class (-t [1]_1, or a cell batch's
// 64 terms -c_m [tau^m]_1) joins the last range only, but every range's emax counts it.
//   glv: every MSM in H windows of half scalars: sets 0..H-1 (MSM#0), H..2H-1 (MSM#1)
//   127-bit r_i: MSM#0 in H windows (sets 0..H-1), MSM#1 in F (sets H..H+F-1)
//   powers (r_i = r^i, full Fr): both MSMs in F windows (sets 0..F-1, F..2F-1)
// cell_terms: the tail terms of a cell batch (0: not one) with its m unique commitments; a cell
// batch is a powers batch, so m = 0 wherever r_i is short.
inline BatchTerms batch_terms(bool glv, bool powers, uint32_t cell_terms, uint32_t H, uint32_t F, size_t n, size_t m,
                              size_t lo, size_t nj, bool last, const BatchScalars& b) {
  const bool cell = cell_terms != 0;
  const uint32_t tail = cell ? cell_terms : 1;
  const uint32_t cnt = (uint32_t)nj, l = (uint32_t)lo;
  const uint32_t cb = (uint32_t)(n + m), tb = cb + (uint32_t)n;  // first C, first tail point
  const uint32_t ph = tb + tail;                                  // GLV: phi(pts[j]) at pts[ph + j]
  BatchTerms r{};
  TermList& tl = r.tl;
  uint32_t k = 0;
  if (glv) {
    const uint32_t* rr = powers ? b.glv_r : b.scal_r;  // r_i = h0 + lambda h1 when full
    tl.c[k++] = {cnt, l, 4, H, 0, 4, rr + 4 * lo};                          // MSM#0: r_i pi_i
    if (powers) tl.c[k++] = {cnt, ph + l, 4, H, 0, 4, rr + 4 * (n + lo)};
    tl.c[k++] = {cnt, cb + l, 4, H, H, 4, rr + 4 * lo};                     // MSM#1: r_i C_i
    if (powers) tl.c[k++] = {cnt, ph + cb + l, 4, H, H, 4, rr + 4 * (n + lo)};
    tl.c[k++] = {cnt, l, 4, H, H, 4, b.glv_s + 4 * lo};                     //        s_i pi_i
    tl.c[k++] = {cnt, ph + l, 4, H, H, 4, b.glv_s + 4 * (n + lo)};
    if (last) {                                                             //        -t G1 (cells: -c_m [tau^m]_1)
      tl.c[k++] = {tail, tb, 4, H, H, cell ? 4u : 0u, b.glv_t};
      tl.c[k++] = {tail, ph + tb, 4, H, H, cell ? 4u : 0u, b.glv_t + 4 * (size_t)tail};
    }
    r.mw = MsmWindows{2, {0, H}, {H, H}};
    r.nsets = 2 * H;
    r.emax = (size_t)(powers ? 6 : 4) * H * nj + 2 * H * tail + 16;
  } else {
    const uint32_t rw = powers ? 8 : 4, R = powers ? F : H;  // r_i: words, windows = MSM#0's sets
    tl.c[k++] = {cnt, l, rw, R, 0, rw, b.scal_r + (size_t)rw * lo};         // MSM#0: r_i pi_i
    tl.c[k++] = {cnt, cb + l, rw, R, R, rw, b.scal_r + (size_t)rw * lo};    // MSM#1: r_i C_i
    tl.c[k++] = {cnt, l, 8, F, R, 8, b.scal_s + 8 * lo};                    //        s_i pi_i
    if (last) tl.c[k++] = {tail, tb, 8, F, R, cell ? 8u : 0u, cell ? b.cell_coef : b.scal_t};
    r.mw = MsmWindows{2, {0, R}, {R, F}};
    r.nsets = R + F;
    r.emax = (size_t)(2 * R + F) * nj + (size_t)F * tail + 16;
  }
  tl.nclass = k;
  for (uint32_t j = 0; j < k; ++j) tl.total += tl.c[j].count;
  return r;
}

// ------------------------------------------------------------------------------ the plan
// Byte sizes of the slot buffers a call needs (Slot's DevBufs of the same names).  0: not used by
// this call (the second store outside parts 2 and 3, the work-queue counter of a static grid).
struct MsmBytes {
  size_t small_nodes, small_flags;  // small form (with res); in a bucket plan only from plan_reserve
  size_t digits, cnt, off, cntb, offb, coarse, ent, total, accq, crowd, sval, skey, acc29, acc29b, R, U, scratch, winsum;
  size_t res;
  size_t rowq, items, cuts;  // row accumulation: counters + histogram, the item list, the join list
};

struct MsmPlan {
  const char* refuse;  // the call is refused with this message (KZGMI_ERR_ARG); nothing else is set
  bool small;          // one wave per term and a summation tree (msm_small.hpp) instead of buckets
  SmallPlan sp;        // small form: the tree, its terms, stored nodes and arrival counters
  uint32_t small_terms, small_nodes, small_flags;
  TermList tl;         // the call's terms (+ each class's offset in the digit array: dig_base)
  size_t ndig;         // window digits of every term
  uint32_t own_npts;   // the slot's own points to put into the accumulation's format first (0: none)
  uint32_t nbuckets, bins, rb_parts;  // Win<wbits>
  uint32_t NB;         // buckets of every set
  size_t nchunks;      // accumulation chunks = the launched threads of a static grid
  size_t acc_threads;  // work-queue form: the launched threads, which take the nchunks chunks (0: static grid)
  bool can_split, split;  // the two MSMs' sets may / do accumulate in two launches
  uint32_t split_set;  // MSM#1's first set
  size_t pieces;       // bucket pieces the launches may flush (two records each, behind the NB buckets)
  size_t crowd_words;  // one list of crowded buckets (a split's second list follows the first)
  bool second;         // this range accumulates into the second store, then merges
  // row accumulation (msm.hpp): the launch takes rows of 64 items, sorted by length, instead of chunks
  bool rows;
  uint32_t row_len;    // L: items are at most this long
  size_t row_items;    // capacity of the item list (three arrays of it)
  size_t row_pieces;   // piece slots of cut buckets: records NB + slot, handed out as buckets are cut
  size_t row_cuts;     // lines of the join list (bucket, first piece slot, pieces)
  MsmBytes bytes;
};

// The terms of tl (classes in order) as one wave each, MSM m's leaves in class order; the tree's
// stored nodes and arrival counters per MSM, level after level (msm_small.hpp).
template <class Cv>
inline void plan_small(MsmPlan& p, const MsmWindows& mw) {
  const TermList& tl = p.tl;
  SmallPlan& sp = p.sp;
  sp.nclass = tl.nclass;
  sp.nmsm = mw.nmsm;
  uint32_t terms = 0, leaves[2] = {0, 0};
  for (uint32_t k = 0; k < tl.nclass; ++k) {
    const uint32_t m = mw.nmsm > 1 && tl.c[k].set_base >= mw.set_base[1] ? 1 : 0;
    sp.term_base[k] = terms;
    sp.msm[k] = m;
    sp.leaf_base[k] = leaves[m];
    terms += tl.c[k].count;
    leaves[m] += tl.c[k].count;
  }
  uint32_t nodes = 0, flags = 0;
  for (uint32_t m = 0; m < 2; ++m) {
    sp.count[m] = leaves[m];
    sp.node_base[m] = nodes;
    sp.flag_base[m] = flags;
    for (uint32_t cnt = leaves[m]; cnt > 1; cnt = (cnt + 1) >> 1) {
      nodes += cnt;
      flags += (cnt + 1) >> 1;
    }
  }
  p.small_terms = terms;
  p.small_nodes = nodes;
  p.small_flags = flags;
  p.bytes.small_nodes = (size_t)(nodes + 1) * SMALL_NODE_WORDS * 4;
  p.bytes.small_flags = (size_t)(flags + 1) * 4;
  p.bytes.res = 2 * sizeof(Xyzz<Cv>);
}

// part (chunked host-buffer batches, enqueue_batch_chunked): 0 the whole call; 1 the first point
// range -- sort + accumulate into the slot's bucket store, no reduction; 2 a middle range -- into
// the second store (acc29b, cntb, offb), merged into the first; 3 the last range -- as 2, then the
// reduction and window combination of the merged store.
// own_pts: the slot's points still have to be put into the accumulation's format.  alone: no
// other slot of the context has a job in flight.  sync_call: a synchronous device-buffer call.
template <class Cv>
MsmPlan plan_msm(const MsmTuning& t, const TermList& tl_in, uint32_t nsets, size_t emax, const MsmWindows& mw, int wbits,
                 int part, bool own_pts, bool alone, bool sync_call, bool async_call = false) {
  using XY = Xyzz<Cv>;
  MsmPlan p{};
  TermList& tl = p.tl = tl_in;
  if (own_pts)
    for (uint32_t k = 0; k < tl.nclass; ++k)
      if (tl.c[k].count) p.own_npts = std::max(p.own_npts, tl.c[k].pt_base + tl.c[k].count);
  p.small = part == 0 && t.small_terms && tl.total <= t.small_terms && mw.nmsm <= 2;
  for (uint32_t k = 0; k < tl.nclass; ++k) p.small = p.small && tl.c[k].win_off == 0;
  if (p.small) {
    plan_small<Cv>(p, mw);
    return p;
  }
  for (uint32_t k = 0; k < tl.nclass; ++k) {
    tl.c[k].dig_base = (uint32_t)p.ndig;
    p.ndig += (size_t)tl.c[k].count * tl.c[k].nwin;
  }
  if (p.ndig >= (1ull << 32)) {
    MsmPlan refused{};
    refused.refuse = "too many window digits for one call";
    return refused;
  }
  p.nbuckets = wbits == 13 ? Win<13>::NBUCKETS : Win<WBITS>::NBUCKETS;
  p.bins = wbits == 13 ? Win<13>::BINS : Win<WBITS>::BINS;
  p.rb_parts = wbits == 13 ? Win<13>::RB_PARTS : Win<WBITS>::RB_PARTS;
  p.NB = nsets * p.nbuckets;
  // accumulation threads: 64-entry chunks (16 for small calls, msm.hpp ACC_CHUNK_SMALL), at most
  // one resident round of them (then equal longer chunks)
  const size_t chunk = emax <= ACC_SMALL_ENTRIES ? ACC_CHUNK_SMALL : ACC_CHUNK;
  size_t nchunks = (emax + chunk - 1) / chunk + 1;
  const size_t cap = t.acc_threads_env ? t.acc_threads_env : (size_t)t.ncu * 4 * kAccWaves<Cv> * 64;
  if (cap && nchunks > cap) nchunks = cap;
  // A call with no other slot of the context in flight is latency-bound: below the cap, give
  // every SIMD the same whole number of waves (shorter equal chunks).  A 2^17 batch at 13 bits
  // is 1.25 waves per SIMD, and its SIMDs with two waves ran 1.5x longer than those with one:
  // 4.36 -> 3.99 ms per batch.  Pipelined calls keep the longer chunks (fewer pieces to join:
  // 2^17 batches 1014 vs 966/s with the rounding; profiles/r03/misc_ab_r03.txt).
  // (kzgmi_ctx_reserve plans with alone set: the piece arrays are sized for the rounded count)
  const size_t simd_lanes = (size_t)t.ncu * 4 * 64;
  if (alone && !t.acc_threads_env && emax > ACC_SMALL_ENTRIES && simd_lanes && nchunks < cap)
    nchunks = std::min(cap, (nchunks + simd_lanes - 1) / simd_lanes * simd_lanes);
  // Large radix-29 calls (the grid at its cap): acc_queue x cap shorter chunks taken from a
  // work queue by the cap's threads (msm.hpp k_accumulate), so an accumulation that starts behind
  // another slot's still ends on every CU at about the same time.  The part arrays and k_fixup
  // are sized for the chunk count.
  if (t.acc_queue > 1 && cap && nchunks == cap && cap % 256 == 0 && emax >= t.acc_queue_from) {
    p.acc_threads = cap;
    nchunks = std::min(cap * (size_t)t.acc_queue, std::max(cap, emax / t.acc_queue_min));
    if (nchunks <= cap) p.acc_threads = 0;
  }
  p.nchunks = nchunks = (nchunks + 255) / 256 * 256;  // = the launched thread count (part arrays indexed by thread)
  // Split accumulation (latency): the two MSMs' sets (MSM#1's a suffix of the sets) accumulate
  // in two launches of the same grid; the first launch's MSM reduces and combines on the
  // context's side stream beside the second launch (split_rev: which MSM goes first).
  p.split_set = mw.nmsm == 2 ? mw.set_base[1] : 0;
  p.can_split = part == 0 && mw.set_base[0] == 0 && p.split_set > 0 && p.split_set + mw.nwin[1] == nsets &&
                mw.nwin[0] == p.split_set && t.split_acc != 0;
  // auto: only where the second MSM's tail is the longer one (BLS12-381 without GLV: 16 windows
  // against 8).  GLV batches (BN254, trusted BLS12-381 points) have 8 windows in both MSMs: the
  // split only adds its side-stream contention (BN254 2^22: 14.70 -> 15.18 ms)
  p.split = p.can_split && (t.split_acc > 0 || (alone && sync_call && emax >= MsmTuning::SPLIT_FROM && mw.nwin[1] > mw.nwin[0]));
  // pieces: [A's first | A's last | B's first | B's last] when A's joins run on the side stream
  p.pieces = p.can_split && t.split_side_fix ? 2 * nchunks : nchunks;
  p.crowd_words = 1 + 3 * (p.pieces / FIX_LP_FROM + 2);  // at most one per FIX_LP_FROM + 1 chunks
  p.second = part >= 2;
  // Rows: only the unsplit static launch into the one store.  By default only asynchronous
  // BLS12-381 batches of at least ROWS_FROM entries: a row queue ends unevenly (its last rows are
  // the shortest, still tens of additions long), which the next batch's accumulation fills in a
  // pipeline and nothing does in a lone call.
  p.row_len = std::min<uint32_t>(std::max<uint32_t>(t.row_len, 1), ROW_LEN_MAX);
  p.rows = part == 0 && !p.split && !p.acc_threads &&
           (t.acc_rows > 0 || (t.acc_rows < 0 && Cv::ID == 0 && async_call && !sync_call && emax >= MsmTuning::ROWS_FROM));
  if (p.rows) {
    // a bucket of cnt > L entries is ceil(cnt / L) <= cnt / L + 1 items and fewer than emax / L
    // buckets are that long: below 2 emax / L piece slots, and as many more items than buckets
    p.row_cuts = emax / p.row_len + 1;
    p.row_pieces = 2 * p.row_cuts;
    p.row_items = ((size_t)p.NB + p.row_pieces + 63) / 64 * 64;
  }
  constexpr size_t rec = (size_t)kW29<Fp29Of<Cv>> * 4;  // a radix-29 record: buckets, bucket pieces, R / U / V
  MsmBytes& z = p.bytes;
  z.digits = p.ndig * 4;
  z.cnt = z.off = (size_t)p.NB * 4;
  if (p.second) z.cntb = z.offb = (size_t)p.NB * 4;
  z.coarse = (size_t)3 * nsets * p.bins * 4;
  z.ent = emax * 8;
  z.total = 16;
  if (p.acc_threads) z.accq = 16;
  z.crowd = 4 * p.crowd_words * (p.can_split ? 2 : 1);
  z.sval = emax * 4 + 16;  // + 16: k_accumulate reads values 4 at a time, up to 3 past the end
  z.skey = emax * 4;
  z.acc29 = ((size_t)p.NB + std::max(2 * p.pieces, p.row_pieces)) * rec;  // (either path may run on a reserved slot)
  if (p.rows) {
    z.rowq = (size_t)RQ_WORDS * 4;
    z.items = 3 * p.row_items * 4;
    z.cuts = 3 * p.row_cuts * 4;
  }
  if (p.second) z.acc29b = ((size_t)p.NB + 2 * nchunks) * rec;
  z.R = (size_t)p.NB / SEG * rec;
  z.U = (size_t)p.NB / SEG * rec * 2;  // U records, then the V records
  z.scratch = (size_t)nsets * p.rb_parts * sizeof(XY);  // k_reduce_bits partial sums
  z.winsum = (size_t)nsets * sizeof(XY);
  z.res = 2 * sizeof(XY);
  return p;
}

// What kzgmi_ctx_reserve sizes a slot for, batches of up to n tuples of one mode: the plan of the
// n-tuple batch as a call with no other slot in flight (the rounded grid: its piece arrays are the
// larger ones).  Two kinds of smaller batch plan something larger, so the largest of each kind is
// planned too: one that takes the small form, whose tree a bucket plan does not size, and one of
// at most ACC_SMALL_ENTRIES entries, whose short chunks can outnumber the chunks of a batch just
// above (its pieces: acc29, crowd).  A smaller batch at the other window width may still need more
// of some buffers.
template <class Cv>
MsmPlan plan_reserve(const MsmTuning& t, bool glv, bool powers, size_t n, bool own_pts, const BatchScalars& sc) {
  auto terms = [&](size_t nb) {
    const int wb = batch_wbits(t, powers, nb);
    return batch_terms(glv, powers, 0, windows_half(wb), windows_full(wb), nb, 0, 0, nb, true, sc);
  };
  auto plan = [&](size_t nb) {
    const BatchTerms bt = terms(nb);
    return plan_msm<Cv>(t, bt.tl, bt.nsets, bt.emax, bt.mw, batch_wbits(t, powers, nb), 0, own_pts, /*alone=*/true,
                        /*sync_call=*/false, /*async_call=*/true);
  };
  // the largest batch of at most n tuples with ok(its terms): ok holds up to some size (0: for none)
  auto largest = [&](auto ok) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
      const size_t mid = lo + (hi - lo + 1) / 2;
      if (ok(terms(mid))) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  MsmPlan p = plan(n);
  if (p.small || p.refuse) return p;
  if (const size_t ns = largest([&](const BatchTerms& b) { return b.tl.total <= t.small_terms; })) {
    const MsmPlan q = plan(ns);
    if (q.small) p.bytes.small_nodes = q.bytes.small_nodes, p.bytes.small_flags = q.bytes.small_flags;
  }
  if (const size_t ns = largest([&](const BatchTerms& b) { return b.emax <= ACC_SMALL_ENTRIES; })) {
    const MsmPlan q = plan(ns);
    if (!q.small && q.nbuckets == p.nbuckets) {
      p.bytes.acc29 = std::max(p.bytes.acc29, q.bytes.acc29);
      p.bytes.crowd = std::max(p.bytes.crowd, q.bytes.crowd);
    }
  }
  return p;
}

}  // namespace kzgmi
