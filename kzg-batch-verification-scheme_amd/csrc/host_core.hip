// The enqueue templates every feature's entry points share: the MSM core (small and bucket forms),
// the Fiat-Shamir transcript, the batch front end + two MSMs + pairing (enqueue_batch, and its
// chunked host-buffer form) and the plain MSM front end.  Instantiated for both curves at the end.
#include "host.hpp"

namespace kzgmi {

// ------------------------------------------------------------------------------ small MSMs
// The terms of tl (classes in order) as one wave each, MSM m's leaves in class order; the tree's
// stored nodes and arrival counters per MSM, level after level (msm_small.hpp).
template <class Cv>
static int run_small_msm(kzgmi_ctx* c, Slot& s, const TermList& tl, const MsmWindows& mw, const Affine<Cv>* pts,
                  const uint8_t* inf, bool own_pts, bool dry) {
  SmallPlan sp{};
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
  CHK(s.small_nodes.ensure((size_t)(nodes + 1) * SMALL_NODE_WORDS * 4));
  CHK(s.small_flags.ensure((size_t)(flags + 1) * 4));
  CHK(s.res.ensure(2 * sizeof(Xyzz<Cv>)));
  if (dry) return 0;
  Roctx rx("kzgmi.msm.small");
  hipStream_t st = s.stream;
  using L = Launch<Cv>;
  if (!pts) pts = s.pts.template as<Affine<Cv>>();
  if (!inf) inf = s.inf.template as<uint8_t>();
  if (own_pts) {  // the slot's points into the radix-29 slots the kernel reads
    uint32_t npts = 0;
    for (uint32_t k = 0; k < tl.nclass; ++k)
      if (tl.c[k].count) npts = std::max(npts, tl.c[k].pt_base + tl.c[k].count);
    L::pts_to29(st, s.pts.template as<Affine<Cv>>(), npts);
  }
  mark(c, s, PH_SORT + 1);
  L::small_msm(st, tl, sp, terms, pts, inf, s.small_nodes.template as<uint32_t>(), s.small_flags.template as<uint32_t>(),
               flags + 1, s.res.template as<Xyzz<Cv>>());
  mark(c, s, PH_ACCUM + 1);
  mark(c, s, PH_REDUCE + 1);
  mark(c, s, PH_COMBINE + 1);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------ MSM core
// part (chunked host-buffer batches, enqueue_batch_chunked): 0 the whole call; 1 the first point
// range -- sort + accumulate into the slot's bucket store, no reduction; 2 a middle range -- into
// the second store (acc29b, cntb, offb), merged into the first; 3 the last range -- as 2, then the
// reduction and window combination of the merged store
template <class Cv>
int HostCore<Cv>::run_msm_core(kzgmi_ctx* c, Slot& s, const TermList& tl_in, uint32_t nsets, size_t emax, const MsmWindows& mw,
                 const Affine<Cv>* pts, const uint8_t* inf, bool pts29, bool dry, int wbits, int part) {
  const uint32_t nbuckets = wbits == 13 ? Win<13>::NBUCKETS : Win<WBITS>::NBUCKETS;
  const uint32_t bins = wbits == 13 ? Win<13>::BINS : Win<WBITS>::BINS;
  const uint32_t rb_parts = wbits == 13 ? Win<13>::RB_PARTS : Win<WBITS>::RB_PARTS;
  // pts == nullptr: the slot's freshly converted points, put into the accumulation's format
  // here unless convert_points stored them in it already (pts29); explicit pts (commit-key
  // rows) are stored in that format already (kzgmi_ck_load)
  const bool own_pts = pts == nullptr && !pts29;
  // small calls: one wave per term and a summation tree (msm_small.hpp) instead of buckets
  {
    bool small = part == 0 && c->small_terms && tl_in.total <= c->small_terms && mw.nmsm <= 2;
    for (uint32_t k = 0; k < tl_in.nclass; ++k) small = small && tl_in.c[k].win_off == 0;
    if (small) return run_small_msm<Cv>(c, s, tl_in, mw, pts, inf, own_pts, dry);
  }
  TermList tl = tl_in;  // + each class's offset in the digit array
  size_t ndig = 0;
  for (uint32_t k = 0; k < tl.nclass; ++k) {
    tl.c[k].dig_base = (uint32_t)ndig;
    ndig += (size_t)tl.c[k].count * tl.c[k].nwin;
  }
  if (ndig >= (1ull << 32)) return fail(KZGMI_ERR_ARG, "too many window digits for one call");
  CHK(s.digits.ensure(ndig * 4));
  using XY = Xyzz<Cv>;
  if (!pts) pts = s.pts.template as<Affine<Cv>>();  // default: the slot's converted points
  if (!inf) inf = s.inf.template as<uint8_t>();
  const uint32_t NB = nsets * nbuckets;
  // accumulation threads: 64-entry chunks (16 for small calls, msm.hpp ACC_CHUNK_SMALL), at most
  // one resident round of them (then equal longer chunks)
  const size_t chunk = emax <= ACC_SMALL_ENTRIES ? ACC_CHUNK_SMALL : ACC_CHUNK;
  size_t nchunks = (emax + chunk - 1) / chunk + 1;
  const size_t cap = c->acc_threads_env ? c->acc_threads_env : (size_t)c->ncu * 4 * kAccWaves<Cv> * 64;
  if (cap && nchunks > cap) nchunks = cap;
  // A call with no other slot of the context in flight is latency-bound: below the cap, give
  // every SIMD the same whole number of waves (shorter equal chunks).  A 2^17 batch at 13 bits
  // is 1.25 waves per SIMD, and its SIMDs with two waves ran 1.5x longer than those with one:
  // 4.36 -> 3.99 ms per batch.  Pipelined calls keep the longer chunks (fewer pieces to join:
  // 2^17 batches 1014 vs 966/s with the rounding; profiles/r03/misc_ab_r03.txt).
  // (kzgmi_ctx_reserve sizes the piece arrays for the rounded count)
  bool alone = true;
  for (const Slot& o : c->slots) alone &= &o == &s || !o.pending;
  alone |= dry;
  const size_t simd_lanes = (size_t)c->ncu * 4 * 64;
  if (alone && !c->acc_threads_env && emax > ACC_SMALL_ENTRIES && simd_lanes && nchunks < cap)
    nchunks = std::min(cap, (nchunks + simd_lanes - 1) / simd_lanes * simd_lanes);
  // Large radix-29 calls (the grid at its cap): c->acc_queue x cap shorter chunks taken from a
  // work queue by the cap's threads (msm.hpp k_accumulate), so an accumulation that starts behind
  // another slot's still ends on every CU at about the same time.  The part arrays and k_fixup
  // are sized for the chunk count.
  size_t acc_threads = 0;
  if (c->acc_queue > 1 && cap && nchunks == cap && cap % 256 == 0 && emax >= c->acc_queue_from) {
    acc_threads = cap;
    nchunks = std::min(cap * (size_t)c->acc_queue, std::max(cap, emax / c->acc_queue_min));
    if (nchunks <= cap) acc_threads = 0;
  }
  nchunks = (nchunks + 255) / 256 * 256;  // = the launched thread count (part arrays indexed by thread)
  // Split accumulation (latency): the two MSMs' sets (MSM#1's a suffix of the sets) accumulate
  // in two launches; the first launch's MSM reduces and combines on the slot's side stream beside
  // the second launch (split_rev: which MSM goes first).
  const uint32_t split_set = mw.nmsm == 2 ? mw.set_base[1] : 0;
  const bool can_split = part == 0 && mw.set_base[0] == 0 && split_set > 0 && split_set + mw.nwin[1] == nsets &&
                         mw.nwin[0] == split_set && c->split_acc != 0;
  // auto: only where the second MSM's tail is the longer one (BLS12-381 without GLV: 16 windows
  // against 8).  GLV batches (BN254, trusted BLS12-381 points) have 8 windows in both MSMs: the
  // split only adds its side-stream contention (BN254 2^22: 14.70 -> 15.18 ms)
  const bool split = can_split && (c->split_acc > 0 || (alone && c->sync_call && emax >= kzgmi_ctx::SPLIT_FROM &&
                                                        mw.nwin[1] > mw.nwin[0]));
  const size_t nchunks_b = nchunks, acc_threads_b = acc_threads;  // the second launch's grid
  // pieces: [A's first | A's last | B's first | B's last] when A's joins run on the side stream
  const size_t pieces = can_split && c->split_side_fix ? nchunks + nchunks_b : std::max(nchunks, nchunks_b);
  const size_t crowd_words = 1 + 3 * (pieces / FIX_LP_FROM + 2);  // at most one per FIX_LP_FROM + 1 chunks
  CHK(s.cnt.ensure((size_t)NB * 4));
  CHK(s.off.ensure((size_t)NB * 4));
  const bool second = part >= 2;  // this range accumulates into the second store, then merges
  if (second) {
    CHK(s.cntb.ensure((size_t)NB * 4));
    CHK(s.offb.ensure((size_t)NB * 4));
  }
  DevBuf& CNT = second ? s.cntb : s.cnt;
  DevBuf& OFF = second ? s.offb : s.off;
  DevBuf& ACC = second ? s.acc29b : s.acc29;
  CHK(s.coarse.ensure((size_t)3 * nsets * bins * 4));
  CHK(s.ent.ensure(emax * 8));
  CHK(s.total.ensure(16));
  if (acc_threads || acc_threads_b) CHK(s.accq.ensure(16));
  CHK(s.crowd.ensure(4 * crowd_words * (can_split ? 2 : 1)));  // a split's second list after the first
  CHK(s.sval.ensure(emax * 4 + 16));  // + 16: k_accumulate reads values 4 at a time, up to 3 past the end
  CHK(s.skey.ensure(emax * 4));
  constexpr int W29 = kW29<Fp29Of<Cv>>;
  // buckets and bucket pieces are radix-29 records in acc29 (msm.hpp)
  CHK(s.acc29.ensure(((size_t)NB + 2 * pieces) * W29 * 4));
  if (second) CHK(s.acc29b.ensure(((size_t)NB + 2 * nchunks) * W29 * 4));
  const size_t seg_rec = (size_t)W29 * 4;  // a radix-29 record
  CHK(s.R.ensure((size_t)NB / SEG * seg_rec));
  CHK(s.U.ensure((size_t)NB / SEG * seg_rec * 2));  // U records, then the V records
  CHK(s.scratch.ensure((size_t)nsets * rb_parts * sizeof(XY)));  // k_reduce_bits partial sums
  CHK(s.winsum.ensure((size_t)nsets * sizeof(XY)));
  CHK(s.res.ensure(2 * sizeof(XY)));
  if (dry) return 0;  // kzgmi_ctx_reserve: workspace sized, nothing enqueued
  if (split && !c->side_stream) {  // at the slot stream's priority, or the device's greatest
    int prio = 0, least = 0, greatest = 0;
    HIPCHK(hipStreamGetPriority(s.stream, &prio));
    if (c->split_side_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) prio = greatest;
    HIPCHK(hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, prio));
  }
  if (split && !s.side_ev[0])
    for (auto& e : s.side_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  Roctx rx("kzgmi.msm.sort+accumulate+reduce+combine");
  hipStream_t st = s.stream;
  using L = Launch<Cv>;
  if (own_pts) {
    uint32_t npts = 0;
    for (uint32_t k = 0; k < tl.nclass; ++k)
      if (tl.c[k].count) npts = std::max(npts, tl.c[k].pt_base + tl.c[k].count);
    L::pts_to29(st, s.pts.template as<Affine<Cv>>(), npts);
  }
  L::sort(st, tl, nsets, inf, s.digits.template as<uint32_t>(), s.coarse.template as<uint32_t>(), s.ent.template as<uint64_t>(), emax,
          (c->sort_split ? L::SORT_SPLIT : 0) | (c->sort_full_bins ? L::SORT_FULL_BINS : 0),
          OFF.template as<uint32_t>(), CNT.template as<uint32_t>(), s.total.template as<uint32_t>(),
          s.sval.template as<uint32_t>(), s.skey.template as<uint32_t>(), wbits);
  mark(c, s, PH_SORT + 1);
  hipEvent_t* order_ev = nullptr;  // accumulation order (kzgmi_ctx::acc_order)
  const int order = emax >= kzgmi_ctx::ACC_ORDER_WIDE ? c->acc_order : c->acc_order_small;
  if (order > 0 && c->slots.size() > 1) {
    constexpr uint64_t M = kzgmi_ctx::kAccOrderMax;
    const uint64_t i = c->acc_launches++;
    if (i >= (uint64_t)order && c->acc_ring[(i - order) % M])  // the accumulation `order` launches back
      HIPCHK(hipStreamWaitEvent(st, c->acc_ring[(i - order) % M], 0));
    order_ev = &c->acc_ring[i % M];  // (launch i - M's event: no later launch waits for it)
    if (!*order_ev) HIPCHK(hipEventCreateWithFlags(order_ev, hipEventDisableTiming));
  }
  if (split) {
    // sets [split_set, nsets) are the sorted entries [coff[split_set * bins], total)
    const uint32_t* mid = s.coarse.template as<uint32_t>() + (size_t)nsets * bins + (size_t)split_set * bins;
    const uint32_t h = split_set, hn = nsets - split_set;
    uint32_t* acc = s.acc29.template as<uint32_t>();
    uint32_t* crowd_a = s.crowd.template as<uint32_t>();
    uint32_t* crowd_b = crowd_a + crowd_words;
    // launch A's pieces follow the buckets, launch B's follow A's: A's joins may run on the side
    // stream while B accumulates.  Order: MSM#1's sets [mid, total) first (split_rev 0), or
    // MSM#0's [0, mid) first (1); the first launch's MSM finishes on the side stream.
    const bool rev = c->split_rev;
    const uint32_t* total_a = rev ? mid : s.total.template as<uint32_t>();
    const uint32_t* lo_a = rev ? nullptr : mid;
    const uint32_t* total_b = rev ? s.total.template as<uint32_t>() : mid;
    const uint32_t* lo_b = rev ? mid : nullptr;
    const uint32_t nb_b = c->split_side_fix ? (uint32_t)(NB + 2 * nchunks) : NB;
    L::accumulate(st, nchunks, total_a, s.sval.template as<uint32_t>(), s.skey.template as<uint32_t>(),
                  s.off.template as<uint32_t>(), s.cnt.template as<uint32_t>(), pts, acc, NB, acc_threads,
                  acc_threads ? s.accq.template as<uint32_t>() : nullptr, crowd_a, lo_a,
                  c->split_side_fix ? nullptr : st);
    hipStream_t sd = c->side_stream;
    HIPCHK(hipEventRecord(s.side_ev[0], st));
    HIPCHK(hipStreamWaitEvent(sd, s.side_ev[0], 0));
    L::accumulate(st, nchunks_b, total_b, s.sval.template as<uint32_t>(), s.skey.template as<uint32_t>(),
                  s.off.template as<uint32_t>(), s.cnt.template as<uint32_t>(), pts, acc, nb_b, acc_threads_b,
                  acc_threads_b ? s.accq.template as<uint32_t>() : nullptr, crowd_b, lo_b, st);
    if (order_ev) HIPCHK(hipEventRecord(*order_ev, st));
    // MSM m's reduction and window combination on stream q: bucket records, R / U+V records, bit
    // sums and window sums at the offsets of its sets
    const size_t nseg = nbuckets / SEG;
    uint32_t* R29 = s.R.template as<uint32_t>();
    uint32_t* U29 = s.U.template as<uint32_t>();
    auto tail = [&](hipStream_t q, int m, bool lowp) {
      const uint32_t s0 = m ? h : 0, ns = m ? hn : h;
      L::reduce(q, ns, s.cnt.template as<uint32_t>() + (size_t)s0 * nbuckets, acc + (size_t)s0 * nbuckets * W29,
                reinterpret_cast<XY*>(R29 + s0 * nseg * W29), reinterpret_cast<XY*>(U29 + 2 * s0 * nseg * W29),
                s.scratch.template as<XY>() + (size_t)s0 * rb_parts, s.winsum.template as<XY>() + s0, wbits, lowp,
                c->seg4_waves, 4 * c->ncu);
      if (q == st) mark(c, s, PH_REDUCE + 1);
      L::window_combine(q, MsmWindows{1, {s0, 0}, {mw.nwin[m], 0}}, s.winsum.template as<XY>(),
                        s.res.template as<XY>() + m, wbits, lowp);
    };
    // side: (A's piece joins,) the first launch's MSM
    if (c->split_side_fix)
      L::fixup(sd, nchunks, total_a, s.skey.template as<uint32_t>(), s.off.template as<uint32_t>(),
               s.cnt.template as<uint32_t>(), acc, NB, crowd_a, lo_a);
    tail(sd, rev ? 0 : 1, c->split_low_prio);
    HIPCHK(hipEventRecord(s.side_ev[1], sd));
    mark(c, s, PH_ACCUM + 1);
    tail(st, rev ? 1 : 0, false);
    HIPCHK(hipStreamWaitEvent(st, s.side_ev[1], 0));
    mark(c, s, PH_COMBINE + 1);
    HIPCHK(hipGetLastError());
    return 0;
  }
  L::accumulate(st, nchunks, s.total.template as<uint32_t>(), s.sval.template as<uint32_t>(), s.skey.template as<uint32_t>(),
                OFF.template as<uint32_t>(), CNT.template as<uint32_t>(), pts, ACC.template as<uint32_t>(), NB,
                acc_threads, acc_threads ? s.accq.template as<uint32_t>() : nullptr, s.crowd.template as<uint32_t>(),
                nullptr, st);
  if (order_ev) HIPCHK(hipEventRecord(*order_ev, st));
  if (second)
    L::merge_buckets(st, NB, s.acc29.template as<uint32_t>(), s.cnt.template as<uint32_t>(),
                     s.acc29b.template as<uint32_t>(), s.cntb.template as<uint32_t>());
  mark(c, s, PH_ACCUM + 1);
  if (part == 1 || part == 2) {
    HIPCHK(hipGetLastError());
    return 0;  // more ranges follow
  }
  L::reduce(st, nsets, s.cnt.template as<uint32_t>(), s.acc29.template as<uint32_t>(), s.R.template as<XY>(),
            s.U.template as<XY>(), s.scratch.template as<XY>(), s.winsum.template as<XY>(), wbits, false, c->seg4_waves,
            4 * c->ncu);
  mark(c, s, PH_REDUCE + 1);
  L::window_combine(st, mw, s.winsum.template as<XY>(), s.res.template as<XY>(), wbits);
  mark(c, s, PH_COMBINE + 1);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------ Fiat-Shamir
static uint32_t next_pow2(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// 4096-leaf subtree roots of tuples [0, n) (global indices offset + i) -> returned device pointer
template <class Cv>
int HostCore<Cv>::enqueue_fs_digests(Slot& s, const void* dC, const void* dpi, const void* dz, const void* dy, size_t n,
                       uint64_t offset, bool compressed, const uint32_t** digests_out) {
  using L = Launch<Cv>;
  const uint32_t nch = (uint32_t)((n + FS_CHUNK - 1) / FS_CHUNK);
  const size_t slots = (size_t)nch * FS_CHUNK;
  CHK(s.fs_leaves.ensure(slots * 32));
  CHK(s.fs_tmp.ensure(slots * 24 + 64));
  HIPCHK(hipMemsetAsync(s.fs_leaves.p, 0, slots * 32, s.stream));
  L::fs_leaves(s.stream, (const uint8_t*)dC, (const uint8_t*)dpi, (const uint8_t*)dz, (const uint8_t*)dy, (uint32_t)n,
               offset, compressed, s.fs_leaves.template as<uint32_t>());
  *digests_out = L::fs_reduce(s.stream, s.fs_leaves.template as<uint32_t>(), (uint32_t)slots, nch,
                              s.fs_tmp.template as<uint32_t>());
  return 0;
}

// chunk digests (device) -> root -> r and its power table in s.pow, r (BE words) in s.chal
template <class Cv>
int HostCore<Cv>::enqueue_fs_challenge(Slot& s, const uint32_t* digests, uint32_t nch, uint64_t n_total) {
  using L = Launch<Cv>;
  const uint32_t p2 = next_pow2(nch);
  CHK(s.fs_top.ensure((size_t)p2 * 32 * 2 + 64));
  CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<typename Cv::FrP>)));
  CHK(s.chal.ensure(32));
  uint32_t* top = s.fs_top.template as<uint32_t>();
  HIPCHK(hipMemcpyAsync(top, digests, (size_t)nch * 32, hipMemcpyDeviceToDevice, s.stream));
  L::fs_pad(s.stream, top, nch, p2);
  const uint32_t* root = L::fs_reduce(s.stream, top, p2, 1, top + 8 * (size_t)p2);
  L::fs_challenge(s.stream, root, n_total, s.pow.p, s.chal.template as<uint32_t>());
  return 0;
}

// the workspaces enqueue_fs_digests + enqueue_fs_challenge grow for a batch of n tuples
template <class Cv>
static int reserve_fs(Slot& s, size_t n) {
  const uint32_t nch = (uint32_t)((n + FS_CHUNK - 1) / FS_CHUNK);
  const size_t slots = (size_t)nch * FS_CHUNK;
  CHK(s.fs_leaves.ensure(slots * 32));
  CHK(s.fs_tmp.ensure(slots * 24 + 64));
  CHK(s.fs_top.ensure((size_t)next_pow2(nch) * 32 * 2 + 64));
  CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<typename Cv::FrP>)));
  CHK(s.chal.ensure(32));
  return 0;
}

// Window width of a call from its entry count at c = 16 (msm.hpp Win): c = 13 for mid-size calls,
// 2^20 < entries <= max13 (batches: 2^15 < n <= 2^17, max13 = 2^22; MSMs: 2^16 < n <= 2^17,
// max13 = 2^21) -- 8x fewer buckets for 5/4 the terms, where the bucket-sum reduction is a large
// share of the pipelined work (2^17-tuple batches 875 -> 1024/s, 2^17-point MSMs 193 -> 224 M
// pts/s; profiles/r03/misc_ab_r03.txt).  Not for larger calls (a 2^18-point MSM: 270 -> 242)
// nor tiny ones, whose latency it raises: the top window of a 10 x 13-bit split of a 128-bit
// magnitude holds 11 bits (of a 20 x 13 split of 256 bits, 9), so its terms crowd into a few
// hundred buckets whose pieces k_fixup joins serially (n = 256: 3.0 -> 3.3 ms).  At 14 bits the
// top windows keep 2 and 4 bits: a 2^17 batch took 19 ms.  KZGMI_WBITS=13/16 forces one.
static int call_wbits(const kzgmi_ctx* c, size_t entries16, size_t max13) {
  if (c->wbits_env == 13 || c->wbits_env == WBITS) return c->wbits_env;
  return entries16 > (size_t(1) << 20) && entries16 <= max13 ? 13 : WBITS;
}
// windows of a 127-bit magnitude (randomisers, GLV halves) and of a full 255-bit scalar at width c
// (signed digits: the top window takes the last carry)
inline uint32_t windows_half(int wb) { return (uint32_t)((128 + wb - 1) / wb); }
inline uint32_t windows_full(int wb) { return (uint32_t)((256 + wb - 1) / wb); }

// ------------------------------------------------------------------------------ batch
template <class Cv>
int HostCore<Cv>::enqueue_batch(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                  const void* dpi, size_t n, const Seed& seed, uint64_t offset, void* d_partial_out,
                  uint32_t flags, bool dry, const void* d_blobs, const CellJob* cell) {
  using XY = Xyzz<Cv>;
  using FrF = Fp<typename Cv::FrP>;
  const bool glv = c->glv_batch &&
                   (Cv::ID == 1 || (flags & (KZGMI_FLAG_SUBGROUP_CHECK | KZGMI_FLAG_TRUSTED_G1)) != 0);
  // MSM#1's tail class: -t [1]_1, or for a cell batch (BLS12-381, powers + compressed + subgroup
  // check) the 64 terms -c_m [tau^m]_1
  const uint32_t tail = cell ? CellLaunch::TERMS : 1;
  // points: [pi (n) | C (n) | tail]; a cell batch keeps its m decoded unique commitments between
  // pi and the n gathered C, so that one subgroup check covers the n + m decoded points
  const size_t CB = n + (cell ? cell->m : 0), TB = CB + n;  // first C, first tail point
  const size_t PH = TB + tail;  // GLV: phi(pts[j]) at pts[PH + j]
  const size_t npts = glv ? 2 * PH : PH;
  using L = Launch<Cv>;
  CHK(s.pts.ensure(npts * sizeof(Affine<Cv>)));
  CHK(s.inf.ensure(npts));
  // powers: r_i = r^i (255-bit, caller-supplied r).  Fiat-Shamir: r from the transcript, then
  // the seeded 127-bit randomisers with seed = r (so 32n MSM entries, as with a host seed).
  const bool powers = (flags & KZGMI_FLAG_POWERS) != 0;
  if (glv) {
    CHK(s.glv_s.ensure(n * 32));
    CHK(s.glv_t.ensure((size_t)tail * 32));
    if (powers) CHK(s.glv_r.ensure(n * 32));
  }
  CHK(s.scal_r.ensure(n * (powers ? 32 : 16)));
  CHK(s.scal_s.ensure(n * 32));
  CHK(s.scal_t.ensure(32));
  CHK(s.tpart.ensure(L::tpart_bytes((uint32_t)n)));
  CHK(s.flags.ensure(16));
  // blob batch (powers mode): z_i, y_i and r are derived on the device, in front(); cell batch:
  // z_k = h_k^64, y_k = 0, r and the 64 coefficients are
  if (d_blobs || cell) {
    CHK(s.blob_z.ensure(n * 32));
    CHK(s.blob_y.ensure(n * 32));
    CHK(s.pow.ensure(FS_POW_BITS * sizeof(FrF)));
    CHK(s.chal.ensure(32));
    if (cell) {
      CHK(s.cell_part.ensure(CellLaunch::part_bytes()));
      CHK(s.cell_coef.ensure(CellLaunch::TERMS * 32));
    }
    dz = s.blob_z.p;
    dy = s.blob_y.p;
  }
  if (dry) {  // kzgmi_ctx_reserve: the randomiser workspaces of this mode, no launches
    if (flags & KZGMI_FLAG_FIAT_SHAMIR) CHK(reserve_fs<Cv>(s, n));
    else if (flags & KZGMI_FLAG_POWERS) CHK(s.pow.ensure(FS_POW_BITS * sizeof(FrF)));
  }
  hipStream_t st = s.stream;
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  Affine<Cv>* pts = s.pts.template as<Affine<Cv>>();
  uint8_t* inf = s.inf.template as<uint8_t>();
  // points that only feed the radix-29 accumulation are converted straight into its format
  // (with GLV their images too: k_endo_points29); decompression and the subgroup check work in
  // the 32-bit form, converted afterwards by run_msm_core's k_pts_to29
  const bool pts29 = !(flags & (KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK));
  const uint32_t nn = (uint32_t)n;
  uint32_t* gs = s.glv_s.template as<uint32_t>();
  uint32_t* gt = s.glv_t.template as<uint32_t>();
  uint32_t* gr = s.glv_r.template as<uint32_t>();
  // decode + validate the points, derive the randomisers and the MSM scalars
  auto front = [&]() -> int {
    Roctx rx("kzgmi.batch.convert+scalars");
    CHK(begin_job(s));
    mark(c, s, 0);
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
    if (cell) {  // the m unique commitments are decoded (and checked) once, then gathered
      L::decompress_points(st, (const uint8_t*)dpi, (uint32_t)n, pts, inf, err);
      L::decompress_points(st, (const uint8_t*)dC, (uint32_t)cell->m, pts + n, inf + n, err);
    } else if (flags & KZGMI_FLAG_COMPRESSED) {
      L::decompress_points(st, (const uint8_t*)dpi, (uint32_t)n, pts, inf, err);
      L::decompress_points(st, (const uint8_t*)dC, (uint32_t)n, pts + n, inf + n, err);
    } else if (glv && pts29) {  // with phi(P) stored by the same pass (no k_endo_points29 over 2n points)
      L::convert_points(st, (const uint8_t*)dpi, (uint32_t)n, pts, inf, err, true, pts + PH, inf + PH);
      L::convert_points(st, (const uint8_t*)dC, (uint32_t)n, pts + n, inf + n, err, true, pts + PH + n, inf + PH + n);
    } else {
      L::convert_points(st, (const uint8_t*)dpi, (uint32_t)n, pts, inf, err, pts29);
      L::convert_points(st, (const uint8_t*)dC, (uint32_t)n, pts + n, inf + n, err, pts29);
    }
    if (cell) {
      if constexpr (Cv::ID == 0) {
        L::subgroup_check(st, pts, inf, (uint32_t)CB, err);
        CellLaunch::gather(st, cell->cidx, nn, (uint32_t)cell->m, pts, inf, nn, (uint32_t)CB);
      }
      // the cell SRS's [tau^m]_1 as the last 64 terms of MSM#1 (their images were made at SRS load)
      const Affine<Cv>* sp = cell->srs->pts.template as<Affine<Cv>>();
      const uint8_t* si = cell->srs->inf.template as<uint8_t>();
      HIPCHK(hipMemcpyAsync(pts + TB, sp, tail * sizeof(Affine<Cv>), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(inf + TB, si, tail, hipMemcpyDeviceToDevice, st));
      if (glv) {
        HIPCHK(hipMemcpyAsync(pts + PH + TB, sp + tail, tail * sizeof(Affine<Cv>), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(inf + PH + TB, si + tail, tail, hipMemcpyDeviceToDevice, st));
        L::endo_points(st, pts, inf, (uint32_t)TB, pts + PH, inf + PH, false);
      }
    } else {
      if (flags & KZGMI_FLAG_SUBGROUP_CHECK) L::subgroup_check(st, pts, inf, (uint32_t)(2 * n), err);
      // the SRS's [1]_1 as the last term of MSM#1: -t [1]_1
      HIPCHK(hipMemcpyAsync(pts + 2 * n, pts29 ? srs->g1_29() : srs->g1.p, sizeof(Affine<Cv>), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(inf + 2 * n, srs->g1.template as<uint8_t>() + sizeof(Affine<Cv>), 1, hipMemcpyDeviceToDevice, st));
      if (glv && pts29)  // the converts stored the 2n images: G1's alone
        L::endo_points(st, pts + 2 * n, inf + 2 * n, 1, pts + PH + 2 * n, inf + PH + 2 * n, true);
      else if (glv)
        L::endo_points(st, pts, inf, (uint32_t)PH, pts + PH, inf + PH, pts29);
    }
    mark(c, s, PH_CONVERT + 1);
    if (flags & KZGMI_FLAG_FIAT_SHAMIR) {  // r from the transcript of this (whole) batch
      const uint32_t* digests = nullptr;
      CHK(HostCore<Cv>::enqueue_fs_digests(s, dC, dpi, dz, dy, n, 0, (flags & KZGMI_FLAG_COMPRESSED) != 0, &digests));
      CHK(HostCore<Cv>::enqueue_fs_challenge(s, digests, (uint32_t)((n + FS_CHUNK - 1) / FS_CHUNK), n));
    } else if (d_blobs) {  // the EIP-4844 transcript: z_i, y_i = p_i(z_i), then r and its power table
      uint8_t* bz = s.blob_z.template as<uint8_t>();
      uint8_t* by = s.blob_y.template as<uint8_t>();
      BlobLaunch::challenges(st, blob_mapping(c, n), (const uint8_t*)d_blobs, (const uint8_t*)dC, (uint32_t)n, bz, err);
      BlobLaunch::eval(st, (const uint8_t*)d_blobs, bz, c->blob_table.p, (uint32_t)n, false, by, err);
      BlobLaunch::batch_challenge(st, (const uint8_t*)dC, bz, by, (const uint8_t*)dpi, (uint32_t)n, s.pow.p,
                                  s.chal.template as<uint32_t>());
    } else if (cell && cell->derive) {  // the EIP-7594 transcript: r and its power table
      CellLaunch::batch_challenge(st, (const uint8_t*)dC, (uint32_t)cell->m, cell->cidx, cell->eidx,
                                  (const uint8_t*)cell->cells, (const uint8_t*)dpi, nn, s.pow.p,
                                  s.chal.template as<uint32_t>());
    } else if (flags & KZGMI_FLAG_POWERS) {  // r supplied by the caller in place of the seed
      CHK(s.pow.ensure(FS_POW_BITS * sizeof(FrF)));
      L::pow_table(st, seed, s.pow.p, err);
    }
    if (cell)  // z_k = h_k^64, y_k = 0 where k_scalar_prep_pow reads them; the indices are checked here
      CellLaunch::z(st, cell->eidx, cell->cidx, nn, (uint32_t)cell->m, c->cell_table.p, s.blob_z.template as<uint8_t>(),
                    s.blob_y.template as<uint8_t>(), err);
    if (powers)
      L::scalar_prep_pow(st, s.pow.p, offset, (const uint8_t*)dz, (const uint8_t*)dy, (uint32_t)n,
                         s.scal_r.template as<uint32_t>(), s.scal_s.template as<uint32_t>(), s.tpart.p,
                         s.scal_t.template as<uint32_t>(), err);
    if (cell)  // -c_m of sum_k r^k I_k, weighted by the r^k just written
      CellLaunch::interp(st, cell->eidx, (const uint8_t*)cell->cells, s.scal_r.template as<uint32_t>(), nn,
                         c->cell_table.p, s.cell_part.p, s.cell_coef.template as<uint32_t>(), nullptr, err);
    if (!powers)
      L::scalar_prep(st, seed, (flags & KZGMI_FLAG_FIAT_SHAMIR) ? s.chal.template as<uint32_t>() : nullptr, offset, (const uint8_t*)dz, (const uint8_t*)dy, (uint32_t)n,
                     s.scal_r.template as<uint32_t>(), s.scal_s.template as<uint32_t>(), s.tpart.p,
                     s.scal_t.template as<uint32_t>(), err, glv ? gs : nullptr, glv ? gs + 4 * (size_t)n : nullptr);
    if (glv) {  // (s_i split by k_scalar_prep itself unless the powers form produced it)
      if (powers) L::glv_split(st, s.scal_s.template as<uint32_t>(), 8, nn, gs, gs + 4 * (size_t)n);
      if (cell) L::glv_split(st, s.cell_coef.template as<uint32_t>(), 8, tail, gt, gt + 4 * (size_t)tail);
      else L::glv_split(st, s.scal_t.template as<uint32_t>(), 8, 1, gt, gt + 4);
      if (powers) L::glv_split(st, s.scal_r.template as<uint32_t>(), 8, nn, gr, gr + 4 * (size_t)n);
    }
    mark(c, s, PH_SCALARS + 1);
    return 0;
  };
  if (!dry) CHK(front());
  TermList tl{};
  const uint32_t ph = (uint32_t)PH, cb = (uint32_t)CB, tb = (uint32_t)TB;  // (cb = n, tb = 2n but for cell batches)
  // c = 16: H = 8 windows for 127-bit magnitudes, F = 16 for full scalars; c = 13: 10 and 20
  const int wb = call_wbits(c, (size_t)(powers ? 48 : 32) * n, size_t(1) << 22);
  const uint32_t H = windows_half(wb), F = windows_full(wb);
  if (glv) {  // every MSM in H windows of half scalars: sets 0..H-1 (MSM#0), H..2H-1 (MSM#1)
    const uint32_t* rr = s.scal_r.template as<uint32_t>();
    uint32_t k = 0;
    if (!powers) {
      tl.c[k++] = {nn, 0, 4, H, 0, 4, rr};                     // MSM#0: r_i pi_i
      tl.c[k++] = {nn, nn, 4, H, H, 4, rr};                    // MSM#1: r_i C_i
    } else {
      tl.c[k++] = {nn, 0, 4, H, 0, 4, gr};                     // MSM#0: r_i pi_i = h0 pi + h1 phi(pi)
      tl.c[k++] = {nn, ph, 4, H, 0, 4, gr + 4 * (size_t)n};
      tl.c[k++] = {nn, cb, 4, H, H, 4, gr};                    // MSM#1: r_i C_i
      tl.c[k++] = {nn, ph + cb, 4, H, H, 4, gr + 4 * (size_t)n};
    }
    tl.c[k++] = {nn, 0, 4, H, H, 4, gs};                       //        s_i pi_i
    tl.c[k++] = {nn, ph, 4, H, H, 4, gs + 4 * (size_t)n};
    tl.c[k++] = {tail, tb, 4, H, H, cell ? 4u : 0u, gt};       //        -t G1 (cells: -c_m [tau^m]_1)
    tl.c[k++] = {tail, ph + tb, 4, H, H, cell ? 4u : 0u, gt + 4 * (size_t)tail};
    tl.nclass = k;
    tl.total = 0;
    for (uint32_t j = 0; j < k; ++j) tl.total += tl.c[j].count;
    const MsmWindows mw{2, {0, H}, {H, H}};
    CHK(HostCore<Cv>::run_msm_core(c, s, tl, 2 * H, (size_t)(powers ? 6 : 4) * H * n + 2 * H * tail + 16, mw, nullptr, nullptr,
                                   pts29, dry, wb));
  } else if (!powers) {  // 127-bit r_i: MSM#0 in H windows (sets 0..H-1), MSM#1 in F (sets H..H+F-1)
    tl.c[0] = {nn, 0, 4, H, 0, 4, s.scal_r.template as<uint32_t>()};          // MSM#0: r_i pi_i
    tl.c[1] = {nn, nn, 4, H, H, 4, s.scal_r.template as<uint32_t>()};         // MSM#1: r_i C_i
    tl.c[2] = {nn, 0, 8, F, H, 8, s.scal_s.template as<uint32_t>()};          //        s_i pi_i
    tl.c[3] = {1, 2 * nn, 8, F, H, 0, s.scal_t.template as<uint32_t>()};      //        -t G1
  }
  if (!glv && powers) {  // r_i = r^i, full Fr: both MSMs in F windows (sets 0..F-1, F..2F-1)
    tl.c[0] = {nn, 0, 8, F, 0, 8, s.scal_r.template as<uint32_t>()};
    tl.c[1] = {nn, cb, 8, F, F, 8, s.scal_r.template as<uint32_t>()};
    tl.c[2] = {nn, 0, 8, F, F, 8, s.scal_s.template as<uint32_t>()};
    tl.c[3] = {1, 2 * nn, 8, F, F, 0, s.scal_t.template as<uint32_t>()};
    if (cell) tl.c[3] = {tail, tb, 8, F, F, 8, s.cell_coef.template as<uint32_t>()};  // -c_m [tau^m]_1
  }
  if (!glv) {
    tl.nclass = 4;
    tl.total = 3 * nn + tail;
    const MsmWindows mw = powers ? MsmWindows{2, {0, F}, {F, F}} : MsmWindows{2, {0, H}, {H, F}};
    CHK(HostCore<Cv>::run_msm_core(c, s, tl, powers ? 2 * F : H + F, (size_t)(powers ? 3 * F : 2 * H + F) * n + (size_t)F * tail + 16, mw,
                                   nullptr, nullptr, pts29, dry, wb));
  }
  if (dry) return 0;
  Roctx rx("kzgmi.batch.pairing");
  if (d_partial_out) {
    L::partial_out(st, s.res.template as<XY>(), 2, err, (XY*)d_partial_out);  // marked if this shard failed
  } else {
    L::pairing_check(st, s.res.template as<XY>(), srs->lines.template as<Line<Cv>>(), srs->q_inf.template as<uint8_t>(),
                     s.flags.template as<int>());
    mark(c, s, PH_PAIRING + 1);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, d_partial_out ? JobKind::BatchPartial : JobKind::Verdict, Cv::ID);
  return 0;
}

// A synchronous host-buffer batch (plain flags, or TRUSTED_G1; BN254 and declared-G1 points take
// the GLV form) as k point ranges on one slot: range j's copy (the context's copy stream) overlaps
// the previous ranges' front end and accumulation on the slot's stream, every range accumulates
// into the same bucket sets (a second store merged into the first, run_msm_core parts 1..3), the
// G1 term joins the last range (its scalar needs every range's r_i y_i), and one reduction,
// combination and pairing decide.  Same r_i (global index), same sums as enqueue_batch; the
// inputs land in the slot's stage buffer.
template <class Cv>
int HostCore<Cv>::enqueue_batch_chunked(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, const uint8_t* hC, const uint8_t* hz,
                          const uint8_t* hy, const uint8_t* hpi, size_t n, const Seed& seed, uint32_t flags, int k) {
  using XY = Xyzz<Cv>;
  using L = Launch<Cv>;
  using FrF = Fp<typename Cv::FrP>;
  const bool glv = c->glv_batch && (Cv::ID == 1 || (flags & KZGMI_FLAG_TRUSTED_G1) != 0);
  const size_t gb = g1_bytes(Cv::ID);
  const size_t PH = 2 * n + 1;  // GLV: phi(pts[j]) at pts[PH + j]
  CHK(s.pts.ensure((glv ? 2 * PH : PH) * sizeof(Affine<Cv>)));
  CHK(s.inf.ensure(glv ? 2 * PH : PH));
  CHK(s.scal_r.ensure(n * 16));
  CHK(s.scal_s.ensure(n * 32));
  CHK(s.scal_t.ensure(32));
  if (glv) {
    CHK(s.glv_s.ensure(n * 32));
    CHK(s.glv_t.ensure(32));
  }
  CHK(s.tpart.ensure(L::tpart_bytes((uint32_t)n)));
  CHK(s.flags.ensure(16));
  CHK(s.stage.ensure(n * (2 * gb + 64)));
  uint8_t* dC = s.stage.template as<uint8_t>();
  uint8_t* dpi = dC + n * gb;
  uint8_t* dz = dC + 2 * n * gb;
  uint8_t* dy = dz + 32 * n;
  Affine<Cv>* pts = s.pts.template as<Affine<Cv>>();
  uint8_t* inf = s.inf.template as<uint8_t>();
  uint32_t* sr = s.scal_r.template as<uint32_t>();
  uint32_t* ss = s.scal_s.template as<uint32_t>();
  uint32_t* stt = s.scal_t.template as<uint32_t>();
  uint32_t* gs = s.glv_s.template as<uint32_t>();  // [h0 x n | h1 x n]
  uint32_t* gt = s.glv_t.template as<uint32_t>();
  FrF* tpart = reinterpret_cast<FrF*>(s.tpart.p);
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  const int wb = call_wbits(c, (size_t)32 * n, size_t(1) << 22);
  const uint32_t H = windows_half(wb), F = windows_full(wb);
  const MsmWindows mw = glv ? MsmWindows{2, {0, H}, {H, H}} : MsmWindows{2, {0, H}, {H, F}};
  const uint32_t nsets = glv ? 2 * H : H + F;
  const uint32_t nn = (uint32_t)n, ph = (uint32_t)PH;
  // the first range short (its copy is the only one nothing overlaps), the others equal
  std::vector<size_t> nk(k);
  {
    const size_t units = (n + FS_CHUNK - 1) / FS_CHUNK;
    const size_t u0 = k > 1 ? std::max<size_t>(1, units / (2 * (size_t)k)) : units;
    nk[0] = std::min(n, u0 * FS_CHUNK);
    const std::vector<size_t> rest = split_units(n - nk[0], k - 1 > 0 ? k - 1 : 1);
    for (int j = 1; j < k; ++j) nk[j] = rest[j - 1];
  }
  auto terms = [&](size_t lo, size_t nj, bool last) {
    TermList tl{};
    const uint32_t l = (uint32_t)lo, m = (uint32_t)nj;
    uint32_t q = 0;
    tl.c[q++] = {m, l, 4, H, 0, 4, sr + 4 * lo};           // MSM#0: r_i pi_i
    tl.c[q++] = {m, nn + l, 4, H, H, 4, sr + 4 * lo};      // MSM#1: r_i C_i
    if (glv) {
      tl.c[q++] = {m, l, 4, H, H, 4, gs + 4 * lo};         //        s_i pi_i = h0 pi + h1 phi(pi)
      tl.c[q++] = {m, ph + l, 4, H, H, 4, gs + 4 * (n + lo)};
      if (last) {
        tl.c[q++] = {1, 2 * nn, 4, H, H, 0, gt};           //        -t G1
        tl.c[q++] = {1, ph + 2 * nn, 4, H, H, 0, gt + 4};
      }
    } else {
      tl.c[q++] = {m, l, 8, F, H, 8, ss + 8 * lo};         //        s_i pi_i
      if (last) tl.c[q++] = {1, 2 * nn, 8, F, H, 0, stt};  //        -t G1
    }
    tl.nclass = q;
    tl.total = 0;
    for (uint32_t j = 0; j < q; ++j) tl.total += tl.c[j].count;
    return tl;
  };
  auto emax_of = [&](size_t nj) {
    return glv ? (size_t)4 * H * nj + 2 * H + 16 : (size_t)(2 * H + F) * nj + F + 16;
  };
  size_t nmax = 0;
  for (size_t v : nk) nmax = std::max(nmax, v);
  // every workspace at its final size before the first launch (a later growth would free a buffer
  // an earlier range's kernels are still using)
  CHK(HostCore<Cv>::run_msm_core(c, s, terms(0, nmax, true), nsets, emax_of(nmax), mw, nullptr, nullptr, true, true, wb, 3));
  hipStream_t st = s.stream, cs = c->h2d_stream;
  if (s.done_rec) HIPCHK(hipStreamWaitEvent(cs, s.done_ev, 0));  // the stage buffer is free
  size_t lo = 0;
  for (int j = 0; j < k; ++j) {
    const size_t nj = nk[j];
    const bool last = j == k - 1;
    CHK(h2d(s, cs, dC + lo * gb, hC + lo * gb, nj * gb));
    CHK(h2d(s, cs, dpi + lo * gb, hpi + lo * gb, nj * gb));
    CHK(h2d(s, cs, dz + 32 * lo, hz + 32 * lo, nj * 32));
    CHK(h2d(s, cs, dy + 32 * lo, hy + 32 * lo, nj * 32));
    CHK(add_dep(s, cs));
    CHK(begin_job(s));  // this range's kernels wait for its copy only
    if (j == 0) {
      mark(c, s, 0);
      HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
      HIPCHK(hipMemcpyAsync(pts + 2 * n, srs->g1_29(), sizeof(Affine<Cv>), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(inf + 2 * n, srs->g1.template as<uint8_t>() + sizeof(Affine<Cv>), 1,
                            hipMemcpyDeviceToDevice, st));
      if (glv) L::endo_points(st, pts + 2 * n, inf + 2 * n, 1, pts + PH + 2 * n, inf + PH + 2 * n, true);
    }
    if (glv) {  // phi(P) stored by the same pass
      L::convert_points(st, dpi + lo * gb, (uint32_t)nj, pts + lo, inf + lo, err, true, pts + PH + lo, inf + PH + lo);
      L::convert_points(st, dC + lo * gb, (uint32_t)nj, pts + n + lo, inf + n + lo, err, true, pts + PH + n + lo,
                        inf + PH + n + lo);
    } else {
      L::convert_points(st, dpi + lo * gb, (uint32_t)nj, pts + lo, inf + lo, err, true);
      L::convert_points(st, dC + lo * gb, (uint32_t)nj, pts + n + lo, inf + n + lo, err, true);
    }
    // range j's per-block r_i y_i sums land at its blocks of tpart (lo is a multiple of PREP_BLOCK)
    L::scalar_prep(st, seed, nullptr, lo, dz + 32 * lo, dy + 32 * lo, (uint32_t)nj, sr + 4 * lo, ss + 8 * lo,
                   tpart + lo / PREP_BLOCK, stt, err, glv ? gs + 4 * lo : nullptr, glv ? gs + 4 * (n + lo) : nullptr);
    if (last) {  // -t over every range (then its GLV halves)
      L::tsum(st, tpart, (uint32_t)((n + PREP_BLOCK - 1) / PREP_BLOCK), stt);
      if (glv) L::glv_split(st, stt, 8, 1, gt, gt + 4);
    }
    const int part = k == 1 ? 0 : j == 0 ? 1 : last ? 3 : 2;
    CHK(HostCore<Cv>::run_msm_core(c, s, terms(lo, nj, last), nsets, emax_of(nj), mw, nullptr, nullptr, true, false, wb, part));
    lo += nj;
  }
  L::pairing_check(st, s.res.template as<XY>(), srs->lines.template as<Line<Cv>>(), srs->q_inf.template as<uint8_t>(),
                   s.flags.template as<int>());
  mark(c, s, PH_PAIRING + 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Verdict, Cv::ID);
  return 0;
}

template <class Cv>
int HostCore<Cv>::enqueue_msm(kzgmi_ctx* c, Slot& s, const void* dpts, const void* dsc, size_t n, bool allow_glv) {
  const bool glv = allow_glv && c->glv_msm && (Cv::ID == 1 || c->msm_trusted_g1);
  CHK(s.pts.ensure((glv ? 2 : 1) * n * sizeof(Affine<Cv>)));
  CHK(s.inf.ensure((glv ? 2 : 1) * n));
  CHK(s.scal_s.ensure(n * 32));
  if (glv) CHK(s.glv_s.ensure(n * 32));
  CHK(s.flags.ensure(16));
  CHK(begin_job(s));
  hipStream_t st = s.stream;
  mark(c, s, 0);
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  Affine<Cv>* pts = s.pts.template as<Affine<Cv>>();
  uint8_t* inf = s.inf.template as<uint8_t>();
  const bool pts29 = true;
  if (glv && pts29)  // phi(P) stored by the converting pass
    Launch<Cv>::convert_points(st, (const uint8_t*)dpts, (uint32_t)n, pts, inf, err, true, pts + n, inf + n);
  else
    Launch<Cv>::convert_points(st, (const uint8_t*)dpts, (uint32_t)n, pts, inf, err, pts29);
  if (glv && !pts29) Launch<Cv>::endo_points(st, pts, inf, (uint32_t)n, pts + n, inf + n, pts29);
  mark(c, s, PH_CONVERT + 1);
  uint32_t* sc = s.scal_s.template as<uint32_t>();
  Launch<Cv>::convert_scalars(st, (const uint8_t*)dsc, (uint32_t)n, sc, err);
  uint32_t* gs = s.glv_s.template as<uint32_t>();
  if (glv) Launch<Cv>::glv_split(st, sc, 8, (uint32_t)n, gs, gs + 4 * n);
  mark(c, s, PH_SCALARS + 1);
  TermList tl{};
  const uint32_t nn = (uint32_t)n;
  const int wb = call_wbits(c, (size_t)16 * n, size_t(1) << 21);
  const uint32_t H = windows_half(wb), F = windows_full(wb);
  if (glv) {  // sum k_i P_i = sum h0_i P_i + h1_i phi(P_i): H windows, H bucket sets
    tl.c[0] = {nn, 0, 4, H, 0, 4, gs};
    tl.c[1] = {nn, nn, 4, H, 0, 4, gs + 4 * n};
    tl.nclass = 2;
    tl.total = 2 * nn;
    const MsmWindows mw{1, {0, 0}, {H, 0}};
    CHK(HostCore<Cv>::run_msm_core(c, s, tl, H, (size_t)2 * H * n + 16, mw, nullptr, nullptr, pts29, false, wb));
  } else {
    tl.c[0] = {nn, 0, 8, F, 0, 8, sc};
    tl.nclass = 1;
    tl.total = nn;
    const MsmWindows mw{1, {0, 0}, {F, 0}};
    CHK(HostCore<Cv>::run_msm_core(c, s, tl, F, (size_t)F * n + 16, mw, nullptr, nullptr, pts29, false, wb));
  }
  s.curve = Cv::ID;
  return 0;
}

template struct HostCore<Bls12_381>;
template struct HostCore<Bn254>;

}  // namespace kzgmi
