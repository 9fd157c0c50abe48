// The enqueue templates every feature's entry points share: the MSM core (small and bucket forms),
// the Fiat-Shamir transcript, the batch front end + two MSMs + pairing (enqueue_batch, and its
// chunked host-buffer form) and the plain MSM front end.  Instantiated for both curves at the end.
#include "host.hpp"

namespace kzgmi {

// ------------------------------------------------------------------------------ MSM core
// Every MSM call is planned as plain data (msm_plan.hpp plan_msm), then the slot's buffers grow to
// the plan's sizes (ensure_msm), then the plan is enqueued.

// no other slot of the context has a job in flight (such a call is latency-bound)
static bool slot_alone(const kzgmi_ctx* c, const Slot& s) {
  bool alone = true;
  for (const Slot& o : c->slots) alone &= &o == &s || !o.pending;
  return alone;
}

// the slot's buffers at the sizes plan p asks for; a refused plan fails here
static int ensure_msm(Slot& s, const MsmPlan& p) {
  if (p.refuse) return fail(KZGMI_ERR_ARG, p.refuse);
  const MsmBytes& z = p.bytes;
  if (p.small) {
    CHK(s.small_nodes.ensure(z.small_nodes));
    CHK(s.small_flags.ensure(z.small_flags));
    return s.res.ensure(z.res);
  }
  CHK(s.digits.ensure(z.digits));
  CHK(s.cnt.ensure(z.cnt));
  CHK(s.off.ensure(z.off));
  if (p.second) {
    CHK(s.cntb.ensure(z.cntb));
    CHK(s.offb.ensure(z.offb));
  }
  CHK(s.coarse.ensure(z.coarse));
  CHK(s.ent.ensure(z.ent));
  CHK(s.total.ensure(z.total));
  if (p.acc_threads) CHK(s.accq.ensure(z.accq));
  CHK(s.crowd.ensure(z.crowd));
  if (p.rows) {
    CHK(s.rowq.ensure(z.rowq));
    CHK(s.items.ensure(z.items));
    CHK(s.cuts.ensure(z.cuts));
  }
  CHK(s.sval.ensure(z.sval));
  CHK(s.skey.ensure(z.skey));
  CHK(s.acc29.ensure(z.acc29));
  if (p.second) CHK(s.acc29b.ensure(z.acc29b));
  CHK(s.R.ensure(z.R));
  CHK(s.U.ensure(z.U));
  CHK(s.scratch.ensure(z.scratch));
  CHK(s.winsum.ensure(z.winsum));
  if (z.small_nodes) {  // plan_reserve: the tree of a smaller call in the small form
    CHK(s.small_nodes.ensure(z.small_nodes));
    CHK(s.small_flags.ensure(z.small_flags));
  }
  return s.res.ensure(z.res);
}

// small calls: one wave per term and a summation tree (msm_small.hpp) instead of buckets
template <class Cv>
static int enqueue_small_msm(kzgmi_ctx* c, Slot& s, const MsmPlan& p, const Affine<Cv>* pts, const uint8_t* inf) {
  Roctx rx("kzgmi.msm.small");
  hipStream_t st = s.stream;
  using L = Launch<Cv>;
  L::pts_to29(st, s.pts.template as<Affine<Cv>>(), p.own_npts);  // into the radix-29 slots the kernel reads
  mark(c, s, PH_SORT + 1);
  L::small_msm(st, p.tl, p.sp, p.small_terms, pts, inf, s.small_nodes.template as<uint32_t>(),
               s.small_flags.template as<uint32_t>(), p.small_flags + 1, s.res.template as<Xyzz<Cv>>());
  mark(c, s, PH_ACCUM + 1);
  mark(c, s, PH_REDUCE + 1);
  mark(c, s, PH_COMBINE + 1);
  HIPCHK(hipGetLastError());
  return 0;
}

// part: the range of a chunked host-buffer batch this call is (msm_plan.hpp plan_msm)
template <class Cv>
int HostCore<Cv>::run_msm_core(kzgmi_ctx* c, Slot& s, const TermList& tl_in, uint32_t nsets, size_t emax, const MsmWindows& mw,
                 const Affine<Cv>* pts, const uint8_t* inf, bool pts29, int wbits, int part) {
  // pts == nullptr: the slot's freshly converted points, put into the accumulation's format
  // here unless convert_points stored them in it already (pts29); explicit pts (commit-key
  // rows) are stored in that format already (kzgmi_ck_load)
  const bool own_pts = pts == nullptr && !pts29;
  const MsmTuning& t = c->tune;
  const MsmPlan p = plan_msm<Cv>(t, tl_in, nsets, emax, mw, wbits, part, own_pts, slot_alone(c, s), c->sync_call,
                                   c->async_call);
  CHK(ensure_msm(s, p));
  using XY = Xyzz<Cv>;
  using L = Launch<Cv>;
  if (!pts) pts = s.pts.template as<Affine<Cv>>();  // default: the slot's converted points
  if (!inf) inf = s.inf.template as<uint8_t>();
  if (p.small) return enqueue_small_msm<Cv>(c, s, p, pts, inf);
  const TermList& tl = p.tl;
  const uint32_t NB = p.NB, nbuckets = p.nbuckets;
  const size_t nchunks = p.nchunks, acc_threads = p.acc_threads;
  uint32_t* const coarse = s.coarse.template as<uint32_t>();
  uint32_t* const total = s.total.template as<uint32_t>();
  uint32_t* const sval = s.sval.template as<uint32_t>();
  uint32_t* const skey = s.skey.template as<uint32_t>();
  uint32_t* const cnt = s.cnt.template as<uint32_t>();
  uint32_t* const off = s.off.template as<uint32_t>();
  uint32_t* const acc = s.acc29.template as<uint32_t>();  // buckets and bucket pieces: radix-29 records (msm.hpp)
  uint32_t* const accq = acc_threads ? s.accq.template as<uint32_t>() : nullptr;
  uint32_t* const crowd = s.crowd.template as<uint32_t>();
  XY* const scratch = s.scratch.template as<XY>();
  XY* const winsum = s.winsum.template as<XY>();
  XY* const res = s.res.template as<XY>();
  if (p.split && !c->side_stream) {  // at the slot stream's priority, or the device's greatest
    int prio = 0, least = 0, greatest = 0;
    HIPCHK(hipStreamGetPriority(s.stream, &prio));
    if (t.split_side_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) prio = greatest;
    HIPCHK(hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, prio));
  }
  if (p.split && !s.side_ev[0])
    for (auto& e : s.side_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  Roctx rx("kzgmi.msm.sort+accumulate+reduce+combine");
  hipStream_t st = s.stream;
  L::pts_to29(st, s.pts.template as<Affine<Cv>>(), p.own_npts);
  // a range of parts 2 and 3 sorts and accumulates into the second store
  L::sort(st, tl, nsets, inf, s.digits.template as<uint32_t>(), coarse, s.ent.template as<uint64_t>(), emax,
          (t.sort_split ? L::SORT_SPLIT : 0) | (t.sort_full_bins ? L::SORT_FULL_BINS : 0),
          p.second ? s.offb.template as<uint32_t>() : off, p.second ? s.cntb.template as<uint32_t>() : cnt, total, sval, skey,
          wbits);
  // rows: the items of the sorted buckets, by length (in front of the ordering wait below: it runs
  // beside the earlier batches' accumulations, like the sort)
  if (p.rows)
    L::row_items(st, off, cnt, NB, p.row_len, s.rowq.template as<uint32_t>(), s.items.template as<uint32_t>(),
                 (uint32_t)p.row_items, s.cuts.template as<uint32_t>(), (uint32_t)p.row_cuts);
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
  if (p.split) {
    // Two launches A and B of the same grid, one per MSM: A's MSM reduces and combines on the
    // context's side stream while B accumulates on the slot's.
    // sets [split_set, nsets) are the sorted entries [coff[split_set * bins], total)
    const uint32_t* mid = coarse + (size_t)nsets * p.bins + (size_t)p.split_set * p.bins;
    const uint32_t h = p.split_set, hn = nsets - p.split_set;
    uint32_t* crowd_b = crowd + p.crowd_words;
    // launch A's pieces follow the buckets, launch B's follow A's: A's joins may run on the side
    // stream while B accumulates.  Order: MSM#0's sets [0, mid) first (split_rev 1, the default),
    // or MSM#1's [mid, total) first (0); the first launch's MSM finishes on the side stream.
    const bool rev = t.split_rev;
    const uint32_t* total_a = rev ? mid : total;
    const uint32_t* lo_a = rev ? nullptr : mid;
    const uint32_t* total_b = rev ? total : mid;
    const uint32_t* lo_b = rev ? mid : nullptr;
    const uint32_t nb_b = t.split_side_fix ? (uint32_t)(NB + 2 * nchunks) : NB;
    L::accumulate(st, nchunks, total_a, sval, skey, off, cnt, pts, acc, NB, acc_threads, accq, crowd, lo_a,
                  t.split_side_fix ? nullptr : st);
    hipStream_t sd = c->side_stream;
    HIPCHK(hipEventRecord(s.side_ev[0], st));
    HIPCHK(hipStreamWaitEvent(sd, s.side_ev[0], 0));
    L::accumulate(st, nchunks, total_b, sval, skey, off, cnt, pts, acc, nb_b, acc_threads, accq, crowd_b, lo_b, st);
    if (order_ev) HIPCHK(hipEventRecord(*order_ev, st));
    // MSM m's reduction and window combination on stream q: bucket records, R / U+V records, bit
    // sums and window sums at the offsets of its sets
    constexpr int W29 = kW29<Fp29Of<Cv>>;
    const size_t nseg = nbuckets / SEG;
    uint32_t* R29 = s.R.template as<uint32_t>();
    uint32_t* U29 = s.U.template as<uint32_t>();
    auto tail = [&](hipStream_t q, int m, bool lowp) {
      const uint32_t s0 = m ? h : 0, ns = m ? hn : h;
      L::reduce(q, ns, cnt + (size_t)s0 * nbuckets, acc + (size_t)s0 * nbuckets * W29,
                reinterpret_cast<XY*>(R29 + s0 * nseg * W29), reinterpret_cast<XY*>(U29 + 2 * s0 * nseg * W29),
                scratch + (size_t)s0 * p.rb_parts, winsum + s0, wbits, lowp, t.seg4_waves, 4 * t.ncu);
      if (q == st) mark(c, s, PH_REDUCE + 1);
      L::window_combine(q, MsmWindows{1, {s0, 0}, {mw.nwin[m], 0}}, winsum, res + m, wbits, lowp);
    };
    // side: (A's piece joins,) the first launch's MSM
    if (t.split_side_fix) L::fixup(sd, nchunks, total_a, skey, off, cnt, acc, NB, crowd, lo_a);
    tail(sd, rev ? 0 : 1, t.split_low_prio);
    HIPCHK(hipEventRecord(s.side_ev[1], sd));
    mark(c, s, PH_ACCUM + 1);
    tail(st, rev ? 1 : 0, false);
    HIPCHK(hipStreamWaitEvent(st, s.side_ev[1], 0));
    mark(c, s, PH_COMBINE + 1);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (p.second) {
    uint32_t* const accb = s.acc29b.template as<uint32_t>();
    uint32_t* const cntb = s.cntb.template as<uint32_t>();
    L::accumulate(st, nchunks, total, sval, skey, s.offb.template as<uint32_t>(), cntb, pts, accb, NB, acc_threads, accq,
                  crowd, nullptr, st);
    if (order_ev) HIPCHK(hipEventRecord(*order_ev, st));
    L::merge_buckets(st, NB, acc, cnt, accb, cntb);
  } else if (p.rows) {
    L::accumulate_rows(st, nchunks, sval, pts, acc, NB, s.rowq.template as<uint32_t>(), s.items.template as<uint32_t>(),
                       (uint32_t)p.row_items, s.cuts.template as<uint32_t>(), (uint32_t)p.row_cuts);
    if (order_ev) HIPCHK(hipEventRecord(*order_ev, st));
  } else {
    L::accumulate(st, nchunks, total, sval, skey, off, cnt, pts, acc, NB, acc_threads, accq, crowd, nullptr, st);
    if (order_ev) HIPCHK(hipEventRecord(*order_ev, st));
  }
  mark(c, s, PH_ACCUM + 1);
  if (part == 1 || part == 2) {
    HIPCHK(hipGetLastError());
    return 0;  // more ranges follow
  }
  L::reduce(st, nsets, cnt, acc, s.R.template as<XY>(), s.U.template as<XY>(), scratch, winsum, wbits, false,
            t.seg4_waves, 4 * t.ncu);
  mark(c, s, PH_REDUCE + 1);
  L::window_combine(st, mw, winsum, res, wbits);
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

// ------------------------------------------------------------------------------ batch
// What the flags make of a batch of n tuples: its randomisers, whether its MSMs take the GLV
// form, and where its points go
struct BatchShape {
  bool glv;
  // powers: r_i = r^i (255-bit, caller-supplied r).  Fiat-Shamir: r from the transcript, then
  // the seeded 127-bit randomisers with seed = r (so 32n MSM entries, as with a host seed).
  bool powers;
  // MSM#1's tail class: -t [1]_1, or for a cell batch (BLS12-381, powers + compressed + subgroup
  // check) the 64 terms -c_m [tau^m]_1
  uint32_t tail;
  // points: [pi (n) | C (n) | tail]; a cell batch keeps its m decoded unique commitments between
  // pi and the n gathered C, so that one subgroup check covers the n + m decoded points
  size_t m, CB, TB;  // first C, first tail point
  size_t PH;         // GLV: phi(pts[j]) at pts[PH + j]
  size_t npts;
  int wb;            // window width: H windows for 127-bit magnitudes, F for full scalars
  uint32_t H, F;     // (c = 16: 8 and 16; c = 13: 10 and 20)
};
template <class Cv>
static BatchShape batch_shape(const kzgmi_ctx* c, size_t n, uint32_t flags, const CellJob* cell) {
  BatchShape b{};
  b.glv = c->glv_batch && (Cv::ID == 1 || (flags & (KZGMI_FLAG_SUBGROUP_CHECK | KZGMI_FLAG_TRUSTED_G1)) != 0);
  b.powers = (flags & KZGMI_FLAG_POWERS) != 0;
  b.tail = cell ? CellLaunch::TERMS : 1;
  b.m = cell ? cell->m : 0;
  b.CB = n + b.m;
  b.TB = b.CB + n;
  b.PH = b.TB + b.tail;
  b.npts = b.glv ? 2 * b.PH : b.PH;
  b.wb = batch_wbits(c->tune, b.powers, n);
  b.H = windows_half(b.wb);
  b.F = windows_full(b.wb);
  return b;
}

// the front end's buffers; derived: a blob or cell batch, whose z_i, y_i and r are derived on the
// device (cell batch: z_k = h_k^64, y_k = 0, r and the 64 coefficients)
template <class Cv>
static int ensure_batch_front(Slot& s, const BatchShape& b, size_t n, bool derived, bool cell) {
  CHK(s.pts.ensure(b.npts * sizeof(Affine<Cv>)));
  CHK(s.inf.ensure(b.npts));
  if (b.glv) {
    CHK(s.glv_s.ensure(n * 32));
    CHK(s.glv_t.ensure((size_t)b.tail * 32));
    if (b.powers) CHK(s.glv_r.ensure(n * 32));
  }
  CHK(s.scal_r.ensure(n * (b.powers ? 32 : 16)));
  CHK(s.scal_s.ensure(n * 32));
  CHK(s.scal_t.ensure(32));
  CHK(s.tpart.ensure(Launch<Cv>::tpart_bytes((uint32_t)n)));
  CHK(s.flags.ensure(16));
  if (derived) {
    CHK(s.blob_z.ensure(n * 32));
    CHK(s.blob_y.ensure(n * 32));
    CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<typename Cv::FrP>)));
    CHK(s.chal.ensure(32));
    if (cell) {
      CHK(s.cell_part.ensure(CellLaunch::part_bytes()));
      CHK(s.cell_coef.ensure(CellLaunch::TERMS * 32));
    }
  }
  return 0;
}

static BatchScalars batch_scalars(const Slot& s) {
  return {s.scal_r.as<uint32_t>(), s.scal_s.as<uint32_t>(), s.scal_t.as<uint32_t>(), s.glv_r.as<uint32_t>(),
          s.glv_s.as<uint32_t>(), s.glv_t.as<uint32_t>(), s.cell_coef.as<uint32_t>()};
}

// kzgmi_ctx_reserve: a slot's workspace at the sizes of batches of up to n tuples in this mode
// (msm_plan.hpp plan_reserve); nothing is enqueued
template <class Cv>
int HostCore<Cv>::reserve_batch(kzgmi_ctx* c, Slot& s, size_t n, uint32_t flags) {
  const BatchShape b = batch_shape<Cv>(c, n, flags, nullptr);
  CHK(ensure_batch_front<Cv>(s, b, n, false, false));
  // the randomiser workspaces of this mode
  if (flags & KZGMI_FLAG_FIAT_SHAMIR) CHK(reserve_fs<Cv>(s, n));
  else if (b.powers) CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<typename Cv::FrP>)));
  const bool own_pts = (flags & (KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK)) != 0;  // (enqueue_batch pts29)
  return ensure_msm(s, plan_reserve<Cv>(c->tune, b.glv, b.powers, n, own_pts, batch_scalars(s)));
}

template <class Cv>
int HostCore<Cv>::enqueue_batch(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                  const void* dpi, size_t n, const Seed& seed, uint64_t offset, void* d_partial_out,
                  uint32_t flags, const void* d_blobs, const CellJob* cell) {
  using XY = Xyzz<Cv>;
  using FrF = Fp<typename Cv::FrP>;
  using L = Launch<Cv>;
  const BatchShape shape = batch_shape<Cv>(c, n, flags, cell);
  const bool glv = shape.glv, powers = shape.powers;
  const uint32_t tail = shape.tail;
  const size_t CB = shape.CB, TB = shape.TB, PH = shape.PH;
  CHK(ensure_batch_front<Cv>(s, shape, n, d_blobs || cell, cell != nullptr));
  if (d_blobs || cell) {
    dz = s.blob_z.p;
    dy = s.blob_y.p;
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
  CHK(front());
  const BatchTerms bt = batch_terms(glv, powers, cell ? tail : 0, shape.H, shape.F, n, shape.m, 0, n, true, batch_scalars(s));
  CHK(HostCore<Cv>::run_msm_core(c, s, bt.tl, bt.nsets, bt.emax, bt.mw, nullptr, nullptr, pts29, shape.wb));
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
  const BatchShape shape = batch_shape<Cv>(c, n, flags, nullptr);
  const bool glv = shape.glv;
  const int wb = shape.wb;
  const size_t gb = g1_bytes(Cv::ID);
  const size_t PH = shape.PH;  // = 2n + 1
  CHK(ensure_batch_front<Cv>(s, shape, n, false, false));
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
    return batch_terms(glv, false, 0, shape.H, shape.F, n, 0, lo, nj, last, batch_scalars(s));
  };
  size_t nmax = 0;
  for (size_t v : nk) nmax = std::max(nmax, v);
  // every workspace at its final size before the first launch (a later growth would free a buffer
  // an earlier range's kernels are still using): the plan of the largest range as a last one
  {
    const BatchTerms bt = terms(0, nmax, true);
    CHK(ensure_msm(s, plan_msm<Cv>(c->tune, bt.tl, bt.nsets, bt.emax, bt.mw, wb, 3, false, /*alone=*/true, c->sync_call)));
  }
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
    const BatchTerms bt = terms(lo, nj, last);
    CHK(HostCore<Cv>::run_msm_core(c, s, bt.tl, bt.nsets, bt.emax, bt.mw, nullptr, nullptr, true, wb, part));
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
  const int wb = call_wbits(c->tune, (size_t)16 * n, size_t(1) << 21);
  const uint32_t H = windows_half(wb), F = windows_full(wb);
  if (glv) {  // sum k_i P_i = sum h0_i P_i + h1_i phi(P_i): H windows, H bucket sets
    tl.c[0] = {nn, 0, 4, H, 0, 4, gs};
    tl.c[1] = {nn, nn, 4, H, 0, 4, gs + 4 * n};
    tl.nclass = 2;
    tl.total = 2 * nn;
    const MsmWindows mw{1, {0, 0}, {H, 0}};
    CHK(HostCore<Cv>::run_msm_core(c, s, tl, H, (size_t)2 * H * n + 16, mw, nullptr, nullptr, pts29, wb));
  } else {
    tl.c[0] = {nn, 0, 8, F, 0, 8, sc};
    tl.nclass = 1;
    tl.total = nn;
    const MsmWindows mw{1, {0, 0}, {F, 0}};
    CHK(HostCore<Cv>::run_msm_core(c, s, tl, F, (size_t)F * n + 16, mw, nullptr, nullptr, pts29, wb));
  }
  s.curve = Cv::ID;
  return 0;
}

template struct HostCore<Bls12_381>;
template struct HostCore<Bn254>;

}  // namespace kzgmi
