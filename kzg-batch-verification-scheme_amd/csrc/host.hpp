// kzgmi host layer: what every host unit (api.hip, host_*.hip) shares -- the context, slot and key
// structs, the error plumbing and the job layer (begin_job .. finish_slot, JobKind / arm, stage_host,
// ensure_once, slot0_utility_job, run_sync).  Declarations and small inline helpers only.  Everything
// with state (the last-error string, the routing depth, the allocation count, the pinned-range map,
// the copy pool) is defined exactly once, in api.hip, and only declared here.
#pragma once
#include "launch.hpp"
#include "msm_plan.hpp"
#include "kzgmi.h"

#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <algorithm>
#include <atomic>
#include <vector>

namespace kzgmi {

extern thread_local std::string g_err;  // kzgmi_last_error() of this host thread
int fail(int code, const std::string& msg);

#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return fail(KZGMI_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define CHK(x)                  \
  do {                          \
    int r_ = (x);               \
    if (r_ != 0) return r_;     \
  } while (0)

// process-wide count of workspace (re)allocations: kzgmi_alloc_count(), so a caller (bench.py,
// tests) can check that kzgmi_ctx_reserve left nothing to allocate inside a timed region
extern std::atomic<uint64_t> g_allocs;

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(KZGMI_ERR_OOM, "hipMalloc failed (" + std::to_string(bytes) + " bytes)");
    cap = bytes;
    g_allocs.fetch_add(1, std::memory_order_relaxed);
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// roctx range over a host-side scope (SURVEY.md 5 tracing): the enqueue of each batch phase and
// every blocking wait, visible in `rocprofv3 --marker-trace` beside the kernels they issue
struct Roctx {
  explicit Roctx(const char* m) { roctxRangePushA(m); }
  ~Roctx() { roctxRangePop(); }
  Roctx(const Roctx&) = delete;
  Roctx& operator=(const Roctx&) = delete;
};

// the batch phases in stream order, then "h2d": the host-to-HBM copy of a host-buffer call
// (kzgmi_batch_verify_ex_async), timed by its own pair of events
const char* const kPhaseNames = "convert,scalars,sort,accumulate,reduce,combine,pairing,h2d";
constexpr int kNumPhases = 8;
constexpr int kNumBatchPhases = 7;
enum Phase { PH_CONVERT = 0, PH_SCALARS, PH_SORT, PH_ACCUM, PH_REDUCE, PH_COMBINE, PH_PAIRING, PH_H2D };
constexpr int EV_H2D0 = kNumBatchPhases + 1, EV_H2D1 = kNumBatchPhases + 2;  // Slot::ev indices
constexpr size_t kRingBytes = size_t(16) << 20;  // pinned staging ring of pageable host inputs (x 2 per slot)

// What a slot's pending job leaves behind, which decides who may chain behind it and which wait
// collects it.  Verdict: host_flags[0] is the pairing's verdict (kzgmi_slot_wait reports it; every
// other kind reports ok = 1).  BatchPartial / MsmPartial: a partial record; a combine of the same
// family may chain behind it on the slot.  MsmResult: an encoded point in host_out (kzgmi_msm_wait
// takes only this kind).  Utility: a job that only reports through the slot's error word.
enum class JobKind { Verdict, BatchPartial, MsmPartial, MsmResult, Utility };

struct Slot {
  hipStream_t stream = nullptr;      // the slot's stream: every job on the slot is issued here
  hipEvent_t done_ev = nullptr;       // the slot's last job issued so far has completed
  bool done_rec = false;
  std::vector<hipEvent_t> dep_pool;   // entry dependencies of the slot's next job (kzgmi_stream_wait, the
  int ndep = 0;                        // H2D copy of host inputs): dep_pool[0, ndep)
  DevBuf pts, inf, scal_r, scal_s, scal_t, tpart, cnt, off, coarse, ent, total, sval, skey;
  DevBuf R, U, scratch, winsum, res, flags, stage, outb;
  DevBuf acc29;                                  // radix-29 bucket records (msm.hpp)
  DevBuf accq;                                   // k_accumulate's work-queue counter (large calls)
  DevBuf crowd;                                  // k_fixup's list of crowded buckets (msm.hpp k_fixup_crowded)
  DevBuf rowq, items, cuts;                      // row accumulation (msm.hpp): counters + histogram, item list, join list
  DevBuf fs_leaves, fs_tmp, fs_top, pow, chal;  // Fiat-Shamir / powers-of-r randomisers
  DevBuf blob_z, blob_y;                         // blob batches: the derived z_i, y_i (n x 32 B each);
                                                 // cell batches: z_k = h_k^64 and y_k = 0
  DevBuf cell_part, cell_coef;                   // cell batches: per-coset coefficients; -c_m (64 x 8 LE words)
  DevBuf cell_tab;                               // the search for invalid cells: c_m of every I_k (n x 64 x 8 LE words)
  DevBuf rec_z;                                  // recover_cells: the call's vanishing-polynomial table (recover.hpp)
  DevBuf fk_coef, fk_scal, fk_a, fk_b, fk_enc;   // cell proofs (fk20.hpp): coefficients, ahat, two point vectors, encodings
  DevBuf bp_q, bp_part, bp_enc;                  // blob proofs (blobproof.hpp): quotients, partial sums and results, encodings
  DevBuf open_zp, open_q, open_aux;              // openings (open.hpp): the points' powers, a group's quotients, run and tile values
  DevBuf open_y, open_rec, open_enc;             // ... the evaluations, the proofs as records, their encodings
  DevBuf ntt_tmp, ntt_call;                      // transforms (ntt.hpp): the ping-pong copy of the data, the call's shift table
  DevBuf g1_a, g1_b, g1_enc;                     // transforms over G1 (g1ntt.hpp): two record vectors, the encodings
  DevBuf oa_scal;                                // open_all: ahat (2n scalars) and the coefficients padded to n
  DevBuf glv_r, glv_s, glv_t;                    // GLV half scalars (glv.hpp): [h0 x n | h1 x n]
  DevBuf digits;                                 // signed window digit codes of every term (msm.hpp)
  DevBuf small_nodes, small_flags;               // small calls' summation tree (msm_small.hpp)
  DevBuf acc29b, cntb, offb;                     // second bucket store of chunked batches (run_msm_core part)
  // the search for invalid tuples (host_find.hip): a level's group table, -t_g, tree nodes and arrival
  // counters (msm_group.hpp), its record pairs and their verdicts
  DevBuf find_tab, find_negt, find_nodes, find_flags, find_rec, find_ok;
  // split accumulation (run_msm_core): the MSM of the first accumulation launch (MSM#0 by default,
  // MsmTuning::split_rev) reduces and combines on the context's one side stream beside the second
  // launch; side_ev[0] = the first launch's sets accumulated, [1] = its MSM combined
  hipEvent_t side_ev[2] = {};
  int* host_flags = nullptr;  // pinned, 4 words: [ok, err, the cell search's front-end error (host_find.hip)]
  uint8_t* host_out = nullptr;  // pinned: encoded MSM result of an async MSM job
  uint8_t* ring[2] = {};        // pinned staging of pageable host inputs (kRingBytes each, lazily)
  hipEvent_t ring_ev[2] = {};   // the DMA that last read ring[b]
  int ring_next = 0;
  hipEvent_t ev[kNumBatchPhases + 3] = {};  // phase marks 0..7, then the H2D pair
  hipEvent_t signal_ev = nullptr;  // kzgmi_slot_signal: this slot's stream -> the caller's stream
  bool ev_used[kNumBatchPhases + 3] = {};
  bool pending = false;
  JobKind kind = JobKind::Verdict;  // of the pending job (arm)
  int curve = 0;
  // every device buffer of the slot (kzgmi_ctx_destroy releases them all: a buffer added above
  // must be listed here)
  template <class F>
  void for_each_buf(F&& f) {
    DevBuf* bufs[] = {&pts, &inf, &scal_r, &scal_s, &scal_t, &tpart, &cnt, &off, &coarse, &ent, &total, &sval, &skey,
                      &R, &U, &scratch, &winsum, &res, &flags, &stage, &outb, &acc29, &accq, &crowd, &rowq, &items, &cuts, &fs_leaves,
                      &fs_tmp, &fs_top, &pow, &chal, &glv_r, &glv_s, &glv_t, &digits, &small_nodes, &small_flags,
                      &acc29b, &cntb, &offb, &blob_z, &blob_y, &cell_part, &cell_coef, &cell_tab, &rec_z,
                      &fk_coef, &fk_scal, &fk_a, &fk_b, &fk_enc, &bp_q, &bp_part, &bp_enc,
                      &open_zp, &open_q, &open_aux, &open_y, &open_rec, &open_enc, &ntt_tmp, &ntt_call, &g1_a, &g1_b, &g1_enc, &oa_scal,
                      &find_tab, &find_negt, &find_nodes, &find_flags, &find_rec, &find_ok};
    for (DevBuf* b : bufs) f(*b);
  }
};

}  // namespace kzgmi
using namespace kzgmi;

struct kzgmi_cell_srs;
struct kzgmi_cell_pk;
struct kzgmi_blob_pk;
struct kzgmi_open_all_key;
struct kzgmi_open_cosets_key;

struct kzgmi_ctx {
  int device = 0;
  std::vector<Slot> slots;
  int user_slots = 0;                   // slots in the caller's numbering (multi-device: over all devices)
  int prio_levels = 1;                  // stream priorities the slot streams cycle through
  bool profiling = false;
  // GLV split of full Fr scalars.  phi(P) = [lambda] P holds only on
  // G1, so BLS12-381 (cofactor > 1) uses it only for points known to be in G1: batch calls
  // with KZGMI_FLAG_SUBGROUP_CHECK or KZGMI_FLAG_TRUSTED_G1, MSMs after kzgmi_set_trusted_g1.
  // BN254 G1 is the whole curve (cofactor 1): always.
  bool glv_msm = true;      // enable knobs (kzgmi_set_glv; A/B measurements)
  bool glv_batch = true;
  bool msm_trusted_g1 = false;
  MsmTuning tune;  // what plan_msm decides an MSM call by (msm_plan.hpp): the device's CUs and the KZGMI_* knobs
  FindTuning find_tune;        // the search's fan-out, crossover and workspace bound (find_plan.hpp)
  uint64_t find_stats[4] = {};  // of the last search: levels, bucket jobs, grouped wave-terms, pairings
  int host_chunks_env = 0;       // KZGMI_HOST_CHUNKS: ranges of a synchronous host-buffer batch (batch_host_chunked)
  int host_chunk_mode = 0;       // KZGMI_HOST_CHUNK_MODE=1: shard partials even where one bucket store applies
  // set by the synchronous device-buffer call while it enqueues: only such calls split (the first
  // batch of a pipeline is alone when it is enqueued too, and split it cost the 20-step bench
  // ~1 ms: its two launches, then a gap while the next batch's front end ran)
  bool sync_call = false;
  // set by the asynchronous device-buffer batch call while it enqueues: only such calls (and not
  // the synchronous one, which enqueues through it) accumulate in rows (msm_plan.hpp MsmPlan::rows)
  bool async_call = false;
  // accumulation order: a slot's k_accumulate waits for the accumulation D launches before it
  // (any slot), so at most D run at once and they start in submission order.  Without it 16
  // slots in flight ran their accumulations in bursts and their tails (pairing: one CU) together,
  // with no accumulation beside them, and the oldest batch -- the one the caller waits on to
  // reuse its slot -- finished last (tools/trace_gaps.py).  D = acc_order for calls of at least
  // ACC_ORDER_WIDE entries, acc_order_small below (a 2^17 batch's accumulation does not fill
  // the chip): pipelined 2^20 batches 184.7 vs 183.5/s (BN254 361 vs 347), 2^17 batches 1074 vs
  // 1028/s with D = 4 (925 with 2) -- profiles/r05/ab_acc_order*.txt.  Only where every slot has
  // a hardware queue of its own: a stream waiting for the event holds up the other slots of its
  // queue (at the default 4 queues 2^20 batches ran 160 vs 173/s with the order).
  // KZGMI_ACC_ORDER, KZGMI_ACC_ORDER_SMALL (0: off; set: also on shared queues)
  static constexpr int kAccOrderMax = 8;
  static constexpr size_t ACC_ORDER_WIDE = size_t(1) << 23;
  int acc_order = 2, acc_order_small = 4;
  hipEvent_t acc_ring[kAccOrderMax] = {};  // launch i's event at i % kAccOrderMax
  uint64_t acc_launches = 0;
  double phase_ms[kNumPhases] = {};  // running sums since profiling was (re)enabled
  // host-buffer inputs of every slot are copied on ONE stream, in submission order: each
  // batch's copy then gets the whole link and completes first-in first-out (16 concurrent
  // 256-MiB copies on the slots' own streams shared the link and all finished late)
  hipStream_t h2d_stream = nullptr;  // created with the context
  // The split accumulation's side stream: ONE per context, created at the first split.  Splits run
  // only on calls with no other slot in flight, so one suffices -- and every extra stream takes a
  // hardware queue: a side stream per slot (17 + 16 queues) oversubscribed the device's queue
  // slots and the whole 16-slot pipeline ran 180 -> 120 batch-verifies/s (gpurun call r6f)
  hipStream_t side_stream = nullptr;
  int phase_calls = 0;
  DevBuf table[2], table_base[2];
  bool table_ready[2] = {false, false};
  DevBuf lines_tmp, tmp;
  // EIP-4844 blob front end (blob.hpp): the evaluation domain, built at the first blob call
  DevBuf blob_table;
  bool blob_table_ready = false;
  // KZGMI_BLOB_HASH=lane|wave forces the blob hash's mapping (A/B, tools/bench_blobs.py); 0: blob_mapping()
  int blob_hash = 0;
  // Openings (host_open.hip): the points of a call are taken in groups whose quotients hold at most this
  // many scalars (256 MiB), at least one point per group.  KZGMI_OPEN_GROUP (tests: groups at small sizes)
  size_t open_group = size_t(1) << 23;
  // EIP-7594 cell front end (cell.hpp): the coset table, built at the first cell call
  DevBuf cell_table;
  bool cell_table_ready = false;
  // EIP-7594 cell extension and recovery (recover.hpp): twiddles and scale factors, built at the first such call
  DevBuf ntt_table;
  bool ntt_table_ready = false;
  // Power-of-two transforms over Fr (ntt.hpp): each curve's root tables, built at its first transform.
  // ntt_pass_bits: the most bits of a pass, KZGMI_NTT_PASS_BITS (tests: plans of many passes at small
  // sizes); ntt_tile_bits: a workgroup's tile, KZGMI_NTT_TILE_BITS (A/B, tools/bench_ntt.py)
  DevBuf fr_ntt_table[2];
  bool fr_ntt_table_ready[2] = {false, false};
  uint32_t ntt_pass_bits = NTT_WIDEST_BITS, ntt_tile_bits = NTT_TILE_BITS;  // (a pass has at most ntt_tile_bits - 2 bits)
  // Transforms over G1 (g1ntt.hpp): the stage form, KZGMI_G1NTT_FORM=thread|wave forces one (tests, measurements)
  int g1ntt_form = G1NTT_FORM_AUTO;
  DevBuf gath;                       // multi-device: partial records gathered from every device
  DevBuf mdig, mdig_all;             // multi-device Fiat-Shamir: this device's / every device's subtree roots
  std::vector<kzgmi_ctx*> peers;     // multi-device: contexts of device_ids[1..] (kzgmi_ctx_create, n_devices > 1)
  std::vector<kzgmi_srs*> srs_list;  // live SRS objects: detached (device memory freed) on destroy
  std::vector<kzgmi_ck*> ck_list;    // live commit keys: same
  std::vector<kzgmi_cell_srs*> cell_srs_list;  // live cell SRS objects: same (their inner kzgmi_srs is in srs_list)
  std::vector<kzgmi_cell_pk*> cell_pk_list;    // live cell proof keys: same
  std::vector<kzgmi_blob_pk*> blob_pk_list;    // live blob proof keys: same
  std::vector<kzgmi_open_all_key*> open_all_key_list;  // live open_all keys (host_g1ntt.hip): same, through open_all_keys_detach
  std::vector<kzgmi_open_cosets_key*> open_cosets_key_list;  // live open_cosets keys (host_g1ntt.hip): same, by the same call
};

// prover commit key: rows w = 0..15 of 2^(16 w)-shifted SRS points, [row][point] Montgomery affine
struct kzgmi_ck {
  int curve = 0;
  size_t n = 0;
  kzgmi_ctx* ctx = nullptr;
  DevBuf pts, inf;
};
constexpr int CK_ROWS = 16;  // 16-bit windows of a 255-bit Fr scalar

struct kzgmi_srs {
  int curve = 0;
  kzgmi_ctx* ctx = nullptr;
  DevBuf lines, q, q_inf;
  DevBuf g1;                        // the SRS's [1]_1: Montgomery affine point + its infinity byte after it,
  size_t g1_29_off = 0;             // then the same point in the accumulation's radix-29 format
  void* g1_29() const { return static_cast<uint8_t*>(g1.p) + g1_29_off; }
  std::vector<kzgmi_srs*> peers;    // multi-device context: the same SRS on each peer device
};

// EIP-7594 cell SRS: an ordinary SRS for ([tau^0]_1, [1]_2, [tau^64]_2) and the 64 monomial points
struct kzgmi_cell_srs {
  kzgmi_ctx* ctx = nullptr;
  kzgmi_srs* srs = nullptr;
  DevBuf pts;                       // [tau^m]_1, m < 64, Montgomery affine, then their images phi([tau^m]_1) (GLV)
  DevBuf inf;                       // the 128 infinity bytes (all zero: checked at load)
  std::vector<kzgmi_cell_srs*> peers;  // multi-device context: the same SRS on each peer device
};

// EIP-7594 cell proof key (fk20.hpp): xhat, the transforms of the monomial SRS, as a table of window multiples
struct kzgmi_cell_pk {
  kzgmi_ctx* ctx = nullptr;
  DevBuf tab;                       // [base][window][multiple] Montgomery affine
  DevBuf tab_inf;                   // per base: xhat[base] is the point at infinity
};

// EIP-4844 blob proof key (blobproof.hpp): the 4096 Lagrange points as a table of window multiples
struct kzgmi_blob_pk {
  kzgmi_ctx* ctx = nullptr;
  DevBuf tab;                       // [base][window][multiple] Montgomery affine
  DevBuf tab_inf;                   // per base: the point at infinity (all zero: checked at load)
};

namespace kzgmi {

// an EIP-7594 cell batch for enqueue_batch: dC holds the m unique commitments, the device arrays
// commitment_indices / cell_indices (uint64 x n) and cells (n x 2048 B) come with it
struct CellJob {
  const kzgmi_cell_srs* srs;
  const void* cidx;
  const void* eidx;
  const void* cells;
  size_t m;
  bool derive;  // r from the transcript, on the device; else the caller's r is in the Seed
};

inline int set_dev(kzgmi_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  return 0;
}

// Start a job on slot s: its work goes on s.stream after the entry dependencies recorded since
// the slot's previous job (kzgmi_stream_wait, the H2D copy of host inputs).  Every entry point
// that issues work on a slot calls this first.
inline int begin_job(Slot& s) {
  for (int k = 0; k < s.ndep; ++k) HIPCHK(hipStreamWaitEvent(s.stream, s.dep_pool[k], 0));
  s.ndep = 0;
  return 0;
}

// The job's last operation is issued: done_ev marks its completion (kzgmi_slot_wait, the next
// job's begin_job, kzgmi_slot_signal)
inline int end_job(Slot& s) {
  HIPCHK(hipEventRecord(s.done_ev, s.stream));
  s.done_rec = true;
  return 0;
}

// Host wait for the slot's last job (an event, not a stream sync: an entry dependency recorded
// for the slot's next job must not be waited for here)
inline int sync_slot(Slot& s) {
  if (s.done_rec) HIPCHK(hipEventSynchronize(s.done_ev));
  return 0;
}
inline int sync_job(Slot& s) {
  CHK(end_job(s));
  return sync_slot(s);
}

// A new entry dependency of the slot's next job: work enqueued so far on `stream`
inline int add_dep(Slot& s, hipStream_t stream) {
  if (s.ndep == (int)s.dep_pool.size()) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s.dep_pool.push_back(e);
  }
  HIPCHK(hipEventRecord(s.dep_pool[s.ndep], stream));
  s.ndep += 1;
  return 0;
}

inline void mark(kzgmi_ctx* c, Slot& s, int idx) {
  if (!c->profiling) return;
  if (!s.ev[idx]) (void)hipEventCreate(&s.ev[idx]);
  (void)hipEventRecord(s.ev[idx], s.stream);
  s.ev_used[idx] = true;
}

constexpr uint32_t kAllFlags = KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK | KZGMI_FLAG_POWERS |
                               KZGMI_FLAG_FIAT_SHAMIR | KZGMI_FLAG_TRUSTED_G1;

// The blob hash's mapping (blob.hpp): a lane per blob at every n -- the wave-per-blob form lost
// at n = 6, 64 and 4096 alike (profiles/blob/bench_blobs.md), so there is no crossover to switch on
inline int blob_mapping(const kzgmi_ctx* c, size_t n) {
  (void)n;
  return c->blob_hash ? c->blob_hash : BlobLaunch::HASH_LANE;
}

template <class F>
int dispatch(int curve, F&& f) {
  if (curve == 0) return f(Bls12_381{});
  if (curve == 1) return f(Bn254{});
  return fail(KZGMI_ERR_ARG, "unknown curve");
}

inline size_t g1_bytes(int curve) { return curve == 0 ? 96 : 64; }
inline size_t g2_bytes(int curve) { return curve == 0 ? 192 : 128; }

inline int check_ctx(kzgmi_ctx* c, int slot = 0) {
  if (!c) return fail(KZGMI_ERR_ARG, "null context");
  if (slot < 0 || slot >= (int)c->slots.size()) return fail(KZGMI_ERR_ARG, "bad slot");
  return set_dev(c);
}

inline kzgmi_ctx* dev_ctx(kzgmi_ctx* c, int d) { return d == 0 ? c : c->peers[d - 1]; }

// Multi-device context (kzgmi_ctx_create with D > 1 devices): the caller's slot s runs on device
// s % D as that device's local slot s / D -- whole batches / MSMs per device, each device with
// its own lane pipeline; caller slot d < D is device d's local slot 0, which is also the
// device's shard slot of the synchronous strong split.  Only the outermost C-ABI call of a
// host thread translates (entry points calling each other pass local slots): t_route_depth.
extern thread_local int t_route_depth;
struct RouteGuard {
  RouteGuard() { ++t_route_depth; }
  ~RouteGuard() { --t_route_depth; }
  RouteGuard(const RouteGuard&) = delete;
  RouteGuard& operator=(const RouteGuard&) = delete;
};
int route_slot(kzgmi_ctx*& c, const kzgmi_srs** srs, int& slot);
#define KZ_ROUTE(c, srsp, slot) \
  RouteGuard route_guard_;       \
  CHK(route_slot(c, srsp, slot))

// synchronous entry points that run on slot 0 must not overwrite a pending async job's
// flags / result buffers (its later kzgmi_slot_wait would report theirs)
int slot0_idle(kzgmi_ctx* c);

Seed make_seed(const uint8_t* seed32, uint8_t (&buf)[32]);
int map_device_err(uint32_t e);
void collect_phases(kzgmi_ctx* c, Slot& s);
int finish_slot(kzgmi_ctx* c, Slot& s, int* ok_out);

// The slot's job is issued: pending until a wait collects it
inline void arm(Slot& s, JobKind kind, int curve) {
  s.pending = true;
  s.kind = kind;
  s.curve = curve;
}
// The "accepts, nothing enqueued" form of a job (curve < 0: the slot keeps its curve)
inline int arm_empty(Slot& s, JobKind kind, int curve = -1) {
  CHK(sync_slot(s));  // host_flags may still be the target of a copy
  s.host_flags[0] = 1;
  s.host_flags[1] = 0;
  arm(s, kind, curve < 0 ? s.curve : curve);
  return 0;
}

// A device table built once per context: launch() fills buf on st, which is waited for
template <class F>
int ensure_once(bool& ready, DevBuf& buf, size_t bytes, hipStream_t st, F&& launch) {
  if (ready) return 0;
  CHK(buf.ensure(bytes));
  launch();
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  ready = true;
  return 0;
}

// the cell coset table of this context's device (cell.hpp), built at the first call that reads it
inline int ensure_cell_table(kzgmi_ctx* c, hipStream_t st) {
  return ensure_once(c->cell_table_ready, c->cell_table, CellLaunch::table_bytes(), st,
                     [&] { CellLaunch::table(st, c->cell_table.p); });
}
// a live cell SRS of this context (an SRS of another kind, or of another context, is not in the list)
inline bool is_cell_srs(const kzgmi_ctx* c, const kzgmi_cell_srs* cs) {
  return cs && std::find(c->cell_srs_list.begin(), c->cell_srs_list.end(), cs) != c->cell_srs_list.end();
}

// A synchronous utility job on slot s whose kernels report through the slot's error word:
// launch(s, err) enqueues them
template <class F>
int utility_job(kzgmi_ctx* c, Slot& s, F&& launch) {
  CHK(begin_job(s));
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
  CHK(launch(s, s.flags.template as<uint32_t>() + 1));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
  CHK(end_job(s));
  arm(s, JobKind::Utility, s.curve);
  return finish_slot(c, s, nullptr);
}
// ... on slot 0 (idle on every device), after prepare(s) has built the tables it reads
template <class P, class F>
int slot0_utility_job(kzgmi_ctx* c, P&& prepare, F&& launch) {
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  CHK(s.flags.ensure(16));
  CHK(prepare(s));
  return utility_job(c, s, launch);
}

// A synchronous device-buffer verify: enqueue() issues the job on slot 0 with sync_call set (only
// such calls split their accumulation, kzgmi_ctx::sync_call), then the slot is waited for
template <class F>
int run_sync(kzgmi_ctx* c, F&& enqueue, int* ok_out) {
  if (!c) return fail(KZGMI_ERR_ARG, "null context");
  if (!ok_out) return fail(KZGMI_ERR_ARG, "null ok_out");
  {
    struct Guard {
      kzgmi_ctx* c;
      explicit Guard(kzgmi_ctx* c_) : c(c_) { c->sync_call = true; }
      ~Guard() { c->sync_call = false; }
    } guard(c);
    CHK(enqueue());
  }
  return kzgmi_slot_wait(c, 0, ok_out);
}

// a challenge's 8 big-endian words (as the device leaves them in Slot::chal) -> its 32 bytes
inline void words_be(const uint32_t (&w)[8], uint8_t* out32) {
  for (int k = 0; k < 8; ++k)
    for (int b = 0; b < 4; ++b) out32[4 * k + b] = (uint8_t)(w[k] >> (24 - 8 * b));
}

int h2d(Slot& s, hipStream_t cs, void* dst, const void* src, size_t bytes);

// Host arrays into the slot's stage buffer: region i takes items[i].bytes rounded up to 16, in
// order from the buffer's start, and dev[i] is its device address.  The regions with a source are
// copied on the context's FIFO copy stream after the slot's previous job (the stage buffer is then
// free), and the slot's next job waits for the copy only; a region without one is output or slack.
// profile: the copy is timed as the h2d phase.
struct StageItem {
  const void* src;
  size_t bytes;
};
int stage_host(kzgmi_ctx* c, Slot& s, const StageItem* items, int count, uint8_t** dev, bool profile = false);

// ---- host_core.hip: the enqueue functions every feature shares, instantiated there for both curves
template <class Cv>
struct HostCore {
  static int run_msm_core(kzgmi_ctx* c, Slot& s, const TermList& tl_in, uint32_t nsets, size_t emax,
                          const MsmWindows& mw, const Affine<Cv>* pts = nullptr, const uint8_t* inf = nullptr,
                          bool pts29 = false, int wbits = WBITS, int part = 0);
  static int enqueue_fs_digests(Slot& s, const void* dC, const void* dpi, const void* dz, const void* dy, size_t n,
                                uint64_t offset, bool compressed, const uint32_t** digests_out);
  static int enqueue_fs_challenge(Slot& s, const uint32_t* digests, uint32_t nch, uint64_t n_total);
  static int enqueue_batch(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                           const void* dpi, size_t n, const Seed& seed, uint64_t offset, void* d_partial_out,
                           uint32_t flags, const void* d_blobs = nullptr, const CellJob* cell = nullptr);
  static int reserve_batch(kzgmi_ctx* c, Slot& s, size_t n, uint32_t flags);
  static int enqueue_batch_chunked(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, const uint8_t* hC, const uint8_t* hz,
                                   const uint8_t* hy, const uint8_t* hpi, size_t n, const Seed& seed, uint32_t flags,
                                   int k);
  static int enqueue_msm(kzgmi_ctx* c, Slot& s, const void* dpts, const void* dsc, size_t n, bool allow_glv = true);
};
extern template struct HostCore<Bls12_381>;
extern template struct HostCore<Bn254>;

// ---- host_ntt.hip: the transforms over Fr, instantiated there for both curves
template <class Cv>
struct HostNtt {
  // The passes of count transforms of 2^logn on s.stream, inside the caller's job (behind begin_job and
  // the zeroed error word `err`): d_in -> d_out (the same array, or disjoint ones), either side big-endian
  // bytes or 8 canonical little-endian words.  flags and the shift (nullptr: 1) are checked by the caller
  // (ntt_check_args).  Grows the slot's scratch and builds the curve's tables at their first use.
  static int enqueue(kzgmi_ctx* c, Slot& s, const void* d_in, unsigned logn, size_t count, uint32_t flags, const Seed* shift,
                     bool read_be, bool write_be, void* d_out, uint32_t* err);
};
extern template struct HostNtt<Bls12_381>;
extern template struct HostNtt<Bn254>;
// logn, count, flags and shift32 of a transform call (shift_out / has_shift: s for HostNtt::enqueue)
int ntt_check_args(int curve, unsigned logn, size_t count, uint32_t flags, const uint8_t* shift32, Seed* shift_out,
                   bool* has_shift);

// ---- host_g1ntt.hip: kzgmi_ctx_destroy's detach of the context's live open_all and open_cosets keys (device
// memory freed; a later kzgmi_open_all_key_free or kzgmi_open_cosets_key_free only deletes the struct)
void open_all_keys_detach(kzgmi_ctx* c);

// ---- host_batch.hip: the chunk digests of kzgmi_fs_chunk_digests_device, enqueued on slot 0's stream (no wait)
int fs_chunk_digests_enqueue(kzgmi_ctx* c, kzgmi_curve curve, const void* dC, const void* dz, const void* dy,
                             const void* dpi, size_t n, uint64_t index_offset, uint32_t flags, void* d_out);

// ---- host_multi.hip: the synchronous host-buffer calls of a device-list context
std::vector<size_t> split_units(size_t n, int D);  // balanced ranges in units of 4096 tuples
int batch_multi_host(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* commitments, const uint8_t* zs,
                     const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t* seed32, uint32_t flags,
                     int* ok_out);
int msm_multi_host(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* points, const uint8_t* scalars, size_t n,
                   uint8_t* out);

}  // namespace kzgmi
