// kzgmi host orchestration + C-ABI (layers L3/L4 of SURVEY.md section 1), first of the host units
// that together implement include/kzgmi.h (host.hpp; the features are in host_*.hip).
//
// This unit: the definitions of the shared state and of the job layer's out-of-line parts, the
// context lifecycle, SRS load, settings and diagnostics, pinned host memory.  Device memory lives
// in per-slot workspaces owned by the context and is grown on demand (never inside a timed steady
// state).  Every compute path is HIP-only: without a device the calls fail with KZGMI_ERR_DEVICE
// (no CPU fallback).
// Reference: none (LICENSE only); boundary contract = SURVEY.md 8b, BASELINE.json:5.
#include "host.hpp"
#include "copy_pool.hpp"

#include <sys/random.h>
#include <map>
#include <mutex>
#define KZ_STR2(x) #x
#define KZ_STR(x) KZ_STR2(x)

namespace kzgmi {

// the shared state of the host units: defined here and nowhere else (host.hpp declares it)
thread_local std::string g_err = "";
thread_local int t_route_depth = 0;
std::atomic<uint64_t> g_allocs{0};

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

void collect_phases(kzgmi_ctx* c, Slot& s) {
  if (!c->profiling) return;
  // phase k spans from the latest earlier recorded mark to mark k+1
  for (int k = 0; k < kNumBatchPhases; ++k) {
    if (!s.ev_used[k + 1]) continue;
    int j = k;
    while (j >= 0 && !s.ev_used[j]) --j;
    if (j < 0) continue;
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.ev[j], s.ev[k + 1]) == hipSuccess) c->phase_ms[k] += ms;
  }
  if (s.ev_used[EV_H2D0] && s.ev_used[EV_H2D1]) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.ev[EV_H2D0], s.ev[EV_H2D1]) == hipSuccess) c->phase_ms[PH_H2D] += ms;
  }
  c->phase_calls += 1;
  for (bool& u : s.ev_used) u = false;
}

Seed make_seed(const uint8_t* seed32, uint8_t (&buf)[32]) {
  if (seed32) {
    memcpy(buf, seed32, 32);
  } else {
    size_t got = 0;
    while (got < 32) {
      ssize_t r = getrandom(buf + got, 32 - got, 0);
      if (r > 0) got += (size_t)r;
    }
  }
  Seed s;
  for (int k = 0; k < 8; ++k)
    s.w[k] = (uint32_t)buf[4 * k] << 24 | (uint32_t)buf[4 * k + 1] << 16 | (uint32_t)buf[4 * k + 2] << 8 | buf[4 * k + 3];
  return s;
}

int map_device_err(uint32_t e) {
  switch (e) {
    case DERR_NONE: return 0;
    case DERR_ENCODING: return fail(KZGMI_ERR_ENCODING, "invalid point encoding");
    case DERR_NOT_ON_CURVE: return fail(KZGMI_ERR_NOT_ON_CURVE, "point not on curve");
    case DERR_SCALAR: return fail(KZGMI_ERR_SCALAR, "non-canonical scalar (>= r)");
    case DERR_NOT_IN_SUBGROUP: return fail(KZGMI_ERR_NOT_IN_SUBGROUP, "point not in the order-r subgroup");
    case DERR_ARG: return fail(KZGMI_ERR_ARG, "an index read on the device is out of range (cell_index >= 128 or commitment_index >= m) or repeated, or the cells given to recover_cells are inconsistent");
    case DERR_SHARD: return fail(KZGMI_ERR_SHARD, "a gathered partial record is marked failed (its shard was rejected)");
    default: return fail(KZGMI_ERR_DEVICE, "unknown device error");
  }
}

int finish_slot(kzgmi_ctx* c, Slot& s, int* ok_out) {
  {
    Roctx rx("kzgmi.slot_wait");
    CHK(sync_slot(s));
  }
  s.pending = false;
  collect_phases(c, s);
  int e = map_device_err((uint32_t)s.host_flags[1]);
  if (e) return e;
  if (ok_out) *ok_out = s.kind == JobKind::Verdict ? s.host_flags[0] : 1;
  return 0;
}

int route_slot(kzgmi_ctx*& c, const kzgmi_srs** srs, int& slot) {
  if (t_route_depth != 1 || !c || c->peers.empty()) return 0;
  const int D = 1 + (int)c->peers.size();
  if (slot < 0 || slot >= c->user_slots) return fail(KZGMI_ERR_ARG, "bad slot");
  const int d = slot % D;
  if (srs && *srs) {
    if ((*srs)->ctx != c || (*srs)->peers.size() != c->peers.size())
      return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
    if (d > 0) *srs = (*srs)->peers[d - 1];
  }
  c = dev_ctx(c, d);
  slot /= D;
  return 0;
}

// synchronous entry points that run on slot 0 must not overwrite a pending async job's
// flags / result buffers (its later kzgmi_slot_wait would report theirs)
int slot0_idle(kzgmi_ctx* c) {
  if (c->slots[0].pending)
    return fail(KZGMI_ERR_ARG, "slot 0 busy: complete its pending job (kzgmi_slot_wait / kzgmi_msm_wait) first");
  for (size_t d = 0; d < c->peers.size(); ++d)  // multi-device: the shard slots (caller slots 1..D-1)
    if (c->peers[d]->slots[0].pending)
      return fail(KZGMI_ERR_ARG, "slot " + std::to_string(d + 1) + " busy: a synchronous multi-device call uses "
                                 "every device's first slot");
  return 0;
}

}  // namespace kzgmi

namespace {

// ---------------------------------------------------------------- host buffers (PCIe path)
// Pinned host ranges the library may DMA from directly: kzgmi_host_alloc blocks and
// kzgmi_host_register'ed ranges, keyed by start address.
struct HostRange {
  uintptr_t hi;
  bool owned;  // kzgmi_host_alloc (hipHostFree) vs kzgmi_host_register (hipHostUnregister)
};
std::mutex g_host_mu;
std::map<uintptr_t, HostRange> g_host;

bool host_pinned(const void* p, size_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  std::lock_guard<std::mutex> lk(g_host_mu);
  auto it = g_host.upper_bound(a);
  if (it == g_host.begin()) return false;
  --it;
  return a >= it->first && a + bytes <= it->second.hi;
}

// The staging copy's pool (copy_pool.hpp): KZGMI_COPY_THREADS threads, the caller included
// (default 8), fixed at the first staged copy of the process.
kzgmi::CopyPool* copy_pool() {
  static kzgmi::CopyPool* p = [] {  // never destroyed: its workers are detached
    const char* e = getenv("KZGMI_COPY_THREADS");
    return new kzgmi::CopyPool(e ? std::max(1, atoi(e)) : 8);
  }();
  return p;
}
}  // namespace

namespace kzgmi {

// enqueue host -> device on the copy stream cs: pinned ranges by DMA directly (asynchronous);
// pageable ones through the slot's two pinned ring buffers, the host copy of chunk k+1
// overlapping the DMA of chunk k (the call returns when the last chunk is staged)
int h2d(Slot& s, hipStream_t cs, void* dst, const void* src, size_t bytes) {
  if (!bytes) return 0;
  if (host_pinned(src, bytes)) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs));
    return 0;
  }
  for (int b = 0; b < 2; ++b) {
    if (!s.ring[b]) {
      if (hipHostMalloc((void**)&s.ring[b], kRingBytes, hipHostMallocDefault) != hipSuccess) {
        s.ring[b] = nullptr;
        return fail(KZGMI_ERR_OOM, "pinned staging allocation failed");
      }
      g_allocs.fetch_add(1, std::memory_order_relaxed);
    }
    if (!s.ring_ev[b]) {
      HIPCHK(hipEventCreateWithFlags(&s.ring_ev[b], hipEventDisableTiming));
      HIPCHK(hipEventRecord(s.ring_ev[b], cs));  // so the first wait on it has a record
    }
  }
  for (size_t off = 0; off < bytes; off += kRingBytes) {
    const size_t len = std::min(kRingBytes, bytes - off);
    const int b = s.ring_next;
    s.ring_next ^= 1;
    HIPCHK(hipEventSynchronize(s.ring_ev[b]));  // its previous DMA has read it
    copy_pool()->copy(s.ring[b], (const uint8_t*)src + off, len);
    HIPCHK(hipMemcpyAsync((uint8_t*)dst + off, s.ring[b], len, hipMemcpyHostToDevice, cs));
    HIPCHK(hipEventRecord(s.ring_ev[b], cs));
  }
  return 0;
}

int stage_host(kzgmi_ctx* c, Slot& s, const StageItem* items, int count, uint8_t** dev, bool profile) {
  size_t total = 0;
  for (int i = 0; i < count; ++i) total += (items[i].bytes + 15) / 16 * 16;
  CHK(s.stage.ensure(total));
  uint8_t* at = s.stage.template as<uint8_t>();
  for (int i = 0; i < count; ++i) {
    dev[i] = at;
    at += (items[i].bytes + 15) / 16 * 16;
  }
  hipStream_t cs = c->h2d_stream;
  // the copy overwrites s.stage: after the slot's previous job
  if (s.done_rec) HIPCHK(hipStreamWaitEvent(cs, s.done_ev, 0));
  profile = profile && c->profiling;
  if (profile) {
    if (!s.ev[EV_H2D0]) HIPCHK(hipEventCreate(&s.ev[EV_H2D0]));
    if (!s.ev[EV_H2D1]) HIPCHK(hipEventCreate(&s.ev[EV_H2D1]));
    HIPCHK(hipEventRecord(s.ev[EV_H2D0], cs));
  }
  for (int i = 0; i < count; ++i)
    if (items[i].src) CHK(h2d(s, cs, dev[i], items[i].src, items[i].bytes));
  if (profile) HIPCHK(hipEventRecord(s.ev[EV_H2D1], cs));
  return add_dep(s, cs);  // the job's kernels wait for its copy only
}

}  // namespace kzgmi

// ================================================================================ C ABI
extern "C" {

const char* kzgmi_version(void) { return "kzgmi 0.6 (abi " KZ_STR(KZGMI_ABI_VERSION) ", gfx950, HIP)"; }
int kzgmi_abi_version(void) { return KZGMI_ABI_VERSION; }
uint64_t kzgmi_alloc_count(void) { return g_allocs.load(std::memory_order_relaxed); }
const char* kzgmi_last_error(void) { return g_err.c_str(); }
const char* kzgmi_phase_names(void) { return kPhaseNames; }

int kzgmi_ctx_create_device(kzgmi_ctx** out, int device_id, int pipeline_slots) {
  if (!out || device_id < 0 || pipeline_slots < 1 || pipeline_slots > 64) return fail(KZGMI_ERR_ARG, "bad ctx args");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id)
    return fail(KZGMI_ERR_DEVICE, "no HIP device " + std::to_string(device_id) + " (found " + std::to_string(ndev) + ")");
  HIPCHK(hipSetDevice(device_id));
  kzgmi_ctx* c = new kzgmi_ctx();
  c->device = device_id;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && ncu > 0)
    c->tune.ncu = ncu;
  if (const char* e = getenv("KZGMI_ACC_THREADS")) c->tune.acc_threads_env = (size_t)strtoull(e, nullptr, 10);
  if (const char* e = getenv("KZGMI_ACC_QUEUE")) c->tune.acc_queue = atoi(e);
  if (const char* e = getenv("KZGMI_ACC_QUEUE_MIN")) c->tune.acc_queue_min = std::max<size_t>(4, strtoull(e, nullptr, 10));
  if (const char* e = getenv("KZGMI_ACC_QUEUE_FROM")) c->tune.acc_queue_from = strtoull(e, nullptr, 10);
  if (const char* e = getenv("KZGMI_SORT_SPLIT")) c->tune.sort_split = atoi(e) != 0;
  if (const char* e = getenv("KZGMI_SORT_FULL_BINS")) c->tune.sort_full_bins = atoi(e) != 0;
  if (const char* e = getenv("KZGMI_WBITS")) c->tune.wbits_env = atoi(e);
  if (const char* e = getenv("KZGMI_SMALL_TERMS")) c->tune.small_terms = (uint32_t)strtoul(e, nullptr, 10);
  if (const char* e = getenv("KZGMI_HOST_CHUNKS")) c->host_chunks_env = std::max(1, atoi(e));
  if (const char* e = getenv("KZGMI_HOST_CHUNK_MODE")) c->host_chunk_mode = atoi(e);
  if (const char* e = getenv("KZGMI_SPLIT_ACC")) c->tune.split_acc = atoi(e) < 0 ? -1 : std::min(1, atoi(e));
  if (const char* e = getenv("KZGMI_ACC_ROWS")) c->tune.acc_rows = atoi(e) < 0 ? -1 : std::min(1, atoi(e));
  if (const char* e = getenv("KZGMI_SPLIT_LOWPRIO")) c->tune.split_low_prio = atoi(e) != 0;
  if (const char* e = getenv("KZGMI_SEG4_WAVES")) c->tune.seg4_waves = std::max(0, atoi(e));
  if (const char* e = getenv("KZGMI_SPLIT_SIDEFIX")) c->tune.split_side_fix = atoi(e) != 0;
  if (const char* e = getenv("KZGMI_SPLIT_SIDEPRIO")) c->tune.split_side_prio = atoi(e) != 0;
  if (const char* e = getenv("KZGMI_SPLIT_REV")) c->tune.split_rev = atoi(e) != 0;
  if (const char* e = getenv("KZGMI_BLOB_HASH"))
    c->blob_hash = !strcmp(e, "lane") ? BlobLaunch::HASH_LANE : !strcmp(e, "wave") ? BlobLaunch::HASH_WAVE : 0;
  if (const char* e = getenv("KZGMI_OPEN_GROUP")) c->open_group = std::max<size_t>(1, strtoull(e, nullptr, 10));
  if (const char* e = getenv("KZGMI_NTT_TILE_BITS"))
    c->ntt_tile_bits = std::min<uint32_t>(std::max<uint32_t>(NTT_MIN_TILE_BITS, (uint32_t)atoi(e)), NTT_MAX_TILE_BITS);
  if (const char* e = getenv("KZGMI_G1NTT_FORM"))
    c->g1ntt_form = !strcmp(e, "thread") ? G1NTT_FORM_THREAD : !strcmp(e, "wave") ? G1NTT_FORM_WAVE : G1NTT_FORM_AUTO;
  if (const char* e = getenv("KZGMI_NTT_PASS_BITS"))
    c->ntt_pass_bits = std::min<uint32_t>(std::max<uint32_t>(NTT_MIN_PASS_BITS, (uint32_t)atoi(e)), NTT_WIDEST_BITS);
  // HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless set before the runtime
  // starts) and serialises the streams of one queue, so every slot in flight needs a queue of its
  // own (16 slots on 24 queues pipeline; 24 on 24 ran 3.6x slower).  The runtime keeps that many
  // queues PER STREAM PRIORITY: when the slots (+ the copy stream) outnumber the queues, the slot
  // streams cycle through the device's priority levels, which multiplies the queues they get --
  // at the default 4 queues, 2^20 batches run 173 vs 161/s (0.96 of the 179.5/s on 24 queues)
  // and 2^17 batches 814 vs 577/s (profiles/r05/ab_stream_prio*.txt).  KZGMI_STREAM_PRIO=0/1
  // forces it off / on.
  const char* qenv = getenv("GPU_MAX_HW_QUEUES");
  const int queues = qenv ? std::max(1, atoi(qenv)) : 4;
  int prio_least = 0, prio_greatest = 0;
  bool spread = pipeline_slots + 1 > queues;
  if (const char* e = getenv("KZGMI_STREAM_PRIO")) spread = atoi(e) != 0;
  spread = spread && hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess &&
           prio_least != prio_greatest;
  c->prio_levels = spread ? std::abs(prio_least - prio_greatest) + 1 : 1;
  {
    static std::atomic<bool> warned{false};
    if (pipeline_slots > 1 && pipeline_slots + 1 > queues * c->prio_levels && !getenv("KZGMI_QUIET") &&
        !warned.exchange(true))
      fprintf(stderr, "kzgmi: %d pipeline slots on %d hardware queues (GPU_MAX_HW_QUEUES x %d stream priorities): "
                      "slots sharing a queue run one after another\n",
              pipeline_slots, queues * c->prio_levels, c->prio_levels);
  }
  if (pipeline_slots + 1 > queues * c->prio_levels) c->acc_order = c->acc_order_small = 0;  // shared queues
  if (const char* e = getenv("KZGMI_ACC_ORDER")) c->acc_order = std::min(std::max(0, atoi(e)), kzgmi_ctx::kAccOrderMax);
  if (const char* e = getenv("KZGMI_ACC_ORDER_SMALL"))
    c->acc_order_small = std::min(std::max(0, atoi(e)), kzgmi_ctx::kAccOrderMax);
  bool okc = hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking) == hipSuccess;
  c->slots.resize(pipeline_slots);
  c->user_slots = pipeline_slots;
  for (size_t k = 0; k < c->slots.size() && okc; ++k) {
    Slot& s = c->slots[k];
    const int step = prio_least > prio_greatest ? 1 : -1;  // from the greatest priority towards the least
    okc = (spread ? hipStreamCreateWithPriority(&s.stream, hipStreamNonBlocking,
                                                prio_greatest + step * (int)(k % c->prio_levels))
                  : hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) == hipSuccess;
    okc = okc && hipEventCreateWithFlags(&s.done_ev, hipEventDisableTiming) == hipSuccess &&
          hipEventCreateWithFlags(&s.signal_ev, hipEventDisableTiming) == hipSuccess &&
          hipHostMalloc((void**)&s.host_flags, 16, hipHostMallocDefault) == hipSuccess &&
          hipHostMalloc((void**)&s.host_out, 128, hipHostMallocDefault) == hipSuccess;
  }
  if (!okc) {
    kzgmi_ctx_destroy(c);
    return fail(KZGMI_ERR_DEVICE, "stream/event/pinned allocation failed");
  }
  *out = c;
  return 0;
}

void kzgmi_ctx_destroy(kzgmi_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->side_stream) {  // its kernels read slot buffers: drained before any is released
    (void)hipStreamSynchronize(c->side_stream);
    (void)hipStreamDestroy(c->side_stream);
  }
  for (auto& s : c->slots) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    s.for_each_buf([](DevBuf& b) { b.release(); });
    for (auto& e : s.ev)
      if (e) (void)hipEventDestroy(e);
    if (s.signal_ev) (void)hipEventDestroy(s.signal_ev);
    if (s.done_ev) (void)hipEventDestroy(s.done_ev);
    for (auto& e : s.dep_pool) (void)hipEventDestroy(e);
    for (int b = 0; b < 2; ++b) {
      if (s.ring_ev[b]) (void)hipEventDestroy(s.ring_ev[b]);
      if (s.ring[b]) (void)hipHostFree(s.ring[b]);
    }
    for (auto& e : s.side_ev)
      if (e) (void)hipEventDestroy(e);
    if (s.host_flags) (void)hipHostFree(s.host_flags);
    if (s.host_out) (void)hipHostFree(s.host_out);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  for (hipEvent_t e : c->acc_ring)
    if (e) (void)hipEventDestroy(e);
  for (int k = 0; k < 2; ++k) { c->table[k].release(); c->table_base[k].release(); }
  if (c->h2d_stream) {
    (void)hipStreamSynchronize(c->h2d_stream);
    (void)hipStreamDestroy(c->h2d_stream);
  }

  c->lines_tmp.release();
  c->tmp.release();
  c->blob_table.release();
  c->cell_table.release();
  c->ntt_table.release();
  for (DevBuf& b : c->fr_ntt_table) b.release();
  for (kzgmi_cell_srs* cs : c->cell_srs_list) {  // detach: later kzgmi_cell_srs_free() only deletes the structs
    cs->pts.release();
    cs->inf.release();
    cs->ctx = nullptr;
  }
  for (kzgmi_cell_pk* pk : c->cell_pk_list) {  // detach: later kzgmi_cell_pk_free() only deletes the struct
    pk->tab.release();
    pk->tab_inf.release();
    pk->ctx = nullptr;
  }
  for (kzgmi_blob_pk* pk : c->blob_pk_list) {  // detach: later kzgmi_blob_pk_free() only deletes the struct
    pk->tab.release();
    pk->tab_inf.release();
    pk->ctx = nullptr;
  }
  open_all_keys_detach(c);
  for (kzgmi_ck* ck : c->ck_list) {  // detach: later kzgmi_ck_free() only deletes the struct
    ck->pts.release();
    ck->inf.release();
    ck->ctx = nullptr;
  }
  for (kzgmi_srs* srs : c->srs_list) {  // detach: later kzgmi_srs_free() only deletes the struct
    srs->lines.release();
    srs->q.release();
    srs->q_inf.release();
    srs->g1.release();
    srs->ctx = nullptr;
  }
  c->gath.release();
  c->mdig.release();
  c->mdig_all.release();
  std::vector<kzgmi_ctx*> peers;
  peers.swap(c->peers);
  delete c;
  for (kzgmi_ctx* p : peers) kzgmi_ctx_destroy(p);
}

int kzgmi_ctx_reserve(kzgmi_ctx* c, kzgmi_curve curve, size_t n, uint32_t flags) {
  CHK(check_ctx(c));
  if (flags & ~kAllFlags) return fail(KZGMI_ERR_ARG, "unknown flags");
  if ((flags & KZGMI_FLAG_POWERS) && (flags & KZGMI_FLAG_FIAT_SHAMIR))
    return fail(KZGMI_ERR_ARG, "KZGMI_FLAG_POWERS and KZGMI_FLAG_FIAT_SHAMIR are exclusive");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "batch too large (max 2^26 tuples per call)");
  for (auto& s : c->slots)
    if (s.pending) return fail(KZGMI_ERR_ARG, "kzgmi_ctx_reserve with jobs in flight");
  for (auto& s : c->slots) {
    if (n) CHK(dispatch(curve, [&](auto cv) -> int { return HostCore<decltype(cv)>::reserve_batch(c, s, n, flags); }));
    for (auto& e : s.ev)  // the phase events kzgmi_set_profiling records
      if (!e) HIPCHK(hipEventCreate(&e));
  }
  // multi-device context: every device's slots take whole batches of up to n (the async entry
  // points pipeline them per device; the synchronous split runs smaller shards on the same slots)
  for (kzgmi_ctx* p : c->peers) CHK(kzgmi_ctx_reserve(p, curve, n, flags));
  return set_dev(c);
}

int kzgmi_srs_load(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* g1, const uint8_t* g2, const uint8_t* tau_g2,
                   kzgmi_srs** out) {
  CHK(check_ctx(c));
  if (!g2 || !tau_g2 || !out) return fail(KZGMI_ERR_ARG, "null srs argument");
  *out = nullptr;
  CHK(slot0_idle(c));
  int rc = dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    const size_t gb = g2_bytes(Cv::ID), g1b = g1_bytes(Cv::ID);
    kzgmi_srs* srs = new kzgmi_srs();
    srs->curve = Cv::ID;
    srs->ctx = c;
    int r = 0;
    if ((r = s.stage.ensure(2 * gb + g1b)) || (r = s.flags.ensure(16)) || (r = srs->q.ensure(2 * sizeof(G2Aff<Cv>))) ||
        (r = srs->q_inf.ensure(16)) || (r = srs->lines.ensure(2 * Launch<Cv>::num_lines() * sizeof(Line<Cv>))) ||
        (r = srs->g1.ensure(2 * sizeof(Affine<Cv>) + 16))) {
      delete srs;
      return r;
    }
    // slot 0 = [tau]_2, slot 1 = [1]_2, then [1]_1
    std::vector<uint8_t> h(2 * gb + g1b);
    memcpy(h.data(), tau_g2, gb);
    memcpy(h.data() + gb, g2, gb);
    if (g1) memcpy(h.data() + 2 * gb, g1, g1b);
    if (int rb = begin_job(s)) {
      kzgmi_srs_free(srs);
      return rb;
    }
    hipStream_t st = s.stream;
    Affine<Cv>* g1p = srs->g1.template as<Affine<Cv>>();
    uint8_t* g1inf = srs->g1.template as<uint8_t>() + sizeof(Affine<Cv>);
    uint8_t g1inf_h = 0;
    bool okk = hipMemcpyAsync(s.stage.p, h.data(), h.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
               hipMemsetAsync(s.flags.p, 0, 16, st) == hipSuccess;
    if (okk) {
      uint32_t* err = s.flags.template as<uint32_t>() + 1;
      Launch<Cv>::convert_g2(st, s.stage.template as<uint8_t>(), 2, srs->q.template as<G2Aff<Cv>>(), srs->q_inf.template as<uint8_t>(),
                                         err);
      Launch<Cv>::precompute_lines(st, srs->q.template as<G2Aff<Cv>>(), srs->lines.template as<Line<Cv>>());
      if (g1) {  // validated like any input point, and it must be in G1 (GLV and the check rely on it)
        Launch<Cv>::convert_points(st, s.stage.template as<uint8_t>() + 2 * gb, 1, g1p, g1inf, err);
        Launch<Cv>::subgroup_check(st, g1p, g1inf, 1, err);
      } else {   // NULL: the standard generator
        Launch<Cv>::set_generator(st, g1p, g1inf);
      }
      srs->g1_29_off = sizeof(Affine<Cv>) + 16;
      Affine<Cv>* g1p29 = static_cast<Affine<Cv>*>(srs->g1_29());
      okk = hipMemcpyAsync(g1p29, g1p, sizeof(Affine<Cv>), hipMemcpyDeviceToDevice, st) == hipSuccess;
      Launch<Cv>::pts_to29(st, g1p29, 1);
      okk = okk && hipGetLastError() == hipSuccess &&
            hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipMemcpyAsync(&g1inf_h, g1inf, 1, hipMemcpyDeviceToHost, st) == hipSuccess && sync_job(s) == 0;
    }
    if (!okk) {
      kzgmi_srs_free(srs);
      return fail(KZGMI_ERR_DEVICE, "srs upload/precompute failed");
    }
    int e = map_device_err((uint32_t)s.host_flags[1]);
    if (!e && g1inf_h) e = fail(KZGMI_ERR_ARG, "SRS G1 element is the point at infinity");
    if (e) {
      kzgmi_srs_free(srs);
      return e;
    }
    c->srs_list.push_back(srs);
    *out = srs;
    return 0;
  });
  if (rc) return rc;
  for (kzgmi_ctx* p : c->peers) {  // multi-device context: the same SRS on every device
    kzgmi_srs* ps = nullptr;
    if (int r = kzgmi_srs_load(p, curve, g1, g2, tau_g2, &ps)) {
      kzgmi_srs_free(*out);
      *out = nullptr;
      return r;
    }
    (*out)->peers.push_back(ps);
  }
  return set_dev(c);
}

void kzgmi_srs_free(kzgmi_srs* srs) {
  if (!srs) return;
  for (kzgmi_srs* p : srs->peers) kzgmi_srs_free(p);
  srs->peers.clear();
  if (kzgmi_ctx* c = srs->ctx) {  // still attached: free its device memory on its device
    (void)hipSetDevice(c->device);
    auto& v = c->srs_list;
    v.erase(std::remove(v.begin(), v.end(), srs), v.end());
    srs->lines.release();
    srs->q.release();
    srs->q_inf.release();
    srs->g1.release();
  }
  delete srs;  // a detached SRS (its context already destroyed) owns no device memory
}

int kzgmi_slot_wait(kzgmi_ctx* c, int slot, int* ok_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  Slot& s = c->slots[slot];
  if (!s.pending) return fail(KZGMI_ERR_ARG, "slot has no pending batch");
  return finish_slot(c, s, ok_out);
}

// ------------------------------------------------------------------------------ pinned host memory
int kzgmi_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return fail(KZGMI_ERR_ARG, "bad argument");
  *out = nullptr;
  void* p = nullptr;
  HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  std::lock_guard<std::mutex> lk(g_host_mu);
  g_host[(uintptr_t)p] = HostRange{(uintptr_t)p + bytes, true};
  *out = p;
  return 0;
}

void kzgmi_host_free(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host.find((uintptr_t)p);
    if (it == g_host.end() || !it->second.owned) return;  // not ours: leave it alone
    g_host.erase(it);
  }
  (void)hipHostFree(p);
}

int kzgmi_host_register(void* p, size_t bytes) {
  if (!p || bytes == 0) return fail(KZGMI_ERR_ARG, "bad argument");
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    if (g_host.count((uintptr_t)p)) return fail(KZGMI_ERR_ARG, "range already registered");
  }
  HIPCHK(hipHostRegister(p, bytes, hipHostRegisterDefault));
  std::lock_guard<std::mutex> lk(g_host_mu);
  g_host[(uintptr_t)p] = HostRange{(uintptr_t)p + bytes, false};
  return 0;
}

int kzgmi_host_unregister(void* p) {
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host.find((uintptr_t)p);
    if (it == g_host.end() || it->second.owned) return fail(KZGMI_ERR_ARG, "range was not registered");
    g_host.erase(it);
  }
  HIPCHK(hipHostUnregister(p));
  return 0;
}

// ------------------------------------------------------------------------------ profiling
int kzgmi_set_glv(kzgmi_ctx* c, int msm, int batch) {
  CHK(check_ctx(c));
  for (auto& s : c->slots)
    if (s.pending) return fail(KZGMI_ERR_ARG, "kzgmi_set_glv with jobs in flight");
  c->glv_msm = msm != 0;
  c->glv_batch = batch != 0;
  for (kzgmi_ctx* p : c->peers) CHK(kzgmi_set_glv(p, msm, batch));
  return set_dev(c);
}

int kzgmi_set_split_acc(kzgmi_ctx* c, int mode) {
  CHK(check_ctx(c));
  if (mode < -1 || mode > 1) return fail(KZGMI_ERR_ARG, "split mode must be -1, 0 or 1");
  for (auto& s : c->slots)
    if (s.pending) return fail(KZGMI_ERR_ARG, "kzgmi_set_split_acc with jobs in flight");
  c->tune.split_acc = mode;
  for (kzgmi_ctx* p : c->peers) CHK(kzgmi_set_split_acc(p, mode));
  return set_dev(c);
}

int kzgmi_set_trusted_g1(kzgmi_ctx* c, int on) {
  CHK(check_ctx(c));
  for (auto& s : c->slots)
    if (s.pending) return fail(KZGMI_ERR_ARG, "kzgmi_set_trusted_g1 with jobs in flight");
  c->msm_trusted_g1 = on != 0;
  for (kzgmi_ctx* p : c->peers) CHK(kzgmi_set_trusted_g1(p, on));
  return set_dev(c);
}

int kzgmi_set_profiling(kzgmi_ctx* c, int on) {
  if (!c) return fail(KZGMI_ERR_ARG, "null context");
  c->profiling = on != 0;
  for (int k = 0; k < kNumPhases; ++k) c->phase_ms[k] = 0;
  c->phase_calls = 0;
  // multi-device context: every device records its phases; kzgmi_get_phase_ms reports the
  // primary device's (the peers' shards run the same phases concurrently)
  for (kzgmi_ctx* p : c->peers) CHK(kzgmi_set_profiling(p, on));
  return 0;
}

int kzgmi_get_phase_ms(kzgmi_ctx* c, double* out, int max_n) {
  if (!c || !out) return fail(KZGMI_ERR_ARG, "null argument");
  int k = max_n < kNumPhases ? max_n : kNumPhases;
  for (int i = 0; i < k; ++i) out[i] = c->phase_calls ? c->phase_ms[i] / c->phase_calls : 0.0;
  return k;
}

// ------------------------------------------------------------------------------ stream order
int kzgmi_stream_wait(kzgmi_ctx* c, int slot, void* stream) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  // an entry dependency of the slot's next job (begin_job), whichever lane that job starts in
  return add_dep(c->slots[slot], (hipStream_t)stream);
}

int kzgmi_slot_signal(kzgmi_ctx* c, int slot, void* stream) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  Slot& s = c->slots[slot];
  if (!s.signal_ev) HIPCHK(hipEventCreateWithFlags(&s.signal_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(s.signal_ev, s.stream));
  HIPCHK(hipStreamWaitEvent((hipStream_t)stream, s.signal_ev, 0));
  return 0;
}

}  // extern "C"
