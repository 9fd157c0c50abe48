// Batch verification entry points: device and host buffers (staged, or chunked over point ranges),
// shard partials and their combine, the last combination, point validation, the Fiat-Shamir utilities.
#include "host.hpp"

extern "C" {

int kzgmi_batch_verify_device_async(kzgmi_ctx* c, const kzgmi_srs* srs, int slot, const void* dC, const void* dz,
                                    const void* dy, const void* dpi, size_t n, const uint8_t* seed32) {
  return kzgmi_batch_verify_device_ex_async(c, srs, slot, dC, dz, dy, dpi, n, seed32, 0);
}

int kzgmi_batch_verify_device_ex_async(kzgmi_ctx* c, const kzgmi_srs* srs, int slot, const void* dC, const void* dz,
                                       const void* dy, const void* dpi, size_t n, const uint8_t* seed32,
                                       uint32_t flags) {
  KZ_ROUTE(c, &srs, slot);
  if (flags & ~kAllFlags) return fail(KZGMI_ERR_ARG, "unknown flags");
  if ((flags & KZGMI_FLAG_POWERS) && (flags & KZGMI_FLAG_FIAT_SHAMIR))
    return fail(KZGMI_ERR_ARG, "KZGMI_FLAG_POWERS and KZGMI_FLAG_FIAT_SHAMIR are exclusive");
  if ((flags & KZGMI_FLAG_POWERS) && !seed32) return fail(KZGMI_ERR_ARG, "KZGMI_FLAG_POWERS needs r in seed32");
  CHK(check_ctx(c, slot));
  if (!srs || srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (n && (!dC || !dz || !dy || !dpi)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "batch too large (max 2^26 tuples per call)");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  uint8_t sb[32];
  Seed seed = make_seed(seed32, sb);
  if (n == 0) {
    CHK(set_dev(c));
    return arm_empty(s, JobKind::Verdict);
  }
  Roctx rx("kzgmi_batch_verify_device_ex_async");
  struct Guard {  // (kzgmi_ctx::async_call)
    kzgmi_ctx* c;
    explicit Guard(kzgmi_ctx* c_) : c(c_) { c->async_call = true; }
    ~Guard() { c->async_call = false; }
  } guard(c);
  return dispatch(srs->curve, [&](auto cv) -> int {
    return HostCore<decltype(cv)>::enqueue_batch(c, s, srs, dC, dz, dy, dpi, n, seed, 0, nullptr, flags);
  });
}

int kzgmi_batch_verify_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                              const void* dpi, size_t n, const uint8_t* seed32, int* ok_out) {
  return run_sync(c, [&] { return kzgmi_batch_verify_device_async(c, srs, 0, dC, dz, dy, dpi, n, seed32); }, ok_out);
}

}  // extern "C"
namespace {
// The host arrays of one batch into the slot's stage buffer on the context's FIFO copy stream
// (pinned ranges DMA'd directly, pageable ones staged by the copy pool before this returns); the
// slot's next job waits for the copy.
int stage_host_batch(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, uint32_t flags, const uint8_t* commitments,
                     const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t** dC_out,
                     const uint8_t** dz_out, const uint8_t** dy_out, const uint8_t** dpi_out) {
  const size_t gb = (flags & KZGMI_FLAG_COMPRESSED) ? g1_bytes(srs->curve) / 2 : g1_bytes(srs->curve);
  const StageItem items[4] = {{commitments, n * gb}, {proofs, n * gb}, {zs, n * 32}, {ys, n * 32}};
  uint8_t* d[4];
  CHK(stage_host(c, s, items, 4, d, /*profile=*/true));
  *dC_out = d[0];
  *dpi_out = d[1];
  *dz_out = d[2];
  *dy_out = d[3];
  return 0;
}

// Synchronous host-buffer batches on one device: the PCIe copy (~5 ms per 2^20 batch) would sit
// in front of the whole computation.  Split into k point ranges (units of 4096 tuples) on slots
// 0..k-1: range j's shard partial starts as soon as its own copy has landed, while the next
// range copies, and one combine + pairing on slot 0 decides (the same sums: r_i use the global
// index; a failed range marks its partial records, so the combine reports its error).  Batches
// without flags (or with TRUSTED_G1) instead accumulate every range into one bucket store
// (enqueue_batch_chunked): no per-range reduction.  From 2^17 tuples: 4 ranges with one store (2^20 pinned: 13.7 -> 11.0
// ms, pageable 14.1 -> 11.3), 2 with partials (12.1 / 12.5 ms; profiles/r05/host_latency_*.txt).
// KZGMI_HOST_CHUNKS overrides (1: never); not with Fiat-Shamir (the challenge needs every range
// first) or when slots 0..k-1 are not all idle.
bool one_store_flags(uint32_t flags) { return (flags & ~KZGMI_FLAG_TRUSTED_G1) == 0; }
int host_chunks(const kzgmi_ctx* c, size_t n, uint32_t flags, int curve) {
  (void)curve;
  if (flags & KZGMI_FLAG_FIAT_SHAMIR) return 1;
  const bool one_store = one_store_flags(flags) && c->host_chunk_mode != 1;
  int k = n >= (size_t(1) << 17) ? (one_store ? 4 : 2) : 1;
  if (c->host_chunks_env) k = c->host_chunks_env;
  k = std::min<int>(k, (int)((n + FS_CHUNK - 1) / FS_CHUNK));
  // the one-store form runs every range on slot 0 (slot0_idle checked it); the shard-partial
  // form takes slots 0..k-1, which must exist and be idle
  if (one_store) return std::max(k, 1);
  k = std::min<int>(k, (int)c->slots.size());
  for (int j = 0; j < k; ++j)
    if (c->slots[j].pending) return 1;
  return std::max(k, 1);
}

int batch_host_chunked(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* commitments, const uint8_t* zs,
                       const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t* seed32, uint32_t flags,
                       int k, int* ok_out) {
  Roctx rx("kzgmi_batch_verify_ex.chunked");
  uint8_t sb[32];
  if (!seed32) {  // one verifier-private seed for every range
    make_seed(nullptr, sb);
    seed32 = sb;
  }
  if (one_store_flags(flags) && c->host_chunk_mode != 1) {
    // one bucket store for every range (no per-range reduction)
    Slot& s = c->slots[0];
    uint8_t sb2[32];
    const Seed seed = make_seed(seed32, sb2);
    const int r = dispatch(srs->curve, [&](auto cv) -> int {
      return HostCore<decltype(cv)>::enqueue_batch_chunked(c, s, srs, commitments, zs, ys, proofs, n, seed, flags, k);
    });
    if (r) {
      // whatever was enqueued drains before the error returns: the slot's kernels of this call
      // (end_job never ran, so done_ev still marks the previous job) and the copies that may
      // still read the caller's buffers
      const std::string msg = g_err;
      (void)hipStreamSynchronize(s.stream);
      (void)hipStreamSynchronize(c->h2d_stream);
      s.ndep = 0;
      s.pending = false;
      return fail(r, msg);
    }
    return kzgmi_slot_wait(c, 0, ok_out);
  }
  const size_t gb = (flags & KZGMI_FLAG_COMPRESSED) ? g1_bytes(srs->curve) / 2 : g1_bytes(srs->curve);
  const size_t rec = 2 * kzgmi_partial_bytes((kzgmi_curve)srs->curve);
  CHK(c->gath.ensure((size_t)k * rec));
  const std::vector<size_t> nk = split_units(n, k);
  size_t lo = 0;
  int started = 0, r = 0;
  for (int j = 0; j < k && !r; ++j) {
    const uint8_t *dC, *dz, *dy, *dpi;
    r = stage_host_batch(c, c->slots[j], srs, flags, commitments + lo * gb, zs + lo * 32, ys + lo * 32,
                         proofs + lo * gb, nk[j], &dC, &dz, &dy, &dpi);
    if (!r)
      r = kzgmi_batch_partial_device_async(c, srs, j, dC, dz, dy, dpi, nk[j], lo, seed32, flags,
                                           (uint8_t*)c->gath.p + (size_t)j * rec);
    if (!r) ++started;
    lo += nk[j];
  }
  // every started range completes before the combine reads the records (a range's own error is
  // carried by its marked records)
  const std::string msg = r ? g_err : std::string();
  for (int j = 0; j < started; ++j) (void)kzgmi_slot_wait(c, j, nullptr);
  if (r) return fail(r, msg);
  return kzgmi_batch_combine_device(c, srs, c->gath.p, k, ok_out);
}
}  // namespace
extern "C" {

int kzgmi_batch_verify(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* commitments, const uint8_t* zs,
                       const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t* seed32, int* ok_out) {
  return kzgmi_batch_verify_ex(c, srs, commitments, zs, ys, proofs, n, seed32, 0, ok_out);
}

int kzgmi_batch_verify_ex(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* commitments, const uint8_t* zs,
                          const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t* seed32, uint32_t flags,
                          int* ok_out) {
  CHK(check_ctx(c));
  if (!srs || !ok_out) return fail(KZGMI_ERR_ARG, "null argument");
  if (srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (n && (!commitments || !zs || !ys || !proofs)) return fail(KZGMI_ERR_ARG, "null input");
  CHK(slot0_idle(c));
  if (!c->peers.empty()) return batch_multi_host(c, srs, commitments, zs, ys, proofs, n, seed32, flags, ok_out);
  const int k = host_chunks(c, n, flags, srs->curve);
  if (k > 1) return batch_host_chunked(c, srs, commitments, zs, ys, proofs, n, seed32, flags, k, ok_out);
  CHK(kzgmi_batch_verify_ex_async(c, srs, 0, commitments, zs, ys, proofs, n, seed32, flags));
  return kzgmi_slot_wait(c, 0, ok_out);
}

int kzgmi_batch_verify_ex_async(kzgmi_ctx* c, const kzgmi_srs* srs, int slot, const uint8_t* commitments,
                                const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, size_t n,
                                const uint8_t* seed32, uint32_t flags) {
  if (!srs) return fail(KZGMI_ERR_ARG, "null argument");
  KZ_ROUTE(c, &srs, slot);
  CHK(check_ctx(c, slot));
  if (srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (n && (!commitments || !zs || !ys || !proofs)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "batch too large (max 2^26 tuples per call)");
  if (flags & ~kAllFlags) return fail(KZGMI_ERR_ARG, "unknown flags");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (n == 0) return kzgmi_batch_verify_device_ex_async(c, srs, slot, nullptr, nullptr, nullptr, nullptr, 0, seed32, flags);
  Roctx rx("kzgmi_batch_verify_ex_async");
  const uint8_t *dC, *dz, *dy, *dpi;
  CHK(stage_host_batch(c, s, srs, flags, commitments, zs, ys, proofs, n, &dC, &dz, &dy, &dpi));
  const int r = kzgmi_batch_verify_device_ex_async(c, srs, slot, dC, dz, dy, dpi, n, seed32, flags);
  if (c->profiling) s.ev_used[EV_H2D0] = s.ev_used[EV_H2D1] = (r == 0);
  return r;
}

int kzgmi_last_combination(kzgmi_ctx* c, uint8_t* a_out, uint8_t* b_out) {
  CHK(check_ctx(c));
  if (!a_out || !b_out) return fail(KZGMI_ERR_ARG, "null output");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  if (!s.res.p) return fail(KZGMI_ERR_ARG, "no batch has run on slot 0");
  return dispatch(s.curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    const size_t gb = g1_bytes(Cv::ID);
    CHK(s.outb.ensure(2 * gb));
    CHK(begin_job(s));
    Launch<Cv>::encode_points(s.stream, s.res.template as<Xyzz<Cv>>(), 2, s.outb.template as<uint8_t>());
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> h(2 * gb);
    HIPCHK(hipMemcpyAsync(h.data(), s.outb.p, 2 * gb, hipMemcpyDeviceToHost, s.stream));
    CHK(sync_job(s));
    memcpy(a_out, h.data(), gb);
    memcpy(b_out, h.data() + gb, gb);
    return 0;
  });
}

// ------------------------------------------------------------------------------ multi-GPU
size_t kzgmi_partial_bytes(kzgmi_curve curve) {
  return curve == KZGMI_BLS12_381 ? sizeof(Xyzz<Bls12_381>) : sizeof(Xyzz<Bn254>);
}

int kzgmi_batch_partial_device_async(kzgmi_ctx* c, const kzgmi_srs* srs, int slot, const void* dC, const void* dz,
                                     const void* dy, const void* dpi, size_t n, uint64_t index_offset,
                                     const uint8_t* seed32, uint32_t flags, void* d_partial_out) {
  KZ_ROUTE(c, &srs, slot);
  Roctx rx("kzgmi_batch_partial_device_async");
  if (flags & ~kAllFlags) return fail(KZGMI_ERR_ARG, "unknown flags");
  if (flags & KZGMI_FLAG_FIAT_SHAMIR)
    return fail(KZGMI_ERR_ARG, "shards take the Fiat-Shamir r as seed32 (see kzgmi_fs_challenge_from_digests_device)");
  // r^i is built from the FS_POW_BITS = 32 low bits of the global index (fs.hpp): indices at or
  // above 2^32 would wrap and repeat randomisers
  if ((flags & KZGMI_FLAG_POWERS) && (index_offset > (1ull << 32) || n > (1ull << 32) - index_offset))
    return fail(KZGMI_ERR_ARG, "KZGMI_FLAG_POWERS needs index_offset + n <= 2^32");
  CHK(check_ctx(c, slot));
  if (!srs || srs->ctx != c || !d_partial_out) return fail(KZGMI_ERR_ARG, "bad argument");
  if (!seed32) return fail(KZGMI_ERR_ARG, "sharded verification needs an explicit shared seed");
  if (n && (!dC || !dz || !dy || !dpi)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "batch too large (max 2^26 tuples per call)");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  uint8_t sb[32];
  Seed seed = make_seed(seed32, sb);
  return dispatch(srs->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    if (n == 0) {  // empty shard: both partials are the point at infinity (zz = 0)
      CHK(s.flags.ensure(16));
      CHK(begin_job(s));
      HIPCHK(hipMemsetAsync(d_partial_out, 0, 2 * sizeof(Xyzz<Cv>), s.stream));
      HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));  // a chained combine keeps the error word
      CHK(end_job(s));
      return arm_empty(s, JobKind::BatchPartial, Cv::ID);
    }
    return HostCore<Cv>::enqueue_batch(c, s, srs, dC, dz, dy, dpi, n, seed, index_offset, d_partial_out, flags);
  });
}

int kzgmi_batch_partial_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                               const void* dpi, size_t n, uint64_t index_offset, const uint8_t* seed32,
                               void* d_partial_out) {
  CHK(kzgmi_batch_partial_device_async(c, srs, 0, dC, dz, dy, dpi, n, index_offset, seed32, 0, d_partial_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

int kzgmi_batch_combine_device_async(kzgmi_ctx* c, const kzgmi_srs* srs, int slot, const void* d_partials,
                                     int n_parts) {
  KZ_ROUTE(c, &srs, slot);
  CHK(check_ctx(c, slot));
  if (!srs || srs->ctx != c || !d_partials || n_parts < 1) return fail(KZGMI_ERR_ARG, "bad argument");
  Slot& s = c->slots[slot];
  // chained: behind this slot's own pending batch partial (one kzgmi_slot_wait completes both;
  // the partial's error word is kept, the pairing writes the verdict word)
  const bool chain = s.pending && s.kind == JobKind::BatchPartial;
  if (s.pending && !chain) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (chain && s.curve != srs->curve) return fail(KZGMI_ERR_ARG, "chained combine: curve differs from the partial's");
  return dispatch(srs->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using XY = Xyzz<Cv>;
    CHK(s.res.ensure(2 * sizeof(XY)));
    CHK(s.flags.ensure(16));
    CHK(begin_job(s));  // chained: the lane the partial ended in
    hipStream_t st = s.stream;
    if (!chain) {
      HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
      mark(c, s, PH_COMBINE);
    }
    Launch<Cv>::sum_partials(st, (const XY*)d_partials, (uint32_t)n_parts, 2, 2, s.res.template as<XY>(),
                             s.flags.template as<uint32_t>() + 1);
    Launch<Cv>::pairing_check(st, s.res.template as<XY>(), srs->lines.template as<Line<Cv>>(),
                              srs->q_inf.template as<uint8_t>(), s.flags.template as<int>());
    mark(c, s, PH_PAIRING + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
    CHK(end_job(s));
    arm(s, JobKind::Verdict, Cv::ID);
    return 0;
  });
}

int kzgmi_batch_combine_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* d_partials, int n_parts, int* ok_out) {
  if (!ok_out) return fail(KZGMI_ERR_ARG, "null ok_out");
  CHK(kzgmi_batch_combine_device_async(c, srs, 0, d_partials, n_parts));
  return kzgmi_slot_wait(c, 0, ok_out);
}

int kzgmi_g1_validate_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_points, size_t n, uint32_t flags) {
  CHK(check_ctx(c));
  if (flags & ~(KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK)) return fail(KZGMI_ERR_ARG, "unknown flags");
  if (n && !d_points) return fail(KZGMI_ERR_ARG, "null input");
  if (n > (1u << 27)) return fail(KZGMI_ERR_ARG, "too many points (max 2^27 per call)");
  if (n == 0) return 0;
  Slot& s = c->slots[0];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot 0 busy: call kzgmi_slot_wait first");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using L = Launch<Cv>;
    CHK(s.pts.ensure(n * sizeof(Affine<Cv>)));
    CHK(s.inf.ensure(n));
    CHK(s.flags.ensure(16));
    return utility_job(c, s, [&](Slot&, uint32_t* err) -> int {
      hipStream_t st = s.stream;
      if (flags & KZGMI_FLAG_COMPRESSED)
        L::decompress_points(st, (const uint8_t*)d_points, (uint32_t)n, s.pts.template as<Affine<Cv>>(),
                             s.inf.template as<uint8_t>(), err);
      else
        L::convert_points(st, (const uint8_t*)d_points, (uint32_t)n, s.pts.template as<Affine<Cv>>(),
                          s.inf.template as<uint8_t>(), err);
      if (flags & KZGMI_FLAG_SUBGROUP_CHECK)
        L::subgroup_check(st, s.pts.template as<Affine<Cv>>(), s.inf.template as<uint8_t>(), (uint32_t)n, err);
      return 0;
    });
  });
}

}  // extern "C"

// the chunk digests of kzgmi_fs_chunk_digests_device, enqueued on slot 0's stream (no wait)
int kzgmi::fs_chunk_digests_enqueue(kzgmi_ctx* c, kzgmi_curve curve, const void* dC, const void* dz, const void* dy,
                                    const void* dpi, size_t n, uint64_t index_offset, uint32_t flags, void* d_out) {
  CHK(check_ctx(c));
  if (!d_out || (n && (!dC || !dz || !dy || !dpi)) || n == 0) return fail(KZGMI_ERR_ARG, "bad argument");
  if (index_offset % FS_CHUNK) return fail(KZGMI_ERR_ARG, "index_offset must be a multiple of 4096");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "too many tuples (max 2^26 per call)");
  Slot& s = c->slots[0];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot 0 busy: call kzgmi_slot_wait first");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    const uint32_t* dg = nullptr;
    CHK(begin_job(s));
    CHK(HostCore<Cv>::enqueue_fs_digests(s, dC, dpi, dz, dy, n, index_offset, (flags & KZGMI_FLAG_COMPRESSED) != 0, &dg));
    const size_t nch = (n + FS_CHUNK - 1) / FS_CHUNK;
    HIPCHK(hipMemcpyAsync(d_out, dg, nch * 32, hipMemcpyDeviceToDevice, s.stream));
    HIPCHK(hipGetLastError());
    return end_job(s);
  });
}

extern "C" {

int kzgmi_fs_chunk_digests_device(kzgmi_ctx* c, kzgmi_curve curve, const void* dC, const void* dz, const void* dy,
                                  const void* dpi, size_t n, uint64_t index_offset, uint32_t flags, void* d_out) {
  CHK(fs_chunk_digests_enqueue(c, curve, dC, dz, dy, dpi, n, index_offset, flags, d_out));
  return sync_slot(c->slots[0]);
}

int kzgmi_fs_challenge_from_digests_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_digests, size_t nchunks,
                                           uint64_t n_total, uint8_t* r_out) {
  CHK(check_ctx(c));
  if (!d_digests || !r_out || nchunks == 0 || nchunks > (1u << 22)) return fail(KZGMI_ERR_ARG, "bad argument");
  if ((n_total + FS_CHUNK - 1) / FS_CHUNK != nchunks) return fail(KZGMI_ERR_ARG, "nchunks != ceil(n_total / 4096)");
  Slot& s = c->slots[0];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot 0 busy: call kzgmi_slot_wait first");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    CHK(begin_job(s));
    CHK(HostCore<Cv>::enqueue_fs_challenge(s, (const uint32_t*)d_digests, (uint32_t)nchunks, n_total));
    uint32_t w[8];
    HIPCHK(hipMemcpyAsync(w, s.chal.p, 32, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipGetLastError());
    CHK(sync_job(s));
    words_be(w, r_out);
    return 0;
  });
}

int kzgmi_fs_challenge_device(kzgmi_ctx* c, kzgmi_curve curve, const void* dC, const void* dz, const void* dy,
                              const void* dpi, size_t n, uint32_t flags, uint8_t* r_out) {
  CHK(check_ctx(c));
  if (!r_out || n == 0 || !dC || !dz || !dy || !dpi) return fail(KZGMI_ERR_ARG, "bad argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "too many tuples (max 2^26 per call)");
  Slot& s = c->slots[0];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot 0 busy: call kzgmi_slot_wait first");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    const uint32_t* dg = nullptr;
    CHK(begin_job(s));
    CHK(HostCore<Cv>::enqueue_fs_digests(s, dC, dpi, dz, dy, n, 0, (flags & KZGMI_FLAG_COMPRESSED) != 0, &dg));
    CHK(HostCore<Cv>::enqueue_fs_challenge(s, dg, (uint32_t)((n + FS_CHUNK - 1) / FS_CHUNK), n));
    uint32_t w[8];
    HIPCHK(hipMemcpyAsync(w, s.chal.p, 32, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipGetLastError());
    CHK(sync_job(s));
    words_be(w, r_out);
    return 0;
  });
}

}  // extern "C"
