// Device-list contexts (kzgmi_ctx_create over several devices) and the calls that shard one batch
// or MSM over them.
#include "host.hpp"

extern "C" {

// ------------------------------------------------------------------------------ multi-device context
int kzgmi_ctx_create(kzgmi_ctx** out, const int* device_ids, int n_devices, int pipeline_slots) {
  if (!out || !device_ids || n_devices < 1 || n_devices > 64) return fail(KZGMI_ERR_ARG, "bad ctx args");
  *out = nullptr;
  if (pipeline_slots < 1 || pipeline_slots > 64) return fail(KZGMI_ERR_ARG, "bad ctx args");
  kzgmi_ctx* c = nullptr;
  // every device holds ceil(slots / n_devices) local slots (route_slot)
  const int local = (pipeline_slots + n_devices - 1) / n_devices;
  CHK(kzgmi_ctx_create_device(&c, device_ids[0], local));
  for (int k = 1; k < n_devices; ++k) {
    kzgmi_ctx* p = nullptr;
    if (int r = kzgmi_ctx_create_device(&p, device_ids[k], local)) {
      kzgmi_ctx_destroy(c);
      return r;
    }
    c->peers.push_back(p);
  }
  c->user_slots = pipeline_slots;
  CHK(set_dev(c));
  *out = c;
  return 0;
}

int kzgmi_ctx_num_devices(const kzgmi_ctx* c) { return c ? 1 + (int)c->peers.size() : 0; }

int kzgmi_slot_device(const kzgmi_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= c->user_slots) return fail(KZGMI_ERR_ARG, "bad slot");
  const int D = 1 + (int)c->peers.size();
  return slot % D == 0 ? c->device : c->peers[slot % D - 1]->device;
}

}  // extern "C"

// Shards run concurrently (one async partial per device on its slot 0), the partial records are
// copied to the primary device (hipMemcpyPeer over xGMI: 2 XYZZ records per device), and the
// primary sums them and runs the pairing check -- the single-process form of the RCCL
// all-gather that kzgmi/distributed.py does across processes.
namespace {

// wait every device's slot 0 (first error wins; every slot is completed either way)
int wait_all(kzgmi_ctx* c, int started) {
  int first = 0;
  std::string msg;
  for (int d = 0; d < started; ++d) {
    int r = kzgmi_slot_wait(dev_ctx(c, d), 0, nullptr);
    if (r && !first) {
      first = r;
      msg = g_err;
    }
  }
  if (first) return fail(first, msg);
  return 0;
}

// children's records (in their `gath`, complete: wait_all synchronised every peer's slot 0) ->
// c->gath[d], copied on the primary's slot-0 stream, the stream kzgmi_batch_combine_device /
// kzgmi_msm_combine_device then read them on -- so the order is explicit, not left to how the
// runtime orders a null-stream peer copy against a non-blocking stream
int gather_records(kzgmi_ctx* c, size_t rec) {
  CHK(set_dev(c));
  CHK(begin_job(c->slots[0]));  // the combine's job starts in the same lane, behind these copies
  for (size_t d = 1; d <= c->peers.size(); ++d) {
    kzgmi_ctx* p = c->peers[d - 1];
    HIPCHK(hipMemcpyPeerAsync((uint8_t*)c->gath.p + d * rec, c->device, p->gath.p, p->device, rec, c->slots[0].stream));
  }
  return 0;
}

int batch_multi(kzgmi_ctx* c, const kzgmi_srs* srs, const void* const* dC, const void* const* dz,
                const void* const* dy, const void* const* dpi, const size_t* nd, const uint8_t* seed32,
                uint32_t flags, int* ok_out) {
  const int D = 1 + (int)c->peers.size();
  if (srs->peers.size() != c->peers.size()) return fail(KZGMI_ERR_ARG, "srs was not loaded on this context");
  const kzgmi_curve curve = (kzgmi_curve)srs->curve;
  const size_t rec = 2 * kzgmi_partial_bytes(curve);
  std::vector<uint64_t> off(D + 1, 0);
  for (int d = 0; d < D; ++d) {
    if (nd[d] && (!dC[d] || !dz[d] || !dy[d] || !dpi[d])) return fail(KZGMI_ERR_ARG, "null input");
    if (nd[d] > (1u << 26)) return fail(KZGMI_ERR_ARG, "shard too large (max 2^26 tuples per device)");
    off[d + 1] = off[d] + nd[d];
  }
  uint8_t sb[32];
  if (flags & KZGMI_FLAG_FIAT_SHAMIR) {  // one transcript over the whole batch: subtree roots gathered
    if (flags & KZGMI_FLAG_POWERS) return fail(KZGMI_ERR_ARG, "KZGMI_FLAG_POWERS and KZGMI_FLAG_FIAT_SHAMIR are exclusive");
    const uint64_t ntot = off[D];
    if (ntot == 0) {
      *ok_out = 1;
      return 0;
    }
    const size_t nch_tot = (ntot + FS_CHUNK - 1) / FS_CHUNK;
    CHK(c->mdig_all.ensure(nch_tot * 32));
    // every device hashes its subtrees concurrently (enqueued first), then each device's
    // digests are waited for and copied to the primary, ordered before the challenge derivation
    // on the primary's slot-0 stream
    for (int d = 0; d < D; ++d) {
      if (!nd[d]) continue;
      if (off[d] % FS_CHUNK) return fail(KZGMI_ERR_ARG, "Fiat-Shamir shards must start at multiples of 4096 tuples");
      kzgmi_ctx* p = dev_ctx(c, d);
      const size_t nch = (nd[d] + FS_CHUNK - 1) / FS_CHUNK;
      CHK(set_dev(p));
      CHK(p->mdig.ensure(nch * 32));
      CHK(fs_chunk_digests_enqueue(p, curve, dC[d], dz[d], dy[d], dpi[d], nd[d], off[d],
                                   flags & KZGMI_FLAG_COMPRESSED, p->mdig.p));
    }
    size_t at = 0;
    for (int d = 0; d < D; ++d) {
      if (!nd[d]) continue;
      kzgmi_ctx* p = dev_ctx(c, d);
      const size_t nch = (nd[d] + FS_CHUNK - 1) / FS_CHUNK;
      CHK(set_dev(p));
      CHK(sync_slot(p->slots[0]));
      CHK(set_dev(c));
      CHK(begin_job(c->slots[0]));  // the challenge's job follows in this lane
      HIPCHK(hipMemcpyPeerAsync((uint8_t*)c->mdig_all.p + at * 32, c->device, p->mdig.p, p->device, nch * 32,
                                c->slots[0].stream));
      at += nch;
    }
    CHK(kzgmi_fs_challenge_from_digests_device(c, curve, c->mdig_all.p, nch_tot, ntot, sb));
    seed32 = sb;
    flags &= ~KZGMI_FLAG_FIAT_SHAMIR;
  } else if (!seed32) {
    uint8_t tmp[32];
    make_seed(nullptr, tmp);  // one verifier-private seed shared by every shard
    memcpy(sb, tmp, 32);
    seed32 = sb;
  }
  CHK(set_dev(c));
  CHK(c->gath.ensure(D * rec));
  for (int d = 0; d < D; ++d) {
    kzgmi_ctx* p = dev_ctx(c, d);
    int r = 0;
    if (d > 0) {
      r = set_dev(p);
      if (!r) r = p->gath.ensure(rec);
    }
    if (!r)
      r = kzgmi_batch_partial_device_async(p, d == 0 ? srs : srs->peers[d - 1], 0, dC[d], dz[d], dy[d], dpi[d], nd[d],
                                           off[d], seed32, flags, d == 0 ? c->gath.p : p->gath.p);
    if (r) {
      std::string msg = g_err;
      (void)wait_all(c, d);
      return fail(r, msg);
    }
  }
  CHK(wait_all(c, D));
  CHK(gather_records(c, rec));
  return kzgmi_batch_combine_device(c, srs, c->gath.p, D, ok_out);
}

int msm_multi(kzgmi_ctx* c, kzgmi_curve curve, const void* const* dp, const void* const* ds, const size_t* nd,
              uint8_t* out) {
  const int D = 1 + (int)c->peers.size();
  if (curve != KZGMI_BLS12_381 && curve != KZGMI_BN254) return fail(KZGMI_ERR_ARG, "unknown curve");
  const size_t rec = kzgmi_partial_bytes(curve);
  CHK(set_dev(c));
  CHK(c->gath.ensure(D * rec));
  for (int d = 0; d < D; ++d) {
    kzgmi_ctx* p = dev_ctx(c, d);
    int r = 0;
    if (d > 0) {
      r = set_dev(p);
      if (!r) r = p->gath.ensure(rec);
    }
    if (!r) r = kzgmi_msm_partial_device_async(p, curve, 0, dp[d], ds[d], nd[d], d == 0 ? c->gath.p : p->gath.p);
    if (r) {
      std::string msg = g_err;
      (void)wait_all(c, d);
      return fail(r, msg);
    }
  }
  CHK(wait_all(c, D));
  CHK(gather_records(c, rec));
  return kzgmi_msm_combine_device(c, curve, c->gath.p, D, out);
}

}  // namespace

// balanced split of n tuples/points over the devices in units of 4096 (Fiat-Shamir subtrees)
std::vector<size_t> kzgmi::split_units(size_t n, int D) {
  const size_t units = (n + FS_CHUNK - 1) / FS_CHUNK;
  std::vector<size_t> nd(D);
  size_t lo = 0;
  for (int d = 0; d < D; ++d) {
    size_t u1 = units * (d + 1) / D;
    size_t hi = std::min(n, u1 * FS_CHUNK);
    nd[d] = hi - lo;
    lo = hi;
  }
  return nd;
}

int kzgmi::batch_multi_host(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* commitments, const uint8_t* zs,
                     const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t* seed32, uint32_t flags,
                     int* ok_out) {
  const int D = 1 + (int)c->peers.size();
  const size_t gb = (flags & KZGMI_FLAG_COMPRESSED) ? g1_bytes(srs->curve) / 2 : g1_bytes(srs->curve);
  std::vector<size_t> nd = split_units(n, D);
  std::vector<const void*> pC(D), pz(D), py(D), ppi(D);
  size_t lo = 0;
  for (int d = 0; d < D; ++d) {
    kzgmi_ctx* p = dev_ctx(c, d);
    Slot& s = p->slots[0];
    CHK(set_dev(p));
    CHK(s.stage.ensure(nd[d] * (2 * gb + 64)));
    uint8_t* base = s.stage.template as<uint8_t>();
    pC[d] = base;
    ppi[d] = base + nd[d] * gb;
    pz[d] = base + 2 * nd[d] * gb;
    py[d] = base + 2 * nd[d] * gb + 32 * nd[d];
    CHK(begin_job(s));  // the shard's job starts in the same lane, behind these copies
    if (nd[d]) {
      HIPCHK(hipMemcpyAsync((void*)pC[d], commitments + lo * gb, nd[d] * gb, hipMemcpyHostToDevice, s.stream));
      HIPCHK(hipMemcpyAsync((void*)ppi[d], proofs + lo * gb, nd[d] * gb, hipMemcpyHostToDevice, s.stream));
      HIPCHK(hipMemcpyAsync((void*)pz[d], zs + lo * 32, nd[d] * 32, hipMemcpyHostToDevice, s.stream));
      HIPCHK(hipMemcpyAsync((void*)py[d], ys + lo * 32, nd[d] * 32, hipMemcpyHostToDevice, s.stream));
    }
    lo += nd[d];
  }
  return batch_multi(c, srs, pC.data(), pz.data(), py.data(), ppi.data(), nd.data(), seed32, flags, ok_out);
}

int kzgmi::msm_multi_host(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* points, const uint8_t* scalars, size_t n,
                   uint8_t* out) {
  const int D = 1 + (int)c->peers.size();
  const size_t gb = g1_bytes(curve);
  std::vector<size_t> nd = split_units(n, D);
  std::vector<const void*> pp(D), ps(D);
  size_t lo = 0;
  for (int d = 0; d < D; ++d) {
    kzgmi_ctx* p = dev_ctx(c, d);
    Slot& s = p->slots[0];
    CHK(set_dev(p));
    CHK(s.stage.ensure(nd[d] * (gb + 32)));
    pp[d] = s.stage.p;
    ps[d] = s.stage.template as<uint8_t>() + nd[d] * gb;
    CHK(begin_job(s));
    if (nd[d]) {
      HIPCHK(hipMemcpyAsync((void*)pp[d], points + lo * gb, nd[d] * gb, hipMemcpyHostToDevice, s.stream));
      HIPCHK(hipMemcpyAsync((void*)ps[d], scalars + lo * 32, nd[d] * 32, hipMemcpyHostToDevice, s.stream));
    }
    lo += nd[d];
  }
  return msm_multi(c, curve, pp.data(), ps.data(), nd.data(), out);
}

extern "C" {

int kzgmi_batch_verify_multi_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* const* d_commitments,
                                    const void* const* d_zs, const void* const* d_ys, const void* const* d_proofs,
                                    const size_t* n_per_device, const uint8_t* seed32, uint32_t flags, int* ok_out) {
  CHK(check_ctx(c));
  if (!srs || srs->ctx != c || !ok_out || !d_commitments || !d_zs || !d_ys || !d_proofs || !n_per_device)
    return fail(KZGMI_ERR_ARG, "bad argument");
  if (flags & ~kAllFlags) return fail(KZGMI_ERR_ARG, "unknown flags");
  if ((flags & KZGMI_FLAG_POWERS) && !seed32) return fail(KZGMI_ERR_ARG, "KZGMI_FLAG_POWERS needs r in seed32");
  CHK(slot0_idle(c));
  return batch_multi(c, srs, d_commitments, d_zs, d_ys, d_proofs, n_per_device, seed32, flags, ok_out);
}

int kzgmi_msm_g1_multi_device(kzgmi_ctx* c, kzgmi_curve curve, const void* const* d_points,
                              const void* const* d_scalars, const size_t* n_per_device, uint8_t* out) {
  CHK(check_ctx(c));
  if (!d_points || !d_scalars || !n_per_device || !out) return fail(KZGMI_ERR_ARG, "bad argument");
  CHK(slot0_idle(c));
  return msm_multi(c, curve, d_points, d_scalars, n_per_device, out);
}

}  // extern "C"
