// The Ethereum front ends (BLS12-381 only): EIP-4844 blob batches, EIP-7594 cell batches, cell
// extension / recovery, cell proof generation (FK20) and EIP-4844 commitments and proofs, with their
// utilities.
#include "host.hpp"

namespace {
constexpr size_t kBlobMax = size_t(1) << 20;  // blobs per call
constexpr uint32_t kBlobFlags = KZGMI_FLAG_POWERS | KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK;

// the tables of this context's device, built at the first call that reads them (on st, waited
// for): the blob evaluation domain, the cell coset table (host.hpp ensure_cell_table), the transforms'
// twiddles and scale factors
int ensure_blob_table(kzgmi_ctx* c, hipStream_t st) {
  return ensure_once(c->blob_table_ready, c->blob_table, BlobLaunch::table_bytes(), st,
                     [&] { BlobLaunch::domain(st, c->blob_table.p); });
}
int ensure_ntt_table(kzgmi_ctx* c, hipStream_t st) {
  return ensure_once(c->ntt_table_ready, c->ntt_table, RecoverLaunch::table_bytes(), st,
                     [&] { RecoverLaunch::table(st, c->ntt_table.p); });
}

// slot-0 utility jobs (slot0_utility_job) of the blob and of the cell front end
template <class F>
int blob_slot0_job(kzgmi_ctx* c, F&& launch) {
  return slot0_utility_job(c, [&](Slot& s) { return ensure_blob_table(c, s.stream); }, launch);
}
template <class F>
int cell_slot0_job(kzgmi_ctx* c, F&& launch) {
  return slot0_utility_job(c, [&](Slot& s) { return ensure_cell_table(c, s.stream); }, launch);
}
}  // namespace
extern "C" {

int kzgmi_blob_challenges_device(kzgmi_ctx* c, const void* d_blobs, const void* d_commitments48, size_t n,
                                 void* d_zs_out) {
  CHK(check_ctx(c));
  if (n && (!d_blobs || !d_commitments48 || !d_zs_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  if (n == 0) return 0;
  return blob_slot0_job(c, [&](Slot& s, uint32_t* err) -> int {
    BlobLaunch::challenges(s.stream, blob_mapping(c, n), (const uint8_t*)d_blobs, (const uint8_t*)d_commitments48,
                           (uint32_t)n, (uint8_t*)d_zs_out, err);
    return 0;
  });
}

int kzgmi_blob_eval_device(kzgmi_ctx* c, const void* d_blobs, const void* d_zs, size_t n, void* d_ys_out) {
  CHK(check_ctx(c));
  if (n && (!d_blobs || !d_zs || !d_ys_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  if (n == 0) return 0;
  return blob_slot0_job(c, [&](Slot& s, uint32_t* err) -> int {
    BlobLaunch::eval(s.stream, (const uint8_t*)d_blobs, (const uint8_t*)d_zs, c->blob_table.p, (uint32_t)n, true,
                     (uint8_t*)d_ys_out, err);
    return 0;
  });
}

int kzgmi_blob_batch_challenge_device(kzgmi_ctx* c, const void* d_commitments48, const void* d_zs, const void* d_ys,
                                      const void* d_proofs48, size_t n, uint8_t r_out[32]) {
  CHK(check_ctx(c));
  if (!r_out || (n && (!d_commitments48 || !d_zs || !d_ys || !d_proofs48))) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  uint32_t w[8];
  CHK(blob_slot0_job(c, [&](Slot& s, uint32_t*) -> int {
    CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<Bls12_381::FrP>)));
    CHK(s.chal.ensure(32));
    BlobLaunch::batch_challenge(s.stream, (const uint8_t*)d_commitments48, (const uint8_t*)d_zs, (const uint8_t*)d_ys,
                                (const uint8_t*)d_proofs48, (uint32_t)n, s.pow.p, s.chal.template as<uint32_t>());
    HIPCHK(hipMemcpyAsync(w, s.chal.p, 32, hipMemcpyDeviceToHost, s.stream));
    return 0;
  }));
  words_be(w, r_out);
  return 0;
}

int kzgmi_verify_blob_batch_device_async(kzgmi_ctx* c, const kzgmi_srs* srs, int slot, const void* d_blobs,
                                         const void* d_commitments48, const void* d_proofs48, size_t n) {
  KZ_ROUTE(c, &srs, slot);
  CHK(check_ctx(c, slot));
  if (!srs || srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (srs->curve != 0) return fail(KZGMI_ERR_ARG, "blob verification is BLS12-381 only");
  if (n && (!d_blobs || !d_commitments48 || !d_proofs48)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (n == 0) return arm_empty(s, JobKind::Verdict);  // accepts
  Roctx rx("kzgmi_verify_blob_batch_device_async");
  CHK(ensure_blob_table(c, s.stream));
  return HostCore<Bls12_381>::enqueue_batch(c, s, srs, d_commitments48, nullptr, nullptr, d_proofs48, n, Seed{}, 0, nullptr,
                                            kBlobFlags, d_blobs);
}

int kzgmi_verify_blob_batch_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* d_blobs,
                                   const void* d_commitments48, const void* d_proofs48, size_t n, int* ok_out) {
  return run_sync(
      c, [&] { return kzgmi_verify_blob_batch_device_async(c, srs, 0, d_blobs, d_commitments48, d_proofs48, n); }, ok_out);
}

int kzgmi_verify_blob_batch(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* blobs, const uint8_t* commitments48,
                            const uint8_t* proofs48, size_t n, int* ok_out) {
  CHK(check_ctx(c));
  if (!srs || !ok_out) return fail(KZGMI_ERR_ARG, "null argument");
  if (srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (srs->curve != 0) return fail(KZGMI_ERR_ARG, "blob verification is BLS12-381 only");
  if (n && (!blobs || !commitments48 || !proofs48)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  uint8_t* d[3] = {};  // blobs, commitments, proofs in the slot's stage buffer
  const StageItem items[3] = {{blobs, n * BlobLaunch::BYTES}, {commitments48, n * 48}, {proofs48, n * 48}};
  if (n) CHK(stage_host(c, s, items, 3, d));
  return kzgmi_verify_blob_batch_device(c, srs, d[0], d[1], d[2], n, ok_out);
}

// ------------------------------------------------------------------------------ EIP-7594 cells
}  // extern "C"
namespace {
constexpr size_t kCellMax = size_t(1) << 20;  // cells (and unique commitments) per call

Seed seed_of(const uint8_t* r32) {
  uint8_t sb[32];
  if (r32) return make_seed(r32, sb);
  return Seed{};
}
}  // namespace
extern "C" {

void kzgmi_cell_srs_free(kzgmi_cell_srs* cs) {
  if (!cs) return;
  for (kzgmi_cell_srs* p : cs->peers) {
    p->srs = nullptr;  // the inner SRS of a peer is a peer of this one's inner SRS: freed with it
    kzgmi_cell_srs_free(p);
  }
  cs->peers.clear();
  if (kzgmi_ctx* c = cs->ctx) {
    (void)hipSetDevice(c->device);
    auto& v = c->cell_srs_list;
    v.erase(std::remove(v.begin(), v.end(), cs), v.end());
    cs->pts.release();
    cs->inf.release();
  }
  kzgmi_srs_free(cs->srs);
  delete cs;
}

int kzgmi_cell_srs_load(kzgmi_ctx* c, const uint8_t* g1_monomial, const uint8_t* g2, const uint8_t* tau64_g2,
                        kzgmi_cell_srs** out) {
  CHK(check_ctx(c));
  if (!g1_monomial || !g2 || !tau64_g2 || !out) return fail(KZGMI_ERR_ARG, "null cell srs argument");
  *out = nullptr;
  CHK(slot0_idle(c));
  using Cv = Bls12_381;
  using L = Launch<Cv>;
  constexpr uint32_t T = CellLaunch::TERMS;
  kzgmi_srs* inner = nullptr;
  CHK(kzgmi_srs_load(c, KZGMI_BLS12_381, g1_monomial, g2, tau64_g2, &inner));  // ([tau^0]_1, [1]_2, [tau^64]_2)
  // every device of a multi-device context gets its own copy of the 64 points
  std::vector<kzgmi_cell_srs*> made;
  auto undo = [&](int rc) {
    for (kzgmi_cell_srs* m : made) {
      m->srs = nullptr;
      m->peers.clear();
      kzgmi_cell_srs_free(m);
    }
    kzgmi_srs_free(inner);
    return rc;
  };
  for (size_t d = 0; d <= c->peers.size(); ++d) {
    kzgmi_ctx* dc = dev_ctx(c, (int)d);
    if (int r = set_dev(dc)) return undo(r);
    Slot& s = dc->slots[0];
    kzgmi_cell_srs* cs = new kzgmi_cell_srs();
    cs->ctx = dc;
    cs->srs = d == 0 ? inner : inner->peers[d - 1];
    dc->cell_srs_list.push_back(cs);
    made.push_back(cs);
    int r = 0;
    if ((r = s.stage.ensure(T * 96)) || (r = s.flags.ensure(16)) || (r = cs->pts.ensure(2 * T * sizeof(Affine<Cv>))) ||
        (r = cs->inf.ensure(2 * T)) || (r = begin_job(s)))
      return undo(r);
    hipStream_t st = s.stream;
    Affine<Cv>* pts = cs->pts.template as<Affine<Cv>>();
    uint8_t* inf = cs->inf.template as<uint8_t>();
    uint8_t inf_h[T] = {};
    bool okk = hipMemcpyAsync(s.stage.p, g1_monomial, T * 96, hipMemcpyHostToDevice, st) == hipSuccess &&
               hipMemsetAsync(s.flags.p, 0, 16, st) == hipSuccess;
    if (okk) {  // validated like any input point, and in G1 (GLV and the check rely on it)
      uint32_t* err = s.flags.template as<uint32_t>() + 1;
      L::convert_points(st, s.stage.template as<uint8_t>(), T, pts, inf, err);
      L::subgroup_check(st, pts, inf, T, err);
      L::endo_points(st, pts, inf, T, pts + T, inf + T, false);
      okk = hipGetLastError() == hipSuccess &&
            hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipMemcpyAsync(inf_h, inf, T, hipMemcpyDeviceToHost, st) == hipSuccess && sync_job(s) == 0;
    }
    if (!okk) return undo(fail(KZGMI_ERR_DEVICE, "cell srs upload failed"));
    int e = map_device_err((uint32_t)s.host_flags[1]);
    for (uint32_t k = 0; !e && k < T; ++k)
      if (inf_h[k]) e = fail(KZGMI_ERR_ARG, "cell SRS G1 element is the point at infinity");
    if (e) return undo(e);
  }
  for (size_t d = 1; d < made.size(); ++d) made[0]->peers.push_back(made[d]);
  *out = made[0];
  return set_dev(c);
}

int kzgmi_cell_batch_challenge_device(kzgmi_ctx* c, const void* d_commitments48, size_t m,
                                      const void* d_commitment_indices, const void* d_cell_indices,
                                      const void* d_cells, const void* d_proofs48, size_t n, uint8_t r_out[32]) {
  CHK(check_ctx(c));
  if (!r_out || (m && !d_commitments48) || (n && (!d_commitment_indices || !d_cell_indices || !d_cells || !d_proofs48)))
    return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kCellMax || m > kCellMax) return fail(KZGMI_ERR_ARG, "too many cells (max 2^20 per call)");
  uint32_t w[8];
  CHK(cell_slot0_job(c, [&](Slot& s, uint32_t*) -> int {
    CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<Bls12_381::FrP>)));
    CHK(s.chal.ensure(32));
    CellLaunch::batch_challenge(s.stream, (const uint8_t*)d_commitments48, (uint32_t)m, d_commitment_indices,
                                d_cell_indices, (const uint8_t*)d_cells, (const uint8_t*)d_proofs48, (uint32_t)n,
                                s.pow.p, s.chal.template as<uint32_t>());
    HIPCHK(hipMemcpyAsync(w, s.chal.p, 32, hipMemcpyDeviceToHost, s.stream));
    return 0;
  }));
  words_be(w, r_out);
  return 0;
}

int kzgmi_cell_interp_device(kzgmi_ctx* c, const void* d_cell_indices, const void* d_cells, size_t n,
                             const uint8_t r32[32], void* d_coeffs_out) {
  CHK(check_ctx(c));
  if (!r32 || !d_coeffs_out || (n && (!d_cell_indices || !d_cells))) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kCellMax) return fail(KZGMI_ERR_ARG, "too many cells (max 2^20 per call)");
  using L = Launch<Bls12_381>;
  const Seed seed = seed_of(r32);
  return cell_slot0_job(c, [&](Slot& s, uint32_t* err) -> int {
    const uint32_t nn = (uint32_t)n;
    CHK(s.pow.ensure(FS_POW_BITS * sizeof(Fp<Bls12_381::FrP>)));
    CHK(s.blob_z.ensure(n * 32));
    CHK(s.blob_y.ensure(n * 32));
    CHK(s.scal_r.ensure(n * 32));
    CHK(s.scal_s.ensure(n * 32));
    CHK(s.scal_t.ensure(32));
    CHK(s.tpart.ensure(L::tpart_bytes(nn)));
    CHK(s.cell_part.ensure(CellLaunch::part_bytes()));
    CHK(s.cell_coef.ensure(CellLaunch::TERMS * 32));
    hipStream_t st = s.stream;
    L::pow_table(st, seed, s.pow.p, err);
    if (n) {  // r^k through the batch path's own kernel (z_k, y_k as the batch has them)
      CellLaunch::z(st, d_cell_indices, nullptr, nn, 0, c->cell_table.p, s.blob_z.template as<uint8_t>(),
                    s.blob_y.template as<uint8_t>(), err);
      L::scalar_prep_pow(st, s.pow.p, 0, s.blob_z.template as<uint8_t>(), s.blob_y.template as<uint8_t>(), nn,
                         s.scal_r.template as<uint32_t>(), s.scal_s.template as<uint32_t>(), s.tpart.p,
                         s.scal_t.template as<uint32_t>(), err);
    }
    CellLaunch::interp(st, d_cell_indices, (const uint8_t*)d_cells, s.scal_r.template as<uint32_t>(), nn,
                       c->cell_table.p, s.cell_part.p, s.cell_coef.template as<uint32_t>(), (uint8_t*)d_coeffs_out, err);
    return 0;
  });
}

int kzgmi_verify_cell_batch_device_async(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, int slot,
                                         const void* d_commitments48, size_t m, const void* d_commitment_indices,
                                         const void* d_cell_indices, const void* d_cells, const void* d_proofs48,
                                         size_t n, const uint8_t* r32) {
  if (!c) return fail(KZGMI_ERR_ARG, "null context");
  if (!is_cell_srs(c, csrs)) return fail(KZGMI_ERR_ARG, "not a cell srs of this context (kzgmi_cell_srs_load)");
  {
    kzgmi_ctx* c0 = c;
    const int slot0 = slot;
    KZ_ROUTE(c, nullptr, slot);
    if (c != c0) {  // a peer device of a multi-device context: its copy of the SRS
      const int D = 1 + (int)c0->peers.size();
      if (csrs->peers.size() != c0->peers.size()) return fail(KZGMI_ERR_ARG, "cell srs does not belong to this context");
      csrs = csrs->peers[slot0 % D - 1];
    }
    CHK(check_ctx(c, slot));
    if (n && (!d_commitments48 || !d_commitment_indices || !d_cell_indices || !d_cells || !d_proofs48))
      return fail(KZGMI_ERR_ARG, "null input");
    if (n > kCellMax || m > kCellMax) return fail(KZGMI_ERR_ARG, "too many cells (max 2^20 per call)");
    if (n && !m) return fail(KZGMI_ERR_ARG, "cells without commitments");
    Slot& s = c->slots[slot];
    if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
    if (n == 0) return arm_empty(s, JobKind::Verdict);  // accepts
    Roctx rx("kzgmi_verify_cell_batch_device_async");
    CHK(ensure_cell_table(c, s.stream));
    const CellJob job{csrs, d_commitment_indices, d_cell_indices, d_cells, m, r32 == nullptr};
    return HostCore<Bls12_381>::enqueue_batch(c, s, csrs->srs, d_commitments48, nullptr, nullptr, d_proofs48, n, seed_of(r32), 0,
                                              nullptr, kBlobFlags, nullptr, &job);
  }
}

int kzgmi_verify_cell_batch_device(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, const void* d_commitments48, size_t m,
                                   const void* d_commitment_indices, const void* d_cell_indices, const void* d_cells,
                                   const void* d_proofs48, size_t n, const uint8_t* r32, int* ok_out) {
  return run_sync(c, [&] {
    return kzgmi_verify_cell_batch_device_async(c, csrs, 0, d_commitments48, m, d_commitment_indices, d_cell_indices,
                                                d_cells, d_proofs48, n, r32);
  }, ok_out);
}

int kzgmi_verify_cell_batch(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, const uint8_t* commitments48, size_t m,
                            const uint64_t* commitment_indices, const uint64_t* cell_indices, const uint8_t* cells,
                            const uint8_t* proofs48, size_t n, const uint8_t* r32, int* ok_out) {
  CHK(check_ctx(c));
  if (!ok_out) return fail(KZGMI_ERR_ARG, "null argument");
  if (!is_cell_srs(c, csrs)) return fail(KZGMI_ERR_ARG, "not a cell srs of this context (kzgmi_cell_srs_load)");
  if (n && (!commitments48 || !commitment_indices || !cell_indices || !cells || !proofs48))
    return fail(KZGMI_ERR_ARG, "null input");
  if (n > kCellMax || m > kCellMax) return fail(KZGMI_ERR_ARG, "too many cells (max 2^20 per call)");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  uint8_t* d[6] = {};  // the five arrays in the slot's stage buffer, then 16 bytes of slack
  const StageItem items[6] = {{commitments48, 48 * m}, {commitment_indices, 8 * n}, {cell_indices, 8 * n},
                              {cells, n * CellLaunch::BYTES}, {proofs48, 48 * n}, {nullptr, 16}};
  if (n) CHK(stage_host(c, s, items, 6, d));
  return kzgmi_verify_cell_batch_device(c, csrs, d[0], m, d[1], d[2], d[3], d[4], n, r32, ok_out);
}

// ------------------------------------------------------------------------------ EIP-7594 cell extension / recovery
}  // extern "C"
namespace {
constexpr size_t kRecoverMaxBlobs = 4096;  // blobs per call: 256 KiB of output each

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// The argument checks every form shares; d_idx == nullptr: compute_cells (in: nb blobs), else
// recover_cells (in: nb x k cells)
int check_cells_args(const void* d_idx, size_t k, const void* d_in, size_t nb, const void* d_out, bool device) {
  if (d_idx && (k < RecoverLaunch::MIN_CELLS || k > RecoverLaunch::MAX_CELLS))
    return fail(KZGMI_ERR_ARG, "recover_cells takes 64 to 128 cells per blob");
  if (nb > kRecoverMaxBlobs) return fail(KZGMI_ERR_ARG, "too many blobs (max 4096 per call)");
  if (nb && (!d_in || !d_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device || nb == 0) return 0;
  if (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_idx) & 15) return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t in_bytes = nb * (d_idx ? k * CellLaunch::BYTES : BlobLaunch::BYTES);
  if (ranges_overlap(d_in, in_bytes, d_out, nb * RecoverLaunch::OUT_BYTES) ||
      (d_idx && ranges_overlap(d_idx, 8 * k, d_out, nb * RecoverLaunch::OUT_BYTES)))
    return fail(KZGMI_ERR_ARG, "the output overlaps an input");
  return 0;
}

constexpr size_t kFftMax = 4096;  // transforms per kzgmi_g1_fft128_device call

// The argument checks every proof form shares; d_idx == nullptr: compute (in: nb blobs, the cells
// optional), else recover (in: nb x k cells, the cells required)
int check_proofs_args(const void* d_idx, size_t k, const void* d_in, size_t nb, const void* d_cells,
                      const void* d_proofs, bool device) {
  if (d_idx || d_cells) {
    CHK(check_cells_args(d_idx, k, d_in, nb, d_cells, device));
  } else {
    if (nb > kRecoverMaxBlobs) return fail(KZGMI_ERR_ARG, "too many blobs (max 4096 per call)");
    if (nb && !d_in) return fail(KZGMI_ERR_ARG, "null argument");
  }
  if (nb && !d_proofs) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device || nb == 0) return 0;
  if (((uintptr_t)d_in | (uintptr_t)d_proofs) & 15) return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t in_bytes = nb * (d_idx ? k * CellLaunch::BYTES : BlobLaunch::BYTES), pf = nb * Fk20Launch::PROOFS_BYTES;
  if (ranges_overlap(d_in, in_bytes, d_proofs, pf) || (d_idx && ranges_overlap(d_idx, 8 * k, d_proofs, pf)) ||
      (d_cells && ranges_overlap(d_cells, nb * RecoverLaunch::OUT_BYTES, d_proofs, pf)))
    return fail(KZGMI_ERR_ARG, "the output overlaps an input or the other output");
  return 0;
}

int check_cell_pk(const kzgmi_ctx* c, const kzgmi_cell_pk* pk) {
  if (!pk || std::find(c->cell_pk_list.begin(), c->cell_pk_list.end(), pk) == c->cell_pk_list.end())
    return fail(KZGMI_ERR_ARG, "not a cell proof key of this context (kzgmi_cell_pk_load)");
  return 0;
}

// One extension / recovery job on slot s (any slot): completes with kzgmi_slot_wait like a partial
// job, its kernels reporting through the slot's error word.  d_idx: nb x k cells are recovered into
// d_cells; else nb blobs are extended into d_cells (where given).  With a proof key (of this
// device) the FK20 pipeline follows into d_proofs, on the blobs or on the first half of every
// recovered blob.
int enqueue_cells_job(kzgmi_ctx* c, Slot& s, const kzgmi_cell_pk* pk, const void* d_idx, size_t k, const void* d_in,
                      size_t nb, void* d_cells, void* d_proofs) {
  using L = Launch<Bls12_381>;
  using XY = Xyzz<Bls12_381>;
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (nb == 0) return arm_empty(s, JobKind::Utility, 0);  // succeeds, writes nothing
  const uint32_t n = (uint32_t)nb, np = n * Fk20Launch::N;
  CHK(s.flags.ensure(16));
  if (pk) {
    CHK(s.fk_coef.ensure(Fk20Launch::coef_bytes(n)));
    CHK(s.fk_scal.ensure(Fk20Launch::scal_bytes(n)));
    CHK(s.fk_a.ensure((size_t)np * sizeof(XY)));
    CHK(s.fk_b.ensure((size_t)np * sizeof(XY)));
    CHK(s.fk_enc.ensure((size_t)np * (96 + 48)));
  }
  if (d_idx) {
    CHK(s.rec_z.ensure(RecoverLaunch::z_bytes()));
    CHK(ensure_cell_table(c, s.stream));
  }
  CHK(ensure_ntt_table(c, s.stream));
  CHK(begin_job(s));
  hipStream_t st = s.stream;
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  const uint8_t* blobs = (const uint8_t*)d_in;
  size_t stride = BlobLaunch::BYTES;
  if (d_idx) {
    RecoverLaunch::recover(st, d_idx, (uint32_t)k, (const uint8_t*)d_in, n, c->cell_table.p, c->ntt_table.p,
                           s.rec_z.p, (uint8_t*)d_cells, err);
    blobs = (const uint8_t*)d_cells;  // cells 0..63 are the blob's bytes
    stride = RecoverLaunch::OUT_BYTES;
  } else if (d_cells) {
    RecoverLaunch::compute(st, blobs, n, c->ntt_table.p, (uint8_t*)d_cells, err);
  }
  if (pk) {
    uint8_t* scal = s.fk_scal.template as<uint8_t>();
    XY* a = s.fk_a.template as<XY>();
    XY* b = s.fk_b.template as<XY>();
    uint8_t* enc = s.fk_enc.template as<uint8_t>();
    uint8_t* enc48 = enc + (size_t)np * 96;
    Fk20Launch::scalars(st, blobs, stride, n, c->ntt_table.p, true, s.fk_coef.p, scal, err);
    Fk20Launch::msm(st, scal, n, pk->tab.p, pk->tab_inf.template as<uint8_t>(), a);
    Fk20Launch::fft(st, a, n, c->ntt_table.p, true);
    Fk20Launch::shift(st, a, n, b);
    Fk20Launch::fft(st, b, n, c->ntt_table.p, false);
    L::encode_points(st, b, np, enc);
    L::compress_points(st, enc, np, enc48);
    Fk20Launch::emit(st, enc48, (size_t)np * 48, err, d_proofs);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Utility, 0);
  return 0;
}

// The host form of each (idx == nullptr: from blobs; proofs: with cell proofs, the cells then
// optional): [indices | input | cells | proofs] in slot 0's stage buffer, the results copied back
int cells_host(kzgmi_ctx* c, bool proofs, const kzgmi_cell_pk* pk, const uint64_t* idx, size_t k, const uint8_t* in,
               size_t nb, uint8_t* cells_out, uint8_t* proofs_out) {
  CHK(check_ctx(c));
  if (proofs) {
    CHK(check_cell_pk(c, pk));
    CHK(check_proofs_args(idx, k, in, nb, cells_out, proofs_out, false));
  } else {
    CHK(check_cells_args(idx, k, in, nb, cells_out, false));
  }
  CHK(slot0_idle(c));
  if (nb == 0) return 0;
  Slot& s = c->slots[0];
  const size_t in_bytes = nb * (idx ? k * CellLaunch::BYTES : BlobLaunch::BYTES);
  const size_t cell_bytes = cells_out ? nb * RecoverLaunch::OUT_BYTES : 0, pf = proofs ? nb * Fk20Launch::PROOFS_BYTES : 0;
  const StageItem items[4] = {{idx, 8 * k}, {in, in_bytes}, {nullptr, cell_bytes}, {nullptr, pf}};
  uint8_t* d[4];
  CHK(stage_host(c, s, items, 4, d));
  CHK(enqueue_cells_job(c, s, proofs ? pk : nullptr, idx ? d[0] : nullptr, k, d[1], nb, cells_out ? d[2] : nullptr, d[3]));
  CHK(finish_slot(c, s, nullptr));
  if (cells_out) HIPCHK(hipMemcpy(cells_out, d[2], cell_bytes, hipMemcpyDeviceToHost));
  if (proofs) HIPCHK(hipMemcpy(proofs_out, d[3], pf, hipMemcpyDeviceToHost));
  return 0;
}

// The synchronous device form of each: its async form on slot 0 (idle on every device), waited for
template <class F>
int run_slot0(kzgmi_ctx* c, F&& enqueue) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(enqueue());
  return kzgmi_slot_wait(c, 0, nullptr);
}
}  // namespace
extern "C" {

int kzgmi_compute_cells_device_async(kzgmi_ctx* c, int slot, const void* d_blobs, size_t nb, void* d_cells_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  CHK(check_cells_args(nullptr, 0, d_blobs, nb, d_cells_out, true));
  Roctx rx("kzgmi_compute_cells_device_async");
  return enqueue_cells_job(c, c->slots[slot], nullptr, nullptr, 0, d_blobs, nb, d_cells_out, nullptr);
}

int kzgmi_compute_cells_device(kzgmi_ctx* c, const void* d_blobs, size_t nb, void* d_cells_out) {
  return run_slot0(c, [&] { return kzgmi_compute_cells_device_async(c, 0, d_blobs, nb, d_cells_out); });
}

int kzgmi_compute_cells(kzgmi_ctx* c, const uint8_t* blobs, size_t nb, uint8_t* cells_out) {
  return cells_host(c, false, nullptr, nullptr, 0, blobs, nb, cells_out, nullptr);
}

int kzgmi_recover_cells_device_async(kzgmi_ctx* c, int slot, const void* d_cell_indices, size_t k, const void* d_cells,
                                     size_t nb, void* d_cells_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  if (!d_cell_indices) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(check_cells_args(d_cell_indices, k, d_cells, nb, d_cells_out, true));
  Roctx rx("kzgmi_recover_cells_device_async");
  return enqueue_cells_job(c, c->slots[slot], nullptr, d_cell_indices, k, d_cells, nb, d_cells_out, nullptr);
}

int kzgmi_recover_cells_device(kzgmi_ctx* c, const void* d_cell_indices, size_t k, const void* d_cells, size_t nb,
                               void* d_cells_out) {
  return run_slot0(c, [&] { return kzgmi_recover_cells_device_async(c, 0, d_cell_indices, k, d_cells, nb, d_cells_out); });
}

int kzgmi_recover_cells(kzgmi_ctx* c, const uint64_t* cell_indices, size_t k, const uint8_t* cells, size_t nb,
                        uint8_t* cells_out) {
  if (!cell_indices) return fail(KZGMI_ERR_ARG, "null argument");
  return cells_host(c, false, nullptr, cell_indices, k, cells, nb, cells_out, nullptr);
}

// ------------------------------------------------------------------------------ EIP-7594 cell proofs (FK20)

void kzgmi_cell_pk_free(kzgmi_cell_pk* pk) {
  if (!pk) return;
  if (kzgmi_ctx* c = pk->ctx) {
    (void)hipSetDevice(c->device);
    auto& v = c->cell_pk_list;
    v.erase(std::remove(v.begin(), v.end(), pk), v.end());
    pk->tab.release();
    pk->tab_inf.release();
  }
  delete pk;
}

size_t kzgmi_cell_pk_device_bytes(const kzgmi_cell_pk* pk) { return pk ? pk->tab.cap + pk->tab_inf.cap : 0; }

int kzgmi_cell_pk_load(kzgmi_ctx* c, const uint8_t* g1_monomial, kzgmi_cell_pk** out) {
  CHK(check_ctx(c));
  if (!g1_monomial || !out) return fail(KZGMI_ERR_ARG, "null cell proof key argument");
  *out = nullptr;
  CHK(slot0_idle(c));
  using Cv = Bls12_381;
  using L = Launch<Cv>;
  using XY = Xyzz<Cv>;
  constexpr uint32_t T = Fk20Launch::SRS_POINTS;
  Slot& s = c->slots[0];
  CHK(ensure_ntt_table(c, s.stream));
  kzgmi_cell_pk* pk = new kzgmi_cell_pk();
  DevBuf pts, inf, x;  // the validated SRS and the 64 vectors x^(b): needed while the table is built
  auto undo = [&](int rc) {
    pts.release();
    inf.release();
    x.release();
    pk->tab.release();
    pk->tab_inf.release();
    delete pk;
    return rc;
  };
  int r = 0;
  if ((r = s.stage.ensure(T * 96)) || (r = s.flags.ensure(16)) || (r = pts.ensure(T * sizeof(Affine<Cv>))) ||
      (r = inf.ensure(T)) || (r = x.ensure((size_t)Fk20Launch::KEY_TRANSFORMS * Fk20Launch::N * sizeof(XY))) ||
      (r = pk->tab.ensure(Fk20Launch::table_bytes())) || (r = pk->tab_inf.ensure(Fk20Launch::table_flags())) ||
      (r = begin_job(s)))
    return undo(r);
  hipStream_t st = s.stream;
  std::vector<uint8_t> inf_h(T);
  bool okk = hipMemcpyAsync(s.stage.p, g1_monomial, T * 96, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemsetAsync(s.flags.p, 0, 16, st) == hipSuccess;
  if (okk) {  // validated like any input point, and in G1 (the table's rows rely on the order r)
    uint32_t* err = s.flags.template as<uint32_t>() + 1;
    Affine<Cv>* p = pts.template as<Affine<Cv>>();
    L::convert_points(st, s.stage.template as<uint8_t>(), T, p, inf.template as<uint8_t>(), err);
    L::subgroup_check(st, p, inf.template as<uint8_t>(), T, err);
    Fk20Launch::key(st, p, c->ntt_table.p, x.template as<XY>(), pk->tab.p, pk->tab_inf.template as<uint8_t>());
    okk = hipGetLastError() == hipSuccess &&
          hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(inf_h.data(), inf.p, T, hipMemcpyDeviceToHost, st) == hipSuccess && sync_job(s) == 0;
  }
  if (!okk) return undo(fail(KZGMI_ERR_DEVICE, "cell proof key upload/precompute failed"));
  int e = map_device_err((uint32_t)s.host_flags[1]);
  for (uint32_t k = 0; !e && k < T; ++k)
    if (inf_h[k]) e = fail(KZGMI_ERR_ARG, "cell SRS G1 element is the point at infinity");
  if (e) return undo(e);
  pts.release();
  inf.release();
  x.release();
  pk->ctx = c;
  c->cell_pk_list.push_back(pk);
  *out = pk;
  return 0;
}

int kzgmi_compute_cells_and_proofs_device_async(kzgmi_ctx* c, const kzgmi_cell_pk* pk, int slot, const void* d_blobs,
                                                size_t nb, void* d_cells_out, void* d_proofs_out) {
  KZ_ROUTE(c, nullptr, slot);  // (proof keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  CHK(check_cell_pk(c, pk));
  CHK(check_proofs_args(nullptr, 0, d_blobs, nb, d_cells_out, d_proofs_out, true));
  Roctx rx("kzgmi_compute_cells_and_proofs_device_async");
  return enqueue_cells_job(c, c->slots[slot], pk, nullptr, 0, d_blobs, nb, d_cells_out, d_proofs_out);
}

int kzgmi_compute_cells_and_proofs_device(kzgmi_ctx* c, const kzgmi_cell_pk* pk, const void* d_blobs, size_t nb,
                                          void* d_cells_out, void* d_proofs_out) {
  return run_slot0(
      c, [&] { return kzgmi_compute_cells_and_proofs_device_async(c, pk, 0, d_blobs, nb, d_cells_out, d_proofs_out); });
}

int kzgmi_compute_cells_and_proofs(kzgmi_ctx* c, const kzgmi_cell_pk* pk, const uint8_t* blobs, size_t nb,
                                   uint8_t* cells_out, uint8_t* proofs_out) {
  return cells_host(c, true, pk, nullptr, 0, blobs, nb, cells_out, proofs_out);
}

int kzgmi_recover_cells_and_proofs_device_async(kzgmi_ctx* c, const kzgmi_cell_pk* pk, int slot,
                                                const void* d_cell_indices, size_t k, const void* d_cells, size_t nb,
                                                void* d_cells_out, void* d_proofs_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  CHK(check_cell_pk(c, pk));
  if (!d_cell_indices) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(check_proofs_args(d_cell_indices, k, d_cells, nb, d_cells_out, d_proofs_out, true));
  Roctx rx("kzgmi_recover_cells_and_proofs_device_async");
  return enqueue_cells_job(c, c->slots[slot], pk, d_cell_indices, k, d_cells, nb, d_cells_out, d_proofs_out);
}

int kzgmi_recover_cells_and_proofs_device(kzgmi_ctx* c, const kzgmi_cell_pk* pk, const void* d_cell_indices, size_t k,
                                          const void* d_cells, size_t nb, void* d_cells_out, void* d_proofs_out) {
  return run_slot0(c, [&] {
    return kzgmi_recover_cells_and_proofs_device_async(c, pk, 0, d_cell_indices, k, d_cells, nb, d_cells_out, d_proofs_out);
  });
}

int kzgmi_recover_cells_and_proofs(kzgmi_ctx* c, const kzgmi_cell_pk* pk, const uint64_t* cell_indices, size_t k,
                                   const uint8_t* cells, size_t nb, uint8_t* cells_out, uint8_t* proofs_out) {
  if (!cell_indices) return fail(KZGMI_ERR_ARG, "null argument");
  return cells_host(c, true, pk, cell_indices, k, cells, nb, cells_out, proofs_out);
}

int kzgmi_fk20_scalars_device(kzgmi_ctx* c, const void* d_blobs, size_t nb, void* d_out) {
  CHK(check_ctx(c));
  if (nb && (!d_blobs || !d_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (nb > kRecoverMaxBlobs) return fail(KZGMI_ERR_ARG, "too many blobs (max 4096 per call)");
  if (((uintptr_t)d_blobs | (uintptr_t)d_out) & 15) return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  CHK(slot0_idle(c));
  CHK(ensure_ntt_table(c, c->slots[0].stream));
  return cell_slot0_job(c, [&](Slot& s, uint32_t* err) -> int {
    CHK(s.fk_coef.ensure(Fk20Launch::coef_bytes((uint32_t)nb)));
    Fk20Launch::scalars(s.stream, (const uint8_t*)d_blobs, BlobLaunch::BYTES, (uint32_t)nb, c->ntt_table.p, false,
                        s.fk_coef.p, (uint8_t*)d_out, err);
    return 0;
  });
}

int kzgmi_g1_fft128_device(kzgmi_ctx* c, const void* d_points96, size_t count, int inverse, void* d_out96) {
  CHK(check_ctx(c));
  if (count && (!d_points96 || !d_out96)) return fail(KZGMI_ERR_ARG, "null argument");
  if (count > kFftMax) return fail(KZGMI_ERR_ARG, "too many transforms (max 4096 per call)");
  if (((uintptr_t)d_points96 | (uintptr_t)d_out96) & 15) return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  CHK(slot0_idle(c));
  CHK(ensure_ntt_table(c, c->slots[0].stream));
  using Cv = Bls12_381;
  using L = Launch<Cv>;
  using XY = Xyzz<Cv>;
  return cell_slot0_job(c, [&](Slot& s, uint32_t* err) -> int {
    const uint32_t cnt = (uint32_t)count, n = cnt * Fk20Launch::N;
    if (!n) return 0;
    CHK(s.pts.ensure((size_t)n * sizeof(Affine<Cv>)));
    CHK(s.inf.ensure(n));
    CHK(s.fk_a.ensure((size_t)n * sizeof(XY)));
    CHK(s.fk_b.ensure((size_t)n * sizeof(XY)));
    hipStream_t st = s.stream;
    XY* a = s.fk_a.template as<XY>();
    XY* b = s.fk_b.template as<XY>();
    L::convert_points(st, (const uint8_t*)d_points96, n, s.pts.template as<Affine<Cv>>(), s.inf.template as<uint8_t>(), err);
    Fk20Launch::from_affine(st, s.pts.template as<Affine<Cv>>(), s.inf.template as<uint8_t>(), n, a);
    Fk20Launch::fft(st, a, cnt, c->ntt_table.p, inverse != 0);
    if (inverse) Fk20Launch::scale128(st, a, n);
    Fk20Launch::unrev(st, a, cnt, b);
    L::encode_points(st, b, n, (uint8_t*)d_out96);
    return 0;
  });
}

// ------------------------------------------------------------------------------ EIP-4844 commitments and proofs
}  // extern "C"
namespace {
// blob_to_kzg_commitment; compute_kzg_proof (in2 = zs, out2 = ys); compute_blob_kzg_proof (in2 = commitments)
enum class BlobOp { Commit, Proofs, BlobProofs };

int check_blob_pk(const kzgmi_ctx* c, const kzgmi_blob_pk* pk) {
  if (!pk || std::find(c->blob_pk_list.begin(), c->blob_pk_list.end(), pk) == c->blob_pk_list.end())
    return fail(KZGMI_ERR_ARG, "not a blob proof key of this context (kzgmi_blob_pk_load)");
  return 0;
}

size_t blob_in2_bytes(BlobOp op, size_t nb) { return op == BlobOp::Proofs ? 32 * nb : op == BlobOp::BlobProofs ? 48 * nb : 0; }
size_t blob_out2_bytes(BlobOp op, size_t nb) { return op == BlobOp::Proofs ? 32 * nb : 0; }

// The argument checks every form shares
int check_blob_args(BlobOp op, const void* d_blobs, const void* d_in2, size_t nb, const void* d_out, const void* d_out2,
                    bool device) {
  if (nb > kRecoverMaxBlobs) return fail(KZGMI_ERR_ARG, "too many blobs (max 4096 per call)");
  const size_t in2 = blob_in2_bytes(op, nb), out2 = blob_out2_bytes(op, nb);
  if (nb && (!d_blobs || !d_out || (in2 && !d_in2) || (out2 && !d_out2))) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device || nb == 0) return 0;
  if (((uintptr_t)d_blobs | (uintptr_t)d_out | (in2 ? (uintptr_t)d_in2 : 0) | (out2 ? (uintptr_t)d_out2 : 0)) & 15)
    return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t bb = nb * BlobLaunch::BYTES, ob = 48 * nb;
  if (ranges_overlap(d_blobs, bb, d_out, ob) || (in2 && ranges_overlap(d_in2, in2, d_out, ob)) ||
      (out2 && (ranges_overlap(d_blobs, bb, d_out2, out2) || ranges_overlap(d_in2, in2, d_out2, out2) ||
                ranges_overlap(d_out, ob, d_out2, out2))))
    return fail(KZGMI_ERR_ARG, "the output overlaps an input or the other output");
  return 0;
}

// One commitment / proof job on slot s (any slot of the key's device): completes with kzgmi_slot_wait
// like enqueue_cells_job, its kernels reporting through the slot's error word.  d_out (nb x 48 B) and
// d_out2 are written by the emit kernels only, which write nothing once an error is raised.
int enqueue_blob_job(kzgmi_ctx* c, Slot& s, const kzgmi_blob_pk* pk, BlobOp op, const void* d_blobs, const void* d_in2,
                     size_t nb, void* d_out, void* d_out2) {
  using L = Launch<Bls12_381>;
  using XY = Xyzz<Bls12_381>;
  using AF = Affine<Bls12_381>;
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (nb == 0) return arm_empty(s, JobKind::Utility, 0);  // succeeds, writes nothing
  const uint32_t n = (uint32_t)nb;
  CHK(s.flags.ensure(16));
  CHK(s.bp_part.ensure((size_t)n * (BlobProofLaunch::PARTS + 1) * sizeof(XY)));  // the partials, then the sums
  CHK(s.bp_enc.ensure((size_t)n * (96 + 48)));
  if (op != BlobOp::Commit) {
    CHK(s.bp_q.ensure(nb * BlobLaunch::BYTES));
    CHK(s.blob_y.ensure(nb * 32));
    CHK(ensure_blob_table(c, s.stream));
  }
  if (op == BlobOp::BlobProofs) {
    CHK(s.pts.ensure(nb * sizeof(AF)));
    CHK(s.inf.ensure(nb));
    CHK(s.blob_z.ensure(nb * 32));
  }
  CHK(begin_job(s));
  hipStream_t st = s.stream;
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  const uint8_t* blobs = (const uint8_t*)d_blobs;
  const uint8_t* scal = blobs;  // the commitment's scalars are the blob's bytes
  if (op != BlobOp::Commit) {
    const uint8_t* zs = (const uint8_t*)d_in2;
    if (op == BlobOp::BlobProofs) {  // the commitments decoded and checked as a verifier would; z_i from the blob hash
      AF* pts = s.pts.template as<AF>();
      uint8_t* inf = s.inf.template as<uint8_t>();
      L::decompress_points(st, (const uint8_t*)d_in2, n, pts, inf, err);
      L::subgroup_check(st, pts, inf, n, err);
      BlobLaunch::challenges(st, blob_mapping(c, nb), blobs, (const uint8_t*)d_in2, n, s.blob_z.template as<uint8_t>(), err);
      zs = s.blob_z.template as<uint8_t>();
    }
    BlobProofLaunch::quotient(st, blobs, zs, c->blob_table.p, n, op == BlobOp::Proofs, s.blob_y.template as<uint8_t>(),
                              s.bp_q.template as<uint8_t>(), err);
    scal = s.bp_q.template as<uint8_t>();
  }
  XY* parts = s.bp_part.template as<XY>();
  XY* res = parts + (size_t)n * BlobProofLaunch::PARTS;
  uint8_t* enc = s.bp_enc.template as<uint8_t>();
  uint8_t* enc48 = enc + (size_t)n * 96;
  BlobProofLaunch::msm(st, scal, n, op == BlobOp::Commit, pk->tab.p, pk->tab_inf.template as<uint8_t>(), parts, res, err);
  L::encode_points(st, res, n, enc);
  L::compress_points(st, enc, n, enc48);
  Fk20Launch::emit(st, enc48, (size_t)n * 48, err, d_out);
  if (op == BlobOp::Proofs) Fk20Launch::emit(st, s.blob_y.p, (size_t)n * 32, err, d_out2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Utility, 0);
  return 0;
}

int blob_job_async(kzgmi_ctx* c, const kzgmi_blob_pk* pk, int slot, const char* name, BlobOp op, const void* d_blobs,
                   const void* d_in2, size_t nb, void* d_out, void* d_out2) {
  KZ_ROUTE(c, nullptr, slot);  // (proof keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  CHK(check_blob_pk(c, pk));
  CHK(check_blob_args(op, d_blobs, d_in2, nb, d_out, d_out2, true));
  Roctx rx(name);
  return enqueue_blob_job(c, c->slots[slot], pk, op, d_blobs, d_in2, nb, d_out, d_out2);
}

// The host form of each: [blobs | zs or commitments | out | ys] in slot 0's stage buffer, the results copied back
int blob_job_host(kzgmi_ctx* c, const kzgmi_blob_pk* pk, BlobOp op, const uint8_t* blobs, const uint8_t* in2, size_t nb,
                  uint8_t* out, uint8_t* out2) {
  CHK(check_ctx(c));
  CHK(check_blob_pk(c, pk));
  CHK(check_blob_args(op, blobs, in2, nb, out, out2, false));
  CHK(slot0_idle(c));
  if (nb == 0) return 0;
  Slot& s = c->slots[0];
  const size_t ib = blob_in2_bytes(op, nb), ob = blob_out2_bytes(op, nb);
  const StageItem items[4] = {{blobs, nb * BlobLaunch::BYTES}, {ib ? in2 : nullptr, ib}, {nullptr, 48 * nb}, {nullptr, ob}};
  uint8_t* d[4];
  CHK(stage_host(c, s, items, 4, d));
  CHK(enqueue_blob_job(c, s, pk, op, d[0], d[1], nb, d[2], d[3]));
  CHK(finish_slot(c, s, nullptr));
  HIPCHK(hipMemcpy(out, d[2], 48 * nb, hipMemcpyDeviceToHost));
  if (ob) HIPCHK(hipMemcpy(out2, d[3], ob, hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace
extern "C" {

void kzgmi_blob_pk_free(kzgmi_blob_pk* pk) {
  if (!pk) return;
  if (kzgmi_ctx* c = pk->ctx) {
    (void)hipSetDevice(c->device);
    auto& v = c->blob_pk_list;
    v.erase(std::remove(v.begin(), v.end(), pk), v.end());
    pk->tab.release();
    pk->tab_inf.release();
  }
  delete pk;
}

size_t kzgmi_blob_pk_device_bytes(const kzgmi_blob_pk* pk) { return pk ? pk->tab.cap + pk->tab_inf.cap : 0; }

int kzgmi_blob_pk_load(kzgmi_ctx* c, const uint8_t* g1_lagrange, kzgmi_blob_pk** out) {
  CHK(check_ctx(c));
  if (!g1_lagrange || !out) return fail(KZGMI_ERR_ARG, "null blob proof key argument");
  *out = nullptr;
  CHK(slot0_idle(c));
  using Cv = Bls12_381;
  using L = Launch<Cv>;
  constexpr uint32_t T = BlobProofLaunch::POINTS;
  Slot& s = c->slots[0];
  kzgmi_blob_pk* pk = new kzgmi_blob_pk();
  DevBuf pts, inf;  // the validated points: needed while the table is built
  auto undo = [&](int rc) {
    pts.release();
    inf.release();
    pk->tab.release();
    pk->tab_inf.release();
    delete pk;
    return rc;
  };
  int r = 0;
  if ((r = s.stage.ensure(T * 96)) || (r = s.flags.ensure(16)) || (r = pts.ensure(T * sizeof(Affine<Cv>))) ||
      (r = inf.ensure(T)) || (r = pk->tab.ensure(BlobProofLaunch::table_bytes())) ||
      (r = pk->tab_inf.ensure(BlobProofLaunch::table_flags())) || (r = begin_job(s)))
    return undo(r);
  hipStream_t st = s.stream;
  std::vector<uint8_t> inf_h(T);
  bool okk = hipMemcpyAsync(s.stage.p, g1_lagrange, T * 96, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemsetAsync(s.flags.p, 0, 16, st) == hipSuccess;
  if (okk) {  // validated like any input point, and in G1 (the table's rows rely on the order r)
    uint32_t* err = s.flags.template as<uint32_t>() + 1;
    Affine<Cv>* p = pts.template as<Affine<Cv>>();
    L::convert_points(st, s.stage.template as<uint8_t>(), T, p, inf.template as<uint8_t>(), err);
    L::subgroup_check(st, p, inf.template as<uint8_t>(), T, err);
    BlobProofLaunch::key(st, p, inf.template as<uint8_t>(), pk->tab.p, pk->tab_inf.template as<uint8_t>());
    okk = hipGetLastError() == hipSuccess &&
          hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipMemcpyAsync(inf_h.data(), inf.p, T, hipMemcpyDeviceToHost, st) == hipSuccess && sync_job(s) == 0;
  }
  if (!okk) return undo(fail(KZGMI_ERR_DEVICE, "blob proof key upload/precompute failed"));
  int e = map_device_err((uint32_t)s.host_flags[1]);
  for (uint32_t k = 0; !e && k < T; ++k)
    if (inf_h[k]) e = fail(KZGMI_ERR_ARG, "blob proof key G1 element is the point at infinity");
  if (e) return undo(e);
  pts.release();
  inf.release();
  pk->ctx = c;
  c->blob_pk_list.push_back(pk);
  *out = pk;
  return 0;
}

int kzgmi_blob_commit_device_async(kzgmi_ctx* c, const kzgmi_blob_pk* pk, int slot, const void* d_blobs, size_t nb,
                                   void* d_commitments48_out) {
  return blob_job_async(c, pk, slot, "kzgmi_blob_commit_device_async", BlobOp::Commit, d_blobs, nullptr, nb,
                        d_commitments48_out, nullptr);
}

int kzgmi_blob_commit_device(kzgmi_ctx* c, const kzgmi_blob_pk* pk, const void* d_blobs, size_t nb,
                             void* d_commitments48_out) {
  return run_slot0(c, [&] { return kzgmi_blob_commit_device_async(c, pk, 0, d_blobs, nb, d_commitments48_out); });
}

int kzgmi_blob_commit(kzgmi_ctx* c, const kzgmi_blob_pk* pk, const uint8_t* blobs, size_t nb, uint8_t* commitments48_out) {
  return blob_job_host(c, pk, BlobOp::Commit, blobs, nullptr, nb, commitments48_out, nullptr);
}

int kzgmi_compute_kzg_proofs_device_async(kzgmi_ctx* c, const kzgmi_blob_pk* pk, int slot, const void* d_blobs,
                                          const void* d_zs, size_t nb, void* d_proofs48_out, void* d_ys_out) {
  return blob_job_async(c, pk, slot, "kzgmi_compute_kzg_proofs_device_async", BlobOp::Proofs, d_blobs, d_zs, nb,
                        d_proofs48_out, d_ys_out);
}

int kzgmi_compute_kzg_proofs_device(kzgmi_ctx* c, const kzgmi_blob_pk* pk, const void* d_blobs, const void* d_zs,
                                    size_t nb, void* d_proofs48_out, void* d_ys_out) {
  return run_slot0(
      c, [&] { return kzgmi_compute_kzg_proofs_device_async(c, pk, 0, d_blobs, d_zs, nb, d_proofs48_out, d_ys_out); });
}

int kzgmi_compute_kzg_proofs(kzgmi_ctx* c, const kzgmi_blob_pk* pk, const uint8_t* blobs, const uint8_t* zs, size_t nb,
                             uint8_t* proofs48_out, uint8_t* ys_out) {
  return blob_job_host(c, pk, BlobOp::Proofs, blobs, zs, nb, proofs48_out, ys_out);
}

int kzgmi_compute_blob_proofs_device_async(kzgmi_ctx* c, const kzgmi_blob_pk* pk, int slot, const void* d_blobs,
                                           const void* d_commitments48, size_t nb, void* d_proofs48_out) {
  return blob_job_async(c, pk, slot, "kzgmi_compute_blob_proofs_device_async", BlobOp::BlobProofs, d_blobs,
                        d_commitments48, nb, d_proofs48_out, nullptr);
}

int kzgmi_compute_blob_proofs_device(kzgmi_ctx* c, const kzgmi_blob_pk* pk, const void* d_blobs,
                                     const void* d_commitments48, size_t nb, void* d_proofs48_out) {
  return run_slot0(
      c, [&] { return kzgmi_compute_blob_proofs_device_async(c, pk, 0, d_blobs, d_commitments48, nb, d_proofs48_out); });
}

int kzgmi_compute_blob_proofs(kzgmi_ctx* c, const kzgmi_blob_pk* pk, const uint8_t* blobs, const uint8_t* commitments48,
                              size_t nb, uint8_t* proofs48_out) {
  return blob_job_host(c, pk, BlobOp::BlobProofs, blobs, commitments48, nb, proofs48_out, nullptr);
}

int kzgmi_blob_quotient_device(kzgmi_ctx* c, const void* d_blobs, const void* d_zs, size_t nb, void* d_ys_out,
                               void* d_q_out) {
  CHK(check_ctx(c));
  if (nb > kRecoverMaxBlobs) return fail(KZGMI_ERR_ARG, "too many blobs (max 4096 per call)");
  if (nb && (!d_blobs || !d_zs || !d_ys_out || !d_q_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (nb == 0) return 0;
  if (((uintptr_t)d_blobs | (uintptr_t)d_zs | (uintptr_t)d_ys_out | (uintptr_t)d_q_out) & 15)
    return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  return blob_slot0_job(c, [&](Slot& s, uint32_t* err) -> int {
    BlobProofLaunch::quotient(s.stream, (const uint8_t*)d_blobs, (const uint8_t*)d_zs, c->blob_table.p, (uint32_t)nb, true,
                              (uint8_t*)d_ys_out, (uint8_t*)d_q_out, err);
    return 0;
  });
}

}  // extern "C"
