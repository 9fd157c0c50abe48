// Power-of-two transforms over G1 (kzgmi_g1_ntt*) and the openings of a polynomial at every point of
// its domain (kzgmi_open_all*), the FK20 single-proof construction over them.  Kernels: g1ntt.hpp;
// DESIGN.md 3i.  The stages of a transform are a plain loop over its spans (Launch::g1ntt_stages):
// there is nothing to plan but the two gathers the call's order flags ask for, decided here.
// Further down, the openings on every coset of a domain (kzgmi_open_cosets*), FK20 multi-proofs over the same
// transforms.  Kernels: cosets.hpp; DESIGN.md 3j.
#include "host.hpp"

struct kzgmi_open_all_key {
  int curve = 0;
  unsigned logn = 0;
  kzgmi_ctx* ctx = nullptr;
  DevBuf xhat;  // DFT_2n(x), 2n XYZZ records in natural order (infinity: zz = 0)
};

struct kzgmi_open_cosets_key {
  int curve = 0;
  unsigned logN = 0, logl = 0;
  kzgmi_ctx* ctx = nullptr;
  DevBuf xhat;  // DFT_2R(x^(b)) for every b < l, 2N XYZZ records, [pos][b] (infinity: zz = 0)
};

namespace kzgmi {
void open_all_keys_detach(kzgmi_ctx* c) {
  for (kzgmi_open_all_key* key : c->open_all_key_list) {
    key->xhat.release();
    key->ctx = nullptr;
  }
  c->open_all_key_list.clear();
  for (kzgmi_open_cosets_key* key : c->open_cosets_key_list) {
    key->xhat.release();
    key->ctx = nullptr;
  }
  c->open_cosets_key_list.clear();
}
}  // namespace kzgmi

namespace {

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}

template <class Cv>
int ensure_roots(kzgmi_ctx* c, hipStream_t st) {
  using L = Launch<Cv>;
  return ensure_once(c->fr_ntt_table_ready[Cv::ID], c->fr_ntt_table[Cv::ID], L::ntt_table_bytes(), st,
                     [&] { L::ntt_roots(st, c->fr_ntt_table[Cv::ID].p); });
}

int check_g1_ntt_args(int curve, const void* in, const void* out, unsigned logn, size_t count, uint32_t flags, bool device) {
  if (curve != KZGMI_BLS12_381 && curve != KZGMI_BN254) return fail(KZGMI_ERR_ARG, "unknown curve");
  if (logn > G1NTT_MAX_LOGN) return fail(KZGMI_ERR_ARG, "transform too large (max 2^20 points)");
  if (flags & ~(uint32_t)(KZGMI_NTT_INVERSE | KZGMI_NTT_BITREV)) return fail(KZGMI_ERR_ARG, "unknown transform flag");
  if (count > (size_t(1) << (G1NTT_MAX_LOGN - logn))) return fail(KZGMI_ERR_ARG, "too many points (count * n is at most 2^20)");
  if (count == 0) return 0;
  if (!in || !out) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device) return 0;
  if (((uintptr_t)in | (uintptr_t)out) & 15) return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t bytes = g1_bytes(curve) * (count << logn);
  if (in != out && overlap(in, bytes, out, bytes))
    return fail(KZGMI_ERR_ARG, "the output overlaps the input (in place: the same pointer)");
  return 0;
}

// count transforms of 2^logn records in a (natural order; inverse && bitrev_in: already gathered by the
// caller) on st; returns the buffer holding the result in the order the flags ask for (a or b)
template <class Cv>
Xyzz<Cv>* enqueue_transform(kzgmi_ctx* c, hipStream_t st, Xyzz<Cv>* a, Xyzz<Cv>* b, unsigned logn, uint32_t count, uint32_t flags,
                            bool scale) {
  using L = Launch<Cv>;
  const uint32_t total = count << logn;
  const bool inverse = flags & KZGMI_NTT_INVERSE;
  L::g1ntt_stages(st, a, logn, count, inverse, c->fr_ntt_table[Cv::ID].p, c->g1ntt_form);
  if (inverse && scale && logn) L::g1ntt_mul(st, a, nullptr, logn, total, a);
  // the stages leave bit-reversed order: the coefficient side of an inverse is always natural, the
  // evaluation side of a forward transform is as the caller asks
  if (!inverse && (flags & KZGMI_NTT_BITREV)) return a;
  if (logn < 2) return a;  // the reversal of 0 or 1 bits is the identity
  L::g1ntt_rev(st, a, logn, total, b);
  return b;
}

template <class Cv>
int enqueue_g1_ntt_job(kzgmi_ctx* c, Slot& s, const void* d_in, unsigned logn, size_t count, uint32_t flags, void* d_out) {
  using L = Launch<Cv>;
  using XY = Xyzz<Cv>;
  using AF = Affine<Cv>;
  const uint32_t total = (uint32_t)(count << logn);
  const size_t gb = g1_bytes(Cv::ID);
  CHK(s.flags.ensure(16));
  CHK(s.pts.ensure((size_t)total * sizeof(AF)));
  CHK(s.inf.ensure(total));
  CHK(s.g1_a.ensure((size_t)total * sizeof(XY)));
  CHK(s.g1_b.ensure((size_t)total * sizeof(XY)));
  CHK(s.g1_enc.ensure((size_t)total * gb));
  CHK(ensure_roots<Cv>(c, s.stream));
  CHK(begin_job(s));
  hipStream_t st = s.stream;
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  XY* a = s.g1_a.template as<XY>();
  L::convert_points(st, (const uint8_t*)d_in, total, s.pts.template as<AF>(), s.inf.template as<uint8_t>(), err);
  const bool rev_in = (flags & KZGMI_NTT_INVERSE) && (flags & KZGMI_NTT_BITREV);
  L::g1ntt_from_affine(st, s.pts.template as<AF>(), s.inf.template as<uint8_t>(), total, logn, rev_in, a);
  const XY* res = enqueue_transform<Cv>(c, st, a, s.g1_b.template as<XY>(), logn, (uint32_t)count, flags, true);
  uint8_t* enc = s.g1_enc.template as<uint8_t>();
  L::encode_points(st, res, total, enc);
  Fk20Launch::emit(st, enc, (size_t)total * gb, err, d_out);  // nothing is written once an error is raised
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Utility, Cv::ID);
  return 0;
}

int check_open_all_key(const kzgmi_ctx* c, const kzgmi_open_all_key* key) {
  if (!key || std::find(c->open_all_key_list.begin(), c->open_all_key_list.end(), key) == c->open_all_key_list.end())
    return fail(KZGMI_ERR_ARG, "not an open_all key of this context (kzgmi_open_all_key_load)");
  return 0;
}

int check_open_all_args(const kzgmi_open_all_key* key, const void* coeffs, size_t m, uint32_t flags, const void* ys,
                        const void* proofs, bool device) {
  const size_t n = size_t(1) << key->logn;
  if (m > n) return fail(KZGMI_ERR_ARG, "more coefficients than the key's domain has points");
  if (flags & ~(uint32_t)KZGMI_NTT_BITREV) return fail(KZGMI_ERR_ARG, "kzgmi_open_all takes KZGMI_NTT_BITREV only");
  if ((m && !coeffs) || !proofs) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device) return 0;
  if (((m ? (uintptr_t)coeffs : 0) | (uintptr_t)ys | (uintptr_t)proofs) & 15)
    return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t cb = 32 * m, yb = ys ? 32 * n : 0, pb = g1_bytes(key->curve) * n;
  if (overlap(coeffs, cb, ys, yb) || overlap(coeffs, cb, proofs, pb) || overlap(ys, yb, proofs, pb))
    return fail(KZGMI_ERR_ARG, "an output overlaps the input or the other output");
  return 0;
}

// One open_all job on slot s (any slot of the key's device), chained on its stream with no host round
// trip; the outputs are written by the emit kernels only
template <class Cv>
int enqueue_open_all_job(kzgmi_ctx* c, Slot& s, const kzgmi_open_all_key* key, const void* d_coeffs, size_t m, uint32_t flags,
                         void* d_ys_out, void* d_proofs_out) {
  using L = Launch<Cv>;
  using XY = Xyzz<Cv>;
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  const unsigned logn = key->logn;
  const uint32_t n = 1u << logn;
  const size_t gb = g1_bytes(Cv::ID);
  CHK(s.flags.ensure(16));
  CHK(s.scal_s.ensure((size_t)n * 32));
  CHK(s.oa_scal.ensure((size_t)3 * n * 32));  // [ahat: 2n | the coefficients padded to n]
  CHK(s.open_y.ensure((size_t)n * 32));
  CHK(s.g1_a.ensure((size_t)2 * n * sizeof(XY)));
  CHK(s.g1_b.ensure((size_t)n * sizeof(XY)));
  CHK(s.g1_enc.ensure((size_t)n * gb));
  CHK(ensure_roots<Cv>(c, s.stream));
  CHK(begin_job(s));
  hipStream_t st = s.stream;
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  uint32_t* coef = s.scal_s.template as<uint32_t>();
  uint32_t* ahat = s.oa_scal.template as<uint32_t>();
  uint32_t* cpad = ahat + (size_t)16 * n;
  XY* a = s.g1_a.template as<XY>();
  XY* b = s.g1_b.template as<XY>();
  L::convert_scalars(st, (const uint8_t*)d_coeffs, (uint32_t)m, coef, err);
  // ahat = DFT_2n(c_0 .. c_{m-1}, 0 ..) / (2n): the inverse G1 transform's factor, folded into its scalars
  L::g1ntt_pad(st, coef, (uint32_t)m, logn + 1, logn + 1, ahat);
  CHK(HostNtt<Cv>::enqueue(c, s, ahat, logn + 1, 1, 0, nullptr, false, false, ahat, err));
  if (d_ys_out) {
    L::g1ntt_pad(st, coef, (uint32_t)m, logn, 0, cpad);
    CHK(HostNtt<Cv>::enqueue(c, s, cpad, logn, 1, flags & KZGMI_NTT_BITREV, nullptr, false, true, s.open_y.p, err));
  }
  L::g1ntt_mul(st, key->xhat.template as<XY>(), ahat, 0, 2 * n, a);         // hhat[pos] = ahat[pos] xhat[pos]
  L::g1ntt_stages(st, a, logn + 1, 1, true, c->fr_ntt_table[Cv::ID].p, c->g1ntt_form);    // unscaled, bit-reversed out
  L::g1ntt_shift(st, a, logn, b);                                          // (h_0 .. h_{n-2}, infinity)
  const XY* res = enqueue_transform<Cv>(c, st, b, a, logn, 1, flags & KZGMI_NTT_BITREV, false);
  uint8_t* enc = s.g1_enc.template as<uint8_t>();
  L::encode_points(st, res, n, enc);
  Fk20Launch::emit(st, enc, (size_t)n * gb, err, d_proofs_out);
  if (d_ys_out) Fk20Launch::emit(st, s.open_y.p, (size_t)n * 32, err, d_ys_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Utility, Cv::ID);
  return 0;
}

int check_open_cosets_key(const kzgmi_ctx* c, const kzgmi_open_cosets_key* key) {
  if (!key || std::find(c->open_cosets_key_list.begin(), c->open_cosets_key_list.end(), key) == c->open_cosets_key_list.end())
    return fail(KZGMI_ERR_ARG, "not an open_cosets key of this context (kzgmi_open_cosets_key_load)");
  return 0;
}

// (count == 0 passes once the shape is in bounds: the callers then write nothing)
int check_open_cosets_args(const kzgmi_open_cosets_key* key, const void* coeffs, size_t m, size_t count, unsigned logk,
                           uint32_t flags, const void* ys, const void* proofs, bool device) {
  const unsigned logN = key->logN, logl = key->logl;
  if (m > (size_t(1) << logN)) return fail(KZGMI_ERR_ARG, "more coefficients than the key's capacity N");
  if (flags & ~(uint32_t)KZGMI_NTT_BITREV) return fail(KZGMI_ERR_ARG, "kzgmi_open_cosets takes KZGMI_NTT_BITREV only");
  if (logk < logN - logl) return fail(KZGMI_ERR_ARG, "too few cosets (K * l is at least N)");
  if (logk > OPEN_COSETS_MAX_LOG_POINTS - logl) return fail(KZGMI_ERR_ARG, "too many evaluations (count * K * l is at most 2^20)");
  if (count > (size_t(1) << (OPEN_COSETS_MAX_LOG_COEFFS - logN)))
    return fail(KZGMI_ERR_ARG, "too many coefficients (count * N is at most 2^19)");
  if (count > (size_t(1) << (OPEN_COSETS_MAX_LOG_POINTS - logk - logl)))
    return fail(KZGMI_ERR_ARG, "too many evaluations (count * K * l is at most 2^20)");
  if (count == 0) return 0;
  if ((m && !coeffs) || !proofs) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device) return 0;
  if (((m ? (uintptr_t)coeffs : 0) | (uintptr_t)ys | (uintptr_t)proofs) & 15)
    return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t cb = 32 * m * count, yb = ys ? (32 * count) << (logk + logl) : 0, pb = (g1_bytes(key->curve) * count) << logk;
  if (overlap(coeffs, cb, ys, yb) || overlap(coeffs, cb, proofs, pb) || overlap(ys, yb, proofs, pb))
    return fail(KZGMI_ERR_ARG, "an output overlaps the input or the other output");
  return 0;
}

// One open_cosets job of count >= 1 polynomials on slot s (any slot of the key's device), chained on its
// stream with no host round trip; the outputs are written by the emit kernels only
template <class Cv>
int enqueue_open_cosets_job(kzgmi_ctx* c, Slot& s, const kzgmi_open_cosets_key* key, const void* d_coeffs, size_t m, size_t count,
                            unsigned logk, uint32_t flags, void* d_ys_out, void* d_proofs_out) {
  using L = Launch<Cv>;
  using XY = Xyzz<Cv>;
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  const unsigned logN = key->logN, logl = key->logl, logr2 = logN - logl + 1, logpts = logk + logl;
  const uint32_t cnt = (uint32_t)count;
  const size_t terms = count << (logN + 1), nproofs = count << logk, npoints = count << logpts;
  const size_t recs = std::max({L::cosets_scratch_records(logN, logl, cnt, c->g1ntt_form), count << logr2, nproofs});
  const size_t gb = g1_bytes(Cv::ID);
  CHK(s.flags.ensure(16));
  CHK(s.scal_s.ensure(count * m * 32));
  // [ahat: count * 2N | ahat in term order: count * 2N | the coefficients padded to K l each]
  CHK(s.oa_scal.ensure((2 * terms + (d_ys_out ? npoints : 0)) * 32));
  if (d_ys_out) CHK(s.open_y.ensure(npoints * 32));
  CHK(s.g1_a.ensure(recs * sizeof(XY)));
  CHK(s.g1_b.ensure(recs * sizeof(XY)));
  CHK(s.g1_enc.ensure(nproofs * gb));
  CHK(ensure_roots<Cv>(c, s.stream));
  CHK(begin_job(s));
  hipStream_t st = s.stream;
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  uint32_t* coef = s.scal_s.template as<uint32_t>();
  uint32_t* ahat = s.oa_scal.template as<uint32_t>();
  uint32_t* scal = ahat + 8 * terms;
  uint32_t* cpad = scal + 8 * terms;
  XY* a = s.g1_a.template as<XY>();
  XY* b = s.g1_b.template as<XY>();
  L::convert_scalars(st, (const uint8_t*)d_coeffs, (uint32_t)(count * m), coef, err);
  // ahat^(b) = DFT_2R(c_b, c_{l+b}, .., 0 x R) / (2R) for every polynomial and b: the inverse G1 transform's factor
  // is folded into its scalars
  L::cosets_pad(st, coef, (uint32_t)m, cnt, logl, logr2, 1u << (logr2 - 1), logr2, ahat);
  CHK(HostNtt<Cv>::enqueue(c, s, ahat, logr2, count << logl, 0, nullptr, false, false, ahat, err));
  const void* ys = s.open_y.p;
  if (d_ys_out) {
    L::cosets_pad(st, coef, (uint32_t)m, cnt, 0, logpts, 1u << logpts, 0, cpad);
    CHK(HostNtt<Cv>::enqueue(c, s, cpad, logpts, count, flags & KZGMI_NTT_BITREV, nullptr, false, true, s.open_y.p, err));
    if (!(flags & KZGMI_NTT_BITREV) && logl && logk) {  // natural order -> coset-major (the same where l or K is 1)
      L::cosets_ys(st, s.open_y.p, logk, logl, cnt, cpad);
      ys = cpad;
    }
  }
  if (logl) L::cosets_scal(st, ahat, logN, logl, cnt, scal);  // [t][b][pos] -> [t][pos][b] (the same where l is 1)
  XY* hhat = L::cosets_products(st, key->xhat.template as<XY>(), logl ? scal : ahat, logN, logl, cnt, c->g1ntt_form, a, b);  // = a
  L::g1ntt_stages(st, hhat, logr2, cnt, true, c->fr_ntt_table[Cv::ID].p, c->g1ntt_form);  // unscaled, bit-reversed out
  L::cosets_shift(st, hhat, logr2, logk, cnt, b);                                            // (H_0 .. H_{R-2}, infinity ..)
  const XY* res = enqueue_transform<Cv>(c, st, b, a, logk, cnt, flags & KZGMI_NTT_BITREV, false);
  uint8_t* enc = s.g1_enc.template as<uint8_t>();
  L::encode_points(st, res, (uint32_t)nproofs, enc);
  Fk20Launch::emit(st, enc, nproofs * gb, err, d_proofs_out);
  if (d_ys_out) Fk20Launch::emit(st, ys, npoints * 32, err, d_ys_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Utility, Cv::ID);
  return 0;
}

}  // namespace

extern "C" {

int kzgmi_g1_ntt_device_async(kzgmi_ctx* c, kzgmi_curve curve, int slot, const void* d_in, unsigned logn, size_t count,
                              uint32_t flags, void* d_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  CHK(check_g1_ntt_args(curve, d_in, d_out, logn, count, flags, true));
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (count == 0) return arm_empty(s, JobKind::Utility, curve);  // succeeds, writes nothing
  Roctx rx("kzgmi_g1_ntt_device_async");
  return dispatch(curve, [&](auto cv) -> int {
    return enqueue_g1_ntt_job<decltype(cv)>(c, s, d_in, logn, count, flags, d_out);
  });
}

int kzgmi_g1_ntt_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_in, unsigned logn, size_t count, uint32_t flags,
                        void* d_out) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(kzgmi_g1_ntt_device_async(c, curve, 0, d_in, logn, count, flags, d_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

// The host form: the points in slot 0's stage buffer, transformed in place there and copied back
int kzgmi_g1_ntt(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* in, unsigned logn, size_t count, uint32_t flags,
                 uint8_t* out) {
  CHK(check_ctx(c));
  CHK(check_g1_ntt_args(curve, in, out, logn, count, flags, false));
  CHK(slot0_idle(c));
  if (count == 0) return 0;
  const size_t bytes = g1_bytes(curve) * (count << logn);
  const StageItem item{in, bytes};
  uint8_t* d = nullptr;
  CHK(stage_host(c, c->slots[0], &item, 1, &d));
  CHK(kzgmi_g1_ntt_device_async(c, curve, 0, d, logn, count, flags, d));
  CHK(kzgmi_slot_wait(c, 0, nullptr));
  HIPCHK(hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// The key: x from the commit key's resident row of powers, its forward 2n-point transform, natural order
int kzgmi_open_all_key_load(kzgmi_ctx* c, const kzgmi_ck* ck, unsigned logn, kzgmi_open_all_key** out) {
  CHK(check_ctx(c));
  if (!out) return fail(KZGMI_ERR_ARG, "null argument");
  if (!ck || ck->ctx != c) return fail(KZGMI_ERR_ARG, "commit key does not belong to this context");
  if (logn > OPEN_ALL_MAX_LOGN) return fail(KZGMI_ERR_ARG, "domain too large (max 2^19 points)");
  const size_t n = size_t(1) << logn;
  if (n - 1 > ck->n) return fail(KZGMI_ERR_ARG, "the domain needs n - 1 commit-key points");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  return dispatch(ck->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using L = Launch<Cv>;
    using XY = Xyzz<Cv>;
    kzgmi_open_all_key* key = new kzgmi_open_all_key();
    key->curve = Cv::ID;
    key->logn = logn;
    key->ctx = c;
    auto build = [&]() -> int {
      CHK(key->xhat.ensure(2 * n * sizeof(XY)));
      CHK(s.g1_a.ensure(2 * n * sizeof(XY)));
      CHK(ensure_roots<Cv>(c, s.stream));
      CHK(begin_job(s));
      hipStream_t st = s.stream;
      XY* a = s.g1_a.template as<XY>();
      L::g1ntt_key_x(st, ck->pts.template as<Affine<Cv>>(), ck->inf.template as<uint8_t>(), logn, a);
      L::g1ntt_stages(st, a, logn + 1, 1, false, c->fr_ntt_table[Cv::ID].p, c->g1ntt_form);
      L::g1ntt_rev(st, a, logn + 1, (uint32_t)(2 * n), key->xhat.template as<XY>());
      HIPCHK(hipGetLastError());
      return sync_job(s);
    };
    if (int r = build()) {
      key->xhat.release();
      delete key;
      return r;
    }
    c->open_all_key_list.push_back(key);
    *out = key;
    return 0;
  });
}

void kzgmi_open_all_key_free(kzgmi_open_all_key* key) {
  if (!key) return;
  if (kzgmi_ctx* c = key->ctx) {
    (void)hipSetDevice(c->device);
    auto& v = c->open_all_key_list;
    v.erase(std::remove(v.begin(), v.end(), key), v.end());
    key->xhat.release();
  }
  delete key;
}

size_t kzgmi_open_all_key_device_bytes(const kzgmi_open_all_key* key) { return key ? key->xhat.cap : 0; }

int kzgmi_open_all_device_async(kzgmi_ctx* c, const kzgmi_open_all_key* key, int slot, const void* d_coeffs, size_t m,
                                uint32_t flags, void* d_ys_out, void* d_proofs_out) {
  KZ_ROUTE(c, nullptr, slot);  // (keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  CHK(check_open_all_key(c, key));
  CHK(check_open_all_args(key, d_coeffs, m, flags, d_ys_out, d_proofs_out, true));
  Roctx rx("kzgmi_open_all_device_async");
  return dispatch(key->curve, [&](auto cv) -> int {
    return enqueue_open_all_job<decltype(cv)>(c, c->slots[slot], key, d_coeffs, m, flags, d_ys_out, d_proofs_out);
  });
}

int kzgmi_open_all_device(kzgmi_ctx* c, const kzgmi_open_all_key* key, const void* d_coeffs, size_t m, uint32_t flags,
                          void* d_ys_out, void* d_proofs_out) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(kzgmi_open_all_device_async(c, key, 0, d_coeffs, m, flags, d_ys_out, d_proofs_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

// The host form: [coeffs | proofs | ys] in slot 0's stage buffer, the results copied back
int kzgmi_open_all(kzgmi_ctx* c, const kzgmi_open_all_key* key, const uint8_t* coeffs, size_t m, uint32_t flags,
                   uint8_t* ys_out, uint8_t* proofs_out) {
  CHK(check_ctx(c));
  CHK(check_open_all_key(c, key));
  CHK(check_open_all_args(key, coeffs, m, flags, ys_out, proofs_out, false));
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  const size_t n = size_t(1) << key->logn, gb = g1_bytes(key->curve);
  const StageItem items[3] = {{m ? coeffs : nullptr, 32 * m}, {nullptr, gb * n}, {nullptr, 32 * n}};
  uint8_t* d[3];
  CHK(stage_host(c, s, items, 3, d));
  CHK(dispatch(key->curve, [&](auto cv) -> int {
    return enqueue_open_all_job<decltype(cv)>(c, s, key, d[0], m, flags, ys_out ? d[2] : nullptr, d[1]);
  }));
  CHK(finish_slot(c, s, nullptr));
  HIPCHK(hipMemcpy(proofs_out, d[1], gb * n, hipMemcpyDeviceToHost));
  if (ys_out) HIPCHK(hipMemcpy(ys_out, d[2], 32 * n, hipMemcpyDeviceToHost));
  return 0;
}

// The key: the l vectors x^(b) from the commit key's resident row of powers, their forward 2R-point transforms
// (the batched stages with count = l), laid out [pos][b] for the products
int kzgmi_open_cosets_key_load(kzgmi_ctx* c, const kzgmi_ck* ck, unsigned logN, unsigned logl, kzgmi_open_cosets_key** out) {
  CHK(check_ctx(c));
  if (!out) return fail(KZGMI_ERR_ARG, "null argument");
  if (!ck || ck->ctx != c) return fail(KZGMI_ERR_ARG, "commit key does not belong to this context");
  if (logN > OPEN_COSETS_MAX_LOG_COEFFS) return fail(KZGMI_ERR_ARG, "capacity too large (max 2^19 coefficients)");
  if (logl > logN) return fail(KZGMI_ERR_ARG, "a coset has at most N points");
  const size_t N = size_t(1) << logN, l = size_t(1) << logl;
  if (N - l > ck->n) return fail(KZGMI_ERR_ARG, "the shape needs N - l commit-key points");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  return dispatch(ck->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using L = Launch<Cv>;
    using XY = Xyzz<Cv>;
    kzgmi_open_cosets_key* key = new kzgmi_open_cosets_key();
    key->curve = Cv::ID;
    key->logN = logN;
    key->logl = logl;
    key->ctx = c;
    auto build = [&]() -> int {
      CHK(key->xhat.ensure(2 * N * sizeof(XY)));
      CHK(s.g1_a.ensure(2 * N * sizeof(XY)));
      CHK(ensure_roots<Cv>(c, s.stream));
      CHK(begin_job(s));
      hipStream_t st = s.stream;
      XY* a = s.g1_a.template as<XY>();
      L::cosets_key_x(st, ck->pts.template as<Affine<Cv>>(), ck->inf.template as<uint8_t>(), logN, logl, a);
      L::g1ntt_stages(st, a, logN - logl + 1, (uint32_t)l, false, c->fr_ntt_table[Cv::ID].p, c->g1ntt_form);
      L::cosets_key_gather(st, a, logN, logl, key->xhat.template as<XY>());
      HIPCHK(hipGetLastError());
      return sync_job(s);
    };
    if (int r = build()) {
      key->xhat.release();
      delete key;
      return r;
    }
    c->open_cosets_key_list.push_back(key);
    *out = key;
    return 0;
  });
}

void kzgmi_open_cosets_key_free(kzgmi_open_cosets_key* key) {
  if (!key) return;
  if (kzgmi_ctx* c = key->ctx) {
    (void)hipSetDevice(c->device);
    auto& v = c->open_cosets_key_list;
    v.erase(std::remove(v.begin(), v.end(), key), v.end());
    key->xhat.release();
  }
  delete key;
}

size_t kzgmi_open_cosets_key_device_bytes(const kzgmi_open_cosets_key* key) { return key ? key->xhat.cap : 0; }

int kzgmi_open_cosets_device_async(kzgmi_ctx* c, const kzgmi_open_cosets_key* key, int slot, const void* d_coeffs, size_t m,
                                   size_t count, unsigned logk, uint32_t flags, void* d_ys_out, void* d_proofs_out) {
  KZ_ROUTE(c, nullptr, slot);  // (keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  CHK(check_open_cosets_key(c, key));
  CHK(check_open_cosets_args(key, d_coeffs, m, count, logk, flags, d_ys_out, d_proofs_out, true));
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (count == 0) return arm_empty(s, JobKind::Utility, key->curve);  // succeeds, writes nothing
  Roctx rx("kzgmi_open_cosets_device_async");
  return dispatch(key->curve, [&](auto cv) -> int {
    return enqueue_open_cosets_job<decltype(cv)>(c, s, key, d_coeffs, m, count, logk, flags, d_ys_out, d_proofs_out);
  });
}

int kzgmi_open_cosets_device(kzgmi_ctx* c, const kzgmi_open_cosets_key* key, const void* d_coeffs, size_t m, size_t count,
                             unsigned logk, uint32_t flags, void* d_ys_out, void* d_proofs_out) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(kzgmi_open_cosets_device_async(c, key, 0, d_coeffs, m, count, logk, flags, d_ys_out, d_proofs_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

// The host form: [coeffs | proofs | ys] in slot 0's stage buffer, the results copied back
int kzgmi_open_cosets(kzgmi_ctx* c, const kzgmi_open_cosets_key* key, const uint8_t* coeffs, size_t m, size_t count, unsigned logk,
                      uint32_t flags, uint8_t* ys_out, uint8_t* proofs_out) {
  CHK(check_ctx(c));
  CHK(check_open_cosets_key(c, key));
  CHK(check_open_cosets_args(key, coeffs, m, count, logk, flags, ys_out, proofs_out, false));
  CHK(slot0_idle(c));
  if (count == 0) return 0;
  Slot& s = c->slots[0];
  const size_t pb = (g1_bytes(key->curve) * count) << logk, yb = (32 * count) << (logk + key->logl);
  const StageItem items[3] = {{m ? coeffs : nullptr, 32 * m * count}, {nullptr, pb}, {nullptr, yb}};
  uint8_t* d[3];
  CHK(stage_host(c, s, items, 3, d));
  CHK(dispatch(key->curve, [&](auto cv) -> int {
    return enqueue_open_cosets_job<decltype(cv)>(c, s, key, d[0], m, count, logk, flags, ys_out ? d[2] : nullptr, d[1]);
  }));
  CHK(finish_slot(c, s, nullptr));
  HIPCHK(hipMemcpy(proofs_out, d[1], pb, hipMemcpyDeviceToHost));
  if (ys_out) HIPCHK(hipMemcpy(ys_out, d[2], yb, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
