// KZG opening proofs over a prover commit key (kzgmi_open*): the scan of open.hpp turns the
// coefficients into y = p(z) and the quotient's coefficients for each point, and the commit's MSM
// (host_msm.hip kzgmi_commit_device_async: 16 classes over the key's shifted rows, one bucket set)
// turns each quotient into its proof.  DESIGN.md 3g.
#include "host.hpp"
#include "open.hpp"

namespace {

constexpr size_t kOpenMaxPoints = 4096;

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}

// points per group: their quotients (m - 1 scalars each) hold at most c->open_group scalars
size_t open_group_points(const kzgmi_ctx* c, size_t m, size_t k) {
  const size_t per = m > 1 ? m - 1 : 1;
  return std::min(k, std::max<size_t>(1, c->open_group / per));
}

// the run values and the two tile arrays of g points, 32 B per value: [runv | tilev | tilec]
size_t open_aux_values(size_t tiles, size_t g) { return g * tiles * (OPEN_BLOCK + 2); }

int check_open_args(const void* coeffs, size_t m, const void* zs, size_t k, const void* ys, const void* out, size_t out_per,
                    bool device) {
  if (m > (size_t(1) << 26)) return fail(KZGMI_ERR_ARG, "too many coefficients (max 2^26)");
  if (k > kOpenMaxPoints) return fail(KZGMI_ERR_ARG, "too many points (max 4096 per call)");
  if ((m && !coeffs) || (k && (!zs || !ys || !out))) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device || k == 0) return 0;
  if (((m ? (uintptr_t)coeffs : 0) | (uintptr_t)zs | (uintptr_t)ys | (uintptr_t)out) & 15)
    return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t cb = 32 * m, zb = 32 * k, ob = out_per * k;
  if (overlap(coeffs, cb, ys, zb) || overlap(coeffs, cb, out, ob) || overlap(zs, zb, ys, zb) || overlap(zs, zb, out, ob) ||
      overlap(ys, zb, out, ob))
    return fail(KZGMI_ERR_ARG, "an output overlaps an input or the other output");
  return 0;
}

// Where an opening's coefficients come from: m coefficients (32 B big-endian each), or with evals the
// m = 2^logn values of the polynomial on the m-th roots of unity (ntt_flags: KZGMI_NTT_BITREV or 0)
struct OpenSource {
  const void* d;
  bool evals;
  unsigned logn;
  uint32_t ntt_flags;
};

// The front end every form shares, which starts the job: on s.stream behind the zeroed error word, the
// coefficients as canonical LE words in s.scal_s (range-checked once per call; from evaluations, the
// inverse transform's passes, whose first range-checks them) and the powers of every point in
// s.open_zp (each point range-checked)
template <class Cv>
int enqueue_open_inputs(kzgmi_ctx* c, Slot& s, const OpenSource& src, size_t m, const void* d_zs, size_t k) {
  using L = Launch<Cv>;
  CHK(s.flags.ensure(16));
  CHK(s.scal_s.ensure(m * 32));
  CHK(s.open_zp.ensure(k * L::open_power_bytes()));
  CHK(begin_job(s));
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  if (src.evals)
    CHK(HostNtt<Cv>::enqueue(c, s, src.d, src.logn, 1, KZGMI_NTT_INVERSE | src.ntt_flags, nullptr, true, false, s.scal_s.p, err));
  else
    L::convert_scalars(s.stream, (const uint8_t*)src.d, (uint32_t)m, s.scal_s.template as<uint32_t>(), err);
  L::open_points(s.stream, (const uint8_t*)d_zs, (uint32_t)k, s.open_zp.template as<uint32_t>(), err);
  return 0;
}

// One opening job on slot s (any slot of the key's device): completes with kzgmi_slot_wait, its
// kernels reporting through the slot's error word.  d_ys_out and d_proofs_out are written by the
// emit kernels only, which write nothing once an error is raised.
template <class Cv>
int enqueue_open_job(kzgmi_ctx* c, Slot& s, const kzgmi_ck* ck, const OpenSource& src, size_t m, const void* d_zs, size_t k,
                     void* d_ys_out, void* d_proofs_out) {
  using L = Launch<Cv>;
  using XY = Xyzz<Cv>;
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (k == 0) return arm_empty(s, JobKind::Utility, Cv::ID);  // succeeds, writes nothing
  const size_t gb = g1_bytes(Cv::ID);
  const size_t tiles = L::open_tiles(m), G = open_group_points(c, m, k), nq = m > 1 ? m - 1 : 0;
  CHK(s.open_y.ensure(k * 32));
  CHK(s.open_rec.ensure(k * sizeof(XY)));
  CHK(s.open_enc.ensure(k * gb));
  CHK(s.open_q.ensure(G * nq * 32));
  CHK(s.open_aux.ensure(open_aux_values(tiles, G) * 32));
  CHK(enqueue_open_inputs<Cv>(c, s, src, m, d_zs, k));
  hipStream_t st = s.stream;
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  XY* rec = s.open_rec.template as<XY>();
  uint8_t* ys = s.open_y.template as<uint8_t>();
  if (m == 0) HIPCHK(hipMemsetAsync(ys, 0, k * 32, st));                 // y = 0
  if (m < 2) HIPCHK(hipMemsetAsync(rec, 0, k * sizeof(XY), st));        // zz = 0: infinity
  const uint32_t* coef = s.scal_s.template as<uint32_t>();
  uint32_t* q = s.open_q.template as<uint32_t>();
  uint32_t* runv = s.open_aux.template as<uint32_t>();
  for (size_t j0 = 0; m && j0 < k; j0 += G) {
    const size_t g = std::min(G, k - j0);
    uint32_t* tilev = runv + 8 * g * tiles * OPEN_BLOCK;
    L::open_quotients(st, coef, (uint32_t)m, s.open_zp.template as<uint32_t>() + 8 * j0 * OPEN_POWERS, (uint32_t)g, runv,
                      tilev, tilev + 8 * g * tiles, ys + 32 * j0, q, false);
    HIPCHK(hipGetLastError());
    for (size_t j = 0; nq && j < g; ++j) {
      // the commit's term list over this point's quotient: row w of the key takes digit w, one bucket set
      TermList tl{};
      for (int w = 0; w < CK_ROWS; ++w)
        tl.c[w] = {(uint32_t)nq, (uint32_t)(w * ck->n), 8, 1, 0, 8, q + 8 * j * nq, (uint32_t)w};
      tl.nclass = CK_ROWS;
      tl.total = (uint32_t)(CK_ROWS * nq);
      MsmWindows mw{1, {0, 0}, {1, 0}};
      CHK(HostCore<Cv>::run_msm_core(c, s, tl, 1, (size_t)CK_ROWS * nq + 16, mw, ck->pts.template as<Affine<Cv>>(),
                                     ck->inf.template as<uint8_t>()));
      HIPCHK(hipMemcpyAsync(rec + j0 + j, s.res.p, sizeof(XY), hipMemcpyDeviceToDevice, st));
    }
  }
  uint8_t* enc = s.open_enc.template as<uint8_t>();
  L::encode_points(st, rec, (uint32_t)k, enc);
  Fk20Launch::emit(st, enc, k * gb, err, d_proofs_out);
  Fk20Launch::emit(st, ys, k * 32, err, d_ys_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(end_job(s));
  arm(s, JobKind::Utility, Cv::ID);
  return 0;
}

int check_open_key(const kzgmi_ctx* c, const kzgmi_ck* ck, size_t m) {
  if (!ck || ck->ctx != c) return fail(KZGMI_ERR_ARG, "commit key does not belong to this context");
  if (m > ck->n) return fail(KZGMI_ERR_ARG, "more coefficients than commit-key points");
  return 0;
}

}  // namespace

extern "C" {

int kzgmi_open_device_async(kzgmi_ctx* c, const kzgmi_ck* ck, int slot, const void* d_coeffs, size_t m, const void* d_zs,
                            size_t k, void* d_ys_out, void* d_proofs_out) {
  KZ_ROUTE(c, nullptr, slot);  // (commit keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  CHK(check_open_key(c, ck, m));
  CHK(check_open_args(d_coeffs, m, d_zs, k, d_ys_out, d_proofs_out, g1_bytes(ck->curve), true));
  Roctx rx("kzgmi_open_device_async");
  return dispatch(ck->curve, [&](auto cv) -> int {
    return enqueue_open_job<decltype(cv)>(c, c->slots[slot], ck, OpenSource{d_coeffs, false, 0, 0}, m, d_zs, k, d_ys_out,
                                          d_proofs_out);
  });
}

int kzgmi_open_device(kzgmi_ctx* c, const kzgmi_ck* ck, const void* d_coeffs, size_t m, const void* d_zs, size_t k,
                      void* d_ys_out, void* d_proofs_out) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(kzgmi_open_device_async(c, ck, 0, d_coeffs, m, d_zs, k, d_ys_out, d_proofs_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

// The host form: [coeffs | zs | proofs | ys] in slot 0's stage buffer, the results copied back
int kzgmi_open(kzgmi_ctx* c, const kzgmi_ck* ck, const uint8_t* coeffs, size_t m, const uint8_t* zs, size_t k,
               uint8_t* ys_out, uint8_t* proofs_out) {
  CHK(check_ctx(c));
  CHK(check_open_key(c, ck, m));
  const size_t gb = g1_bytes(ck->curve);
  CHK(check_open_args(coeffs, m, zs, k, ys_out, proofs_out, gb, false));
  CHK(slot0_idle(c));
  if (k == 0) return 0;
  Slot& s = c->slots[0];
  const StageItem items[4] = {{m ? coeffs : nullptr, 32 * m}, {zs, 32 * k}, {nullptr, gb * k}, {nullptr, 32 * k}};
  uint8_t* d[4];
  CHK(stage_host(c, s, items, 4, d));
  CHK(dispatch(ck->curve, [&](auto cv) -> int {
    return enqueue_open_job<decltype(cv)>(c, s, ck, OpenSource{d[0], false, 0, 0}, m, d[1], k, d[3], d[2]);
  }));
  CHK(finish_slot(c, s, nullptr));
  HIPCHK(hipMemcpy(proofs_out, d[2], gb * k, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ys_out, d[3], 32 * k, hipMemcpyDeviceToHost));
  return 0;
}

// Openings of a polynomial given by its evaluations: the inverse transform into the slot's coefficient
// buffer and the opening on those coefficients, one job
int check_open_evals(const kzgmi_ctx* c, const kzgmi_ck* ck, unsigned logn, uint32_t flags) {
  if (!ck || ck->ctx != c) return fail(KZGMI_ERR_ARG, "commit key does not belong to this context");
  if (logn > NTT_MAX_LOGN) return fail(KZGMI_ERR_ARG, "transform too large (max 2^26 points)");
  if (flags & ~(uint32_t)KZGMI_NTT_BITREV) return fail(KZGMI_ERR_ARG, "kzgmi_open_evals takes KZGMI_NTT_BITREV only");
  if ((size_t(1) << logn) > ck->n) return fail(KZGMI_ERR_ARG, "more evaluations than commit-key points");
  return 0;
}

int kzgmi_open_evals_device_async(kzgmi_ctx* c, const kzgmi_ck* ck, int slot, const void* d_evals, unsigned logn,
                                  uint32_t flags, const void* d_zs, size_t k, void* d_ys_out, void* d_proofs_out) {
  KZ_ROUTE(c, nullptr, slot);  // (commit keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  CHK(check_open_evals(c, ck, logn, flags));
  const size_t m = size_t(1) << logn;
  CHK(check_open_args(d_evals, m, d_zs, k, d_ys_out, d_proofs_out, g1_bytes(ck->curve), true));
  Roctx rx("kzgmi_open_evals_device_async");
  return dispatch(ck->curve, [&](auto cv) -> int {
    return enqueue_open_job<decltype(cv)>(c, c->slots[slot], ck, OpenSource{d_evals, true, logn, flags}, m, d_zs, k, d_ys_out,
                                          d_proofs_out);
  });
}

int kzgmi_open_evals_device(kzgmi_ctx* c, const kzgmi_ck* ck, const void* d_evals, unsigned logn, uint32_t flags,
                            const void* d_zs, size_t k, void* d_ys_out, void* d_proofs_out) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(kzgmi_open_evals_device_async(c, ck, 0, d_evals, logn, flags, d_zs, k, d_ys_out, d_proofs_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

// The host form: [evals | zs | proofs | ys] in slot 0's stage buffer, the results copied back
int kzgmi_open_evals(kzgmi_ctx* c, const kzgmi_ck* ck, const uint8_t* evals, unsigned logn, uint32_t flags, const uint8_t* zs,
                     size_t k, uint8_t* ys_out, uint8_t* proofs_out) {
  CHK(check_ctx(c));
  CHK(check_open_evals(c, ck, logn, flags));
  const size_t m = size_t(1) << logn, gb = g1_bytes(ck->curve);
  CHK(check_open_args(evals, m, zs, k, ys_out, proofs_out, gb, false));
  CHK(slot0_idle(c));
  if (k == 0) return 0;
  Slot& s = c->slots[0];
  const StageItem items[4] = {{evals, 32 * m}, {zs, 32 * k}, {nullptr, gb * k}, {nullptr, 32 * k}};
  uint8_t* d[4];
  CHK(stage_host(c, s, items, 4, d));
  CHK(dispatch(ck->curve, [&](auto cv) -> int {
    return enqueue_open_job<decltype(cv)>(c, s, ck, OpenSource{d[0], true, logn, flags}, m, d[1], k, d[3], d[2]);
  }));
  CHK(finish_slot(c, s, nullptr));
  HIPCHK(hipMemcpy(proofs_out, d[2], gb * k, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ys_out, d[3], 32 * k, hipMemcpyDeviceToHost));
  return 0;
}

int kzgmi_open_quotient_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_coeffs, size_t m, const void* d_zs, size_t k,
                               void* d_ys_out, void* d_q_out) {
  CHK(check_ctx(c));
  if (curve != KZGMI_BLS12_381 && curve != KZGMI_BN254) return fail(KZGMI_ERR_ARG, "unknown curve");
  if (m > (size_t(1) << 26)) return fail(KZGMI_ERR_ARG, "too many coefficients (max 2^26)");
  if (k > kOpenMaxPoints) return fail(KZGMI_ERR_ARG, "too many points (max 4096 per call)");
  if ((m && !d_coeffs) || (k && (!d_zs || !d_ys_out || (m > 1 && !d_q_out)))) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(slot0_idle(c));
  if (k == 0) return 0;
  if (((m ? (uintptr_t)d_coeffs : 0) | (uintptr_t)d_zs | (uintptr_t)d_ys_out | (m > 1 ? (uintptr_t)d_q_out : 0)) & 15)
    return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using L = Launch<Cv>;
    Slot& s = c->slots[0];
    const size_t tiles = L::open_tiles(m), G = open_group_points(c, m, k), nq = m > 1 ? m - 1 : 0;
    CHK(s.open_aux.ensure(open_aux_values(tiles, G) * 32));
    CHK(enqueue_open_inputs<Cv>(c, s, OpenSource{d_coeffs, false, 0, 0}, m, d_zs, k));
    hipStream_t st = s.stream;
    if (m == 0) HIPCHK(hipMemsetAsync(d_ys_out, 0, k * 32, st));
    uint32_t* runv = s.open_aux.template as<uint32_t>();
    for (size_t j0 = 0; m && j0 < k; j0 += G) {
      const size_t g = std::min(G, k - j0);
      uint32_t* tilev = runv + 8 * g * tiles * OPEN_BLOCK;
      L::open_quotients(st, s.scal_s.template as<uint32_t>(), (uint32_t)m,
                        s.open_zp.template as<uint32_t>() + 8 * j0 * OPEN_POWERS, (uint32_t)g, runv, tilev,
                        tilev + 8 * g * tiles, (uint8_t*)d_ys_out + 32 * j0, (uint8_t*)d_q_out + 32 * nq * j0, true);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
    CHK(end_job(s));
    arm(s, JobKind::Utility, Cv::ID);
    return finish_slot(c, s, nullptr);
  });
}

}  // extern "C"
