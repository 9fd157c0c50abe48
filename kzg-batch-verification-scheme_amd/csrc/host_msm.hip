// MSM entry points (whole, sharded partial + combine), the prover commit key, and the diagnostics
// built on them: pairing, generators, G2 multiplication, point compression, the multiplier probe.
#include "host.hpp"

namespace {

// the generator's window table of curve Cv, once per context
template <class Cv>
int ensure_table(kzgmi_ctx* c, hipStream_t st) {
  if (!c->table_ready[Cv::ID]) CHK(c->table_base[Cv::ID].ensure(32 * sizeof(Xyzz<Cv>)));
  return ensure_once(c->table_ready[Cv::ID], c->table[Cv::ID], 32 * 256 * sizeof(Affine<Cv>), st, [&] {
    Launch<Cv>::gen_table(st, c->table_base[Cv::ID].template as<Xyzz<Cv>>(), c->table[Cv::ID].template as<Affine<Cv>>());
  });
}

int read_flags_sync(kzgmi_ctx* c, Slot& s) {
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
  CHK(sync_job(s));
  collect_phases(c, s);
  return map_device_err((uint32_t)s.host_flags[1]);
}

// The MSM of n > 0 points on slot s and its encoded result in s.outb
template <class Cv>
int enqueue_msm_encoded(kzgmi_ctx* c, Slot& s, const void* dpts, const void* dsc, size_t n) {
  CHK(HostCore<Cv>::enqueue_msm(c, s, dpts, dsc, n));
  CHK(s.outb.ensure(g1_bytes(Cv::ID)));
  Launch<Cv>::encode_points(s.stream, s.res.template as<Xyzz<Cv>>(), 1, s.outb.template as<uint8_t>());
  HIPCHK(hipGetLastError());
  return 0;
}

// The MSM of n > 0 points on slot s as a partial record (marked if the shard failed)
template <class Cv>
int enqueue_msm_partial(kzgmi_ctx* c, Slot& s, const void* dpts, const void* dsc, size_t n, void* d_partial_out) {
  CHK(HostCore<Cv>::enqueue_msm(c, s, dpts, dsc, n));
  Launch<Cv>::partial_out(s.stream, s.res.template as<Xyzz<Cv>>(), 1, s.flags.template as<uint32_t>() + 1,
                          (Xyzz<Cv>*)d_partial_out);
  return 0;
}

// The sum of n_parts MSM partial records on slot s and its encoding in s.outb; chain: behind the
// slot's own pending MSM partial, whose error word is kept
template <class Cv>
int enqueue_msm_combine(Slot& s, const void* d_partials, int n_parts, bool chain) {
  using XY = Xyzz<Cv>;
  CHK(s.res.ensure(2 * sizeof(XY)));
  CHK(s.outb.ensure(g1_bytes(Cv::ID)));
  CHK(s.flags.ensure(16));
  CHK(begin_job(s));  // chained: the lane the partial ended in
  if (!chain) HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
  Launch<Cv>::sum_partials(s.stream, (const XY*)d_partials, (uint32_t)n_parts, 1, 1, s.res.template as<XY>(),
                           s.flags.template as<uint32_t>() + 1);
  Launch<Cv>::encode_points(s.stream, s.res.template as<XY>(), 1, s.outb.template as<uint8_t>());
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ prover commit key
int kzgmi_ck_load(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* g1_powers, size_t n, kzgmi_ck** out) {
  CHK(check_ctx(c));
  if (!g1_powers || !out || n == 0) return fail(KZGMI_ERR_ARG, "bad commit key argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "commit key too large (max 2^26 points)");
  Slot& s = c->slots[0];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot 0 busy: call kzgmi_slot_wait first");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using L = Launch<Cv>;
    const size_t gb = g1_bytes(Cv::ID);
    kzgmi_ck* ck = new kzgmi_ck();
    ck->curve = Cv::ID;
    ck->n = n;
    ck->ctx = c;
    int r = 0;
    if ((r = ck->pts.ensure((size_t)CK_ROWS * n * sizeof(Affine<Cv>))) || (r = ck->inf.ensure((size_t)CK_ROWS * n)) ||
        (r = s.stage.ensure(n * gb)) || (r = s.flags.ensure(16))) {
      delete ck;
      return r;
    }
    if (int rb = begin_job(s)) {
      delete ck;
      return rb;
    }
    hipStream_t st = s.stream;
    Affine<Cv>* pts = ck->pts.template as<Affine<Cv>>();
    uint8_t* inf = ck->inf.template as<uint8_t>();
    bool okk = hipMemcpyAsync(s.stage.p, g1_powers, n * gb, hipMemcpyHostToDevice, st) == hipSuccess &&
               hipMemsetAsync(s.flags.p, 0, 16, st) == hipSuccess;
    if (okk) {
      L::convert_points(st, s.stage.template as<uint8_t>(), (uint32_t)n, pts, inf, s.flags.template as<uint32_t>() + 1);
      for (int w = 1; w < CK_ROWS; ++w)
        L::shift_points(st, pts + (size_t)(w - 1) * n, inf + (size_t)(w - 1) * n, (uint32_t)n, pts + (size_t)w * n,
                        inf + (size_t)w * n);
      L::pts_to29(st, pts, (uint32_t)(CK_ROWS * n));  // resident in the accumulation's format
      okk = okk && hipGetLastError() == hipSuccess &&
            hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st) == hipSuccess && sync_job(s) == 0;
    }
    if (!okk) {
      delete ck;
      return fail(KZGMI_ERR_DEVICE, "commit key upload/precompute failed");
    }
    if (int e = map_device_err((uint32_t)s.host_flags[1])) {
      delete ck;
      return e;
    }
    c->ck_list.push_back(ck);
    *out = ck;
    return 0;
  });
}

void kzgmi_ck_free(kzgmi_ck* ck) {
  if (!ck) return;
  if (kzgmi_ctx* c = ck->ctx) {
    (void)hipSetDevice(c->device);
    auto& v = c->ck_list;
    v.erase(std::remove(v.begin(), v.end(), ck), v.end());
    ck->pts.release();
    ck->inf.release();
  }
  delete ck;
}

int kzgmi_commit_device_async(kzgmi_ctx* c, const kzgmi_ck* ck, int slot, const void* d_coeffs, size_t m) {
  KZ_ROUTE(c, nullptr, slot);  // (commit keys live on the primary device: its slots only)
  CHK(check_ctx(c, slot));
  if (!ck || ck->ctx != c) return fail(KZGMI_ERR_ARG, "commit key does not belong to this context");
  if (m && !d_coeffs) return fail(KZGMI_ERR_ARG, "null argument");
  if (m > ck->n) return fail(KZGMI_ERR_ARG, "more coefficients than commit-key points");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_msm_wait first");
  return dispatch(ck->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using L = Launch<Cv>;
    const size_t gb = g1_bytes(Cv::ID);
    CHK(s.flags.ensure(16));
    CHK(s.outb.ensure(gb));
    CHK(s.res.ensure(2 * sizeof(Xyzz<Cv>)));
    CHK(begin_job(s));
    hipStream_t st = s.stream;
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
    if (m == 0) {
      HIPCHK(hipMemsetAsync(s.res.p, 0, sizeof(Xyzz<Cv>), st));  // zz = 0: infinity
    } else {
      CHK(s.scal_s.ensure(m * 32));
      mark(c, s, 0);
      L::convert_scalars(st, (const uint8_t*)d_coeffs, (uint32_t)m, s.scal_s.template as<uint32_t>(),
                         s.flags.template as<uint32_t>() + 1);
      mark(c, s, PH_SCALARS + 1);
      // one class per 16-bit window w: the points of row w (2^(16 w) P_i) take digit w of the
      // coefficient; every class feeds the same bucket set, so no per-window reduction and no
      // window combination
      TermList tl{};
      for (int w = 0; w < CK_ROWS; ++w)
        tl.c[w] = {(uint32_t)m, (uint32_t)(w * ck->n), 8, 1, 0, 8, s.scal_s.template as<uint32_t>(), (uint32_t)w};
      tl.nclass = CK_ROWS;
      tl.total = (uint32_t)(CK_ROWS * m);
      MsmWindows mw{1, {0, 0}, {1, 0}};
      CHK(HostCore<Cv>::run_msm_core(c, s, tl, 1, (size_t)CK_ROWS * m + 16, mw, ck->pts.template as<Affine<Cv>>(),
                                     ck->inf.template as<uint8_t>()));
    }
    Launch<Cv>::encode_points(st, s.res.template as<Xyzz<Cv>>(), 1, s.outb.template as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.host_out, s.outb.p, gb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
    CHK(end_job(s));
    arm(s, JobKind::MsmResult, Cv::ID);
    return 0;
  });
}

int kzgmi_commit_device(kzgmi_ctx* c, const kzgmi_ck* ck, const void* d_coeffs, size_t m, uint8_t* out) {
  if (!out) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(kzgmi_commit_device_async(c, ck, 0, d_coeffs, m));
  return kzgmi_msm_wait(c, 0, out);
}

int kzgmi_commit(kzgmi_ctx* c, const kzgmi_ck* ck, const uint8_t* coeffs, size_t m, uint8_t* out) {
  CHK(check_ctx(c));
  if (!ck || (m && !coeffs)) return fail(KZGMI_ERR_ARG, "null argument");
  if (m == 0) return kzgmi_commit_device(c, ck, nullptr, 0, out);
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  CHK(s.stage.ensure(m * 32));
  CHK(begin_job(s));  // the commit's job starts in the same lane, behind this copy
  HIPCHK(hipMemcpyAsync(s.stage.p, coeffs, m * 32, hipMemcpyHostToDevice, s.stream));
  return kzgmi_commit_device(c, ck, s.stage.p, m, out);
}

int kzgmi_msm_g1_device(kzgmi_ctx* c, kzgmi_curve curve, const void* dpts, const void* dsc, size_t n, uint8_t* out) {
  CHK(check_ctx(c));
  if (!out || (n && (!dpts || !dsc))) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "MSM too large (max 2^26 points per call)");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    const size_t gb = g1_bytes(Cv::ID);
    if (n == 0) {
      memset(out, 0, gb);
      if (Cv::ID == 0) out[0] = 0x40;
      return 0;
    }
    CHK(enqueue_msm_encoded<Cv>(c, s, dpts, dsc, n));
    CHK(read_flags_sync(c, s));
    HIPCHK(hipMemcpy(out, s.outb.p, gb, hipMemcpyDeviceToHost));
    return 0;
  });
}

int kzgmi_msm_g1_device_async(kzgmi_ctx* c, kzgmi_curve curve, int slot, const void* dpts, const void* dsc,
                              size_t n) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  if (n && (!dpts || !dsc)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "MSM too large (max 2^26 points per call)");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_msm_wait first");
  Roctx rx("kzgmi_msm_g1_device_async");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    const size_t gb = g1_bytes(Cv::ID);
    if (n == 0) {
      CHK(arm_empty(s, JobKind::MsmResult, Cv::ID));  // (host_out may still have been a copy target)
      memset(s.host_out, 0, gb);
      if (Cv::ID == 0) s.host_out[0] = 0x40;
      return 0;
    }
    CHK(enqueue_msm_encoded<Cv>(c, s, dpts, dsc, n));
    HIPCHK(hipMemcpyAsync(s.host_out, s.outb.p, gb, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
    CHK(end_job(s));
    arm(s, JobKind::MsmResult, Cv::ID);
    return 0;
  });
}

int kzgmi_msm_wait(kzgmi_ctx* c, int slot, uint8_t* out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  Slot& s = c->slots[slot];
  if (!s.pending || s.kind != JobKind::MsmResult) return fail(KZGMI_ERR_ARG, "slot has no pending MSM");
  int ok = 0;
  CHK(finish_slot(c, s, &ok));
  if (out) memcpy(out, s.host_out, g1_bytes(s.curve));
  return 0;
}

int kzgmi_msm_g1(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* points, const uint8_t* scalars, size_t n,
                 uint8_t* out) {
  CHK(check_ctx(c));
  if (!out || (n && (!points || !scalars))) return fail(KZGMI_ERR_ARG, "null argument");
  if (curve != KZGMI_BLS12_381 && curve != KZGMI_BN254) return fail(KZGMI_ERR_ARG, "unknown curve");
  if (n == 0) return kzgmi_msm_g1_device(c, curve, nullptr, nullptr, 0, out);
  CHK(slot0_idle(c));
  if (!c->peers.empty()) return msm_multi_host(c, curve, points, scalars, n, out);
  Slot& s = c->slots[0];
  const size_t gb = g1_bytes(curve);
  CHK(s.stage.ensure(n * (gb + 32)));
  uint8_t* dp = s.stage.template as<uint8_t>();
  uint8_t* ds = dp + n * gb;
  CHK(begin_job(s));  // the MSM's job starts in the same lane, behind these copies
  HIPCHK(hipMemcpyAsync(dp, points, n * gb, hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(ds, scalars, n * 32, hipMemcpyHostToDevice, s.stream));
  return kzgmi_msm_g1_device(c, curve, dp, ds, n, out);
}

int kzgmi_g1_compress_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_points, size_t n, void* d_out) {
  CHK(check_ctx(c));
  if (n && (!d_points || !d_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > (1u << 27)) return fail(KZGMI_ERR_ARG, "too many points (max 2^27 per call)");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  return dispatch(curve, [&](auto cv) -> int {
    CHK(begin_job(s));
    Launch<decltype(cv)>::compress_points(s.stream, (const uint8_t*)d_points, (uint32_t)n, (uint8_t*)d_out);
    HIPCHK(hipGetLastError());
    CHK(sync_job(s));
    return 0;
  });
}

int kzgmi_msm_partial_device(kzgmi_ctx* c, kzgmi_curve curve, const void* dpts, const void* dsc, size_t n,
                             void* d_partial_out) {
  CHK(check_ctx(c));
  if (!d_partial_out || (n && (!dpts || !dsc))) return fail(KZGMI_ERR_ARG, "bad argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "MSM too large (max 2^26 points per call)");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    if (n == 0) {
      Xyzz<Cv> h;
      memset(&h, 0, sizeof(h));
      HIPCHK(hipMemcpy(d_partial_out, &h, sizeof(h), hipMemcpyHostToDevice));
      return 0;
    }
    CHK(enqueue_msm_partial<Cv>(c, s, dpts, dsc, n, d_partial_out));
    return read_flags_sync(c, s);
  });
}

int kzgmi_msm_partial_device_async(kzgmi_ctx* c, kzgmi_curve curve, int slot, const void* dpts, const void* dsc,
                                   size_t n, void* d_partial_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  Roctx rx("kzgmi_msm_partial_device_async");
  if (!d_partial_out || (n && (!dpts || !dsc))) return fail(KZGMI_ERR_ARG, "bad argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "MSM too large (max 2^26 points per call)");
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    if (n == 0) {
      CHK(s.flags.ensure(16));
      CHK(sync_slot(s));  // host_flags may still be a copy target
      CHK(begin_job(s));
      HIPCHK(hipMemsetAsync(d_partial_out, 0, sizeof(Xyzz<Cv>), s.stream));  // ZZ = 0: infinity
      HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));  // a chained combine keeps the error word
      CHK(end_job(s));
      s.host_flags[0] = 1;
      s.host_flags[1] = 0;
    } else {
      CHK(enqueue_msm_partial<Cv>(c, s, dpts, dsc, n, d_partial_out));
      HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
      CHK(end_job(s));
    }
    arm(s, JobKind::MsmPartial, Cv::ID);
    return 0;
  });
}

int kzgmi_msm_combine_device_async(kzgmi_ctx* c, kzgmi_curve curve, int slot, const void* d_partials, int n_parts) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  if (!d_partials || n_parts < 1) return fail(KZGMI_ERR_ARG, "bad argument");
  Slot& s = c->slots[slot];
  const bool chain = s.pending && s.kind == JobKind::MsmPartial;  // behind this slot's own MSM partial
  if (s.pending && !chain) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_msm_wait first");
  if (chain && s.curve != (int)curve) return fail(KZGMI_ERR_ARG, "chained combine: curve differs from the partial's");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    CHK(enqueue_msm_combine<Cv>(s, d_partials, n_parts, chain));
    HIPCHK(hipMemcpyAsync(s.host_out, s.outb.p, g1_bytes(Cv::ID), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
    CHK(end_job(s));
    arm(s, JobKind::MsmResult, Cv::ID);
    return 0;
  });
}

int kzgmi_msm_combine_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_partials, int n_parts, uint8_t* out) {
  CHK(check_ctx(c));
  if (!d_partials || n_parts < 1 || !out) return fail(KZGMI_ERR_ARG, "bad argument");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    CHK(enqueue_msm_combine<Cv>(s, d_partials, n_parts, false));
    CHK(read_flags_sync(c, s));
    HIPCHK(hipMemcpy(out, s.outb.p, g1_bytes(Cv::ID), hipMemcpyDeviceToHost));
    return 0;
  });
}

// ------------------------------------------------------------------------------ pairing
int kzgmi_pairing(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* g1, const uint8_t* g2, uint8_t* out) {
  CHK(check_ctx(c));
  if (!g1 || !g2 || !out) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(slot0_idle(c));
  // BLS12-381: the pairing program's hard part is the x-chain of 3 (p^4 - p^2 + 1) / r, so it
  // yields e(P, Q)^3 (as the oracle and pyspec do); e(P, Q) = e([3^-1 mod r] P, Q)^3 for P in G1,
  // so P is first scaled by 3^-1 mod r with the library's MSM on one point, GLV forced off (the
  // GLV split is exact only on G1, and kzgmi_set_trusted_g1 must not change this diagnostic)
  uint8_t g1s[96];
  if (curve == KZGMI_BLS12_381) {
    static const uint8_t kInv3[32] = {0x4d, 0x49, 0x1a, 0x37, 0x71, 0x13, 0xa8, 0xda, 0xcc, 0xd1, 0x3a,
                                      0xb0, 0x06, 0x6b, 0xe5, 0x58, 0xe2, 0x7e, 0x6d, 0x57, 0x55, 0x54,
                                      0x3d, 0x54, 0xaa, 0xaa, 0xaa, 0xaa, 0x00, 0x00, 0x00, 0x01};
    using Cv = Bls12_381;
    Slot& s = c->slots[0];
    CHK(s.stage.ensure(96 + 32));
    CHK(s.outb.ensure(96));
    uint8_t* dp = s.stage.template as<uint8_t>();
    CHK(begin_job(s));  // the MSM's job starts in the same lane, behind these copies
    HIPCHK(hipMemcpyAsync(dp, g1, 96, hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(dp + 96, kInv3, 32, hipMemcpyHostToDevice, s.stream));
    CHK(HostCore<Cv>::enqueue_msm(c, s, dp, dp + 96, 1, /*allow_glv=*/false));
    Launch<Cv>::encode_points(s.stream, s.res.template as<Xyzz<Cv>>(), 1, s.outb.template as<uint8_t>());
    HIPCHK(hipGetLastError());
    CHK(read_flags_sync(c, s));
    HIPCHK(hipMemcpy(g1s, s.outb.p, 96, hipMemcpyDeviceToHost));
    g1 = g1s;
  }
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    const size_t gb1 = g1_bytes(Cv::ID), gb2 = g2_bytes(Cv::ID);
    const size_t fb = 12 * Cv::FP_BYTES;
    CHK(s.stage.ensure(gb1 + 2 * gb2 + 64));
    CHK(s.pts.ensure(sizeof(Affine<Cv>)));
    CHK(s.inf.ensure(16));
    CHK(s.flags.ensure(16));
    CHK(s.outb.ensure(fb));
    CHK(c->lines_tmp.ensure(2 * Launch<Cv>::num_lines() * sizeof(Line<Cv>) + 4 * sizeof(G2Aff<Cv>) + 64));
    std::vector<uint8_t> h(gb1 + 2 * gb2);
    memcpy(h.data(), g1, gb1);
    memcpy(h.data() + gb1, g2, gb2);
    memcpy(h.data() + gb1 + gb2, g2, gb2);
    CHK(begin_job(s));
    hipStream_t st = s.stream;
    uint8_t* d = s.stage.template as<uint8_t>();
    Line<Cv>* lines = c->lines_tmp.template as<Line<Cv>>();
    G2Aff<Cv>* q = reinterpret_cast<G2Aff<Cv>*>(lines + 2 * Launch<Cv>::num_lines());
    uint8_t* qinf = s.inf.template as<uint8_t>() + 8;
    HIPCHK(hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
    uint32_t* err = s.flags.template as<uint32_t>() + 1;
    Launch<Cv>::convert_points(st, d, 1, s.pts.template as<Affine<Cv>>(), s.inf.template as<uint8_t>(), err);
    Launch<Cv>::convert_g2(st, d + gb1, 2, q, qinf, err);
    Launch<Cv>::precompute_lines(st, q, lines);
    Launch<Cv>::pairing_one(st, s.pts.template as<Affine<Cv>>(), s.inf.template as<uint8_t>(), lines, qinf, s.outb.template as<uint8_t>());
    HIPCHK(hipGetLastError());
    CHK(read_flags_sync(c, s));
    HIPCHK(hipMemcpy(out, s.outb.p, fb, hipMemcpyDeviceToHost));
    return 0;
  });
}

// ------------------------------------------------------------------------------ generators
int kzgmi_gen_g1(kzgmi_ctx* c, kzgmi_curve curve, const void* d_scalars, size_t n, void* d_points_out) {
  CHK(check_ctx(c));
  if (n && (!d_scalars || !d_points_out)) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    CHK(begin_job(s));
    CHK(ensure_table<Cv>(c, s.stream));
    CHK(s.flags.ensure(16));
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
    if (n)
      Launch<Cv>::gen_g1(s.stream, (const uint8_t*)d_scalars, (uint32_t)n, c->table[Cv::ID].template as<Affine<Cv>>(),
                         (uint8_t*)d_points_out, s.flags.template as<uint32_t>() + 1);
    HIPCHK(hipGetLastError());
    return read_flags_sync(c, s);
  });
}

int kzgmi_gen_tuples(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* tau32, const uint8_t* seed32, size_t n,
                     void* dC, void* dz, void* dy, void* dpi) {
  CHK(check_ctx(c));
  if (!tau32 || !seed32 || (n && (!dC || !dz || !dy || !dpi))) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using FrF = Fp<typename Cv::FrP>;
    Slot& s = c->slots[0];
    CHK(begin_job(s));
    CHK(ensure_table<Cv>(c, s.stream));
    FrF tau;
    for (int k = 0; k < 8; ++k)
      tau.v[k] = (uint32_t)tau32[31 - 4 * k] | (uint32_t)tau32[30 - 4 * k] << 8 | (uint32_t)tau32[29 - 4 * k] << 16 |
                 (uint32_t)tau32[28 - 4 * k] << 24;
    // tau must be canonical
    for (int k = 7; k >= 0; --k) {
      if (tau.v[k] < Cv::FrP::MOD[k]) break;
      if (tau.v[k] > Cv::FrP::MOD[k] || k == 0) return fail(KZGMI_ERR_SCALAR, "tau >= r");
    }
    uint8_t sb[32];
    Seed seed = make_seed(seed32, sb);
    if (n)
      Launch<Cv>::gen_tuples(s.stream, seed, tau.v, (uint32_t)n, c->table[Cv::ID].template as<Affine<Cv>>(),
                                                           (uint8_t*)dC, (uint8_t*)dz, (uint8_t*)dy, (uint8_t*)dpi);
    HIPCHK(hipGetLastError());
    CHK(sync_job(s));
    return 0;
  });
}

int kzgmi_g2_mul(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* g2, const uint8_t* k32, uint8_t* out) {
  CHK(check_ctx(c));
  if (!g2 || !k32 || !out) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    const size_t gb = g2_bytes(Cv::ID);
    CHK(s.stage.ensure(2 * gb + 64));
    CHK(s.inf.ensure(16));
    CHK(s.flags.ensure(16));
    CHK(c->tmp.ensure(2 * sizeof(G2Aff<Cv>)));
    uint32_t k[8];
    for (int j = 0; j < 8; ++j)
      k[j] = (uint32_t)k32[31 - 4 * j] | (uint32_t)k32[30 - 4 * j] << 8 | (uint32_t)k32[29 - 4 * j] << 16 |
             (uint32_t)k32[28 - 4 * j] << 24;
    for (int j = 7; j >= 0; --j) {
      if (k[j] < Cv::FrP::MOD[j]) break;
      if (k[j] > Cv::FrP::MOD[j] || j == 0) return fail(KZGMI_ERR_SCALAR, "k >= r");
    }
    CHK(begin_job(s));
    hipStream_t st = s.stream;
    uint8_t* d = s.stage.template as<uint8_t>();
    HIPCHK(hipMemcpyAsync(d, g2, gb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
    Launch<Cv>::convert_g2(st, d, 1, c->tmp.template as<G2Aff<Cv>>(), s.inf.template as<uint8_t>(),
                           s.flags.template as<uint32_t>() + 1);
    Launch<Cv>::g2_mul(st, c->tmp.template as<G2Aff<Cv>>(), s.inf.template as<uint8_t>(), k, d + gb);
    HIPCHK(hipGetLastError());
    CHK(read_flags_sync(c, s));
    HIPCHK(hipMemcpy(out, d + gb, gb, hipMemcpyDeviceToHost));
    return 0;
  });
}

int kzgmi_probe_fpmul(kzgmi_ctx* c, kzgmi_curve curve, double* muls_per_s) {
  CHK(check_ctx(c));
  if (!muls_per_s) return fail(KZGMI_ERR_ARG, "null argument");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    const uint32_t blocks = 256 * 16, iters = 2048;
    CHK(c->tmp.ensure((size_t)blocks * 256 * 4));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    CHK(begin_job(s));
    Launch<Cv>::fpmul_probe(s.stream, blocks, 16, c->tmp.template as<uint32_t>());  // warm-up
    HIPCHK(hipEventRecord(e0, s.stream));
    Launch<Cv>::fpmul_probe(s.stream, blocks, iters, c->tmp.template as<uint32_t>());
    HIPCHK(hipEventRecord(e1, s.stream));
    CHK(sync_job(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *muls_per_s = (double)blocks * 256.0 * iters * 8.0 / (ms * 1e-3);
    return 0;
  });
}

int kzgmi_partial_encode_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_records, size_t count, uint8_t* out) {
  CHK(check_ctx(c));
  if (!d_records || !out || count == 0 || count > 4096) return fail(KZGMI_ERR_ARG, "bad argument");
  CHK(slot0_idle(c));
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    Slot& s = c->slots[0];
    const size_t gb = g1_bytes(Cv::ID);
    CHK(s.outb.ensure(count * gb));
    CHK(begin_job(s));
    Launch<Cv>::encode_points(s.stream, (const Xyzz<Cv>*)d_records, (uint32_t)count, s.outb.template as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, s.outb.p, count * gb, hipMemcpyDeviceToHost, s.stream));
    CHK(sync_job(s));
    return 0;
  });
}

}  // extern "C"
