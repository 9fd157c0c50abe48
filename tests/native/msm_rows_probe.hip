// Test-only probe of the row accumulation (csrc/msm.hpp k_items_*, k_accumulate_rows, k_join_rows)
// through its shipped launchers, Launch<Cv>::row_items and accumulate_rows of csrc/launch_msm.hip
// (tests/test_gpu_msm_rows.py, tests/test_msm_rows_cpu.py).  It stands on tests/native/msm_probe.hip,
// included whole: the same call description, the same host-side check of a hand-made sorted list
// (nothing is launched on a list the sort could not have written), the same buffers at their planned
// sizes behind guards, poisoned first.  No arithmetic and no kernel of its own.  Built into
// kzgmi/libkzgmi_msmrowsprobe.so, one object per curve; never linked into libkzgmi.so.
//
// A call is msm_probe.hip's desc plus ext (uint64 x 3): MsmTuning::acc_rows, MsmTuning::row_len (L)
// and plan_msm's async_call -- the three inputs of the plan the older description does not carry.
#include "msm_probe.hip"

enum { B_ROWQ = B_COUNT, B_ITEMS, B_CUTS, B_ROWS_COUNT };
constexpr int kRowsPlanWords = 19;

namespace {

bool read_rows_call(const uint64_t* desc, const uint64_t* ext, Call& c) {
  if (!read_call(desc, c)) return false;
  if (ext[1] < 1 || ext[1] > ROW_LEN_MAX) return false;
  c.t.acc_rows = (int)(int64_t)ext[0];
  c.t.row_len = (uint32_t)ext[1];
  c.p = plan_msm<Cv>(c.t, c.tl, c.nsets, c.emax, c.mw, c.wbits, c.part, /*own_pts=*/true, c.alone, c.sync_call, ext[2] != 0);
  return c.p.refuse == nullptr;
}

void rows_guards(Dev& dv, uint32_t* out) {
  for (int i = B_COUNT; i < B_ROWS_COUNT; ++i) out[i] = 2;
  dv.guards(out);
}

struct RowBufs {
  uint32_t *rowq, *items, *cuts;
};
RowBufs row_bufs(Dev& dv, const MsmBytes& z) {
  return {dv.get<uint32_t>(B_ROWQ, z.rowq), dv.get<uint32_t>(B_ITEMS, z.items), dv.get<uint32_t>(B_CUTS, z.cuts)};
}

// read_call for a call that is only planned: the same fields of the description and the same checks
// of them, but any emax a plan takes -- nothing is launched on it, and the planner's threshold for rows
// stands far above the stage tests' bound (MAX_EMAX)
bool read_plan_call(const uint64_t* d, const uint64_t* ext, Call& c) {
  c.t = tuning_of(d);
  c.nsets = (uint32_t)d[15];
  c.emax = (size_t)d[16];
  c.mw = MsmWindows{(uint32_t)d[17], {(uint32_t)d[18], (uint32_t)d[19]}, {(uint32_t)d[20], (uint32_t)d[21]}};
  c.wbits = (int)d[22];
  c.part = (int)d[23];
  c.alone = d[24] != 0;
  c.sync_call = d[25] != 0;
  c.poison = (uint8_t)d[26];
  c.tl = terms_of(d + kDescHead);
  if (c.wbits != 13 && c.wbits != WBITS) return false;
  if (c.nsets < 1 || c.nsets > (uint32_t)MAX_SETS || c.emax < 16 || c.emax >= (size_t(1) << 32)) return false;
  if (c.part < 0 || c.part > 3 || c.tl.nclass > (uint32_t)MAX_CLASSES) return false;
  if (c.mw.nmsm < 1 || c.mw.nmsm > 2) return false;
  for (uint32_t m = 0; m < c.mw.nmsm; ++m)
    if (c.mw.nwin[m] < 1 || c.mw.set_base[m] + c.mw.nwin[m] > c.nsets) return false;
  const uint32_t maxw = c.wbits == 13 ? Win<13>::MAXW : Win<WBITS>::MAXW;
  uint64_t total = 0, entries = 0;
  for (uint32_t k = 0; k < c.tl.nclass; ++k) {
    const TermClass& C = c.tl.c[k];
    if (C.scal_words != 4 && C.scal_words != 8) return false;
    if (C.scal_stride != 0 && C.scal_stride != C.scal_words) return false;
    if (C.nwin < 1 || C.set_base + C.nwin > c.nsets || C.win_off + C.nwin > maxw) return false;
    total += C.count;
    entries += (uint64_t)C.count * C.nwin;
  }
  if (total != c.tl.total || entries + 16 > c.emax) return false;
  if (ext[1] < 1 || ext[1] > ROW_LEN_MAX) return false;
  c.t.acc_rows = (int)(int64_t)ext[0];
  c.t.row_len = (uint32_t)ext[1];
  c.p = plan_msm<Cv>(c.t, c.tl, c.nsets, c.emax, c.mw, c.wbits, c.part, /*own_pts=*/true, c.alone, c.sync_call, ext[2] != 0);
  return c.p.refuse == nullptr;
}

}  // namespace

// the plan's row fields, host code only
int PROBE_FN(rows_plan)(const uint64_t* desc, const uint64_t* ext, uint64_t* o) {
  Call c;
  std::memset(o, 0, kRowsPlanWords * sizeof(uint64_t));
  if (!read_plan_call(desc, ext, c)) return PROBE_ERR_ARG;
  const MsmPlan& p = c.p;
  const MsmBytes& z = p.bytes;
  const uint64_t w[kRowsPlanWords] = {p.small, p.rows, p.row_len, p.row_items, p.row_pieces, p.row_cuts, z.rowq, z.items,
                                      z.cuts, z.acc29, p.NB, p.nchunks, p.pieces, p.split, p.acc_threads,
                                      RQ_NITEMS, RQ_NCUT, RQ_PIECES, RQ_HIST};
  for (uint64_t x : w) *o++ = x;
  return 0;
}

// A hand-made sorted list through pts_to29, row_items and accumulate_rows.  rowq: RQ_WORDS words,
// items: 3 x row_items, cuts: 3 x row_cuts, acc_out: the whole store (NB + piece records)
int PROBE_FN(rows_accumulate)(const uint64_t* desc, const uint64_t* ext, const uint32_t* points, uint32_t npts,
                              const uint32_t* sval, const uint32_t* skey, const uint32_t* off, const uint32_t* cnt,
                              uint32_t total, uint32_t* rowq_out, uint32_t* items_out, uint32_t* cuts_out,
                              uint32_t* acc_out, uint32_t* guards) {
  Call c;
  if (!read_rows_call(desc, ext, c) || c.part != 0) return PROBE_ERR_ARG;
  const MsmPlan& p = c.p;
  if (p.small || !p.rows) return PROBE_ERR_PLAN;
  if (!sorted_ok(p, sval, skey, off, cnt, total, c.emax, npts)) return PROBE_ERR_ARG;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  AF* dpts = dv.get<AF>(B_PTS, (size_t)npts * sizeof(AF));
  uint32_t* dsval = dv.get<uint32_t>(B_SVAL, z.sval);
  uint32_t* doff = dv.get<uint32_t>(B_OFF, z.off);
  uint32_t* dcnt = dv.get<uint32_t>(B_CNT, z.cnt);
  uint32_t* dacc = dv.get<uint32_t>(B_ACC29, z.acc29);
  const RowBufs rb = row_bufs(dv, z);
  dv.put(dpts, points, (size_t)npts * sizeof(AF));
  dv.put(dsval, sval, (size_t)total * 4);
  dv.put(doff, off, z.off);
  dv.put(dcnt, cnt, z.cnt);
  if (rc == 0) {
    L::pts_to29(nullptr, dpts, npts);
    L::row_items(nullptr, doff, dcnt, p.NB, p.row_len, rb.rowq, rb.items, (uint32_t)p.row_items, rb.cuts, (uint32_t)p.row_cuts);
    L::accumulate_rows(nullptr, p.nchunks, dsval, dpts, dacc, p.NB, rb.rowq, rb.items, (uint32_t)p.row_items, rb.cuts,
                       (uint32_t)p.row_cuts);
    dv.finish();
  }
  dv.take(rowq_out, rb.rowq, z.rowq);
  dv.take(items_out, rb.items, z.items);
  dv.take(cuts_out, rb.cuts, z.cuts);
  dv.take(acc_out, dacc, z.acc29);
  rows_guards(dv, guards);
  return rc;
}

// The whole chain on a term list: sort -> items -> rows -> joins -> reduce -> combine; res: 2 points
int PROBE_FN(rows_msm)(const uint64_t* desc, const uint64_t* ext, const uint32_t* scal, uint64_t nscal,
                       const uint32_t* points, const uint8_t* inf, uint32_t npts, uint32_t* rowq_out, uint32_t* res,
                       uint32_t* guards) {
  Call c;
  if (!read_rows_call(desc, ext, c) || c.part != 0) return PROBE_ERR_ARG;
  MsmPlan& p = c.p;
  if (p.small || !p.rows) return PROBE_ERR_PLAN;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  if (!bind_scalars(dv, p, scal, nscal, npts)) return PROBE_ERR_ARG;
  AF* dpts = dv.get<AF>(B_PTS, (size_t)npts * sizeof(AF));
  uint8_t* dinf = dv.get<uint8_t>(B_INF, npts);
  uint32_t* ddig = dv.get<uint32_t>(B_DIGITS, z.digits);
  uint32_t* dcoarse = dv.get<uint32_t>(B_COARSE, z.coarse);
  uint64_t* dent = dv.get<uint64_t>(B_ENT, z.ent);
  uint32_t* dtotal = dv.get<uint32_t>(B_TOTAL, z.total);
  uint32_t* dsval = dv.get<uint32_t>(B_SVAL, z.sval);
  uint32_t* dskey = dv.get<uint32_t>(B_SKEY, z.skey);
  uint32_t* doff = dv.get<uint32_t>(B_OFF, z.off);
  uint32_t* dcnt = dv.get<uint32_t>(B_CNT, z.cnt);
  uint32_t* dacc = dv.get<uint32_t>(B_ACC29, z.acc29);
  XY* dR = dv.get<XY>(B_R, z.R);
  XY* dU = dv.get<XY>(B_U, z.U);
  XY* dscratch = dv.get<XY>(B_SCRATCH, z.scratch);
  XY* dwinsum = dv.get<XY>(B_WINSUM, z.winsum);
  XY* dres = dv.get<XY>(B_RES, z.res);
  const RowBufs rb = row_bufs(dv, z);
  dv.put(dpts, points, (size_t)npts * sizeof(AF));
  dv.put(dinf, inf, npts);
  if (rc == 0) {
    L::pts_to29(nullptr, dpts, npts);
    L::sort(nullptr, p.tl, c.nsets, dinf, ddig, dcoarse, dent, c.emax, 0, doff, dcnt, dtotal, dsval, dskey, c.wbits);
    L::row_items(nullptr, doff, dcnt, p.NB, p.row_len, rb.rowq, rb.items, (uint32_t)p.row_items, rb.cuts, (uint32_t)p.row_cuts);
    L::accumulate_rows(nullptr, p.nchunks, dsval, dpts, dacc, p.NB, rb.rowq, rb.items, (uint32_t)p.row_items, rb.cuts,
                       (uint32_t)p.row_cuts);
    L::reduce(nullptr, c.nsets, dcnt, dacc, dR, dU, dscratch, dwinsum, c.wbits, false, c.t.seg4_waves, 1024);
    L::window_combine(nullptr, c.mw, dwinsum, dres, c.wbits, false);
    dv.finish();
  }
  dv.take(rowq_out, rb.rowq, z.rowq);
  dv.take(res, dres, z.res);
  rows_guards(dv, guards);
  return rc;
}

#if KZ_CURVE == 0
int msmprobe_rows_plan_1(const uint64_t*, const uint64_t*, uint64_t*);
int msmprobe_rows_accumulate_1(const uint64_t*, const uint64_t*, const uint32_t*, uint32_t, const uint32_t*, const uint32_t*,
                               const uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*,
                               uint32_t*);
int msmprobe_rows_msm_1(const uint64_t*, const uint64_t*, const uint32_t*, uint64_t, const uint32_t*, const uint8_t*,
                        uint32_t, uint32_t*, uint32_t*, uint32_t*);

PROBE_API int kzgmi_msmrowsprobe_plan_words() { return kRowsPlanWords; }
PROBE_API int kzgmi_msmrowsprobe_guard_words() { return B_ROWS_COUNT; }
PROBE_API int kzgmi_msmrowsprobe_rowq_words() { return (int)kzgmi::RQ_WORDS; }
PROBE_API int kzgmi_msmrowsprobe_plan(int curve, const uint64_t* desc, const uint64_t* ext, uint64_t* out) {
  PROBE_DISPATCH(rows_plan, desc, ext, out);
}
PROBE_API int kzgmi_msmrowsprobe_accumulate(int curve, const uint64_t* desc, const uint64_t* ext, const uint32_t* points,
                                            uint32_t npts, const uint32_t* sval, const uint32_t* skey, const uint32_t* off,
                                            const uint32_t* cnt, uint32_t total, uint32_t* rowq, uint32_t* items,
                                            uint32_t* cuts, uint32_t* acc, uint32_t* guards) {
  PROBE_DISPATCH(rows_accumulate, desc, ext, points, npts, sval, skey, off, cnt, total, rowq, items, cuts, acc, guards);
}
PROBE_API int kzgmi_msmrowsprobe_msm(int curve, const uint64_t* desc, const uint64_t* ext, const uint32_t* scal,
                                     uint64_t nscal, const uint32_t* points, const uint8_t* inf, uint32_t npts,
                                     uint32_t* rowq, uint32_t* res, uint32_t* guards) {
  PROBE_DISPATCH(rows_msm, desc, ext, scal, nscal, points, inf, npts, rowq, res, guards);
}
#endif
