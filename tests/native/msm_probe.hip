// Test-only probe of the bucket MSM pipeline, one stage per call (tests/test_gpu_msm_stages.py):
// the shipped launchers of csrc/launch_msm.hip -- Launch<Cv>::sort / pts_to29 / accumulate / fixup /
// merge_buckets / reduce / window_combine / small_msm -- on caller-supplied inputs, every output
// copied back.  No field or curve arithmetic lives here and no kernel of its own: buffers are
// filled and read with hipMemset and copies only.  Built into kzgmi/libkzgmi_msmprobe.so, one
// object per curve (-DKZ_CURVE=0/1); never linked into libkzgmi.so.
//
// Every call plans with plan_msm<Cv> (csrc/msm_plan.hpp), as HostCore::run_msm_core does, from the
// caller's MsmTuning, TermList, nsets, emax and MsmWindows, and allocates every buffer at exactly
// its planned size (MsmBytes) followed by a guard of GUARD bytes.  The buffers a stage writes are
// filled with the caller's poison byte first, the guards with GUARD_BYTE; after the stage each
// guard is read back: guards_out[buffer id] = 1 intact, 0 overwritten, 2 not used by this stage.
// Everything runs on the null stream with one synchronise at the end.
//
// Hand-made inputs are checked on the host first and an inconsistent one is refused with
// PROBE_ERR_ARG before anything is launched: the kernels only ever see what the shipped host code
// could hand them (sorted keys non-decreasing and inside the sets, off / cnt agreeing with the
// keys, SV_FIRST on the first entry of a bucket and nowhere else, point indices inside the points
// given, records with normalised limbs).  kzgmi_msmprobe_check_sorted is that check of the
// accumulate stage's arguments alone, host code only, so a test without a GPU can hold the
// hand-made lists to it.
//
// desc (uint64): MsmTuning (tests/native/plan_args.hpp), nsets, emax, MsmWindows (nmsm, set_base
// x 2, nwin x 2), wbits, part, alone, sync_call, poison byte, 0, then the TermList, a class's
// `scal` being the word offset of its first scalar in the scalar array of the call.
// The ctypes side and the names of the guard ids are in tests/msmprobe.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "plan_args.hpp"
#include "launch_msm.hip"

#if KZ_CURVE == 0
#define PROBE_FN(name) msmprobe_##name##_0
#else
#define PROBE_FN(name) msmprobe_##name##_1
#endif

enum { PROBE_ERR_CURVE = -1, PROBE_ERR_ARG = -2, PROBE_ERR_PLAN = -3, PROBE_ERR_HIP = 1000 };
// guard ids (tests/msmprobe.py GUARDS)
enum {
  B_DIGITS, B_CNT, B_OFF, B_COARSE, B_ENT, B_TOTAL, B_ACCQ, B_CROWD, B_SVAL, B_SKEY, B_ACC29, B_ACC29B, B_CNTB,
  B_R, B_U, B_SCRATCH, B_WINSUM, B_RES, B_PTS, B_INF, B_SCAL, B_NODES, B_FLAGS, B_SNAP, B_COUNT
};
constexpr int kDescHead = 28, kPlanWords = 2 + 14 + 21 + 3 + kzgmi::MAX_CLASSES + 3;

namespace {
using namespace kzgmi;
using namespace kzgmi_probe;
using Cv = KZ_CURVE_T;
using L = Launch<Cv>;
using XY = Xyzz<Cv>;
using AF = Affine<Cv>;
constexpr size_t GUARD = 4096;
constexpr uint8_t GUARD_BYTE = 0x5C;
constexpr int W29 = kW29<Fp29Of<Cv>>, N29 = Fp29Of<Cv>::N;
constexpr size_t REC = (size_t)W29 * 4;
constexpr size_t MAX_EMAX = size_t(1) << 22;  // the stage tests stay far below

#define PROBE_HIP(call)                                                \
  do {                                                                 \
    const hipError_t err_ = (call);                                    \
    if (err_ != hipSuccess && rc == 0) rc = PROBE_ERR_HIP + (int)err_; \
  } while (0)

struct Call {
  MsmTuning t;
  TermList tl;
  uint32_t nsets;
  size_t emax;
  MsmWindows mw;
  int wbits, part;
  bool alone, sync_call;
  uint8_t poison;
  MsmPlan p;
};

// the call's description and its plan; false: refused (nothing may be launched)
bool read_call(const uint64_t* d, Call& c) {
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
  if (c.nsets < 1 || c.nsets > (uint32_t)MAX_SETS || c.emax < 16 || c.emax > MAX_EMAX) return false;
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
  c.p = plan_msm<Cv>(c.t, c.tl, c.nsets, c.emax, c.mw, c.wbits, c.part, /*own_pts=*/true, c.alone, c.sync_call);
  return c.p.refuse == nullptr;
}

// device buffers of one call: planned size + guard, freed on every path
struct Dev {
  struct B { uint8_t* p; size_t bytes; int id; };
  std::vector<B> bufs;
  int rc = 0;
  uint8_t poison;
  explicit Dev(uint8_t poison_byte) : poison(poison_byte) {}
  template <class T>
  T* get(int id, size_t bytes) {
    void* d = nullptr;
    PROBE_HIP(hipMalloc(&d, bytes + GUARD));
    if (!d) return nullptr;
    bufs.push_back({static_cast<uint8_t*>(d), bytes, id});
    if (bytes) PROBE_HIP(hipMemset(d, poison, bytes));
    PROBE_HIP(hipMemset(static_cast<uint8_t*>(d) + bytes, GUARD_BYTE, GUARD));
    return static_cast<T*>(d);
  }
  void put(void* dst, const void* src, size_t bytes) {
    if (rc == 0 && bytes) PROBE_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  }
  void take(void* dst, const void* src, size_t bytes) {
    if (rc == 0 && bytes) PROBE_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  }
  void finish() {
    if (rc == 0) PROBE_HIP(hipGetLastError());
    if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
  }
  void guards(uint32_t* out) {
    for (int i = 0; i < B_COUNT; ++i) out[i] = 2;
    std::vector<uint8_t> g(GUARD);
    for (const B& b : bufs) {
      take(g.data(), b.p + b.bytes, GUARD);
      bool ok = rc == 0;
      for (size_t i = 0; ok && i < GUARD; ++i) ok = g[i] == GUARD_BYTE;
      out[b.id] = ok ? 1 : 0;
    }
  }
  ~Dev() {
    for (const B& b : bufs) (void)hipFree(b.p);
  }
};

// the scalars on the device and the classes' pointers into them; false: a class reads outside
bool bind_scalars(Dev& dv, MsmPlan& p, const uint32_t* scal, uint64_t nscal, uint32_t npts) {
  for (uint32_t k = 0; k < p.tl.nclass; ++k) {
    const TermClass& C = p.tl.c[k];
    const uint64_t o = (uint64_t)(uintptr_t)C.scal;  // word offset; 16-B aligned: the kernels load uint4
    const uint64_t words = C.scal_stride ? (uint64_t)C.count * C.scal_stride : C.scal_words;
    if (o % 4 || o + (C.count ? words : 0) > nscal) return false;
    if ((uint64_t)C.pt_base + C.count > npts) return false;
    // full scalars stay below 2^255 (convert_scalars admits values below r only): the narrowed
    // coarse bins of a short top window (SetShift) rest on it
    for (uint64_t i = 0; C.scal_words == 8 && i < (C.scal_stride ? C.count : (C.count ? 1u : 0u)); ++i)
      if (scal[o + i * C.scal_stride + 7] >> 31) return false;
  }
  uint32_t* d = dv.get<uint32_t>(B_SCAL, nscal * 4);
  dv.put(d, scal, nscal * 4);
  for (uint32_t k = 0; k < p.tl.nclass; ++k) p.tl.c[k].scal = d + (uintptr_t)p.tl.c[k].scal;
  return true;
}

// records with cnt != 0 must have normalised limbs (all but each coordinate's top one below 2^29)
bool records_ok(const uint32_t* cnt, const uint32_t* rec, uint32_t nb) {
  for (uint32_t b = 0; b < nb; ++b) {
    if (!cnt[b]) continue;
    for (int k = 0; k < W29; ++k)
      if ((k + 1) % N29 && rec[(size_t)b * W29 + k] >> 29) return false;
  }
  return true;
}
// [nb records] with every cnt == 0 record left as poison
std::vector<uint32_t> stage_records(const uint32_t* cnt, const uint32_t* rec, uint32_t nb, uint8_t poison) {
  std::vector<uint32_t> v((size_t)nb * W29, 0x01010101u * poison);
  for (uint32_t b = 0; b < nb; ++b)
    if (cnt[b]) std::memcpy(&v[(size_t)b * W29], rec + (size_t)b * W29, REC);
  return v;
}

// a hand-made or sorted entry list against the contract of the sort's outputs
bool sorted_ok(const MsmPlan& p, const uint32_t* sval, const uint32_t* skey, const uint32_t* off, const uint32_t* cnt,
               uint32_t total, size_t emax, uint32_t npts) {
  if ((size_t)total + 16 > emax) return false;
  std::vector<uint32_t> seen(p.NB, 0);
  for (uint32_t e = 0; e < total; ++e) {
    const uint32_t key = skey[e];
    if (key >= p.NB || (e && key < skey[e - 1])) return false;
    const bool first = e == 0 || key != skey[e - 1];
    if (first && (off[key] != e || cnt[key] == 0 || (size_t)e + cnt[key] > total)) return false;
    if (!first && e >= off[key] + cnt[key]) return false;
    if (((sval[e] & SV_FIRST) != 0) != first) return false;
    if (((sval[e] & ~SV_FIRST) >> 1) >= npts) return false;
    seen[key] = 1;
  }
  for (uint32_t b = 0; b < p.NB; ++b)
    if (!seen[b] && cnt[b]) return false;
  return true;
}

// the accumulate stage's arguments: 0 and the call read, or the refusal (no HIP call is made here)
int accumulate_args(const uint64_t* desc, uint32_t npts, const uint32_t* sval, const uint32_t* skey, const uint32_t* off,
                    const uint32_t* cnt, uint32_t total, uint32_t mid, Call& c) {
  if (!read_call(desc, c) || c.part != 0) return PROBE_ERR_ARG;
  const MsmPlan& p = c.p;
  if (p.small) return PROBE_ERR_PLAN;
  if (!sorted_ok(p, sval, skey, off, cnt, total, c.emax, npts)) return PROBE_ERR_ARG;
  if (p.split) {
    if (!c.t.split_side_fix || mid > total) return PROBE_ERR_ARG;  // the launches' pieces must not share records
    const uint32_t k0 = p.split_set * p.nbuckets;
    if ((mid > 0 && skey[mid - 1] >= k0) || (mid < total && skey[mid] < k0)) return PROBE_ERR_ARG;
  }
  return 0;
}

}  // namespace

// the check the accumulate stage makes of its arguments before it launches, alone (no GPU needed)
int PROBE_FN(check_sorted)(const uint64_t* desc, uint32_t npts, const uint32_t* sval, const uint32_t* skey,
                           const uint32_t* off, const uint32_t* cnt, uint32_t total, uint32_t mid) {
  Call c;
  return accumulate_args(desc, npts, sval, skey, off, cnt, total, mid, c);
}

int PROBE_FN(plan)(const uint64_t* desc, uint64_t* o) {
  Call c;
  std::memset(o, 0, kPlanWords * sizeof(uint64_t));
  if (!read_call(desc, c)) {
    o[0] = 1;
    return PROBE_ERR_ARG;
  }
  const MsmPlan& p = c.p;
  const MsmBytes& z = p.bytes;
  const uint64_t w[] = {0, p.small, p.ndig, p.own_npts, p.nbuckets, p.bins, p.rb_parts, p.NB, p.nchunks, p.acc_threads,
                        p.can_split, p.split, p.split_set, p.pieces, p.crowd_words, p.second,
                        z.small_nodes, z.small_flags, z.digits, z.cnt, z.off, z.cntb, z.offb, z.coarse, z.ent, z.total,
                        z.accq, z.crowd, z.sval, z.skey, z.acc29, z.acc29b, z.R, z.U, z.scratch, z.winsum, z.res,
                        p.small_terms, p.small_nodes, p.small_flags};
  for (uint64_t x : w) *o++ = x;
  for (int k = 0; k < MAX_CLASSES; ++k) *o++ = p.tl.c[k].dig_base;
  *o++ = W29;
  *o++ = sizeof(XY) / 4;
  *o++ = sizeof(AF) / 4;
  return 0;
}

// digits: ndig words; coarse: 3 nsets bins (counts, offsets, cursors); sval, skey: emax words (the
// entries from *total on stay poison); off, cnt: NB words
int PROBE_FN(sort)(const uint64_t* desc, const uint32_t* scal, uint64_t nscal, const uint8_t* inf, uint32_t npts,
                   uint32_t* digits, uint32_t* coarse, uint32_t* total, uint32_t* sval, uint32_t* skey, uint32_t* off,
                   uint32_t* cnt, uint32_t* guards) {
  Call c;
  if (!read_call(desc, c) || c.part != 0) return PROBE_ERR_ARG;
  MsmPlan& p = c.p;
  if (p.small) return PROBE_ERR_PLAN;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  if (!bind_scalars(dv, p, scal, nscal, npts)) return PROBE_ERR_ARG;
  uint8_t* dinf = dv.get<uint8_t>(B_INF, npts);
  uint32_t* ddig = dv.get<uint32_t>(B_DIGITS, z.digits);
  uint32_t* dcoarse = dv.get<uint32_t>(B_COARSE, z.coarse);
  uint64_t* dent = dv.get<uint64_t>(B_ENT, z.ent);
  uint32_t* dtotal = dv.get<uint32_t>(B_TOTAL, z.total);
  uint32_t* dsval = dv.get<uint32_t>(B_SVAL, z.sval);
  uint32_t* dskey = dv.get<uint32_t>(B_SKEY, z.skey);
  uint32_t* doff = dv.get<uint32_t>(B_OFF, z.off);
  uint32_t* dcnt = dv.get<uint32_t>(B_CNT, z.cnt);
  dv.put(dinf, inf, npts);
  if (rc == 0) {
    L::sort(nullptr, p.tl, c.nsets, dinf, ddig, dcoarse, dent, c.emax,
            (c.t.sort_split ? L::SORT_SPLIT : 0) | (c.t.sort_full_bins ? L::SORT_FULL_BINS : 0), doff, dcnt, dtotal, dsval,
            dskey, c.wbits);
    dv.finish();
  }
  dv.take(digits, ddig, z.digits);
  dv.take(coarse, dcoarse, z.coarse);
  dv.take(total, dtotal, 4);
  dv.take(sval, dsval, c.emax * 4);
  dv.take(skey, dskey, z.skey);
  dv.take(off, doff, z.off);
  dv.take(cnt, dcnt, z.cnt);
  dv.guards(guards);
  return rc;
}

// points: npts affine points in 32-bit Montgomery words (put into the accumulation's format here);
// sval, skey: total words; off, cnt: NB words; mid: the first entry of set split_set (read only by a
// split plan, which runs its two launches one after the other in the order split_rev says).
// acc_mid: the whole bucket store (NB + 2 pieces records) after k_accumulate alone, acc_out: after
// the joins; crowd: the crowded lists (a split's second behind the first)
int PROBE_FN(accumulate)(const uint64_t* desc, const uint32_t* points, uint32_t npts, const uint32_t* sval,
                         const uint32_t* skey, const uint32_t* off, const uint32_t* cnt, uint32_t total, uint32_t mid,
                         uint32_t* acc_mid, uint32_t* acc_out, uint32_t* crowd_out, uint32_t* guards) {
  Call c;
  if (const int bad = accumulate_args(desc, npts, sval, skey, off, cnt, total, mid, c)) return bad;
  const MsmPlan& p = c.p;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  AF* dpts = dv.get<AF>(B_PTS, (size_t)npts * sizeof(AF));
  uint32_t* dcoarse = dv.get<uint32_t>(B_COARSE, z.coarse);
  uint32_t* dtotal = dv.get<uint32_t>(B_TOTAL, z.total);
  uint32_t* dsval = dv.get<uint32_t>(B_SVAL, z.sval);
  uint32_t* dskey = dv.get<uint32_t>(B_SKEY, z.skey);
  uint32_t* doff = dv.get<uint32_t>(B_OFF, z.off);
  uint32_t* dcnt = dv.get<uint32_t>(B_CNT, z.cnt);
  uint32_t* dacc = dv.get<uint32_t>(B_ACC29, z.acc29);
  uint32_t* dsnap = dv.get<uint32_t>(B_SNAP, z.acc29);
  uint32_t* dcrowd = dv.get<uint32_t>(B_CROWD, z.crowd);
  uint32_t* daccq = p.acc_threads ? dv.get<uint32_t>(B_ACCQ, z.accq) : nullptr;
  dv.put(dpts, points, (size_t)npts * sizeof(AF));
  dv.put(dsval, sval, (size_t)total * 4);
  dv.put(dskey, skey, (size_t)total * 4);
  dv.put(doff, off, z.off);
  dv.put(dcnt, cnt, z.cnt);
  dv.put(dtotal, &total, 4);
  uint32_t* dmid = dcoarse + (size_t)c.nsets * p.bins + (size_t)p.split_set * p.bins;  // run_msm_core's `mid`
  if (p.split) dv.put(dmid, &mid, 4);
  if (rc == 0) {
    L::pts_to29(nullptr, dpts, npts);
    if (p.split) {
      const bool rev = c.t.split_rev;
      const uint32_t* total_a = rev ? dmid : dtotal;
      const uint32_t* lo_a = rev ? nullptr : dmid;
      const uint32_t* total_b = rev ? dtotal : dmid;
      const uint32_t* lo_b = rev ? dmid : nullptr;
      const uint32_t nb_b = (uint32_t)(p.NB + 2 * p.nchunks);
      uint32_t* crowd_b = dcrowd + p.crowd_words;
      L::accumulate(nullptr, p.nchunks, total_a, dsval, dskey, doff, dcnt, dpts, dacc, p.NB, p.acc_threads, daccq, dcrowd,
                    lo_a, nullptr);
      L::accumulate(nullptr, p.nchunks, total_b, dsval, dskey, doff, dcnt, dpts, dacc, nb_b, p.acc_threads, daccq, crowd_b,
                    lo_b, nullptr);
      PROBE_HIP(hipMemcpyAsync(dsnap, dacc, z.acc29, hipMemcpyDeviceToDevice, nullptr));
      L::fixup(nullptr, p.nchunks, total_b, dskey, doff, dcnt, dacc, nb_b, crowd_b, lo_b);
      L::fixup(nullptr, p.nchunks, total_a, dskey, doff, dcnt, dacc, p.NB, dcrowd, lo_a);
    } else {
      L::accumulate(nullptr, p.nchunks, dtotal, dsval, dskey, doff, dcnt, dpts, dacc, p.NB, p.acc_threads, daccq, dcrowd,
                    nullptr, nullptr);
      PROBE_HIP(hipMemcpyAsync(dsnap, dacc, z.acc29, hipMemcpyDeviceToDevice, nullptr));
      L::fixup(nullptr, p.nchunks, dtotal, dskey, doff, dcnt, dacc, p.NB, dcrowd, nullptr);
    }
    dv.finish();
  }
  dv.take(acc_mid, dsnap, z.acc29);
  dv.take(acc_out, dacc, z.acc29);
  dv.take(crowd_out, dcrowd, z.crowd);
  dv.guards(guards);
  return rc;
}

// two bucket stores (NB records each, the records of empty buckets ignored and left as poison) and
// their counts, planned as a range of part 2 or 3; the merged store and counts out
int PROBE_FN(merge)(const uint64_t* desc, const uint32_t* acc_a, const uint32_t* cnt_a, const uint32_t* acc_b,
                    const uint32_t* cnt_b, uint32_t* acc_out, uint32_t* cnt_out, uint32_t* guards) {
  Call c;
  if (!read_call(desc, c) || c.part < 2) return PROBE_ERR_ARG;
  const MsmPlan& p = c.p;
  if (p.small) return PROBE_ERR_PLAN;
  if (!records_ok(cnt_a, acc_a, p.NB) || !records_ok(cnt_b, acc_b, p.NB)) return PROBE_ERR_ARG;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  uint32_t* dacc = dv.get<uint32_t>(B_ACC29, z.acc29);
  uint32_t* daccb = dv.get<uint32_t>(B_ACC29B, z.acc29b);
  uint32_t* dcnt = dv.get<uint32_t>(B_CNT, z.cnt);
  uint32_t* dcntb = dv.get<uint32_t>(B_CNTB, z.cntb);
  const std::vector<uint32_t> a = stage_records(cnt_a, acc_a, p.NB, c.poison), b = stage_records(cnt_b, acc_b, p.NB, c.poison);
  dv.put(dacc, a.data(), (size_t)p.NB * REC);
  dv.put(daccb, b.data(), (size_t)p.NB * REC);
  dv.put(dcnt, cnt_a, z.cnt);
  dv.put(dcntb, cnt_b, z.cntb);
  if (rc == 0) {
    L::merge_buckets(nullptr, p.NB, dacc, dcnt, daccb, dcntb);
    dv.finish();
  }
  dv.take(acc_out, dacc, (size_t)p.NB * REC);
  dv.take(cnt_out, dcnt, z.cnt);
  dv.guards(guards);
  return rc;
}

// cnt: NB words, acc: NB records (those of empty buckets ignored: the store holds poison there, as
// do its piece records); R: NB / 16 records, U: twice as many (U, then V), scratch: nsets rb_parts
// points, winsum: nsets points (field.hpp words)
int PROBE_FN(reduce)(const uint64_t* desc, const uint32_t* cnt, const uint32_t* acc, int low_prio, int simds,
                     uint32_t* R, uint32_t* U, uint32_t* scratch, uint32_t* winsum, uint32_t* guards) {
  Call c;
  if (!read_call(desc, c) || simds < 1) return PROBE_ERR_ARG;
  const MsmPlan& p = c.p;
  if (p.small) return PROBE_ERR_PLAN;
  if (!records_ok(cnt, acc, p.NB)) return PROBE_ERR_ARG;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  uint32_t* dacc = dv.get<uint32_t>(B_ACC29, z.acc29);
  uint32_t* dcnt = dv.get<uint32_t>(B_CNT, z.cnt);
  XY* dR = dv.get<XY>(B_R, z.R);
  XY* dU = dv.get<XY>(B_U, z.U);
  XY* dscratch = dv.get<XY>(B_SCRATCH, z.scratch);
  XY* dwinsum = dv.get<XY>(B_WINSUM, z.winsum);
  const std::vector<uint32_t> a = stage_records(cnt, acc, p.NB, c.poison);
  dv.put(dacc, a.data(), (size_t)p.NB * REC);
  dv.put(dcnt, cnt, z.cnt);
  if (rc == 0) {
    L::reduce(nullptr, c.nsets, dcnt, dacc, dR, dU, dscratch, dwinsum, c.wbits, low_prio != 0, c.t.seg4_waves, simds);
    dv.finish();
  }
  dv.take(R, dR, z.R);
  dv.take(U, dU, z.U);
  dv.take(scratch, dscratch, z.scratch);
  dv.take(winsum, dwinsum, z.winsum);
  dv.guards(guards);
  return rc;
}

// winsum: nsets points; res: 2 points (those past nmsm stay poison)
int PROBE_FN(combine)(const uint64_t* desc, const uint32_t* winsum, int low_prio, uint32_t* res, uint32_t* guards) {
  Call c;
  if (!read_call(desc, c)) return PROBE_ERR_ARG;
  const MsmPlan& p = c.p;
  if (p.small) return PROBE_ERR_PLAN;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  XY* dwinsum = dv.get<XY>(B_WINSUM, z.winsum);
  XY* dres = dv.get<XY>(B_RES, z.res);
  dv.put(dwinsum, winsum, z.winsum);
  if (rc == 0) {
    L::window_combine(nullptr, c.mw, dwinsum, dres, c.wbits, low_prio != 0);
    dv.finish();
  }
  dv.take(res, dres, z.res);
  dv.guards(guards);
  return rc;
}

// a term list whose plan takes the small form; res: 2 points
int PROBE_FN(small)(const uint64_t* desc, const uint32_t* scal, uint64_t nscal, const uint32_t* points, const uint8_t* inf,
                    uint32_t npts, uint32_t* res, uint32_t* guards) {
  Call c;
  if (!read_call(desc, c) || c.part != 0) return PROBE_ERR_ARG;
  MsmPlan& p = c.p;
  if (!p.small) return PROBE_ERR_PLAN;
  const MsmBytes& z = p.bytes;
  Dev dv(c.poison);
  int& rc = dv.rc;
  if (!bind_scalars(dv, p, scal, nscal, npts)) return PROBE_ERR_ARG;
  AF* dpts = dv.get<AF>(B_PTS, (size_t)npts * sizeof(AF));
  uint8_t* dinf = dv.get<uint8_t>(B_INF, npts);
  uint32_t* dnodes = dv.get<uint32_t>(B_NODES, z.small_nodes);
  uint32_t* dflags = dv.get<uint32_t>(B_FLAGS, z.small_flags);
  XY* dres = dv.get<XY>(B_RES, z.res);
  dv.put(dpts, points, (size_t)npts * sizeof(AF));
  dv.put(dinf, inf, npts);
  if (rc == 0) {
    L::pts_to29(nullptr, dpts, npts);
    L::small_msm(nullptr, p.tl, p.sp, p.small_terms, dpts, dinf, dnodes, dflags, p.small_flags + 1, dres);
    dv.finish();
  }
  dv.take(res, dres, z.res);
  dv.guards(guards);
  return rc;
}

#if KZ_CURVE == 0
int msmprobe_plan_1(const uint64_t*, uint64_t*);
int msmprobe_check_sorted_1(const uint64_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                            uint32_t, uint32_t);
int msmprobe_sort_1(const uint64_t*, const uint32_t*, uint64_t, const uint8_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                    uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*);
int msmprobe_accumulate_1(const uint64_t*, const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*,
                          const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*);
int msmprobe_merge_1(const uint64_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*,
                     uint32_t*, uint32_t*);
int msmprobe_reduce_1(const uint64_t*, const uint32_t*, const uint32_t*, int, int, uint32_t*, uint32_t*, uint32_t*,
                      uint32_t*, uint32_t*);
int msmprobe_combine_1(const uint64_t*, const uint32_t*, int, uint32_t*, uint32_t*);
int msmprobe_small_1(const uint64_t*, const uint32_t*, uint64_t, const uint32_t*, const uint8_t*, uint32_t, uint32_t*,
                     uint32_t*);

#define PROBE_API extern "C" __attribute__((visibility("default")))
// kzgmi_msmprobe_<stage>(curve, the stage's arguments): the curve's instance, or PROBE_ERR_CURVE
#define PROBE_DISPATCH(stage, ...)                          \
  if (curve == 0) return msmprobe_##stage##_0(__VA_ARGS__); \
  if (curve == 1) return msmprobe_##stage##_1(__VA_ARGS__); \
  return PROBE_ERR_CURVE
PROBE_API int kzgmi_msmprobe_plan_words() { return kPlanWords; }
PROBE_API int kzgmi_msmprobe_guard_words() { return B_COUNT; }
PROBE_API int kzgmi_msmprobe_plan(int curve, const uint64_t* desc, uint64_t* out) { PROBE_DISPATCH(plan, desc, out); }
PROBE_API int kzgmi_msmprobe_check_sorted(int curve, const uint64_t* desc, uint32_t npts, const uint32_t* sval,
                                          const uint32_t* skey, const uint32_t* off, const uint32_t* cnt, uint32_t total,
                                          uint32_t mid) {
  PROBE_DISPATCH(check_sorted, desc, npts, sval, skey, off, cnt, total, mid);
}
PROBE_API int kzgmi_msmprobe_sort(int curve, const uint64_t* desc, const uint32_t* scal, uint64_t nscal, const uint8_t* inf,
                                  uint32_t npts, uint32_t* digits, uint32_t* coarse, uint32_t* total, uint32_t* sval,
                                  uint32_t* skey, uint32_t* off, uint32_t* cnt, uint32_t* guards) {
  PROBE_DISPATCH(sort, desc, scal, nscal, inf, npts, digits, coarse, total, sval, skey, off, cnt, guards);
}
PROBE_API int kzgmi_msmprobe_accumulate(int curve, const uint64_t* desc, const uint32_t* points, uint32_t npts,
                                        const uint32_t* sval, const uint32_t* skey, const uint32_t* off, const uint32_t* cnt,
                                        uint32_t total, uint32_t mid, uint32_t* acc_mid, uint32_t* acc_out,
                                        uint32_t* crowd_out, uint32_t* guards) {
  PROBE_DISPATCH(accumulate, desc, points, npts, sval, skey, off, cnt, total, mid, acc_mid, acc_out, crowd_out, guards);
}
PROBE_API int kzgmi_msmprobe_merge(int curve, const uint64_t* desc, const uint32_t* acc_a, const uint32_t* cnt_a,
                                   const uint32_t* acc_b, const uint32_t* cnt_b, uint32_t* acc_out, uint32_t* cnt_out,
                                   uint32_t* guards) {
  PROBE_DISPATCH(merge, desc, acc_a, cnt_a, acc_b, cnt_b, acc_out, cnt_out, guards);
}
PROBE_API int kzgmi_msmprobe_reduce(int curve, const uint64_t* desc, const uint32_t* cnt, const uint32_t* acc, int low_prio,
                                    int simds, uint32_t* R, uint32_t* U, uint32_t* scratch, uint32_t* winsum,
                                    uint32_t* guards) {
  PROBE_DISPATCH(reduce, desc, cnt, acc, low_prio, simds, R, U, scratch, winsum, guards);
}
PROBE_API int kzgmi_msmprobe_combine(int curve, const uint64_t* desc, const uint32_t* winsum, int low_prio, uint32_t* res,
                                     uint32_t* guards) {
  PROBE_DISPATCH(combine, desc, winsum, low_prio, res, guards);
}
PROBE_API int kzgmi_msmprobe_small(int curve, const uint64_t* desc, const uint32_t* scal, uint64_t nscal,
                                   const uint32_t* points, const uint8_t* inf, uint32_t npts, uint32_t* res,
                                   uint32_t* guards) {
  PROBE_DISPATCH(small, desc, scal, nscal, points, inf, npts, res, guards);
}
#endif
