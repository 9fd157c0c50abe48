// Test-only probe of the MSM plan (csrc/msm_plan.hpp), never linked into libkzgmi.so: plan_msm,
// plan_reserve, batch_terms and call_wbits behind a C ABI of flat integer arrays, so tests/test_msm_plan_cpu.py can
// check them without a GPU.  Host code only: nothing here touches the HIP runtime.
// tests/planprobe.py names the fields of every array in the order they are written here.
#include "plan_args.hpp"

using namespace kzgmi;
using namespace kzgmi_probe;

namespace {

BatchScalars scalars_of(const uint64_t* scal7) {
  auto ptr = [&](int i) { return reinterpret_cast<const uint32_t*>((uintptr_t)scal7[i]); };
  return {ptr(0), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6)};
}

template <class Cv>
void plan_out(const MsmPlan& p, uint64_t* o) {
  *o++ = p.refuse != nullptr;
  *o++ = p.small;
  *o++ = p.sp.nclass;
  *o++ = p.sp.nmsm;
  for (int k = 0; k < MAX_CLASSES; ++k) *o++ = p.sp.term_base[k];
  for (int k = 0; k < MAX_CLASSES; ++k) *o++ = p.sp.leaf_base[k];
  for (int k = 0; k < MAX_CLASSES; ++k) *o++ = p.sp.msm[k];
  for (int m = 0; m < 2; ++m) *o++ = p.sp.count[m];
  for (int m = 0; m < 2; ++m) *o++ = p.sp.node_base[m];
  for (int m = 0; m < 2; ++m) *o++ = p.sp.flag_base[m];
  *o++ = p.small_terms;
  *o++ = p.small_nodes;
  *o++ = p.small_flags;
  o = put_terms(o, p.tl);
  const MsmBytes& z = p.bytes;
  const uint64_t w[] = {p.ndig, p.own_npts, p.nbuckets, p.bins, p.rb_parts, p.NB, p.nchunks, p.acc_threads, p.can_split,
                        p.split, p.split_set, p.pieces, p.crowd_words, p.second,
                        z.small_nodes, z.small_flags, z.digits, z.cnt, z.off, z.cntb, z.offb, z.coarse, z.ent, z.total,
                        z.accq, z.crowd, z.sval, z.skey, z.acc29, z.acc29b, z.R, z.U, z.scratch, z.winsum, z.res};
  for (uint64_t x : w) *o++ = x;
}

}  // namespace

extern "C" {

// the refusal's message (nullptr: the plan was made)
const char* kzgmi_planprobe_plan(int curve, const uint64_t* tuning, const uint64_t* terms, uint32_t nsets, uint64_t emax,
                                 const uint32_t* mw5, int wbits, int part, int own_pts, int alone, int sync_call,
                                 uint64_t* out) {
  const MsmTuning t = tuning_of(tuning);
  const TermList tl = terms_of(terms);
  const MsmWindows mw{mw5[0], {mw5[1], mw5[2]}, {mw5[3], mw5[4]}};
  if (curve == 0) {
    const MsmPlan p = plan_msm<Bls12_381>(t, tl, nsets, (size_t)emax, mw, wbits, part, own_pts != 0, alone != 0, sync_call != 0);
    plan_out<Bls12_381>(p, out);
    return p.refuse;
  }
  const MsmPlan p = plan_msm<Bn254>(t, tl, nsets, (size_t)emax, mw, wbits, part, own_pts != 0, alone != 0, sync_call != 0);
  plan_out<Bn254>(p, out);
  return p.refuse;
}

// plan_reserve of a batch mode (n > 0); scal7 as below
void kzgmi_planprobe_reserve(int curve, const uint64_t* tuning, int glv, int powers, uint64_t n, int own_pts,
                             const uint64_t* scal7, uint64_t* out) {
  const MsmTuning t = tuning_of(tuning);
  const BatchScalars b = scalars_of(scal7);
  if (curve == 0) plan_out<Bls12_381>(plan_reserve<Bls12_381>(t, glv != 0, powers != 0, (size_t)n, own_pts != 0, b), out);
  else plan_out<Bn254>(plan_reserve<Bn254>(t, glv != 0, powers != 0, (size_t)n, own_pts != 0, b), out);
}

// scal7: the addresses of scal_r, scal_s, scal_t, glv_r, glv_s, glv_t, cell_coef;
// out: the term list, then mw (5), nsets, emax
void kzgmi_planprobe_batch_terms(int glv, int powers, uint32_t cell_terms, uint32_t H, uint32_t F, uint64_t n, uint64_t m,
                                 uint64_t lo, uint64_t nj, int last, const uint64_t* scal7, uint64_t* out) {
  const BatchScalars b = scalars_of(scal7);
  const BatchTerms r = batch_terms(glv != 0, powers != 0, cell_terms, H, F, (size_t)n, (size_t)m, (size_t)lo, (size_t)nj,
                                   last != 0, b);
  uint64_t* o = put_terms(out, r.tl);
  const uint64_t w[] = {r.mw.nmsm, r.mw.set_base[0], r.mw.set_base[1], r.mw.nwin[0], r.mw.nwin[1], r.nsets, r.emax};
  for (uint64_t x : w) *o++ = x;
}

int kzgmi_planprobe_wbits(const uint64_t* tuning, uint64_t entries16, uint64_t max13) {
  return call_wbits(tuning_of(tuning), (size_t)entries16, (size_t)max13);
}
uint32_t kzgmi_planprobe_windows(int wb, int full) { return full ? windows_full(wb) : windows_half(wb); }

}  // extern "C"
