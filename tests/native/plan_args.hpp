// The flat integer forms in which the test-only probes (plan_probe.hip, msm_probe.hip) take an
// MsmTuning and a TermList across their C ABI; tests/planprobe.py names the fields in this order.
#pragma once
#include "msm_plan.hpp"

namespace kzgmi_probe {
using namespace kzgmi;

constexpr int kTuningWords = 15;
inline MsmTuning tuning_of(const uint64_t* v) {
  MsmTuning t;
  t.ncu = (int)v[0];
  t.acc_threads_env = (size_t)v[1];
  t.acc_queue = (int)v[2];
  t.acc_queue_min = (size_t)v[3];
  t.acc_queue_from = (size_t)v[4];
  t.sort_split = v[5] != 0;
  t.sort_full_bins = v[6] != 0;
  t.wbits_env = (int)v[7];
  t.small_terms = (uint32_t)v[8];
  t.split_acc = (int)(int64_t)v[9];
  t.split_low_prio = v[10] != 0;
  t.split_side_fix = v[11] != 0;
  t.split_side_prio = v[12] != 0;
  t.split_rev = v[13] != 0;
  t.seg4_waves = (int)v[14];
  return t;
}

// nclass, total, then MAX_CLASSES x (count, pt_base, scal_words, nwin, set_base, scal_stride, scal, win_off, dig_base)
constexpr int kClassWords = 9, kTermWords = 2 + MAX_CLASSES * kClassWords;
inline TermList terms_of(const uint64_t* v) {
  TermList tl{};
  tl.nclass = (uint32_t)v[0];
  tl.total = (uint32_t)v[1];
  for (int k = 0; k < MAX_CLASSES; ++k) {
    const uint64_t* c = v + 2 + k * kClassWords;
    tl.c[k] = {(uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3], (uint32_t)c[4], (uint32_t)c[5],
               reinterpret_cast<const uint32_t*>((uintptr_t)c[6]), (uint32_t)c[7], (uint32_t)c[8]};
  }
  return tl;
}
inline uint64_t* put_terms(uint64_t* o, const TermList& tl) {
  *o++ = tl.nclass;
  *o++ = tl.total;
  for (int k = 0; k < MAX_CLASSES; ++k) {
    const TermClass& c = tl.c[k];
    const uint64_t w[kClassWords] = {c.count, c.pt_base, c.scal_words, c.nwin, c.set_base, c.scal_stride,
                                     (uint64_t)(uintptr_t)c.scal, c.win_off, c.dig_base};
    for (uint64_t x : w) *o++ = x;
  }
  return o;
}

}  // namespace kzgmi_probe
