// Test-only probe of the search plan (csrc/find_plan.hpp), never linked into libkzgmi.so: find_split,
// find_next_level, find_group_plan, find_level_fanout, find_level_path, find_group_chunk and the
// shipped FindTuning behind a C ABI of flat integer arrays, so tests/test_find_plan_cpu.py can check
// them without a GPU.  Host code only: nothing here touches the HIP runtime.  tests/findprobe.py
// names the fields of every array in the order they are written here.
#include "find_plan.hpp"

using namespace kzgmi;

namespace {
FindTuning tuning_of(const uint64_t* v) {
  FindTuning t;
  t.fanout = (uint32_t)v[0];
  t.bucket_fanout = (uint32_t)v[1];
  t.group_terms = (uint32_t)v[2];
  t.group_bytes = (size_t)v[3];
  return t;
}
}  // namespace

extern "C" {

// the shipped defaults: fanout, bucket_fanout, group_terms, group_bytes, then FIND_MAX_BAD, FIND_MAX_RANGES, bytes
// of a stored node
void kzgmi_findprobe_tuning(uint64_t* out7) {
  const FindTuning t;
  out7[0] = t.fanout;
  out7[1] = t.bucket_fanout;
  out7[2] = t.group_terms;
  out7[3] = t.group_bytes;
  out7[4] = FIND_MAX_BAD;
  out7[5] = FIND_MAX_RANGES;
  out7[6] = SMALL_NODE_WORDS * 4;
}

// out: F (lo, hi) pairs; returns the number of parts
uint32_t kzgmi_findprobe_split(uint64_t lo, uint64_t hi, uint32_t F, uint64_t* out) {
  return find_split(lo, hi, F, reinterpret_cast<FindRange*>(out));
}

// parts: nparts (lo, hi) pairs; out3: n_suspects, n_bad, more; bad_out: max_bad; suspects_out: max_bad pairs
void kzgmi_findprobe_next_level(const uint64_t* parts, const int32_t* ok, uint64_t nparts, uint64_t max_bad,
                                const uint64_t* bad_in, uint64_t n_bad_in, int more_in, uint64_t* bad_out,
                                uint64_t* suspects_out, uint64_t* out3) {
  const FindLevel r = find_next_level(reinterpret_cast<const FindRange*>(parts), ok, (size_t)nparts, (size_t)max_bad, bad_in,
                                      (size_t)n_bad_in, more_in != 0, bad_out, reinterpret_cast<FindRange*>(suspects_out));
  out3[0] = r.n_suspects;
  out3[1] = r.n_bad;
  out3[2] = r.more;
}

// ranges: G (lo, hi) pairs; table: G x 8 words (lo, len, wave_base, node_base A, B, flag_base A, B, 0);
// out9: waves, nodes, flags, bytes_nodes, bytes_flags, bytes_table, bytes_negt, bytes, fits
void kzgmi_findprobe_group_plan(const uint64_t* ranges, uint64_t G, uint32_t* table, uint64_t* out9) {
  const FindGroupPlan p = find_group_plan(reinterpret_cast<const FindRange*>(ranges), (size_t)G,
                                          reinterpret_cast<FindGroup*>(table));
  const uint64_t w[9] = {p.waves, p.nodes, p.flags, p.bytes_nodes, p.bytes_flags, p.bytes_table, p.bytes_negt, p.bytes,
                         p.fits};
  for (int i = 0; i < 9; ++i) out9[i] = w[i];
}

int kzgmi_findprobe_level_path(const uint64_t* parts, uint64_t nparts, const uint64_t* tuning4) {
  return find_level_path(reinterpret_cast<const FindRange*>(parts), (size_t)nparts, tuning_of(tuning4));
}

uint32_t kzgmi_findprobe_level_fanout(const uint64_t* suspects, uint64_t ns, const uint64_t* tuning4) {
  return find_level_fanout(reinterpret_cast<const FindRange*>(suspects), (size_t)ns, tuning_of(tuning4));
}

uint64_t kzgmi_findprobe_group_chunk(const uint64_t* ranges, uint64_t G, const uint64_t* tuning4) {
  return find_group_chunk(reinterpret_cast<const FindRange*>(ranges), (size_t)G, tuning_of(tuning4));
}

}  // extern "C"
