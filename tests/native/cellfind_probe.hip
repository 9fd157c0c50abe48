// Test-only probe of the search plan's tail parameter (csrc/find_plan.hpp), never linked into
// libkzgmi.so: find_wave_terms, find_group_plan and find_group_chunk with the tail length a range of
// EIP-7594 cells takes (64) or any other, behind a C ABI of flat integer arrays, so
// tests/test_cell_find_plan_cpu.py can check them without a GPU.  Host code only: nothing here touches
// the HIP runtime.  The arrays are those of tests/native/find_probe.hip (tests/cellfindprobe.py).
#include "find_plan.hpp"

using namespace kzgmi;

extern "C" {

uint64_t kzgmi_cellfindprobe_wave_terms(uint64_t len, uint32_t tail) { return find_wave_terms(len, tail); }

// ranges: G (lo, hi) pairs; table: G x 8 words (lo, len, wave_base, node_base A, B, flag_base A, B, 0);
// out9: waves, nodes, flags, bytes_nodes, bytes_flags, bytes_table, bytes_negt, bytes, fits
void kzgmi_cellfindprobe_group_plan(const uint64_t* ranges, uint64_t G, uint32_t tail, uint32_t* table, uint64_t* out9) {
  const FindGroupPlan p = find_group_plan(reinterpret_cast<const FindRange*>(ranges), (size_t)G,
                                          reinterpret_cast<FindGroup*>(table), tail);
  const uint64_t w[9] = {p.waves, p.nodes, p.flags, p.bytes_nodes, p.bytes_flags, p.bytes_table, p.bytes_negt, p.bytes,
                         p.fits};
  for (int i = 0; i < 9; ++i) out9[i] = w[i];
}

// tuning4: fanout, bucket_fanout, group_terms, group_bytes
uint64_t kzgmi_cellfindprobe_group_chunk(const uint64_t* ranges, uint64_t G, const uint64_t* tuning4, uint32_t tail) {
  FindTuning t;
  t.fanout = (uint32_t)tuning4[0];
  t.bucket_fanout = (uint32_t)tuning4[1];
  t.group_terms = (uint32_t)tuning4[2];
  t.group_bytes = (size_t)tuning4[3];
  return find_group_chunk(reinterpret_cast<const FindRange*>(ranges), (size_t)G, t, tail);
}

}  // extern "C"
