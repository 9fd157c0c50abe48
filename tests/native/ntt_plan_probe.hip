// Test-only probe of the transform plan (csrc/ntt_plan.hpp), never linked into libkzgmi.so: ntt_plan
// and the shipped constants behind a C ABI of flat integer arrays, so tests/test_ntt_cpu.py can check
// them without a GPU.  Host code only: nothing here touches the HIP runtime.  tests/nttplanprobe.py
// names the fields of every array in the order they are written here.
#include "ntt_plan.hpp"

using namespace kzgmi;

extern "C" {

// max logn, shipped tile bits, B (shipped most bits of a pass), least bound, most passes, min / max tile bits
void kzgmi_nttplanprobe_constants(uint32_t* out7) {
  out7[0] = NTT_MAX_LOGN;
  out7[1] = NTT_TILE_BITS;
  out7[2] = NTT_MAX_BITS;
  out7[3] = NTT_MIN_PASS_BITS;
  out7[4] = NTT_MAX_PASSES;
  out7[5] = NTT_MIN_TILE_BITS;
  out7[6] = NTT_MAX_TILE_BITS;
}

// passes: NTT_MAX_PASSES x 5 words (bits, lstride, lprev, tw_step, flags); out2: npass, scratch bytes;
// returns 1, or 0 where ntt_plan refuses the arguments
int kzgmi_nttplanprobe_plan(uint32_t logn, uint64_t count, uint32_t flags, int shift, uint32_t bound, int read_be,
                            int write_be, uint32_t* passes, uint64_t* out2) {
  NttPlan p;
  if (!ntt_plan(logn, count, flags, shift != 0, bound, read_be != 0, write_be != 0, &p)) return 0;
  for (uint32_t k = 0; k < p.npass; ++k) {
    const NttPass& q = p.pass[k];
    const uint32_t w[5] = {q.bits, q.lstride, q.lprev, q.tw_step, q.flags};
    for (int i = 0; i < 5; ++i) passes[5 * k + i] = w[i];
  }
  out2[0] = p.npass;
  out2[1] = ntt_scratch_bytes(p);
  return 1;
}

}  // extern "C"
