// Launchers of the transforms over Fr (compiled once per curve).  Kernels: ntt.hpp.
#include "launch.hpp"
#include "ntt.hpp"

namespace kzgmi {

template <class Cv>
size_t Launch<Cv>::ntt_table_bytes() {
  return (size_t)NTT_T_ENTRIES * 32;
}
template <class Cv>
size_t Launch<Cv>::ntt_call_bytes() {
  return (size_t)NTT_CALL_ENTRIES * 32;
}
template <class Cv>
void Launch<Cv>::ntt_roots(hipStream_t st, void* table) {
  k_ntt_roots<Cv><<<grid_for(NTT_T_ENTRIES, 256), 256, 0, st>>>((uint32_t*)table);
}
template <class Cv>
void Launch<Cv>::ntt_call_table(hipStream_t st, const Seed* shift, bool inverse, uint32_t logn, void* tab) {
  k_ntt_call_table<Cv><<<grid_for(NTT_CALL_ENTRIES, 256), 256, 0, st>>>(shift ? *shift : Seed{}, shift ? 1 : 0, inverse ? 1 : 0,
                                                                         logn, (uint32_t*)tab);
}
template <class Cv>
void Launch<Cv>::ntt_pass(hipStream_t st, uint32_t tile_bits, const NttPass& pass, uint32_t logn, uint64_t count, const void* in,
                          void* out, const void* roots, const void* call, uint32_t* err) {
  if (!count) return;
  NttPassArgs a{in, out, count << (logn - pass.bits), logn, pass.bits, pass.lstride, pass.lprev, pass.tw_step, pass.flags};
  const uint32_t lc = tile_bits - pass.bits;  // columns of a tile
  const unsigned grid = (unsigned)((a.cols + (uint64_t(1) << lc) - 1) >> lc);
  const uint32_t* rt = (const uint32_t*)roots;
  const uint32_t* ct = (const uint32_t*)call;
  switch (tile_bits) {
    case 10: k_ntt_pass<Cv, 10><<<grid, 256, 0, st>>>(a, rt, ct, err); break;
    case 11: k_ntt_pass<Cv, 11><<<grid, 512, 0, st>>>(a, rt, ct, err); break;
    default: k_ntt_pass<Cv, 12><<<grid, 1024, 0, st>>>(a, rt, ct, err); break;
  }
}

using C_ = KZ_CURVE_T;
template size_t Launch<C_>::ntt_table_bytes();
template size_t Launch<C_>::ntt_call_bytes();
template void Launch<C_>::ntt_roots(hipStream_t, void*);
template void Launch<C_>::ntt_call_table(hipStream_t, const Seed*, bool, uint32_t, void*);
template void Launch<C_>::ntt_pass(hipStream_t, uint32_t, const NttPass&, uint32_t, uint64_t, const void*, void*, const void*,
                                   const void*, uint32_t*);

}  // namespace kzgmi
