// Launchers of the transforms over G1 and of kzgmi_open_all's kernels (compiled once per curve).
// Kernels: g1ntt.hpp.
#include "launch.hpp"
#include "g1ntt.hpp"

namespace kzgmi {

template <class Cv>
void Launch<Cv>::g1ntt_from_affine(hipStream_t st, const AF* pts, const uint8_t* inf, uint32_t total, uint32_t logn, bool rev,
                                   XY* out) {
  if (total) k_g1ntt_from_affine<Cv><<<grid_for(total, 256), 256, 0, st>>>(pts, inf, total, logn, rev ? 1 : 0, out);
}
template <class Cv>
void Launch<Cv>::g1ntt_stages(hipStream_t st, XY* data, uint32_t logn, uint32_t count, bool inverse, const void* roots,
                              int form) {
  if (!count || !logn) return;
  const uint32_t nbfly = count << (logn - 1);  // the same in every stage: one form per call
  const bool wave = form == G1NTT_FORM_WAVE || (form != G1NTT_FORM_THREAD && nbfly <= G1NTT_WAVE_MAX_BFLY);
  const uint32_t* rt = (const uint32_t*)roots;
  for (uint32_t ls = logn; ls-- > 0;) {
    if (wave) k_g1ntt_stage_wave<Cv><<<nbfly, 64, 0, st>>>(data, logn, ls, inverse ? 1 : 0, rt);
    else k_g1ntt_stage<Cv><<<grid_for(nbfly, G1NTT_THREADS), G1NTT_THREADS, 0, st>>>(data, nbfly, logn, ls, inverse ? 1 : 0, rt);
  }
}
template <class Cv>
void Launch<Cv>::g1ntt_mul(hipStream_t st, const XY* in, const uint32_t* scal, uint32_t logn, uint32_t total, XY* out) {
  if (total) k_g1ntt_mul<Cv><<<grid_for(total, G1NTT_THREADS), G1NTT_THREADS, 0, st>>>(in, scal, logn, total, out);
}
template <class Cv>
void Launch<Cv>::g1ntt_rev(hipStream_t st, const XY* in, uint32_t logn, uint32_t total, XY* out) {
  if (total) k_g1ntt_rev<Cv><<<grid_for(total, 256), 256, 0, st>>>(in, logn, total, out);
}
template <class Cv>
void Launch<Cv>::g1ntt_key_x(hipStream_t st, const AF* srs29, const uint8_t* srs_inf, uint32_t logn, XY* x) {
  k_g1ntt_key_x<Cv><<<grid_for(size_t(2) << logn, 256), 256, 0, st>>>(srs29, srs_inf, logn, x);
}
template <class Cv>
void Launch<Cv>::g1ntt_shift(hipStream_t st, const XY* ihat, uint32_t logn, XY* d) {
  k_g1ntt_shift<Cv><<<grid_for(size_t(1) << logn, 256), 256, 0, st>>>(ihat, logn, d);
}
template <class Cv>
void Launch<Cv>::g1ntt_pad(hipStream_t st, const uint32_t* coef, uint32_t m, uint32_t lg, uint32_t halvings, uint32_t* a) {
  const uint32_t total = 1u << lg;
  k_g1ntt_pad<<<grid_for(total, 256), 256, 0, st>>>(coef, m, total, a);
  if (halvings) k_g1ntt_halve<Cv><<<grid_for(total, 256), 256, 0, st>>>(a, halvings, total);
}

using C_ = KZ_CURVE_T;
template void Launch<C_>::g1ntt_from_affine(hipStream_t, const Affine<C_>*, const uint8_t*, uint32_t, uint32_t, bool, Xyzz<C_>*);
template void Launch<C_>::g1ntt_stages(hipStream_t, Xyzz<C_>*, uint32_t, uint32_t, bool, const void*, int);
template void Launch<C_>::g1ntt_mul(hipStream_t, const Xyzz<C_>*, const uint32_t*, uint32_t, uint32_t, Xyzz<C_>*);
template void Launch<C_>::g1ntt_rev(hipStream_t, const Xyzz<C_>*, uint32_t, uint32_t, Xyzz<C_>*);
template void Launch<C_>::g1ntt_key_x(hipStream_t, const Affine<C_>*, const uint8_t*, uint32_t, Xyzz<C_>*);
template void Launch<C_>::g1ntt_shift(hipStream_t, const Xyzz<C_>*, uint32_t, Xyzz<C_>*);
template void Launch<C_>::g1ntt_pad(hipStream_t, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t*);

}  // namespace kzgmi
