// Launchers of kzgmi_open_cosets's kernels (compiled once per curve).  Kernels: cosets.hpp.
#include "launch.hpp"
#include "cosets.hpp"

namespace kzgmi {

namespace {
// the products' form for a call of `terms` scalar multiples: the stages' rule (Launch::g1ntt_stages)
bool cosets_wave(int form, uint32_t terms) {
  return form == G1NTT_FORM_WAVE || (form != G1NTT_FORM_THREAD && terms <= G1NTT_WAVE_MAX_BFLY);
}
// log2 of the records per position that the product kernel leaves: l in the wave form, l / 64 (at least 1) in the thread form
uint32_t cosets_logw(bool wave, uint32_t logl) { return wave ? logl : logl - std::min(logl, 6u); }
}  // namespace

template <class Cv>
void Launch<Cv>::cosets_key_x(hipStream_t st, const AF* srs29, const uint8_t* srs_inf, uint32_t logN, uint32_t logl, XY* x) {
  k_cosets_key_x<Cv><<<grid_for(size_t(2) << logN, 256), 256, 0, st>>>(srs29, srs_inf, logN, logl, x);
}
template <class Cv>
void Launch<Cv>::cosets_key_gather(hipStream_t st, const XY* xs, uint32_t logN, uint32_t logl, XY* out) {
  k_cosets_key_gather<Cv><<<grid_for(size_t(2) << logN, 256), 256, 0, st>>>(xs, logN, logl, out);
}
template <class Cv>
void Launch<Cv>::cosets_pad(hipStream_t st, const uint32_t* coef, uint32_t m, uint32_t count, uint32_t logl, uint32_t loglen,
                            uint32_t ulim, uint32_t halvings, uint32_t* a) {
  const uint32_t total = count << (logl + loglen);
  if (!total) return;
  k_cosets_pad<<<grid_for(total, 256), 256, 0, st>>>(coef, m, logl, loglen, ulim, total, a);
  if (halvings) k_g1ntt_halve<Cv><<<grid_for(total, 256), 256, 0, st>>>(a, halvings, total);
}
template <class Cv>
void Launch<Cv>::cosets_scal(hipStream_t st, const uint32_t* ahat, uint32_t logN, uint32_t logl, uint32_t count, uint32_t* out) {
  const uint32_t terms = count << (logN + 1);
  if (terms) k_cosets_scal<<<grid_for(terms, 256), 256, 0, st>>>(ahat, logN, logl, terms, out);
}
template <class Cv>
size_t Launch<Cv>::cosets_scratch_records(uint32_t logN, uint32_t logl, uint32_t count, int form) {
  const uint32_t logr2 = logN - logl + 1;
  return ((size_t)count << logr2) << cosets_logw(cosets_wave(form, count << (logN + 1)), logl);
}
template <class Cv>
typename Launch<Cv>::XY* Launch<Cv>::cosets_products(hipStream_t st, const XY* key, const uint32_t* scal, uint32_t logN,
                                                     uint32_t logl, uint32_t count, int form, XY* a, XY* b) {
  const uint32_t terms = count << (logN + 1), npos = count << (logN - logl + 1);
  if (!terms) return a;
  const bool wave = cosets_wave(form, terms);
  uint32_t logw = cosets_logw(wave, logl);
  uint32_t folds = (logw + 5) / 6;  // each brings up to 64 records of a position together
  XY* out = folds & 1 ? b : a;      // so that the last lands in a
  if (wave) k_cosets_mul_wave<Cv><<<terms, 64, 0, st>>>(key, scal, logN, out);
  else k_cosets_mul<Cv><<<grid_for(terms, G1NTT_THREADS), G1NTT_THREADS, 0, st>>>(key, scal, logN, logl, terms, out);
  while (logw) {
    const uint32_t lseg = std::min(logw, 6u);
    logw -= lseg;
    const uint32_t nout = npos << logw;
    XY* next = out == a ? b : a;
    k_cosets_fold<Cv><<<grid_for((size_t)nout << lseg, G1NTT_THREADS), G1NTT_THREADS, 0, st>>>(out, lseg, nout, next);
    out = next;
  }
  return out;
}
template <class Cv>
void Launch<Cv>::cosets_shift(hipStream_t st, const XY* ihat, uint32_t logr2, uint32_t logk, uint32_t count, XY* d) {
  const uint32_t total = count << logk;
  if (total) k_cosets_shift<Cv><<<grid_for(total, 256), 256, 0, st>>>(ihat, logr2, logk, total, d);
}
template <class Cv>
void Launch<Cv>::cosets_ys(hipStream_t st, const void* y, uint32_t logk, uint32_t logl, uint32_t count, void* out) {
  const uint32_t total = count << (logk + logl);
  if (total) k_cosets_ys<<<grid_for(total, 256), 256, 0, st>>>((const uint4*)y, logk, logl, total, (uint4*)out);
}

using C_ = KZ_CURVE_T;
template void Launch<C_>::cosets_key_x(hipStream_t, const Affine<C_>*, const uint8_t*, uint32_t, uint32_t, Xyzz<C_>*);
template void Launch<C_>::cosets_key_gather(hipStream_t, const Xyzz<C_>*, uint32_t, uint32_t, Xyzz<C_>*);
template void Launch<C_>::cosets_pad(hipStream_t, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*);
template void Launch<C_>::cosets_scal(hipStream_t, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t*);
template size_t Launch<C_>::cosets_scratch_records(uint32_t, uint32_t, uint32_t, int);
template Xyzz<C_>* Launch<C_>::cosets_products(hipStream_t, const Xyzz<C_>*, const uint32_t*, uint32_t, uint32_t, uint32_t, int,
                                               Xyzz<C_>*, Xyzz<C_>*);
template void Launch<C_>::cosets_shift(hipStream_t, const Xyzz<C_>*, uint32_t, uint32_t, uint32_t, Xyzz<C_>*);
template void Launch<C_>::cosets_ys(hipStream_t, const void*, uint32_t, uint32_t, uint32_t, void*);

}  // namespace kzgmi
