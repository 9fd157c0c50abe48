// EIP-7594 cell proof generation launchers (BLS12-381 only: compiled once).  Kernels: fk20.hpp.
#include "launch.hpp"
#include "fk20.hpp"

namespace kzgmi {

size_t Fk20Launch::table_bytes() { return FK_TABLE_POINTS * sizeof(FkAF); }
size_t Fk20Launch::table_flags() { return FK_BASES; }
size_t Fk20Launch::coef_bytes(uint32_t nb) { return (size_t)nb * NTT_N * sizeof(BlobF); }
size_t Fk20Launch::scal_bytes(uint32_t nb) { return (size_t)nb * FK_BASES * 32; }

void Fk20Launch::fft(hipStream_t st, XY* data, uint32_t count, const void* ntt_table, bool inverse) {
  if (!count) return;
  for (uint32_t half = FK_N / 2; half >= 1; half >>= 1)
    k_fk20_bfly<<<count * (FK_N / 2), 64, 0, st>>>(data, half, (const BlobF*)ntt_table + NTT_T_TW, inverse ? 1 : 0);
}

void Fk20Launch::key(hipStream_t st, const AF* srs, const void* ntt_table, XY* x, void* table, uint8_t* tab_inf) {
  k_fk20_xvec<<<grid_for(FK_BASES, 256), 256, 0, st>>>(srs, x);
  fft(st, x, KEY_TRANSFORMS, ntt_table, false);
  k_fk20_table<<<grid_for((size_t)FK_BASES * FK_WINDOWS, 256), 256, 0, st>>>(x, (FkAF*)table, tab_inf);
}

void Fk20Launch::scalars(hipStream_t st, const uint8_t* blobs, size_t stride, uint32_t nb, const void* ntt_table,
                         bool fold128, void* coef, uint8_t* scal, uint32_t* err) {
  if (!nb) return;
  const BlobF* t = (const BlobF*)ntt_table;
  k_fk20_coeffs<<<nb, NTT_THREADS, 0, st>>>(blobs, stride, t, fold128 ? 7 : 0, (BlobF*)coef, err);
  k_fk20_dft<<<dim3(FK_COLS, nb), FK_N, 0, st>>>((const BlobF*)coef, t + NTT_T_TW, scal);
}

void Fk20Launch::msm(hipStream_t st, const uint8_t* scal, uint32_t nb, const void* table, const uint8_t* tab_inf,
                     XY* out) {
  if (nb) k_fk20_msm<<<nb * FK_N, FK_MSM_THREADS, 0, st>>>(scal, (const FkAF*)table, tab_inf, out);
}

void Fk20Launch::scale128(hipStream_t st, XY* data, uint32_t n) {
  if (n) k_fk20_scale128<<<n, 64, 0, st>>>(data);
}
void Fk20Launch::shift(hipStream_t st, const XY* h, uint32_t count, XY* d) {
  if (count) k_fk20_shift<<<count, FK_N, 0, st>>>(h, d);
}
void Fk20Launch::unrev(hipStream_t st, const XY* in, uint32_t count, XY* out) {
  if (count) k_fk20_unrev<<<count, FK_N, 0, st>>>(in, out);
}
void Fk20Launch::from_affine(hipStream_t st, const AF* pts, const uint8_t* inf, uint32_t n, XY* out) {
  if (n) k_fk20_from_affine<<<grid_for(n, 256), 256, 0, st>>>(pts, inf, n, out);
}
void Fk20Launch::emit(hipStream_t st, const void* in, size_t bytes, const uint32_t* err, void* out) {
  const size_t n = bytes / 16;
  if (n) k_fk20_emit<<<grid_for(n, 256), 256, 0, st>>>((const uint4*)in, n, err, (uint4*)out);
}

}  // namespace kzgmi
