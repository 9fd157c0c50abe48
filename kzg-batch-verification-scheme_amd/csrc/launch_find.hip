// Launchers of the grouped small MSMs (compiled once per curve, -DKZ_CURVE=0/1).  See msm_group.hpp.
#include "launch.hpp"
#include "msm_group.hpp"

namespace kzgmi {

template <class Cv>
void Launch<Cv>::group_msm(hipStream_t st, const FindGroup* table, uint32_t G, uint32_t waves, uint32_t n,
                           const Seed& seed, uint64_t index_offset, const uint8_t* ys, const uint32_t* scal_r,
                           const uint32_t* scal_s, uint32_t* negt, const AF* pts, const uint8_t* inf, uint32_t* nodes,
                           uint32_t* flags, size_t flag_words, XY* res) {
  if (!G) return;
  (void)hipMemsetAsync(flags, 0, flag_words * 4, st);  // every launch: a slot's next call reuses the buffer
  k_group_tsum<Cv><<<G, 256, 0, st>>>(table, seed, index_offset, ys, negt);
  const GroupBatch b{n, G, scal_r, scal_s, negt};
  k_group_msm<Cv><<<waves, 64, 0, st>>>(b, table, pts, inf, nodes, flags, res);
}

template <class Cv>
void Launch<Cv>::group_msm_cells(hipStream_t st, const FindGroup* table, uint32_t G, uint32_t waves, uint32_t n,
                                 const Seed& seed, uint64_t index_offset, const uint32_t* coef, const uint32_t* scal_r,
                                 const uint32_t* scal_s, uint32_t* negt, const AF* pts, const uint8_t* inf,
                                 uint32_t* nodes, uint32_t* flags, size_t flag_words, XY* res) {
  if (!G) return;
  (void)hipMemsetAsync(flags, 0, flag_words * 4, st);
  k_cell_range_fold<Cv><<<G, 256, 0, st>>>(table, seed, index_offset, coef, negt);
  const GroupBatch b{n, G, scal_r, scal_s, negt};
  k_group_msm<Cv, 64><<<waves, 64, 0, st>>>(b, table, pts, inf, nodes, flags, res);
}

template <class Cv>
void Launch<Cv>::mark_records(hipStream_t st, XY* recs, uint32_t count, const uint32_t* err) {
  if (count) k_mark_records<Cv><<<grid_for(count, 256), 256, 0, st>>>(recs, count, err);
}

template <class Cv>
void Launch<Cv>::check_marks(hipStream_t st, const XY* recs, uint32_t count, uint32_t* err) {
  if (count) k_check_marks<Cv><<<grid_for(count, 256), 256, 0, st>>>(recs, count, err);
}

using C_ = KZ_CURVE_T;
template void Launch<C_>::group_msm(hipStream_t, const FindGroup*, uint32_t, uint32_t, uint32_t, const Seed&, uint64_t,
                                    const uint8_t*, const uint32_t*, const uint32_t*, uint32_t*, const Affine<C_>*,
                                    const uint8_t*, uint32_t*, uint32_t*, size_t, Xyzz<C_>*);
#if KZ_CURVE == 0  // cells are BLS12-381 only
template void Launch<C_>::group_msm_cells(hipStream_t, const FindGroup*, uint32_t, uint32_t, uint32_t, const Seed&,
                                          uint64_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*,
                                          const Affine<C_>*, const uint8_t*, uint32_t*, uint32_t*, size_t, Xyzz<C_>*);
#endif
template void Launch<C_>::mark_records(hipStream_t, Xyzz<C_>*, uint32_t, const uint32_t*);
template void Launch<C_>::check_marks(hipStream_t, const Xyzz<C_>*, uint32_t, uint32_t*);

}  // namespace kzgmi
