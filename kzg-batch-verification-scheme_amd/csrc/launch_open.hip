// Launchers of the opening scan (compiled once per curve).  Kernels: open.hpp.
#include "launch.hpp"
#include "open.hpp"

namespace kzgmi {

template <class Cv>
uint32_t Launch<Cv>::open_tiles(size_t m) {
  return (uint32_t)((m + OPEN_TILE - 1) / OPEN_TILE);
}
template <class Cv>
size_t Launch<Cv>::open_power_bytes() {
  return (size_t)OPEN_POWERS * 32;
}
template <class Cv>
void Launch<Cv>::open_points(hipStream_t st, const uint8_t* zs, uint32_t k, uint32_t* zp, uint32_t* err) {
  if (k) k_open_points<Cv><<<grid_for(k, 64), 64, 0, st>>>(zs, k, zp, err);
}
template <class Cv>
void Launch<Cv>::open_quotients(hipStream_t st, const uint32_t* coef, uint32_t m, const uint32_t* zp, uint32_t g,
                           uint32_t* runv, uint32_t* tilev, uint32_t* tilec, uint8_t* ys, void* q, bool be) {
  if (!m || !g) return;
  const uint32_t tiles = open_tiles(m);
  const dim3 grid(tiles, g);
  k_open_tiles<Cv><<<grid, OPEN_BLOCK, 0, st>>>(coef, m, zp, runv, tilev);
  k_open_carry<Cv><<<g, OPEN_BLOCK, 0, st>>>(zp, tilev, tiles, tilec, ys);
  if (m < 2) return;
  if (be) k_open_quotient<Cv, true><<<grid, OPEN_BLOCK, 0, st>>>(coef, m, zp, runv, tilec, (uint32_t*)q);
  else k_open_quotient<Cv, false><<<grid, OPEN_BLOCK, 0, st>>>(coef, m, zp, runv, tilec, (uint32_t*)q);
}

using C_ = KZ_CURVE_T;
template uint32_t Launch<C_>::open_tiles(size_t);
template size_t Launch<C_>::open_power_bytes();
template void Launch<C_>::open_points(hipStream_t, const uint8_t*, uint32_t, uint32_t*, uint32_t*);
template void Launch<C_>::open_quotients(hipStream_t, const uint32_t*, uint32_t, const uint32_t*, uint32_t, uint32_t*, uint32_t*,
                                    uint32_t*, uint8_t*, void*, bool);

}  // namespace kzgmi
