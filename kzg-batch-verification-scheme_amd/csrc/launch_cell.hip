// EIP-7594 cell front-end launchers (BLS12-381 only: compiled once).  Kernels: cell.hpp.
#include "launch.hpp"
#include "cell.hpp"

namespace kzgmi {

size_t CellLaunch::table_bytes() { return CELL_TABLE * sizeof(BlobF); }
size_t CellLaunch::part_bytes() { return (size_t)CELL_COSETS * CELL_N * sizeof(BlobF); }

void CellLaunch::table(hipStream_t st, void* table) {
  k_cell_table<<<grid_for(CELL_TABLE, 64), 64, 0, st>>>((BlobF*)table);
}

void CellLaunch::z(hipStream_t st, const void* cell_indices, const void* commitment_indices, uint32_t n, uint32_t m,
                   const void* table, uint8_t* zs, uint8_t* ys, uint32_t* err) {
  if (n)
    k_cell_z<<<grid_for(n, 256), 256, 0, st>>>((const uint64_t*)cell_indices, (const uint64_t*)commitment_indices, n, m,
                                               (const BlobF*)table, zs, ys, err);
}

void CellLaunch::gather(hipStream_t st, const void* commitment_indices, uint32_t n, uint32_t m, Affine<Bls12_381>* pts,
                        uint8_t* inf, uint32_t src, uint32_t dst) {
  if (n)
    k_cell_gather<Bls12_381><<<grid_for(n, 256), 256, 0, st>>>((const uint64_t*)commitment_indices, n, m, pts, inf, src,
                                                               dst);
}

void CellLaunch::interp(hipStream_t st, const void* cell_indices, const uint8_t* cells, const uint32_t* rk, uint32_t n,
                        const void* table, void* part, uint32_t* neg_le, uint8_t* coeffs_be, uint32_t* err) {
  k_cell_fold_intt<<<CELL_COSETS, CELL_N, 0, st>>>((const uint64_t*)cell_indices, cells, rk, n, (const BlobF*)table,
                                                   (BlobF*)part, err);
  k_cell_sum<<<1, CELL_N, 0, st>>>((const BlobF*)part, neg_le, coeffs_be);
}

void CellLaunch::coeffs(hipStream_t st, const void* cell_indices, const uint8_t* cells, uint32_t n, const void* table,
                        uint32_t* coef_le, uint8_t* coeffs_be, uint32_t* err) {
  if (n)
    k_cell_coeffs<<<grid_for(n, CELL_COEFF_PACK), 64 * CELL_COEFF_PACK, 0, st>>>(
        (const uint64_t*)cell_indices, cells, n, (const BlobF*)table, coef_le, coeffs_be, err);
}

void CellLaunch::batch_challenge(hipStream_t st, const uint8_t* commitments, uint32_t m, const void* commitment_indices,
                                 const void* cell_indices, const uint8_t* cells, const uint8_t* proofs, uint32_t n,
                                 void* pow, uint32_t* chal_out) {
  k_cell_batch_challenge<<<1, 64, 0, st>>>(commitments, m, (const uint64_t*)commitment_indices,
                                           (const uint64_t*)cell_indices, cells, proofs, n, (BlobF*)pow, chal_out);
}

}  // namespace kzgmi
