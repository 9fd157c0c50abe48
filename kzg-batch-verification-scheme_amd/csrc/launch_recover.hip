// EIP-7594 cell extension and recovery launchers (BLS12-381 only: compiled once).  Kernels: recover.hpp.
#include "launch.hpp"
#include "recover.hpp"

namespace kzgmi {

size_t RecoverLaunch::table_bytes() { return NTT_TABLE * sizeof(BlobF); }
size_t RecoverLaunch::z_bytes() { return REC_Z_BYTES; }

void RecoverLaunch::table(hipStream_t st, void* table) {
  k_ntt_table<<<grid_for(NTT_TABLE, 256), 256, 0, st>>>((BlobF*)table);
}

void RecoverLaunch::compute(hipStream_t st, const uint8_t* blobs, uint32_t nb, const void* table, uint8_t* out,
                            uint32_t* err) {
  if (nb) k_compute_cells<<<nb, NTT_THREADS, 0, st>>>(blobs, (const BlobF*)table, out, err);
}

void RecoverLaunch::recover(hipStream_t st, const void* cell_indices, uint32_t k, const uint8_t* cells, uint32_t nb,
                            const void* cell_table, const void* table, void* z, uint8_t* out, uint32_t* err) {
  BlobF* zt = (BlobF*)z;
  int32_t* pos = reinterpret_cast<int32_t*>(zt + REC_Z_F);
  k_recover_z<<<1, REC_Z_THREADS, 0, st>>>((const uint64_t*)cell_indices, k, (const BlobF*)cell_table,
                                         (const BlobF*)table + NTT_T_TW, zt, pos, err);
  if (nb) k_recover_cells<<<nb, NTT_THREADS, 0, st>>>(cells, k, (const BlobF*)table, zt, pos, out, err);
}

}  // namespace kzgmi
