// EIP-4844 commitment and proof generation launchers (BLS12-381 only: compiled once).  Kernels: blobproof.hpp.
#include "launch.hpp"
#include "blobproof.hpp"

namespace kzgmi {

size_t BlobProofLaunch::table_bytes() { return BP_TABLE_POINTS * sizeof(FkAF); }
size_t BlobProofLaunch::table_flags() { return BP_BASES; }

void BlobProofLaunch::key(hipStream_t st, const AF* pts, const uint8_t* inf, void* table, uint8_t* tab_inf) {
  k_blob_table<<<grid_for((size_t)BP_BASES * FK_WINDOWS, 256), 256, 0, st>>>(pts, inf, (FkAF*)table, tab_inf);
}

void BlobProofLaunch::quotient(hipStream_t st, const uint8_t* blobs, const uint8_t* zs, const void* domain, uint32_t nb,
                               bool range_check, uint8_t* ys, uint8_t* q, uint32_t* err) {
  if (nb)
    k_blob_quotient<<<nb, BLOB_EVAL_THREADS, 0, st>>>(blobs, zs, (const BlobF*)domain, range_check ? 1 : 0, ys, q, err);
}

void BlobProofLaunch::msm(hipStream_t st, const uint8_t* scal, uint32_t nb, bool range_check, const void* table,
                          const uint8_t* tab_inf, XY* parts, XY* out, uint32_t* err) {
  if (!nb) return;
  k_blob_msm<<<nb * BP_CHUNKS, FK_MSM_THREADS, 0, st>>>(scal, (const FkAF*)table, tab_inf, range_check ? 1 : 0, parts, err);
  k_blob_msm_join<<<nb, BP_CHUNKS, 0, st>>>(parts, out);
}

}  // namespace kzgmi
