// EIP-4844 blob front-end launchers (BLS12-381 only: compiled once).  Kernels: blob.hpp.
#include "launch.hpp"
#include "blob.hpp"

namespace kzgmi {

size_t BlobLaunch::table_bytes() { return BLOB_TABLE * sizeof(BlobF); }

void BlobLaunch::domain(hipStream_t st, void* table) {
  k_blob_domain<<<BLOB_N / 256, 256, 0, st>>>((BlobF*)table);
}

void BlobLaunch::challenges(hipStream_t st, int mapping, const uint8_t* blobs, const uint8_t* commitments, uint32_t n,
                            uint8_t* zs, uint32_t* err) {
  if (!n) return;
  if (mapping == HASH_WAVE) k_blob_challenge<true><<<n, 64, 0, st>>>(blobs, commitments, n, zs, err);
  else k_blob_challenge<false><<<grid_for(n, 64), 64, 0, st>>>(blobs, commitments, n, zs, err);
}

void BlobLaunch::eval(hipStream_t st, const uint8_t* blobs, const uint8_t* zs, const void* table, uint32_t n,
                      bool range_check, uint8_t* ys, uint32_t* err) {
  if (n) k_blob_eval<<<n, BLOB_EVAL_THREADS, 0, st>>>(blobs, zs, (const BlobF*)table, range_check ? 1 : 0, ys, err);
}

void BlobLaunch::batch_challenge(hipStream_t st, const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys,
                                 const uint8_t* proofs, uint32_t n, void* pow, uint32_t* chal_out) {
  k_blob_batch_challenge<<<1, 64, 0, st>>>(commitments, zs, ys, proofs, n, (BlobF*)pow, chal_out);
}

}  // namespace kzgmi
