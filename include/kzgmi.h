/* kzgmi -- MI355X-native KZG batch verifier: the drop-in C-ABI boundary.
 *
 * Reference interface replaced: the reference snapshot contains no code
 * (/root/reference/LICENSE:1-201 only), so there is no reference FFI
 * to cite line by line.  This header realises the contract of SURVEY.md section 8b, which
 * keeps the north-star entry point `batch_verify(commitments, zs, ys, proofs, srs)`
 * (BASELINE.json:5) behind a thin C ABI; every entry point below cites the spec line it
 * implements.  Plain pointers and sizes only; no torch or HIP types in any signature.
 *
 * Conventions:
 *   - Encodings are big-endian canonical.  Fr scalar: 32 B, value < r.
 *     G1: BLS12-381 96 B x||y, infinity = 0x40 || 95 zero bytes (ZCash uncompressed flags);
 *         BN254 64 B x||y, infinity = 64 zero bytes.
 *     G2: x.c1||x.c0||y.c1||y.c0 (192 B BLS12-381 / 128 B BN254), same infinity rules.
 *   - Points must be on the curve (checked: KZGMI_ERR_NOT_ON_CURVE).  Subgroup membership is
 *     checked only with KZGMI_FLAG_SUBGROUP_CHECK (the *_ex entry points, SURVEY.md 8f item
 *     1), which also accept compressed G1 inputs (KZGMI_FLAG_COMPRESSED):
 *       BLS12-381 48 B ZCash (0x80 compressed, 0x40 infinity, 0x20 larger y),
 *       BN254 32 B gnark-crypto (top bits 0b10 smaller y, 0b11 larger y, 0b01 infinity).
 *   - Return value 0 = OK, negative = error (see KZGMI_ERR_*).  Invalid input is an error,
 *     never "ok = 0".  kzgmi_last_error() gives a thread-local message.
 *   - Threading: one ctx per host thread; calls on one ctx are serialised by the caller.
 *   - Device-memory ordering: the library runs on its own non-blocking HIP streams, one per
 *     pipeline slot (+ one for host-buffer copies).  HIP gives streams GPU_MAX_HW_QUEUES hardware
 *     queues per stream priority (4 by default) and streams sharing a queue run one after
 *     another: when the slots outnumber the queues the slot streams cycle through the device's
 *     stream priorities (KZGMI_STREAM_PRIO=0/1 forces it off/on), which keeps 16 slots at 0.96
 *     of their 24-queue rate at the default 4 queues.  With a queue per slot, the batches'
 *     bucket accumulations also start in submission order (at most 2 -- 4 for small batches --
 *     at once; KZGMI_ACC_ORDER / KZGMI_ACC_ORDER_SMALL), so slots complete in the order they were
 *     submitted.  A caller that produced device inputs on
 *     another stream (e.g. a torch stream) must order the slot's next job after it --
 *     kzgmi_stream_wait(ctx, slot, stream) (no host sync), or synchronise that stream -- before
 *     the call that reads them.  Device outputs
 *     (partials, digests, generated points) are complete when the call, or the
 *     kzgmi_slot_wait / kzgmi_msm_wait that completes it, returns.  Device buffers passed to
 *     an async call must stay allocated until its wait returns.
 *   - Randomisers: r_i = int_be(SHA256(seed || le64(i))[0:16]) >> 1 (1 if zero); 127-bit,
 *     counter mode, so a shard [off, off+n) derives its own r_i with no communication.
 *     seed == NULL draws 32 bytes from the OS CSPRNG (verifier-private randomness).
 *   - Batch check: A = sum r_i pi_i; B = sum r_i C_i + sum (r_i z_i) pi_i - (sum r_i y_i) G1;
 *     accept iff e(A, [tau]_2) * e(-B, [1]_2) == 1.  n == 0 accepts.
 *   - The hot path runs only on the GPU: without a usable HIP device every compute entry
 *     point fails with KZGMI_ERR_DEVICE (there is no CPU fallback).
 */
#ifndef KZGMI_H
#define KZGMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { KZGMI_BLS12_381 = 0, KZGMI_BN254 = 1 } kzgmi_curve;

/* ABI revision of this header.  2: kzgmi_srs_load gained the g1 argument (3rd position),
 * kzgmi_ctx_reserve / kzgmi_alloc_count / kzgmi_abi_version were added.  3: kzgmi_pairing
 * returns the standard e(P, Q) on BLS12-381 (was its cube).  4: kzgmi_ctx_create takes the
 * SURVEY.md 8b device list (the single-device form is kzgmi_ctx_create_device; the ABI-3
 * kzgmi_ctx_create_multi is gone), and the pipelined host-buffer entry
 * kzgmi_batch_verify_ex_async, the pinned-host helpers kzgmi_host_* and kzgmi_slot_signal were
 * added.  5: partial records carry their shard's error (KZGMI_ERR_SHARD; combines fail on a
 * marked record), kzgmi_stream_wait orders the slot's NEXT job, multi-device contexts pipeline
 * whole batches per device through the async entry points (kzgmi_slot_device).  6: the EIP-4844
 * blob entry points kzgmi_blob_*_device and kzgmi_verify_blob_batch* were added; still 6 (additive):
 * the EIP-7594 cell entry points kzgmi_cell_* and kzgmi_verify_cell_batch*, and the cell extension
 * and recovery entry points kzgmi_compute_cells* and kzgmi_recover_cells*, and the cell proof entry
 * points kzgmi_cell_pk_*, kzgmi_*_cells_and_proofs*, kzgmi_fk20_scalars_device, kzgmi_g1_fft128_device,
 * and the EIP-4844 producer entry points kzgmi_blob_pk_*, kzgmi_blob_commit*, kzgmi_compute_kzg_proofs*,
 * kzgmi_compute_blob_proofs*, kzgmi_blob_quotient_device, and the search entry points
 * kzgmi_batch_check_partials_device, kzgmi_batch_range_partials_device, kzgmi_batch_find_invalid*,
 * kzgmi_verify_blob_batch_find_invalid*, kzgmi_find_invalid_stats, and the cell search entry points
 * kzgmi_cell_coeffs_device, kzgmi_cell_range_partials_device, kzgmi_verify_cell_batch_find_invalid*,
 * and the opening entry points kzgmi_open*, kzgmi_open_quotient_device, and the transform entry points
 * kzgmi_fr_ntt* with the evaluation-form openings kzgmi_open_evals*, and the transforms over G1
 * kzgmi_g1_ntt* with the openings at every point of a domain, kzgmi_open_all_key_* and kzgmi_open_all*,
 * and the openings on every coset of a domain, kzgmi_open_cosets_key_* and kzgmi_open_cosets*.
 * A caller built
 * against another revision must not bind the library: compare with kzgmi_abi_version(). */
#define KZGMI_ABI_VERSION 6

#define KZGMI_OK 0
#define KZGMI_ERR_ARG (-1)
#define KZGMI_ERR_ENCODING (-2)
#define KZGMI_ERR_NOT_ON_CURVE (-3)
#define KZGMI_ERR_SCALAR (-4)
#define KZGMI_ERR_DEVICE (-5)
#define KZGMI_ERR_OOM (-6)
#define KZGMI_ERR_NOT_IN_SUBGROUP (-7)
#define KZGMI_ERR_SHARD (-8) /* a gathered partial record marks a shard that failed on its own device */

/* flags of the *_ex entry points */
#define KZGMI_FLAG_COMPRESSED 1u     /* commitments/proofs are compressed G1 encodings */
#define KZGMI_FLAG_SUBGROUP_CHECK 2u /* reject points outside the order-r subgroup (BLS12-381;
                                        BN254 G1 has cofactor 1, the flag is a no-op there) */
#define KZGMI_FLAG_POWERS 4u         /* r_i = r^i with r = int_be(seed32) < r supplied by the caller
                                        (e.g. the EIP-4844 verify_kzg_proof_batch challenge) */
#define KZGMI_FLAG_FIAT_SHAMIR 8u    /* deterministic randomisers from the inputs: a challenge r
                                        derived on the GPU -- leaf_i = SHA256("KZGMI_FS_LEAF_V1" ||
                                        be64(i) || C_i || pi_i || z_i || y_i) (points compressed),
                                        binary Merkle root over max(4096, next_pow2(n)) zero-padded
                                        leaf slots, r = int_be(SHA256("KZGMI_FS_ROOT_V1" || be64(n)
                                        || root)) mod r (1 if 0) -- then the counter-mode 127-bit
                                        r_i above with seed = be32(r); seed32 is ignored */
#define KZGMI_FLAG_TRUSTED_G1 16u    /* the caller guarantees every C_i / pi_i is in G1 (e.g. it was
                                        subgroup-checked when deserialised): lets BLS12-381 use the
                                        GLV endomorphism, which is exact only on G1 (kzgmi_set_glv).
                                        Results for inputs outside G1 are then unspecified. */

typedef struct kzgmi_ctx kzgmi_ctx; /* one GPU (or a device list), its streams and workspaces */
typedef struct kzgmi_srs kzgmi_srs; /* {G1, [1]_2, [tau]_2} + precomputed Miller lines */
typedef struct kzgmi_ck kzgmi_ck;   /* prover commit key: [tau^i]_1 + fixed-base tables */

/* Version string of the library build. */
const char* kzgmi_version(void);
/* KZGMI_ABI_VERSION the library was built with. */
int kzgmi_abi_version(void);
/* Thread-local description of the last error. */
const char* kzgmi_last_error(void);

/* SURVEY.md 8b kzgmi_ctx_create(out, device_ids, n_devices), plus the pipeline depth: one
 * context over a device list (one process driving several GPUs; a device id may repeat;
 * n_devices = 1 is the common single-GPU context).  device_ids[0] is the primary device: every
 * synchronous single-device entry point below runs there.  `pipeline_slots` >= 1 (at most 64) is
 * the number of independent workspaces for the async entry points (1 is enough for the
 * synchronous calls; over several devices see kzgmi_slot_device); each holds ~1.3 GiB at
 * n = 2^20.  With n_devices > 1 the synchronous host-buffer
 * entry points kzgmi_batch_verify / kzgmi_batch_verify_ex / kzgmi_msm_g1 split their input by
 * point range over all devices (balanced, in units of 4096), run the shards concurrently and
 * combine the partial sums on the primary; kzgmi_batch_verify_multi_device /
 * kzgmi_msm_g1_multi_device take shards already resident on each device.  The exchange is 2
 * (batch) or 1 (MSM) partial records per device, copied to the primary with hipMemcpyPeerAsync
 * (xGMI) on the primary after every shard completed; processes that own one GPU each instead
 * all-gather kzgmi_batch_partial_device records over RCCL.  Every device gets
 * ceil(pipeline_slots / n_devices) workspaces, and the async entry points run whole batches per
 * device (kzgmi_slot_device). */
int kzgmi_ctx_create(kzgmi_ctx** out, const int* device_ids, int n_devices, int pipeline_slots);
/* The n_devices = 1 case of kzgmi_ctx_create, by device id (>= 0). */
int kzgmi_ctx_create_device(kzgmi_ctx** out, int device_id, int pipeline_slots);
void kzgmi_ctx_destroy(kzgmi_ctx* ctx);
int kzgmi_ctx_num_devices(const kzgmi_ctx* ctx);
/* Multi-device context: the async entry points (kzgmi_*_async, kzgmi_slot_wait, kzgmi_msm_wait,
 * kzgmi_stream_wait, kzgmi_slot_signal) pipeline WHOLE batches per device -- caller slot `slot`
 * (0 <= slot < pipeline_slots) runs on device device_ids[slot % n_devices], which this returns;
 * device pointers passed to that slot must live there.  Each device holds
 * ceil(pipeline_slots / n_devices) slots; caller slots 0 .. n_devices-1 are the devices' first
 * slots, which the synchronous split calls use.  Single-device context: device_ids[0]. */
int kzgmi_slot_device(const kzgmi_ctx* ctx, int slot);

/* Size every pipeline slot's device workspace (and, on a multi-device context, each device's
 * shard workspace) for batches of up to n tuples of `curve` verified with `flags`
 * (KZGMI_FLAG_*), and create the profiling events, so that later batch calls of at most that
 * size and mode allocate nothing.  Workspaces otherwise grow on first use; a caller timing a
 * steady state calls this first.  No job may be in flight.  On a multi-device context each
 * peer is sized for its share of the library's own balanced split (what the host-buffer entry
 * points use): shards passed to kzgmi_batch_verify_multi_device that are larger than
 * ceil(n / n_devices) rounded up to 4096 still grow the peer's workspace on first use.  The
 * host-buffer entry points also use a per-slot device staging buffer (n x (2 G1 + 64) B) and,
 * for pageable inputs, a per-slot pinned ring (2 x 16 MiB): these are made on a slot's first
 * host-buffer call, so a timed steady state of host-buffer calls warms every slot once first. */
int kzgmi_ctx_reserve(kzgmi_ctx* ctx, kzgmi_curve curve, size_t n, uint32_t flags);
/* Process-wide number of device workspace allocations the library has made so far (a timed
 * region that leaves it unchanged allocated nothing). */
uint64_t kzgmi_alloc_count(void);

/* Order the next job issued on slot `slot` after all work enqueued so far on `hip_stream` (a
 * hipStream_t of the ctx's primary device, passed as void*; NULL = the null stream), without a
 * host sync.  Several calls before one job all apply. */
int kzgmi_stream_wait(kzgmi_ctx* ctx, int slot, void* hip_stream);
/* The other direction: order all work enqueued later on `hip_stream` (a hipStream_t of the
 * primary device; NULL = the null stream) after everything enqueued so far on slot `slot`,
 * without a host sync -- e.g. an RCCL all-gather of a kzgmi_batch_partial_device_async partial
 * issued on the caller's stream.  The slot's job still completes (and reports its errors) with
 * kzgmi_slot_wait. */
int kzgmi_slot_signal(kzgmi_ctx* ctx, int slot, void* hip_stream);

/* Page-locked host memory for the host-buffer entry points: input arrays that lie inside a
 * kzgmi_host_alloc block or a kzgmi_host_register'ed range are copied to HBM by DMA on the
 * slot's stream, asynchronously (PCIe at full rate, overlapped with other slots' kernels).
 * Other (pageable) host memory is first copied by the calling thread(s) into the slot's own
 * pinned staging ring.  kzgmi_host_register pins an existing allocation (hipHostRegister);
 * unregister/free only when no job reading it is in flight. */
int kzgmi_host_alloc(size_t bytes, void** out);
void kzgmi_host_free(void* p);
int kzgmi_host_register(void* p, size_t bytes);
int kzgmi_host_unregister(void* p);

/* SURVEY.md 8b kzgmi_srs_load (BASELINE.json:5 "srs" = {G1, [1]_2, [tau]_2}): host encodings
 * of the SRS's G1 element g1 (the base of the -t G1 term; validated, must be a G1 member
 * other than infinity; g1 == NULL means the standard generator), the G2 generator and
 * [tau]_2.  Precomputes the Miller-loop line coefficients on the device(s). */
int kzgmi_srs_load(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* g1, const uint8_t* g2,
                   const uint8_t* tau_g2, kzgmi_srs** out);
void kzgmi_srs_free(kzgmi_srs* srs);

/* BASELINE.json:5 batch_verify(commitments, zs, ys, proofs, srs) -- host buffers (copied to
 * HBM, i.e. the PCIe-inclusive path; see kzgmi_batch_verify_ex_async for how).  *ok_out = 1
 * accept, 0 reject.  From 2^17 tuples the copy overlaps the computation: the batch is copied in
 * point ranges and each range's work starts when its copy lands (slot 0; slots 0-1 for
 * compressed, subgroup-checked and powers-of-r batches, which must then be idle too; not with
 * Fiat-Shamir).  KZGMI_HOST_CHUNKS=1 in the environment before kzgmi_ctx_create turns it off.
 * Calls of at most 4096 MSM terms (a batch has 3n + 1; with GLV 2 (2n + 1)) take a one-wave-
 * per-term path instead of the bucket method (KZGMI_SMALL_TERMS=<terms> moves the limit). */
int kzgmi_batch_verify(kzgmi_ctx* ctx, const kzgmi_srs* srs, const uint8_t* commitments,
                       const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, size_t n,
                       const uint8_t* seed32, int* ok_out);

/* Same check with the four input arrays already resident in device memory (device
 * pointers on ctx's device).  Synchronous. */
int kzgmi_batch_verify_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_commitments,
                              const void* d_zs, const void* d_ys, const void* d_proofs, size_t n,
                              const uint8_t* seed32, int* ok_out);

/* Pipelined form: enqueue on workspace `slot` (0 <= slot < pipeline_slots) and return at
 * once; kzgmi_slot_wait() blocks until that slot's verdict is ready.  Independent batches
 * on different slots overlap on the GPU (latency-bound tails of one batch run beside the
 * bucket accumulation of the next). */
int kzgmi_batch_verify_device_async(kzgmi_ctx* ctx, const kzgmi_srs* srs, int slot,
                                    const void* d_commitments, const void* d_zs, const void* d_ys,
                                    const void* d_proofs, size_t n, const uint8_t* seed32);
int kzgmi_slot_wait(kzgmi_ctx* ctx, int slot, int* ok_out);

/* batch_verify with input-format / validation flags (KZGMI_FLAG_*).
 * flags = 0 is exactly kzgmi_batch_verify / kzgmi_batch_verify_device_async. */
int kzgmi_batch_verify_ex(kzgmi_ctx* ctx, const kzgmi_srs* srs, const uint8_t* commitments,
                          const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, size_t n,
                          const uint8_t* seed32, uint32_t flags, int* ok_out);
int kzgmi_batch_verify_device_ex_async(kzgmi_ctx* ctx, const kzgmi_srs* srs, int slot,
                                       const void* d_commitments, const void* d_zs,
                                       const void* d_ys, const void* d_proofs, size_t n,
                                       const uint8_t* seed32, uint32_t flags);
/* BASELINE.json:5 batch_verify from HOST buffers, pipelined: the H2D copy of the four arrays is
 * enqueued on slot `slot`'s stream ahead of the batch's kernels, so the copy of one batch runs
 * beside the kernels of the batches on the other slots; kzgmi_slot_wait() returns the verdict.
 * Arrays inside pinned memory (kzgmi_host_alloc / kzgmi_host_register) are DMA'd directly and
 * the call returns at once -- they must stay allocated and unmodified until the wait returns.
 * Pageable arrays are copied through the slot's pinned staging ring before the call returns
 * (they may be reused at once; the call then costs the host-side copy).  On a multi-device
 * context the whole batch runs on the slot's device (kzgmi_slot_device); kzgmi_batch_verify_ex
 * splits one batch over all devices instead.
 * kzgmi_batch_verify / kzgmi_batch_verify_ex are this on slot 0 followed by the wait. */
int kzgmi_batch_verify_ex_async(kzgmi_ctx* ctx, const kzgmi_srs* srs, int slot,
                                const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys,
                                const uint8_t* proofs, size_t n, const uint8_t* seed32,
                                uint32_t flags);

/* Multi-device context (kzgmi_ctx_create with n_devices > 1): device d holds n_per_device[d] tuples
 * (global indices follow device order) at d_*[d], device pointers on device_ids[d].  flags as
 * kzgmi_batch_verify_ex; with KZGMI_FLAG_FIAT_SHAMIR every non-empty shard but the last must
 * hold a multiple of 4096 tuples.  Synchronous. */
int kzgmi_batch_verify_multi_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* const* d_commitments,
                                    const void* const* d_zs, const void* const* d_ys,
                                    const void* const* d_proofs, const size_t* n_per_device,
                                    const uint8_t* seed32, uint32_t flags, int* ok_out);

/* Fiat-Shamir challenge of KZGMI_FLAG_FIAT_SHAMIR for a device-resident batch (flags:
 * KZGMI_FLAG_COMPRESSED): r as 32 big-endian bytes. */
int kzgmi_fs_challenge_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_commitments,
                              const void* d_zs, const void* d_ys, const void* d_proofs, size_t n,
                              uint32_t flags, uint8_t* r_out);
/* Multi-GPU form: a shard [index_offset, index_offset + n) with index_offset % 4096 == 0
 * writes its ceil(n / 4096) subtree roots (32 B each) to d_out; gather all shards' roots in
 * order and derive r with kzgmi_fs_challenge_from_digests_device, then verify each shard
 * with kzgmi_batch_partial_device_async(..., flags 0, seed32 = be32(r)). */
int kzgmi_fs_chunk_digests_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_commitments,
                                  const void* d_zs, const void* d_ys, const void* d_proofs, size_t n,
                                  uint64_t index_offset, uint32_t flags, void* d_out);
int kzgmi_fs_challenge_from_digests_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_digests,
                                           size_t nchunks, uint64_t n_total, uint8_t* r_out);

/* ---- EIP-4844 blob batches (Deneb polynomial-commitments verify_blob_kzg_proof_batch) -------
 * BLS12-381 only (an SRS of another curve: KZGMI_ERR_ARG), domain size 4096.  A blob is 4096 x
 * 32 B big-endian canonical Fr (an element >= r: KZGMI_ERR_SCALAR); commitments and proofs are
 * 48 B ZCash compressed G1, always decoded with KZGMI_FLAG_COMPRESSED |
 * KZGMI_FLAG_SUBGROUP_CHECK semantics and error codes.  Device arrays are 16-byte aligned.
 *   z_i = int_be(SHA256("FSBLOBVERIFY_V1_" || be128(4096) || blob_i || C_i)) mod r
 *   y_i = p_i(z_i), p_i given by its values blob_i[j] at dom[j] = w^rev12(j), w = 7^((r-1)/4096)
 *   r   = int_be(SHA256("RCKZGBATCH___V1_" || be64(4096) || be64(n) ||
 *                       (C_i || be32B(z_i) || be32B(y_i) || pi_i for each i))) mod r
 *   verdict: the KZGMI_FLAG_POWERS check with r_i = r^i (r = 0 gives 1, 0, 0, ...); n == 0 accepts.
 * (blob_to_kzg_commitment is kzgmi_commit over a commit key of the Lagrange-form SRS in
 * bit-reversed order.)
 * The three stages, synchronous on slot 0 -- d_zs_out / d_ys_out: n x 32 B; kzgmi_blob_eval_device
 * takes any z < r, points of the domain included: */
int kzgmi_blob_challenges_device(kzgmi_ctx* ctx, const void* d_blobs, const void* d_commitments48,
                                 size_t n, void* d_zs_out);
int kzgmi_blob_eval_device(kzgmi_ctx* ctx, const void* d_blobs, const void* d_zs, size_t n,
                           void* d_ys_out);
int kzgmi_blob_batch_challenge_device(kzgmi_ctx* ctx, const void* d_commitments48, const void* d_zs,
                                      const void* d_ys, const void* d_proofs48, size_t n,
                                      uint8_t r_out[32]);
/* The whole verification: the three stages and the batch check chained on the slot's stream with
 * no host round trip (z_i, y_i and the power table live in the slot's workspace, grown on first
 * use).  Host buffers (staged on slot 0 like kzgmi_batch_verify: pinned ranges by DMA, pageable
 * ones through the slot's ring), device buffers, and the pipelined device form, whose verdict
 * kzgmi_slot_wait returns.  kzgmi_last_combination works after the synchronous forms.  On a
 * multi-device context the whole batch runs on the slot's device. */
int kzgmi_verify_blob_batch(kzgmi_ctx* ctx, const kzgmi_srs* srs, const uint8_t* blobs,
                            const uint8_t* commitments48, const uint8_t* proofs48, size_t n,
                            int* ok_out);
int kzgmi_verify_blob_batch_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_blobs,
                                   const void* d_commitments48, const void* d_proofs48, size_t n,
                                   int* ok_out);
int kzgmi_verify_blob_batch_device_async(kzgmi_ctx* ctx, const kzgmi_srs* srs, int slot,
                                         const void* d_blobs, const void* d_commitments48,
                                         const void* d_proofs48, size_t n);

/* ---- EIP-4844 commitments and proofs (Deneb polynomial-commitments blob_to_kzg_commitment,
 * compute_kzg_proof, compute_blob_kzg_proof) -- BLS12-381 only, with the blob conventions above.
 * With v_j = blob element j = p(dom[j]) and L_j = [l_j(tau)]_1 for the Lagrange polynomial l_j of dom[j]:
 *     commitment = sum_j v_j L_j
 *     y = p(z),  q_j = (v_j - y) / (dom[j] - z),  proof = sum_j q_j L_j       (q = (p - y) / (X - z) on dom)
 *     z = dom[m]:  y = v_m,  q_m = sum_{i != m} (v_i - y) dom[i] / (z (z - dom[i]))
 * Both sums are one fixed-base MSM over the blob proof key: the 4096 points as a table of window
 * multiples (kzgmi_blob_pk_device_bytes: 256 MiB, 4096 x 64 x 8 rows of 96 B in 128 B slots, plus one
 * flag byte per point), batched over the nb blobs of a call.
 * g1_lagrange: 4096 x 96 B uncompressed, point j = L_j (the trusted setup's Lagrange points in
 * bit-reversed order).  Validated like kzgmi_cell_pk_load's points: encoding, on curve, in G1, each
 * with its own code; the point at infinity: KZGMI_ERR_ARG.  The loader does not (cannot) check that
 * the points are a Lagrange basis: it is a fixed-base key over any 4096 G1 points.  The key lives on
 * the context's primary device and works with that device's slots only; a key of another context:
 * KZGMI_ERR_ARG.
 * blob_commit: nb blobs -> nb x 48 B ZCash compressed commitments (infinity: 0xC0 and 47 zero bytes).
 * compute_kzg_proofs: zs nb x 32 B big-endian (z >= r: KZGMI_ERR_SCALAR) -> proofs nb x 48 B and
 * ys nb x 32 B; any z < r, points of the domain included.
 * compute_blob_proofs: commitments nb x 48 B, decoded and subgroup-checked with
 * KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK semantics and error codes; z_i is the blob's
 * challenge, hashed on the device -> proofs nb x 48 B (what kzgmi_verify_blob_batch accepts).
 * A blob element >= r: KZGMI_ERR_SCALAR.  nb == 0 succeeds and writes nothing; nb > 4096:
 * KZGMI_ERR_ARG.  Device arrays are 16-byte aligned; outputs overlap neither the inputs nor each
 * other.  The host forms stage through slot 0 and copy the results back; the synchronous device forms
 * run on slot 0; the async forms run on any slot and complete with kzgmi_slot_wait (ok_out = 1), which
 * reports the device-side errors.  A call that fails writes no output and leaves its slot usable.
 * Scratch (the quotients at nb x 128 KiB, the partial sums, the decoded commitments) lives in the
 * slot's workspace (grown on first use, counted by kzgmi_alloc_count). */
typedef struct kzgmi_blob_pk kzgmi_blob_pk;
int kzgmi_blob_pk_load(kzgmi_ctx* ctx, const uint8_t* g1_lagrange, kzgmi_blob_pk** out);
void kzgmi_blob_pk_free(kzgmi_blob_pk* pk);
size_t kzgmi_blob_pk_device_bytes(const kzgmi_blob_pk* pk);
int kzgmi_blob_commit(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, const uint8_t* blobs, size_t nb,
                      uint8_t* commitments48_out);
int kzgmi_blob_commit_device(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, const void* d_blobs, size_t nb,
                             void* d_commitments48_out);
int kzgmi_blob_commit_device_async(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, int slot, const void* d_blobs, size_t nb,
                                   void* d_commitments48_out);
int kzgmi_compute_kzg_proofs(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, const uint8_t* blobs, const uint8_t* zs,
                             size_t nb, uint8_t* proofs48_out, uint8_t* ys_out);
int kzgmi_compute_kzg_proofs_device(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, const void* d_blobs, const void* d_zs,
                                    size_t nb, void* d_proofs48_out, void* d_ys_out);
int kzgmi_compute_kzg_proofs_device_async(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, int slot, const void* d_blobs,
                                          const void* d_zs, size_t nb, void* d_proofs48_out, void* d_ys_out);
int kzgmi_compute_blob_proofs(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, const uint8_t* blobs,
                              const uint8_t* commitments48, size_t nb, uint8_t* proofs48_out);
int kzgmi_compute_blob_proofs_device(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, const void* d_blobs,
                                     const void* d_commitments48, size_t nb, void* d_proofs48_out);
int kzgmi_compute_blob_proofs_device_async(kzgmi_ctx* ctx, const kzgmi_blob_pk* pk, int slot, const void* d_blobs,
                                           const void* d_commitments48, size_t nb, void* d_proofs48_out);
/* Diagnostic (synchronous, slot 0), like kzgmi_blob_eval_device: y_i = p_i(z_i) -> d_ys_out (nb x 32 B)
 * and the quotient's evaluations q_i -> d_q_out (nb x 128 KiB, 32 B big-endian each, blob layout).
 * Unlike the calls above it writes straight to the caller's arrays, which it does not check for
 * overlap: on an error (an element or z >= r) their contents are unspecified. */
int kzgmi_blob_quotient_device(kzgmi_ctx* ctx, const void* d_blobs, const void* d_zs, size_t nb, void* d_ys_out,
                               void* d_q_out);

/* ---- EIP-7594 cell batches (PeerDAS polynomial-commitments-sampling verify_cell_kzg_proof_batch) --
 * BLS12-381 only.  r is the scalar modulus, w = 7^((r-1)/8192) (its square is the blob domain's
 * root), rev_b is b-bit reversal.  A cell is 64 x 32 B big-endian canonical Fr, 2048 B (an element
 * >= r: KZGMI_ERR_SCALAR).  Element j of a cell with cell_index i (0 <= i < 128) is the polynomial's
 * value at w^rev13(64 i + j) = h_i * w64^rev6(j), with h_i = w^rev7(i) and w64 = w^128; so
 * h_i^64 = (w^64)^rev7(i).  The cell's interpolation polynomial I = p mod (X^64 - h_i^64) is
 *   I(X) = sum_m c_m X^m,  c_m = h_i^-m * 64^-1 * sum_j e_j * w64^(-rev6(j) m).
 * Inputs are deduplicated: commitments48[m] are unique 48 B compressed commitments,
 * commitment_indices[n] and cell_indices[n] are uint64 (little-endian in memory), cells[n] are
 * 2048 B each, proofs48[n] 48 B compressed; commitments and proofs are decoded with
 * KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK semantics and error codes.  Device arrays are
 * 16-byte aligned.  cell_index >= 128 or commitment_index >= m: KZGMI_ERR_ARG (found on the
 * device).  Duplicate (commitment, cell) pairs are legal; n == 0 accepts.
 *   r = int_be(SHA256("RCKZGCBATCH__V1_" || be64(4096) || be64(64) || be64(m) || be64(n)
 *         || C_0 .. C_{m-1}
 *         || for k < n: be64(commitment_indices[k]) || be64(cell_indices[k]) || cells[k] || proofs[k]))
 *       mod r                                           (48 + 48 m + 2112 n message bytes)
 *   verdict: e(sum r^k pi_k, [tau^64]_2) = e(sum r^k C_k + sum r^k h_k^64 pi_k - [sum r^k I_k(tau)]_1, [1]_2)
 *   with weights r^k, k = 0 .. n-1 (r = 0 gives 1, 0, 0, ...).
 * The transcript hash is one sequential SHA-256 (33 compressions per cell), so every verify entry
 * point takes an optional caller-supplied r32 (32 B big-endian, < r): NULL derives r on the device;
 * a caller holding the bytes on the host can hash there.
 * The cell SRS: g1_monomial = [tau^m]_1 for m < 64 (64 x 96 B uncompressed, all validated and in
 * G1), [1]_2 and [tau^64]_2.  It holds an ordinary kzgmi_srs for ([tau^0]_1, [1]_2, [tau^64]_2).
 * Passing anything else where a kzgmi_cell_srs is expected: KZGMI_ERR_ARG. */
typedef struct kzgmi_cell_srs kzgmi_cell_srs;
int kzgmi_cell_srs_load(kzgmi_ctx* ctx, const uint8_t* g1_monomial, const uint8_t* g2, const uint8_t* tau64_g2,
                        kzgmi_cell_srs** out);
void kzgmi_cell_srs_free(kzgmi_cell_srs* srs);
/* The stages, synchronous on slot 0.  kzgmi_cell_interp_device: the aggregated coefficients c_m of
 * sum_k r^k I_k for the given r32 (required) -> d_coeffs_out, 64 x 32 B big-endian. */
int kzgmi_cell_batch_challenge_device(kzgmi_ctx* ctx, const void* d_commitments48, size_t m,
                                      const void* d_commitment_indices, const void* d_cell_indices,
                                      const void* d_cells, const void* d_proofs48, size_t n, uint8_t r_out[32]);
int kzgmi_cell_interp_device(kzgmi_ctx* ctx, const void* d_cell_indices, const void* d_cells, size_t n,
                             const uint8_t r32[32], void* d_coeffs_out);
/* The whole verification, chained on the slot's stream with no host round trip.  Host buffers
 * (staged on slot 0 like kzgmi_verify_blob_batch), device buffers, and the pipelined device form,
 * whose verdict kzgmi_slot_wait returns.  kzgmi_last_combination works after the synchronous
 * forms.  On a multi-device context the whole batch runs on the slot's device. */
int kzgmi_verify_cell_batch(kzgmi_ctx* ctx, const kzgmi_cell_srs* srs, const uint8_t* commitments48, size_t m,
                            const uint64_t* commitment_indices, const uint64_t* cell_indices, const uint8_t* cells,
                            const uint8_t* proofs48, size_t n, const uint8_t* r32, int* ok_out);
int kzgmi_verify_cell_batch_device(kzgmi_ctx* ctx, const kzgmi_cell_srs* srs, const void* d_commitments48, size_t m,
                                   const void* d_commitment_indices, const void* d_cell_indices,
                                   const void* d_cells, const void* d_proofs48, size_t n, const uint8_t* r32,
                                   int* ok_out);
int kzgmi_verify_cell_batch_device_async(kzgmi_ctx* ctx, const kzgmi_cell_srs* srs, int slot,
                                         const void* d_commitments48, size_t m, const void* d_commitment_indices,
                                         const void* d_cell_indices, const void* d_cells, const void* d_proofs48,
                                         size_t n, const uint8_t* r32);
/* Locating the invalid cells of a rejected cell batch (the search of "locating the invalid tuples"
 * below, with its conventions: synchronous, slot 0 idle, the context's primary device, an input
 * error -- encoding, curve, subgroup, a cell element >= r, a cell index >= 128, a commitment index
 * >= m -- is the return code with the outputs untouched).  Cell k is invalid iff
 *   e(pi_k, [tau^64]_2) != e(C_{commitment_indices[k]} + z_k pi_k - [I_k(tau)]_1, [1]_2),  z_k = h_{cell_indices[k]}^64;
 * duplicate (commitment, cell) pairs are legal and every index is judged on its own.  A range g of
 * indices passes iff e(A_g, [tau^64]_2) e(-B_g, [1]_2) = 1 for
 *   A_g = sum_{k in g} r_k pi_k,
 *   B_g = sum_{k in g} r_k C_{cidx[k]} + sum_{k in g} (r_k z_k) pi_k - sum_{m < 64} c_m(g) [tau^m]_1,
 *   c_m(g) = sum_{k in g} r_k coef_k[m]   (coef_k: the 64 coefficients of I_k),
 * r_k the 127-bit counter-mode randomiser of the global index k:
 *   r_k = int_be(SHA256(seed32 || le64(k))[0:16]) >> 1, 1 if that is 0
 * (seed32 == NULL: drawn from the OS CSPRNG).  Every level of the search runs in the grouped
 * one-wave-per-term kernel (3 len + 64 terms per range), so a call takes n <= 65536 cells (and
 * m <= 65536 commitments): more is KZGMI_ERR_ARG.  bad_out, max_bad (1 .. 4096), n_bad_out, more_out
 * and n == 0 are as in kzgmi_batch_find_invalid; kzgmi_find_invalid_stats reports the search
 * (bucket jobs: 0, wave-terms: the sum of 3 len + 64 over every tested range).  The host form stages
 * like kzgmi_verify_cell_batch.
 * kzgmi_cell_coeffs_device (diagnostic): c_m of I_k for every cell -> d_coeffs_out, n x 64 x 32 B
 * big-endian, coefficient m of cell k at byte 32 (64 k + m); n <= 65536.
 * kzgmi_cell_range_partials_device: (A_g, B_g) of n_ranges index ranges of one device-resident cell
 * batch whose first cell has global index index_offset, 2 records per range -> d_partials_out;
 * ranges, bounds and errors as kzgmi_batch_range_partials_device (the 256 MiB of trees hold about
 * 160 000 cells over all ranges). */
int kzgmi_cell_coeffs_device(kzgmi_ctx* ctx, const void* d_cell_indices, const void* d_cells, size_t n,
                             void* d_coeffs_out);
int kzgmi_cell_range_partials_device(kzgmi_ctx* ctx, const kzgmi_cell_srs* srs, const void* d_commitments48, size_t m,
                                     const void* d_commitment_indices, const void* d_cell_indices,
                                     const void* d_cells, const void* d_proofs48, size_t n, uint64_t index_offset,
                                     const uint8_t* seed32, const uint64_t* ranges, size_t n_ranges,
                                     void* d_partials_out);
int kzgmi_verify_cell_batch_find_invalid(kzgmi_ctx* ctx, const kzgmi_cell_srs* srs, const uint8_t* commitments48,
                                         size_t m, const uint64_t* commitment_indices, const uint64_t* cell_indices,
                                         const uint8_t* cells, const uint8_t* proofs48, size_t n,
                                         const uint8_t* seed32, uint64_t* bad_out, size_t max_bad, size_t* n_bad_out,
                                         int* more_out);
int kzgmi_verify_cell_batch_find_invalid_device(kzgmi_ctx* ctx, const kzgmi_cell_srs* srs,
                                                const void* d_commitments48, size_t m,
                                                const void* d_commitment_indices, const void* d_cell_indices,
                                                const void* d_cells, const void* d_proofs48, size_t n,
                                                const uint8_t* seed32, uint64_t* bad_out, size_t max_bad,
                                                size_t* n_bad_out, int* more_out);

/* ---- EIP-7594 cell extension and recovery (compute_cells, and the cells of
 * recover_cells_and_kzg_proofs; the proofs: the next section) -- BLS12-381 only, with the cell
 * conventions above.  A blob is 4096 x 32 B big-endian canonical Fr, blob[k] = p(dom[k]) with
 * dom[k] = (w^2)^rev12(k) and deg p < 4096; its 128 cells are 8192 x 32 B = 256 KiB, cell i at byte
 * 2048 i.  An input element >= r: KZGMI_ERR_SCALAR.
 * compute_cells: blobs (nb x 128 KiB) -> cells_out (nb x 256 KiB).  Cells 0..63 are the blob's bytes
 * (rev13(k) = 2 rev12(k) for k < 4096), cells 64..127 are p on w * dom[k], in the same order.
 * recover_cells: k distinct cell indices (uint64, any order, 64 <= k <= 128) SHARED by all nb blobs
 * of the call -- the column shape: the same columns of every blob of a block -- and nb x k cells
 * (cells of blob b at byte 2048 k b, in the order of the indices) -> cells_out, all 128 cells of
 * every blob.  The input of one blob is CONSISTENT if some polynomial of degree < 4096 takes all
 * 64 k given values; it is then unique and the output is its 128 cells, bit-exact.  With k = 64
 * every input is consistent.  If any blob's input is inconsistent the call fails with
 * KZGMI_ERR_ARG and the outputs are unspecified.  k < 64 or k > 128 (checked on the host), a cell
 * index >= 128 or a duplicate index (found on the device): KZGMI_ERR_ARG.
 * nb == 0 succeeds and writes nothing; nb > 4096: KZGMI_ERR_ARG.  Device arrays are 16-byte aligned;
 * outputs must not overlap inputs.  The host-buffer forms stage through slot 0 (like
 * kzgmi_verify_blob_batch) and copy the result back; the synchronous device forms run on slot 0;
 * the async forms run on any slot and complete with kzgmi_slot_wait (ok_out = 1), which reports
 * the device-side errors above.  On a multi-device context the job runs on the slot's device.
 * Scratch lives in the slot's workspace (grown on first use, counted by kzgmi_alloc_count). */
int kzgmi_compute_cells(kzgmi_ctx* ctx, const uint8_t* blobs, size_t nb, uint8_t* cells_out);
int kzgmi_compute_cells_device(kzgmi_ctx* ctx, const void* d_blobs, size_t nb, void* d_cells_out);
int kzgmi_compute_cells_device_async(kzgmi_ctx* ctx, int slot, const void* d_blobs, size_t nb, void* d_cells_out);
int kzgmi_recover_cells(kzgmi_ctx* ctx, const uint64_t* cell_indices, size_t k, const uint8_t* cells, size_t nb,
                        uint8_t* cells_out);
int kzgmi_recover_cells_device(kzgmi_ctx* ctx, const void* d_cell_indices, size_t k, const void* d_cells, size_t nb,
                               void* d_cells_out);
int kzgmi_recover_cells_device_async(kzgmi_ctx* ctx, int slot, const void* d_cell_indices, size_t k,
                                     const void* d_cells, size_t nb, void* d_cells_out);

/* ---- EIP-7594 cell proof generation (compute_cells_and_kzg_proofs, recover_cells_and_kzg_proofs),
 * the FK20 way -- BLS12-381 only, with the cell conventions above.  For a blob with polynomial
 * p(X) = sum_{j < 4096} c_j X^j and z_i = h_i^64,
 *     proof_i = [q_i(tau)]_1,   q_i(X) = (p(X) - I_i(X)) / (X^64 - z_i) = floor(p / (X^64 - z_i))
 * (I_i = p mod (X^64 - z_i): cell i's interpolation polynomial), 48 B ZCash compressed (infinity:
 * 0xC0 and 47 zero bytes); proof i of blob b at byte 48 (128 b + i) of proofs_out.
 * With omega = w^64 (order 128) and S_m = [tau^m]_1:  proof_i = P_{rev7(i)},
 * P_e = sum_{t < 63} omega^(e t) H_t,  H_t = sum_{b < 64} sum_{u <= 62 - t} c_{64 (u + t + 1) + b} S_{64 u + b}.
 * H is computed as 64 cyclic convolutions of length 128: a^(b) = (c_b, c_{64 + b}, .., c_{64 63 + b},
 * 0 x 64), x^(b)[0] = S_b, x^(b)[128 - u] = S_{64 u + b} for u = 1 .. 62 and infinity elsewhere;
 * hhat[pos] = sum_b DFT(a^(b))[pos] DFT(x^(b))[pos] and H_t = IDFT(hhat)[t + 1] (root omega).
 * The cell proof key holds DFT(x^(b)) for every b -- 8192 points that depend on the SRS only -- as a
 * fixed-base window table (kzgmi_cell_pk_device_bytes: about 0.5 GiB).  g1_monomial: [tau^m]_1 for
 * m < 4096, 4096 x 96 B, validated like kzgmi_cell_srs_load's points (encoding, on curve, in G1, each
 * with its own error code; the point at infinity: KZGMI_ERR_ARG).  The key lives on the context's
 * primary device and works with that device's slots only, as commit keys do; a key of another
 * context: KZGMI_ERR_ARG.
 * compute_cells_and_proofs: cells_out may be NULL (proofs only); otherwise its bytes are those of
 * kzgmi_compute_cells.  recover_cells_and_proofs: kzgmi_recover_cells (cells_out is required),
 * then the proofs of every recovered blob; an inconsistent input fails with KZGMI_ERR_ARG exactly as
 * kzgmi_recover_cells does.  No proof is written by a call that fails.
 * Semantics, errors and sizes otherwise follow kzgmi_compute_cells* / kzgmi_recover_cells*
 * (element >= r: KZGMI_ERR_SCALAR; nb == 0 succeeds and writes nothing; nb > 4096: KZGMI_ERR_ARG;
 * 16-byte aligned device arrays; outputs overlap neither the inputs nor each other; async forms
 * complete with kzgmi_slot_wait).  Scratch lives in the slot's workspace. */
typedef struct kzgmi_cell_pk kzgmi_cell_pk;
int kzgmi_cell_pk_load(kzgmi_ctx* ctx, const uint8_t* g1_monomial, kzgmi_cell_pk** out);
void kzgmi_cell_pk_free(kzgmi_cell_pk* pk);
size_t kzgmi_cell_pk_device_bytes(const kzgmi_cell_pk* pk);
int kzgmi_compute_cells_and_proofs(kzgmi_ctx* ctx, const kzgmi_cell_pk* pk, const uint8_t* blobs, size_t nb,
                                   uint8_t* cells_out, uint8_t* proofs_out);
int kzgmi_compute_cells_and_proofs_device(kzgmi_ctx* ctx, const kzgmi_cell_pk* pk, const void* d_blobs, size_t nb,
                                          void* d_cells_out, void* d_proofs_out);
int kzgmi_compute_cells_and_proofs_device_async(kzgmi_ctx* ctx, const kzgmi_cell_pk* pk, int slot,
                                                const void* d_blobs, size_t nb, void* d_cells_out,
                                                void* d_proofs_out);
int kzgmi_recover_cells_and_proofs(kzgmi_ctx* ctx, const kzgmi_cell_pk* pk, const uint64_t* cell_indices, size_t k,
                                   const uint8_t* cells, size_t nb, uint8_t* cells_out, uint8_t* proofs_out);
int kzgmi_recover_cells_and_proofs_device(kzgmi_ctx* ctx, const kzgmi_cell_pk* pk, const void* d_cell_indices,
                                          size_t k, const void* d_cells, size_t nb, void* d_cells_out,
                                          void* d_proofs_out);
int kzgmi_recover_cells_and_proofs_device_async(kzgmi_ctx* ctx, const kzgmi_cell_pk* pk, int slot,
                                                const void* d_cell_indices, size_t k, const void* d_cells,
                                                size_t nb, void* d_cells_out, void* d_proofs_out);
/* Diagnostics (synchronous, slot 0), like kzgmi_cell_interp_device.
 * fk20_scalars: DFT(a^(b))[pos] of nb device-resident blobs as 32 B big-endian at
 * 32 ((128 blob + pos) 64 + b) of d_out (nb x 256 KiB).
 * g1_fft128: count (<= 4096) independent size-128 DFTs over G1 of uncompressed points (96 B each,
 * validated: encoding, on curve), natural order in and out, root omega; inverse != 0: root omega^-1
 * and the factor 1 / 128. */
int kzgmi_fk20_scalars_device(kzgmi_ctx* ctx, const void* d_blobs, size_t nb, void* d_out);
int kzgmi_g1_fft128_device(kzgmi_ctx* ctx, const void* d_points96, size_t count, int inverse, void* d_out96);

/* Validate n device-resident G1 encodings (flags: KZGMI_FLAG_COMPRESSED,
 * KZGMI_FLAG_SUBGROUP_CHECK): 0 if all are valid, else the first error class found. */
int kzgmi_g1_validate_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_points, size_t n,
                             uint32_t flags);
/* Compress n device-resident uncompressed G1 encodings into d_out (n x 48 B / 32 B).  Input
 * utility for tests and benchmarks: no validation. */
int kzgmi_g1_compress_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_points, size_t n,
                             void* d_out);

/* Diagnostics: the combined points A and B of the last synchronous batch_verify on slot 0
 * (G1 encodings, 2 x G1 bytes), for bit-exact parity tests against the oracle. */
int kzgmi_last_combination(kzgmi_ctx* ctx, uint8_t* a_out, uint8_t* b_out);

/* SURVEY.md 8b kzgmi_msm_g1: sum k_i P_i, host buffers; out = G1 encoding. */
int kzgmi_msm_g1(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* points, const uint8_t* scalars,
                 size_t n, uint8_t* out);
/* Same with device-resident points/scalars (output to host). */
int kzgmi_msm_g1_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_points,
                        const void* d_scalars, size_t n, uint8_t* out);

/* Pipelined MSM (configs[1] throughput): enqueue on workspace `slot` and return at once;
 * kzgmi_msm_wait() blocks until that slot's result is ready and writes the G1 encoding.
 * MSMs on different slots overlap on the GPU exactly like the async batch verifications
 * (kzgmi_slot_wait also completes an MSM job, discarding the point). */
int kzgmi_msm_g1_device_async(kzgmi_ctx* ctx, kzgmi_curve curve, int slot, const void* d_points,
                              const void* d_scalars, size_t n);
int kzgmi_msm_wait(kzgmi_ctx* ctx, int slot, uint8_t* out);

/* ---- multi-GPU point-range sharding ----------------------------
 * A rank verifying tuples [index_offset, index_offset + n) of a global batch writes its
 * partial (A_k, B_k) as 2 opaque partial-point records (kzgmi_partial_bytes() each) to
 * device memory; the records are all-gathered over RCCL and any rank combines them.
 * A shard that fails validation on its own device (an error reported by its wait) still writes
 * its records, MARKED as failed; a shard rejected before anything ran (an error returned by the
 * enqueue call) is marked by the caller filling its records with 0xFF bytes.  Every combine
 * that reads a marked record fails -- with the shard's own error code, or KZGMI_ERR_SHARD -- so
 * no rank can accept a batch one of whose shards was rejected, and every rank still takes part
 * in the collective (kzgmi/distributed.py). */
size_t kzgmi_partial_bytes(kzgmi_curve curve);
/* Encode `count` device-resident partial records (e.g. a shard's A_k, B_k) as G1 encodings
 * (count x G1 bytes, host) -- for checking partials against a CPU reference. */
int kzgmi_partial_encode_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_records, size_t count,
                                uint8_t* out);
int kzgmi_batch_partial_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_commitments,
                               const void* d_zs, const void* d_ys, const void* d_proofs, size_t n,
                               uint64_t index_offset, const uint8_t* seed32, void* d_partial_out);
int kzgmi_batch_combine_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_partials,
                               int n_parts, int* ok_out);
/* Pipelined forms of the two calls above on workspace `slot`; kzgmi_slot_wait() completes
 * them (ok_out = 1 for a partial job, the verdict for a combine job).  A rank keeps several
 * shards in flight exactly like kzgmi_batch_verify_device_async. */
int kzgmi_batch_partial_device_async(kzgmi_ctx* ctx, const kzgmi_srs* srs, int slot,
                                     const void* d_commitments, const void* d_zs, const void* d_ys,
                                     const void* d_proofs, size_t n, uint64_t index_offset,
                                     const uint8_t* seed32, uint32_t flags, void* d_partial_out);
int kzgmi_batch_combine_device_async(kzgmi_ctx* ctx, const kzgmi_srs* srs, int slot,
                                     const void* d_partials, int n_parts);
int kzgmi_msm_partial_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_points,
                             const void* d_scalars, size_t n, void* d_partial_out);
int kzgmi_msm_combine_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_partials,
                             int n_parts, uint8_t* out);
/* sum k_i P_i over shards resident on each device of a multi-device context (see
 * kzgmi_batch_verify_multi_device); out = G1 encoding. */
int kzgmi_msm_g1_multi_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* const* d_points,
                              const void* const* d_scalars, const size_t* n_per_device, uint8_t* out);
/* Pipelined forms: the partial completes with kzgmi_slot_wait, the combine (sum of the
 * gathered records, encoded) with kzgmi_msm_wait. */
int kzgmi_msm_partial_device_async(kzgmi_ctx* ctx, kzgmi_curve curve, int slot, const void* d_points,
                                   const void* d_scalars, size_t n, void* d_partial_out);
int kzgmi_msm_combine_device_async(kzgmi_ctx* ctx, kzgmi_curve curve, int slot,
                                   const void* d_partials, int n_parts);

/* ---- locating the invalid tuples of a rejected batch -----------------------
 * A verify call answers one bit for the whole batch.  These calls say WHICH tuples are wrong, by
 * group testing over index ranges on the device: a range [lo, hi) passes iff
 * e(A, [tau]_2) e(-B, [1]_2) = 1 for A = sum r_i pi_i, B = sum r_i C_i + (r_i z_i) pi_i - (r_i y_i) G1
 * over its tuples, r_i the 127-bit counter-mode randomiser of the GLOBAL index i (as for shards);
 * a failing range is split and its parts are tested, down to single tuples.  The search always uses
 * counter-mode randomisers (seed32, or the OS CSPRNG when NULL), whatever mode produced the
 * rejection: KZGMI_FLAG_POWERS and KZGMI_FLAG_FIAT_SHAMIR are KZGMI_ERR_ARG here; the flags taken
 * are KZGMI_FLAG_COMPRESSED, KZGMI_FLAG_SUBGROUP_CHECK and KZGMI_FLAG_TRUSTED_G1.  All of them are
 * synchronous, run on slot 0 (which must be idle) of the context's primary device, and report an
 * input error (encoding, curve, subgroup, scalar >= r) as their return code with the outputs
 * untouched: localising malformed encodings is out of scope.
 *
 * kzgmi_batch_check_partials_device: the verdict per record pair, ok_out[g] (0 / 1) for
 * (A_g, B_g) = d_partials[2 g], [2 g + 1]; a marked record fails the call with its own code, as
 * kzgmi_batch_combine_device does.  A sharded caller names the failing shard with it. */
int kzgmi_batch_check_partials_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_partials,
                                      size_t n_groups, uint8_t* ok_out);
/* (A_g, B_g) of n_ranges index ranges (uint64 lo, hi pairs on the host, lo < hi <= n, any order,
 * may overlap, n_ranges <= 65536) of one device-resident batch whose first tuple has global index
 * index_offset; 2 records per range -> d_partials_out.  One wave per term in one launch (no
 * buckets): meant for many short ranges; a call whose summation trees would pass the workspace
 * bound (256 MiB: about 160 000 tuples over all ranges) is KZGMI_ERR_ARG. */
int kzgmi_batch_range_partials_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_commitments,
                                      const void* d_zs, const void* d_ys, const void* d_proofs, size_t n,
                                      uint64_t index_offset, const uint8_t* seed32, uint32_t flags,
                                      const uint64_t* ranges, size_t n_ranges, void* d_partials_out);
/* bad_out: the lowest min(max_bad, #invalid) invalid indices, ascending; *n_bad_out their count;
 * *more_out = 1 iff a further invalid tuple exists.  1 <= max_bad <= 4096.  n == 0: none.
 * A tuple is invalid iff e(pi_i, [tau]_2) != e(C_i - y_i G1 + z_i pi_i, [1]_2).  Host arrays are
 * staged like kzgmi_batch_verify_ex's. */
int kzgmi_batch_find_invalid(kzgmi_ctx* ctx, const kzgmi_srs* srs, const uint8_t* commitments,
                             const uint8_t* zs, const uint8_t* ys, const uint8_t* proofs, size_t n,
                             const uint8_t* seed32, uint32_t flags, uint64_t* bad_out, size_t max_bad,
                             size_t* n_bad_out, int* more_out);
int kzgmi_batch_find_invalid_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_commitments,
                                    const void* d_zs, const void* d_ys, const void* d_proofs, size_t n,
                                    const uint8_t* seed32, uint32_t flags, uint64_t* bad_out,
                                    size_t max_bad, size_t* n_bad_out, int* more_out);
/* EIP-4844 blobs: z_i and y_i = p_i(z_i) by the blob stages, then the search on (C_i, z_i, y_i, pi_i)
 * with KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK semantics and verifier-private randomisers:
 * the indices of the blobs kzgmi_verify_blob_batch rejects the batch for. */
int kzgmi_verify_blob_batch_find_invalid(kzgmi_ctx* ctx, const kzgmi_srs* srs, const uint8_t* blobs,
                                         const uint8_t* commitments48, const uint8_t* proofs48, size_t n,
                                         uint64_t* bad_out, size_t max_bad, size_t* n_bad_out,
                                         int* more_out);
int kzgmi_verify_blob_batch_find_invalid_device(kzgmi_ctx* ctx, const kzgmi_srs* srs, const void* d_blobs,
                                                const void* d_commitments48, const void* d_proofs48,
                                                size_t n, uint64_t* bad_out, size_t max_bad,
                                                size_t* n_bad_out, int* more_out);
/* Of the last search on this context: levels, bucket partial jobs, wave-terms of the grouped kernel,
 * pairings. */
int kzgmi_find_invalid_stats(kzgmi_ctx* ctx, uint64_t out[4]);

/* prover-side commitments with a fixed SRS base.  kzgmi_ck_load uploads
 * n G1 powers ([tau^i]_1, host encodings, validated) and precomputes 16 rows of 2^(16 w)-shifted
 * copies on the device (16 n points resident); kzgmi_commit then computes
 * sum_{i < m} coeff_i [tau^i]_1 (coefficients: m x 32 B canonical Fr, m <= n) as ONE bucket
 * set of 16-bit signed digits -- no per-window reduction, no window combination.  The key
 * must be freed before (or is detached by) kzgmi_ctx_destroy. */
int kzgmi_ck_load(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* g1_powers, size_t n, kzgmi_ck** out);
void kzgmi_ck_free(kzgmi_ck* ck);
int kzgmi_commit(kzgmi_ctx* ctx, const kzgmi_ck* ck, const uint8_t* coeffs, size_t m, uint8_t* out);
int kzgmi_commit_device(kzgmi_ctx* ctx, const kzgmi_ck* ck, const void* d_coeffs, size_t m,
                        uint8_t* out);
/* Pipelined form: enqueue on workspace `slot`; kzgmi_msm_wait(ctx, slot, out) returns the
 * commitment (G1 encoding). */
int kzgmi_commit_device_async(kzgmi_ctx* ctx, const kzgmi_ck* ck, int slot, const void* d_coeffs, size_t m);

/* ---- KZG opening proofs over a commit key -- both curves, coefficient form.
 * For p(X) = sum_{i<m} c_i X^i (m <= the key's n) and k points z_0 .. z_{k-1}:
 *     y_j = p(z_j),   q_j = (p - y_j) / (X - z_j)  (degree m - 2),   proof_j = [q_j(tau)]_1 = sum_{i<m-1} q_j[i] [tau^i]_1
 * With Q_m = 0 and Q_i = c_i + z_j Q_{i+1}: y_j = Q_0 and q_j[i-1] = Q_i, 1 <= i < m -- one suffix
 * scan on the device gives the evaluation and every quotient coefficient; each quotient then takes
 * kzgmi_commit's MSM over the key.
 * coeffs: m x 32 B and zs: k x 32 B big-endian canonical Fr (a value >= r: KZGMI_ERR_SCALAR).
 * ys_out: k x 32 B big-endian.  proofs_out: k uncompressed G1 encodings of the key's curve (96 B / 64 B:
 * kzgmi_commit's output format and kzgmi_batch_verify's default input; the point at infinity as
 * everywhere in this header).  m == 0: y = 0, m == 1: y = c_0, and the proof is the point at infinity
 * in both; k == 0 succeeds and writes nothing.  Points may repeat and may be roots of p (coefficient
 * form has no special case).  m > n, k > 4096, or a key of another context: KZGMI_ERR_ARG.  The key
 * lives on the context's primary device and works with that device's slots only.  Device arrays are
 * 16-byte aligned; outputs overlap neither the inputs nor each other.  The host form stages through
 * slot 0 and copies the results back; the synchronous device form runs on slot 0; the async form runs
 * on any slot and completes with kzgmi_slot_wait (ok_out = 1), which reports the device-side errors.
 * A call that fails writes no output and leaves its slot usable.  Scratch lives in the slot's workspace
 * (grown on first use, counted by kzgmi_alloc_count) and is bounded: the points are taken in groups
 * whose quotients hold at most 2^23 scalars (256 MiB; at least one point per group), so a 2^26-term
 * polynomial opened at 4096 points does not allocate k m 32 B.  (KZGMI_OPEN_GROUP, read at context
 * creation, sets that bound in scalars: tests.) */
int kzgmi_open(kzgmi_ctx* ctx, const kzgmi_ck* ck, const uint8_t* coeffs, size_t m, const uint8_t* zs, size_t k,
               uint8_t* ys_out, uint8_t* proofs_out);
int kzgmi_open_device(kzgmi_ctx* ctx, const kzgmi_ck* ck, const void* d_coeffs, size_t m, const void* d_zs, size_t k,
                      void* d_ys_out, void* d_proofs_out);
int kzgmi_open_device_async(kzgmi_ctx* ctx, const kzgmi_ck* ck, int slot, const void* d_coeffs, size_t m,
                            const void* d_zs, size_t k, void* d_ys_out, void* d_proofs_out);
/* Diagnostic (synchronous, slot 0, no key; m <= 2^26): y_j -> d_ys_out (k x 32 B) and Q_1 .. Q_{m-1} of
 * point j -> d_q_out at byte 32 ((m - 1) j + i - 1) for Q_i, big-endian.  Like kzgmi_blob_quotient_device
 * it writes straight to the caller's arrays, which it does not check for overlap: on an error (a
 * coefficient or z >= r) their contents are unspecified. */
int kzgmi_open_quotient_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_coeffs, size_t m, const void* d_zs,
                               size_t k, void* d_ys_out, void* d_q_out);

/* ---- power-of-two number-theoretic transforms over Fr -- both curves, batched.
 * For a curve with scalar modulus r, w_n = g^((r-1)/n) with g = 7 on BLS12-381 (so w_8192 is the w of
 * the EIP-7594 section) and g = 5 on BN254; both generate the whole 2-power subgroup (2-adicity 32 and
 * 28).  n = 2^logn, 0 <= logn <= 26.  count >= 1 independent transforms of one size: transform t is at
 * byte 32 n t of both arrays, count n <= 2^26; count == 0 succeeds and writes nothing.  Values are
 * 32 B big-endian canonical Fr (a value >= r: KZGMI_ERR_SCALAR).  shift32 is a host pointer in every
 * form (like seed32): NULL means s = 1, s >= r gives KZGMI_ERR_SCALAR, s = 0 KZGMI_ERR_ARG.
 *   flags = 0 (forward):  out[j] = sum_{i<n} in[i] (s w_n^j)^i -- the polynomial with coefficients `in`
 *                         evaluated on the coset s <w_n>
 *   KZGMI_NTT_INVERSE:    the inverse map: from v[j] = p(s w_n^j) the n coefficients
 *                         out[i] = s^-i n^-1 sum_j v[j] w_n^(-i j)
 *   KZGMI_NTT_BITREV:     the evaluation side (a forward transform's output, an inverse one's input) is
 *                         in bit-reversed order: index k holds the point s w_n^rev_logn(k), the blob and
 *                         cell order of the EIP sections.  The coefficient side is always in natural order.
 * Any other flag bit, logn > 26 or count n > 2^26: KZGMI_ERR_ARG.  logn = 0 is the identity after the
 * range check.  The host form stages through slot 0 and copies the result back; the synchronous device
 * form runs on slot 0; the async form runs on any slot and completes with kzgmi_slot_wait (ok_out = 1),
 * which reports the device-side errors.  Device arrays are 16-byte aligned; d_out == d_in (in place) is
 * allowed, any other overlap is KZGMI_ERR_ARG.  The range check belongs to the first pass over the data
 * and there is no separate copy of the result: on an error the contents of `out` -- and of `in`, if the
 * call was in place -- are unspecified (as kzgmi_recover_cells); the slot stays usable.  Scratch: per
 * slot at most one more copy of the data (32 count n B; none up to 2^8 points), in the slot's workspace,
 * grown on first use and counted by kzgmi_alloc_count, as are each curve's root tables (544 KiB, built
 * at the curve's first transform) and the slot's shift table (512 KiB): a repeat call of the same shape
 * allocates nothing.  (Read at context creation: KZGMI_NTT_PASS_BITS = 2 .. 8 bounds the bits of one
 * pass over the data -- tests; KZGMI_NTT_TILE_BITS = 10 .. 12 selects a workgroup's tile of 2^10
 * (shipped), 2^11 or 2^12 elements, with passes of at most that less two bits -- measurements.) */
#define KZGMI_NTT_INVERSE 1u
#define KZGMI_NTT_BITREV 2u
int kzgmi_fr_ntt(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* in, unsigned logn, size_t count, uint32_t flags,
                 const uint8_t* shift32, uint8_t* out);
int kzgmi_fr_ntt_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_in, unsigned logn, size_t count, uint32_t flags,
                        const uint8_t* shift32, void* d_out);
int kzgmi_fr_ntt_device_async(kzgmi_ctx* ctx, kzgmi_curve curve, int slot, const void* d_in, unsigned logn, size_t count,
                              uint32_t flags, const uint8_t* shift32, void* d_out);

/* ---- KZG openings of a polynomial given by its evaluations: kzgmi_open on the polynomial whose
 * n = 2^logn values on <w_n> of the key's curve are `evals` (n x 32 B, natural order, or bit-reversed
 * with flags = KZGMI_NTT_BITREV -- no other flag; n <= the key's n).  One job: the inverse transform
 * into a slot buffer, then the opening in coefficient form with m = n, with no host round trip.
 * Outputs, the bound of k <= 4096 points, the conventions of the three forms and the scratch are those
 * of kzgmi_open (plus the transform's); a point of the domain is no special case, its y is the given
 * evaluation.  A value >= r in evals or zs: KZGMI_ERR_SCALAR; a call that fails writes no output. */
int kzgmi_open_evals(kzgmi_ctx* ctx, const kzgmi_ck* ck, const uint8_t* evals, unsigned logn, uint32_t flags,
                     const uint8_t* zs, size_t k, uint8_t* ys_out, uint8_t* proofs_out);
int kzgmi_open_evals_device(kzgmi_ctx* ctx, const kzgmi_ck* ck, const void* d_evals, unsigned logn, uint32_t flags,
                            const void* d_zs, size_t k, void* d_ys_out, void* d_proofs_out);
int kzgmi_open_evals_device_async(kzgmi_ctx* ctx, const kzgmi_ck* ck, int slot, const void* d_evals, unsigned logn,
                                  uint32_t flags, const void* d_zs, size_t k, void* d_ys_out, void* d_proofs_out);

/* ---- power-of-two transforms over G1 -- both curves, batched.  n = 2^logn and w_n exactly
 * as in the kzgmi_fr_ntt section; [k] P is the scalar multiple.  count independent transforms of one size,
 * transform t at byte (96 | 64) n t of both arrays.
 *   flags = 0 (forward):  out[j] = sum_{i<n} [w_n^(i j)] in[i]
 *   KZGMI_NTT_INVERSE:    out[i] = [n^-1] sum_{j<n} [w_n^(-i j)] in[j]
 *   KZGMI_NTT_BITREV:     the evaluation side (a forward transform's output, an inverse one's input) is in
 *                         bit-reversed order, with the same meaning as for kzgmi_fr_ntt
 * 0 <= logn <= 20 and count n <= 2^20; count == 0 succeeds and writes nothing.  Any other flag bit or a
 * bound passed: KZGMI_ERR_ARG.  Points are uncompressed encodings of the curve (96 B / 64 B) in and out,
 * infinity as everywhere in this header.  Inputs are validated as kzgmi_g1_fft128_device validates them:
 * KZGMI_ERR_ENCODING for a bad encoding, KZGMI_ERR_NOT_ON_CURVE for a point off the curve.  There is no
 * subgroup check, and the roots of unity act as integers below r: for on-curve inputs outside G1 the
 * result is unspecified (as the GLV split under KZGMI_FLAG_TRUSTED_G1).  The three forms follow the
 * header's conventions: the host form stages through slot 0; the synchronous device form runs on slot 0;
 * the async form runs on any slot and completes with kzgmi_slot_wait (ok_out = 1), which reports the
 * device-side errors.  Device arrays are 16-byte aligned; d_out == d_in (in place) is allowed, any other
 * overlap is KZGMI_ERR_ARG.  The output is written by one last kernel that writes nothing once an error
 * is raised: a failing call leaves `out` untouched and the slot usable.  Scratch, in the slot's workspace,
 * grown on first use and counted by kzgmi_alloc_count (a repeat call of the same shape allocates nothing):
 * the decoded points, two vectors of count n XYZZ records (192 B / 128 B each) and the encodings; and each
 * curve's root tables of the kzgmi_fr_ntt section.  On BLS12-381 at logn = 7 the result equals
 * kzgmi_g1_fft128_device's.  (Read at context creation: KZGMI_G1NTT_FORM = thread | wave forces one form of
 * the radix-2 stages -- a thread or a wave per butterfly; unset, a call whose stages have at most 2^14
 * butterflies takes the wave form.  The results are identical -- tests, measurements.) */
int kzgmi_g1_ntt(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* in, unsigned logn, size_t count, uint32_t flags,
                 uint8_t* out);
int kzgmi_g1_ntt_device(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_in, unsigned logn, size_t count, uint32_t flags,
                        void* d_out);
int kzgmi_g1_ntt_device_async(kzgmi_ctx* ctx, kzgmi_curve curve, int slot, const void* d_in, unsigned logn, size_t count,
                              uint32_t flags, void* d_out);

/* ---- KZG openings at every point of a domain (FK20).  For p = sum_{i<m} c_i X^i with
 * m <= n = 2^logn (read as zero above m) and every e < n:
 *   ys[e] = p(w_n^e),   proofs[e] = [((p - ys[e]) / (X - w_n^e))(tau)]_1
 * -- entry e is exactly what kzgmi_open returns for z = w_n^e, byte for byte: n uncompressed G1 encodings
 * and n x 32 B big-endian evaluations.  flags = KZGMI_NTT_BITREV puts entry e at index rev_logn(e) of both
 * outputs; no other flag is accepted.  ys_out may be NULL (proofs only).  At logn = 0 the proof is the
 * point at infinity and y = c_0.
 * The key (kzgmi_open_all_key_load) belongs to one commit key's curve and one logn, 0 <= logn <= 19, and
 * needs n - 1 <= the commit key's n.  It is derived on the device from the commit key's resident row of
 * powers (no second upload of the SRS), lives on the context's primary device like the other keys and
 * holds 2n XYZZ records (192 MiB on BLS12-381 at logn = 19: kzgmi_open_all_key_device_bytes); the commit
 * key may be freed afterwards.  Loading runs on slot 0, which must be idle.  An SRS with tau in the
 * domain makes entries of the key infinite; the results are still kzgmi_open's.
 * Errors: KZGMI_ERR_SCALAR for a coefficient >= r; KZGMI_ERR_ARG for m > n, a key of another context,
 * logn out of range, a key needing more powers than the commit key has, a stray flag, misaligned or
 * overlapping device arrays.  The three forms, the alignment rule and the completion of the async form are
 * those of kzgmi_open; outputs overlap neither the input nor each other; a failing call writes no output
 * and leaves the slot usable.  Scratch in the slot's workspace as for kzgmi_g1_ntt with 2n records, plus
 * 5n scalars (the coefficients, their 2n-point transform, a padded copy, the evaluations) and the
 * kzgmi_fr_ntt scratch of a 2n-point transform. */
typedef struct kzgmi_open_all_key kzgmi_open_all_key;
int kzgmi_open_all_key_load(kzgmi_ctx* ctx, const kzgmi_ck* ck, unsigned logn, kzgmi_open_all_key** out);
void kzgmi_open_all_key_free(kzgmi_open_all_key* key);
size_t kzgmi_open_all_key_device_bytes(const kzgmi_open_all_key* key);
int kzgmi_open_all(kzgmi_ctx* ctx, const kzgmi_open_all_key* key, const uint8_t* coeffs, size_t m, uint32_t flags,
                   uint8_t* ys_out, uint8_t* proofs_out);
int kzgmi_open_all_device(kzgmi_ctx* ctx, const kzgmi_open_all_key* key, const void* d_coeffs, size_t m, uint32_t flags,
                          void* d_ys_out, void* d_proofs_out);
int kzgmi_open_all_device_async(kzgmi_ctx* ctx, const kzgmi_open_all_key* key, int slot, const void* d_coeffs, size_t m,
                                uint32_t flags, void* d_ys_out, void* d_proofs_out);

/* ---- KZG openings on every coset of a domain (FK20 multi-proofs) -- both curves, any
 * power-of-two shape.  N = 2^logN is the coefficient capacity, l = 2^logl the coset size, K = 2^logk the
 * number of cosets, n = K l, R = N / l; w_n is the root of the kzgmi_fr_ntt section.  For
 * p = sum_{i<m} c_i X^i with m <= N (read as zero above m) and every coset e < K:
 *   h_e = w_n^e,  z_e = h_e^l,  coset e = { h_e w_l^j : j < l },  w_l = w_n^K
 *   ys[e][j] = p(w_n^(e + K j)),   proofs[e] = [q_e(tau)]_1,  q_e = floor(p / (X^l - z_e))
 * -- the proof that p agrees on coset e with I_e = p mod (X^l - z_e), checked by
 * e(proof_e, [tau^l - z_e]_2) = e(C - [I_e(tau)]_1, [1]_2).  With l = 1 the results are kzgmi_open_all's,
 * with l = N every proof is the point at infinity.  The outputs are coset-major: count x K uncompressed G1
 * encodings and count x K l x 32 B big-endian evaluations, polynomial t's coset e at entry t K + e and its
 * evaluation j at value (t K + e) l + j.  flags = KZGMI_NTT_BITREV puts coset rev_logk(i) at proof index i
 * and p(w_n^rev(k)), rev over logk + logl bits, at value k of a polynomial -- on BLS12-381 at
 * (logN, logl, logk) = (12, 6, 7) exactly the cell and proof order of EIP-7594.  No other flag is accepted.
 * ys_out may be NULL (proofs only).  Polynomial t of the count is at byte 32 m t of coeffs.
 * The key (kzgmi_open_cosets_key_load) belongs to one commit key's curve and one (logN, logl),
 * logl <= logN <= 19, whatever logk a call takes, and needs N - l <= the commit key's n (the highest power
 * read is tau^(N - l - 1)).  It is derived on the device from the commit key's resident row of powers, lives
 * on the context's primary device and holds 2N XYZZ records (kzgmi_open_cosets_key_device_bytes: 1.5 MiB at
 * the EIP-7594 shape); the commit key may be freed afterwards.  Loading runs on slot 0, which must be idle.
 * Bounds of a call: logk >= logN - logl, count N <= 2^19, count K l <= 2^20; count == 0 succeeds and writes
 * nothing.  Errors: KZGMI_ERR_SCALAR for a coefficient >= r; KZGMI_ERR_ARG for a bound, a stray flag, a key
 * of another context, misaligned or overlapping device arrays.  The three forms, the alignment rule, the
 * completion of the async form and the workspace accounting are those of kzgmi_open_all: a failing call
 * writes no output and leaves the slot usable.  KZGMI_G1NTT_FORM=thread|wave forces the form of the
 * products as it does the stages'. */
typedef struct kzgmi_open_cosets_key kzgmi_open_cosets_key;
int kzgmi_open_cosets_key_load(kzgmi_ctx* ctx, const kzgmi_ck* ck, unsigned logN, unsigned logl,
                               kzgmi_open_cosets_key** out);
void kzgmi_open_cosets_key_free(kzgmi_open_cosets_key* key);
size_t kzgmi_open_cosets_key_device_bytes(const kzgmi_open_cosets_key* key);
int kzgmi_open_cosets(kzgmi_ctx* ctx, const kzgmi_open_cosets_key* key, const uint8_t* coeffs, size_t m, size_t count,
                      unsigned logk, uint32_t flags, uint8_t* ys_out, uint8_t* proofs_out);
int kzgmi_open_cosets_device(kzgmi_ctx* ctx, const kzgmi_open_cosets_key* key, const void* d_coeffs, size_t m, size_t count,
                             unsigned logk, uint32_t flags, void* d_ys_out, void* d_proofs_out);
int kzgmi_open_cosets_device_async(kzgmi_ctx* ctx, const kzgmi_open_cosets_key* key, int slot, const void* d_coeffs,
                                   size_t m, size_t count, unsigned logk, uint32_t flags, void* d_ys_out,
                                   void* d_proofs_out);

/* Optimal-ate pairing e(P, Q) for P in G1, Q in G2: 12 Fp values in tower order, big-endian:
 * 576 B (BLS12-381) / 384 B (BN254).  Test/diagnostic utility.  (ABI 2 returned e(P, Q)^3 on
 * BLS12-381, the value the batch check's final exponentiation computes; ABI 3 scales P by
 * 3^-1 mod r first, so the result is the standard e(P, Q) -- for P outside G1 it is not.) */
int kzgmi_pairing(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* g1, const uint8_t* g2,
                  uint8_t* out);
/* (The 3^-1 scaling runs the library's MSM on one point with the GLV split forced off, so the
 * result does not depend on kzgmi_set_trusted_g1 / kzgmi_set_glv.) */

/* ---- synthetic-input generators (device side; used by bench.py and GPU tests) ---------
 * d_points_out[i] = k_i * G1 for device scalars k_i (32 B BE each). */
int kzgmi_gen_g1(kzgmi_ctx* ctx, kzgmi_curve curve, const void* d_scalars, size_t n,
                 void* d_points_out);
/* n valid opening tuples under a toy tau (32 B BE, < r): c_i, z_i, y_i = 253-bit values
 * int_be(SHA256(seed || le64(i) || tag)) & (2^253 - 1), tag = 'c','z','y';
 * q_i = (c_i - y_i)/(tau - z_i); C_i = c_i G1, pi_i = q_i G1.  Device outputs. */
int kzgmi_gen_tuples(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* tau32, const uint8_t* seed32,
                     size_t n, void* d_commitments, void* d_zs, void* d_ys, void* d_proofs);

/* [k]Q for a G2 point Q (host encodings; k = 32 B BE, < r): toy-SRS generation
 * ([tau]_2 from a known tau, SURVEY.md 2 "test-only toy-tau generator"). */
int kzgmi_g2_mul(kzgmi_ctx* ctx, kzgmi_curve curve, const uint8_t* g2, const uint8_t* k32, uint8_t* out);

/* Compute-roofline probe: Montgomery Fp multiplications per second on this GPU (many
 * independent products per thread, whole chip), written to *muls_per_s. */
int kzgmi_probe_fpmul(kzgmi_ctx* ctx, kzgmi_curve curve, double* muls_per_s);

/* GLV endomorphism phi(x, y) = (beta x, y) = [lambda] P.  Full Fr
 * scalars k are split as k = k0 + k1 lambda (|k0|, |k1| < 2^127) so each MSM runs 8 windows
 * over P and phi(P) instead of 16 over P: the same bucket additions, half the bucket sets to
 * reduce and half the window-combination doublings.  phi acts as [lambda] only on G1, so the
 * split is used where the points are G1 members: always on BN254 (cofactor 1); on BLS12-381
 * for batch calls with KZGMI_FLAG_SUBGROUP_CHECK or KZGMI_FLAG_TRUSTED_G1 and for MSMs after
 * kzgmi_set_trusted_g1(ctx, 1).  On G1 the results are identical either way.
 * kzgmi_set_glv switches the split off/on (msm: kzgmi_msm_g1*, batch: s_i, t and r^i of batch
 * verification; default both on) for A/B measurements.  Not allowed while jobs are in flight. */
int kzgmi_set_glv(kzgmi_ctx* ctx, int msm, int batch);
/* Declare that every point passed to kzgmi_msm_g1* on this context is in G1 (default 0). */
int kzgmi_set_trusted_g1(kzgmi_ctx* ctx, int on);
/* Split accumulation of a batch's two MSMs (latency): MSM#0's bucket sets accumulate in a first
 * launch and its reduction + window combination run on a side stream beside MSM#1's launch
 * (KZGMI_SPLIT_REV=0 in the environment at context creation: MSM#1's sets first instead).
 * mode -1 (default): synchronous kzgmi_batch_verify_device calls of >= 2^25 window entries whose
 * second MSM has more windows (no GLV) with no other slot in flight (async calls never split:
 * the first batch of a pipeline is alone too); 0: never;
 * 1: every two-MSM call.
 * Results are identical either way.  Not allowed while jobs are in flight. */
int kzgmi_set_split_acc(kzgmi_ctx* ctx, int mode);

/* ---- profiling -----------------------------------------------------------------------
 * When enabled, every batch / MSM call records HIP events around each phase on the stream
 * its kernels run on; kzgmi_get_phase_ms() returns the per-phase device time (ms) averaged
 * over all calls completed since profiling was (re)enabled, in the order of
 * kzgmi_phase_names() (comma-separated).  Enabling resets the averages.  On a multi-device
 * context the switch applies to every device and the times are the primary device's. */
int kzgmi_set_profiling(kzgmi_ctx* ctx, int on);
const char* kzgmi_phase_names(void);
int kzgmi_get_phase_ms(kzgmi_ctx* ctx, double* out, int max_n);

#ifdef __cplusplus
}
#endif
#endif /* KZGMI_H */
