// EIP-4844 blob front end of batch verification (Deneb polynomial-commitments,
// verify_blob_kzg_proof_batch): per-blob challenge, barycentric evaluation, batch challenge.
// BLS12-381 only, domain size 4096.  Reference: none (LICENSE only); the transcript is restated
// byte by byte in tests/blobref.py.
//
//   z_i = int_be(SHA256("FSBLOBVERIFY_V1_" || be128(4096) || blob_i || C_i)) mod r
//   dom[i] = w^rev12(i), w = 7^((r-1)/4096)
//   y_i = blob_i[j] if z_i = dom[j], else (z_i^4096 - 1)/4096 * sum_j blob_i[j] dom[j] / (z_i - dom[j])
//   r = int_be(SHA256("RCKZGBATCH___V1_" || be64(4096) || be64(n) || (C_i || z_i || y_i || pi_i)_i)) mod r
//
// The blob hash is 2050 strictly sequential compressions, so only blobs are parallel:
// k_blob_challenge<false> gives every blob a lane, k_blob_challenge<true> a whole wave whose
// values are all wave-uniform.  The lane form is the shipped one: 6.0 ms at every n <= 4096
// against 10.4 ms (n <= 64) to 36 ms (n = 4096) for the wave form, which stays for the A/B of
// tools/bench_blobs.py (KZGMI_BLOB_HASH=wave; DESIGN.md has the table).
#pragma once
#include "kernels.hpp"

namespace kzgmi {

using BlobR = Bls12_381FrParams;
using BlobF = Fp<BlobR>;
constexpr uint32_t BLOB_N = 4096;               // field elements per blob
constexpr uint32_t BLOB_BYTES = 32 * BLOB_N;    // 128 KiB
constexpr uint32_t BLOB_TABLE = BLOB_N + 1;     // dom[0 .. 4096) then 4096^-1, Montgomery
constexpr int BLOB_EVAL_THREADS = 512;          // k_blob_eval: thread t owns elements t + 512 k, k < 8
constexpr int BLOB_EVAL_PER = BLOB_N / BLOB_EVAL_THREADS;

// "FSBLOBVERIFY_V1_" / "RCKZGBATCH___V1_" as big-endian words
__constant__ static const uint32_t kBlobTag[4] = {0x4653424cu, 0x4f425645u, 0x52494659u, 0x5f56315fu};
__constant__ static const uint32_t kBlobBatchTag[4] = {0x52434b5au, 0x47424154u, 0x43485f5fu, 0x5f56315fu};

// dom[i] = w^rev12(i) and 4096^-1: 4096 threads, once per context
static __global__ void __launch_bounds__(256) k_blob_domain(BlobF* __restrict__ table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BLOB_N) return;
  const uint32_t e = __brev(i) >> 20;
  BlobF x = BlobF::from_const(BlobR::ROOT4096_M), acc = BlobF::one();
  for (int k = 0; k < 12; ++k) {
    if ((e >> k) & 1) acc = fp_mul(acc, x);
    x = fp_sqr(x);
  }
  table[i] = acc;
  if (i == 0) {
    BlobF nn = BlobF::zero();
    nn.v[0] = BLOB_N;
    table[BLOB_N] = fp_inv_c(fp_to_mont(nn));
  }
}

// ---------------------------------------------------------------------------- blob challenge
// SHA-256 compression in plain integer operations (no v_bitop3, rotations as 64-bit shifts of
// the doubled word) for wave-uniform values: hipcc keeps the whole round function in scalar
// registers (s_lshr_b64 / s_xor_b32 / s_add_i32; ~2500 scalar instructions per compression
// against ~1660 vector ones for sha256_compress, which has v_alignbit and v_bitop3).
KZ_DEV uint32_t blob_ror(uint32_t x, int n) { return (uint32_t)((((uint64_t)x << 32) | x) >> n); }

KZ_DEV void blob_compress_uniform(const uint32_t (&blk)[16], uint32_t (&h)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = blk[i];
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
  uint32_t e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      const uint32_t s0 = blob_ror(w15, 7) ^ blob_ror(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = blob_ror(w2, 17) ^ blob_ror(w2, 19) ^ (w2 >> 10);
      wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
      w[i & 15] = wi;
    }
    const uint32_t S1 = blob_ror(e, 6) ^ blob_ror(e, 11) ^ blob_ror(e, 25);
    const uint32_t ch = g ^ (e & (f ^ g));
    const uint32_t t1 = hh + S1 + ch + kSha256K[i] + wi;
    const uint32_t S0 = blob_ror(a, 2) ^ blob_ror(a, 13) ^ blob_ror(a, 22);
    const uint32_t mj = (a & b) | (c & (a | b));
    const uint32_t t2 = S0 + mj;
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

template <bool WAVE>
KZ_DEV void blob_compress(const uint32_t (&blk)[16], uint32_t (&h)[8]) {
  if constexpr (WAVE) blob_compress_uniform(blk, h);
  else sha256_compress(blk, h);
}

// 8 big-endian words (most significant first) of a blob element: value < r ?
KZ_DEV bool blob_elem_ok(const uint32_t* be) {
  uint32_t bw = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) (void)__builtin_subc(be[7 - k], BlobR::MOD[k], bw, &bw);
  return bw != 0;
}

// int_be(h) mod r for a 256-bit h (< 3r)
KZ_DEV BlobF blob_hash_to_fr(const uint32_t (&h)[8]) {
  BlobF r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = h[7 - k];
  for (int t = 0; t < 3 && !fp_raw_lt_mod(r); ++t) {
    uint32_t bw = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = __builtin_subc(r.v[k], BlobR::MOD[k], bw, &bw);
  }
  return r;
}

// 16 message words starting at 32-bit word `w0` of src (w0 a multiple of 4), byte-swapped
KZ_DEV void blob_load16(const uint32_t* __restrict__ src, uint32_t w0, uint32_t (&m)[16]) {
  const uint4* s = reinterpret_cast<const uint4*>(src + w0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 q = s[k];
    m[4 * k] = __builtin_bswap32(q.x); m[4 * k + 1] = __builtin_bswap32(q.y);
    m[4 * k + 2] = __builtin_bswap32(q.z); m[4 * k + 3] = __builtin_bswap32(q.w);
  }
}

// z_i of blob i.  Message blocks (64 B): block 0 = tag || be128(4096) || element 0; block b,
// 1 <= b <= 2047, = elements 2b - 1, 2b; block 2048 = element 4095 || C[0:32); block 2049 =
// C[32:48) || padding.  Every element is range-checked here, once (DERR_SCALAR).
// WAVE = false: blob i on lane i (64-thread blocks); true: blob i on block i's single wave,
// every value uniform, lane 0 stores.  blobs and commitments 16-byte aligned.
template <bool WAVE>
__global__ void __launch_bounds__(64) k_blob_challenge(const uint8_t* __restrict__ blobs,
                                                       const uint8_t* __restrict__ commitments, uint32_t n,
                                                       uint8_t* __restrict__ zs, uint32_t* __restrict__ err) {
  const uint32_t i = WAVE ? blockIdx.x : blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(blobs + (size_t)i * BLOB_BYTES);
  const uint32_t* cw = reinterpret_cast<const uint32_t*>(commitments + (size_t)i * 48);
  uint32_t h[8], m[16], nx[16];
  sha256_init(h);
  blob_load16(bw, 0, nx);  // elements 0, 1
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = kBlobTag[k];
  m[4] = 0; m[5] = 0; m[6] = 0; m[7] = BLOB_N;
#pragma unroll
  for (int k = 0; k < 8; ++k) m[8 + k] = nx[k];
  bool ok = blob_elem_ok(&m[8]);
  blob_compress<WAVE>(m, h);
  blob_load16(bw, 8, nx);
  for (uint32_t b = 1; b < BLOB_N / 2; ++b) {
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = nx[k];
    // the next block's words are in flight while this one is compressed (the last pass
    // re-reads its own block)
    blob_load16(bw, 16 * (b + 1 < BLOB_N / 2 ? b + 1 : b) - 8, nx);
    ok = ok && blob_elem_ok(&m[0]) && blob_elem_ok(&m[8]);
    blob_compress<WAVE>(m, h);
  }
  uint32_t c[12];
  {
    const uint4* s = reinterpret_cast<const uint4*>(cw);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint4 q = s[k];
      c[4 * k] = __builtin_bswap32(q.x); c[4 * k + 1] = __builtin_bswap32(q.y);
      c[4 * k + 2] = __builtin_bswap32(q.z); c[4 * k + 3] = __builtin_bswap32(q.w);
    }
  }
  {
    const uint4* s = reinterpret_cast<const uint4*>(bw + 8 * (BLOB_N - 1));
    const uint4 q0 = s[0], q1 = s[1];
    m[0] = __builtin_bswap32(q0.x); m[1] = __builtin_bswap32(q0.y); m[2] = __builtin_bswap32(q0.z);
    m[3] = __builtin_bswap32(q0.w); m[4] = __builtin_bswap32(q1.x); m[5] = __builtin_bswap32(q1.y);
    m[6] = __builtin_bswap32(q1.z); m[7] = __builtin_bswap32(q1.w);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) m[8 + k] = c[k];
  ok = ok && blob_elem_ok(&m[0]);
  blob_compress<WAVE>(m, h);
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = c[8 + k];
  m[4] = 0x80000000u;
#pragma unroll
  for (int k = 5; k < 15; ++k) m[k] = 0;
  m[15] = (32 + BLOB_BYTES + 48) * 8;  // message bits
  blob_compress<WAVE>(m, h);
  if (WAVE && threadIdx.x != 0) return;
  if (!ok) raise_err(err, DERR_SCALAR);
  const BlobF z = blob_hash_to_fr(h);
  uint32_t w[8];
  fp_to_be_words(z, w, 0);
  store_words(zs + (size_t)i * 32, w);
}

// ---------------------------------------------------------------------------- evaluation
// y = p(z) for the blob polynomial in evaluation form over dom: one workgroup per blob.  Thread
// t owns elements t + 512 k: the differences z - dom[j] are inverted by Montgomery's trick (one
// fp_inv_c per thread), the terms summed by an LDS tree, and thread 0 applies (z^4096 - 1)/4096.
// z = dom[j] (a zero difference, which would zero the running product) is detected and answers
// blob[j].  range_check: the elements are checked here (DERR_SCALAR) -- the stand-alone
// evaluation; the batch path checked them in k_blob_challenge.
static __global__ void __launch_bounds__(BLOB_EVAL_THREADS) k_blob_eval(const uint8_t* __restrict__ blobs,
                                                                        const uint8_t* __restrict__ zs,
                                                                        const BlobF* __restrict__ table, int range_check,
                                                                        uint8_t* __restrict__ ys,
                                                                        uint32_t* __restrict__ err) {
  __shared__ BlobF red[BLOB_EVAL_THREADS];
  __shared__ uint32_t hit;
  const uint32_t t = threadIdx.x;
  const uint8_t* blob = blobs + (size_t)blockIdx.x * BLOB_BYTES;
  if (t == 0) hit = 0;
  uint32_t wz[8];
  load_words(zs + (size_t)blockIdx.x * 32, wz);
  BlobF zr = fp_from_be_words<BlobR>(wz, 0);
  if (!fp_raw_lt_mod(zr)) {
    if (t == 0) raise_err(err, DERR_SCALAR);
    zr = BlobF::zero();
  }
  const BlobF z = fp_to_mont(zr);
  __syncthreads();
  BlobF pre[BLOB_EVAL_PER];
  BlobF acc = BlobF::one();
#pragma unroll
  for (int k = 0; k < BLOB_EVAL_PER; ++k) {
    const uint32_t j = t + BLOB_EVAL_THREADS * k;
    BlobF d = fp_sub(z, table[j]);
    if (d.is_zero()) {
      hit = j + 1;  // at most one j: the domain points are distinct
      d = BlobF::one();
    }
    pre[k] = acc;
    acc = fp_mul(acc, d);
  }
  BlobF inv = fp_inv_c(acc);
  BlobF sum = BlobF::zero();
#pragma unroll
  for (int k = BLOB_EVAL_PER - 1; k >= 0; --k) {
    const uint32_t j = t + BLOB_EVAL_THREADS * k;
    const BlobF w = table[j];
    BlobF d = fp_sub(z, w);
    if (d.is_zero()) d = BlobF::one();
    const BlobF dinv = fp_mul(inv, pre[k]);
    inv = fp_mul(inv, d);
    uint32_t we[8];
    load_words(blob + (size_t)j * 32, we);
    BlobF e = fp_from_be_words<BlobR>(we, 0);  // standard form
    if (range_check && !fp_raw_lt_mod(e)) {
      raise_err(err, DERR_SCALAR);
      e = BlobF::zero();
    }
    // standard-form e times two Montgomery factors stays in standard form
    sum = fp_add(sum, fp_mul(fp_mul(e, w), dinv));
  }
  red[t] = sum;
  __syncthreads();
  for (int st = BLOB_EVAL_THREADS / 2; st >= 1; st >>= 1) {
    if ((int)t < st) red[t] = fp_add(red[t], red[t + st]);
    __syncthreads();
  }
  if (t != 0) return;
  uint32_t wy[8];
  if (hit) {
    load_words(blob + (size_t)(hit - 1) * 32, wy);
  } else {
    BlobF zn = z;
    for (int k = 0; k < 12; ++k) zn = fp_sqr(zn);
    const BlobF fac = fp_mul(fp_sub(zn, BlobF::one()), table[BLOB_N]);
    fp_to_be_words(fp_mul(red[0], fac), wy, 0);
  }
  store_words(ys + (size_t)blockIdx.x * 32, wy);
}

// ---------------------------------------------------------------------------- batch challenge
// r of the whole batch: one sequential SHA-256 over 32 + 160 n bytes on one wave.  Lanes 0-15
// fetch the next block's words while the current one is compressed (by every lane alike).
// Writes r (8 big-endian words) and the power table r^(2^k) exactly as k_fs_challenge does --
// but r = 0 stays 0 (powers 1, 0, 0, ...: the specification's literal reading).
static __global__ void __launch_bounds__(64) k_blob_batch_challenge(const uint8_t* __restrict__ commitments,
                                                                    const uint8_t* __restrict__ zs,
                                                                    const uint8_t* __restrict__ ys,
                                                                    const uint8_t* __restrict__ proofs, uint32_t n,
                                                                    BlobF* __restrict__ pow,
                                                                    uint32_t* __restrict__ chal_out) {
  const uint32_t lane = threadIdx.x;
  const uint32_t* cw = reinterpret_cast<const uint32_t*>(commitments);
  const uint32_t* zw = reinterpret_cast<const uint32_t*>(zs);
  const uint32_t* yw = reinterpret_cast<const uint32_t*>(ys);
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(proofs);
  const uint64_t nwords = 8 + 40 * (uint64_t)n;           // message words
  const uint64_t nblocks = (4 * nwords + 9 + 63) / 64;    // padded blocks
  const uint64_t bits = 32 * nwords;
  // big-endian word w of the padded message
  auto word = [&](uint64_t w) -> uint32_t {
    if (w < 4) return kBlobBatchTag[w];
    if (w < 8) return w == 5 ? BLOB_N : w == 7 ? n : 0u;
    if (w < nwords) {
      const uint32_t q = (uint32_t)((w - 8) / 40), o = (uint32_t)((w - 8) % 40);
      const uint32_t v = o < 12 ? cw[12 * (size_t)q + o]
                       : o < 20 ? zw[8 * (size_t)q + (o - 12)]
                       : o < 28 ? yw[8 * (size_t)q + (o - 20)]
                                : pw[12 * (size_t)q + (o - 28)];
      return __builtin_bswap32(v);
    }
    if (w == nwords) return 0x80000000u;
    if (w == 16 * nblocks - 2) return (uint32_t)(bits >> 32);
    if (w == 16 * nblocks - 1) return (uint32_t)bits;
    return 0u;
  };
  uint32_t h[8];
  sha256_init(h);
  uint32_t nxt = lane < 16 ? word(lane) : 0u;
  for (uint64_t b = 0; b < nblocks; ++b) {
    const uint32_t cur = nxt;
    if (b + 1 < nblocks && lane < 16) nxt = word(16 * (b + 1) + lane);
    // every lane keeps its own copy of the block and the state in vector registers: the
    // compression measured 2.9 us there against 5.1 us on wave-uniform scalar values
    uint32_t blk[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) blk[k] = (uint32_t)__shfl((int)cur, k);
    sha256_compress(blk, h);
  }
  if (lane != 0) return;
  const BlobF r = blob_hash_to_fr(h);
#pragma unroll
  for (int k = 0; k < 8; ++k) chal_out[k] = r.v[7 - k];
  BlobF x = fp_to_mont(r);
  for (int k = 0; k < FS_POW_BITS; ++k) {
    pow[k] = x;
    x = fp_sqr(x);
  }
}

}  // namespace kzgmi
