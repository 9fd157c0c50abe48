// What a power-of-two transform over Fr (ntt.hpp, host_ntt.hip) decides on the host, as plain data:
// the passes over HBM of one call, each with its bits, element stride, twiddle step and the work
// folded into its load or store.  Nothing here allocates, launches or reads the environment.
// tests/native/ntt_plan_probe.hip exposes it to a test that needs no GPU; tests/nttref.py
// (transform_planned) runs a plan the way the kernels do.  DESIGN.md 3h.
//
// n = 2^logn is taken as a P-digit number, i = a_0 M_0 + a_1 M_1 + ... + a_{P-1}, digit p of
// 2^bits_p values with the stride M_p = n / (R_0 .. R_p), most significant first.  Pass p transforms
// digit p in place of it -- the 2^bits_p elements M_p apart, for every value of the other digits --
// after multiplying element a_p by w_{R_0 .. R_p}^(a_p kappa), kappa = k_0 + k_1 R_0 + ... the output
// digits already made.  A sub-transform leaves its outputs in bit-reversed order in its digit (a
// decimation-in-frequency network), so the digits above pass p's, read as one number h, hold
// kappa = bitrev(h) and no pass needs a digit loop.  The last pass writes X[kappa + k_{P-1} n / R_{P-1}]
// in natural or bit-reversed order: the only pass that does not write where it read.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kzgmi {

constexpr uint32_t NTT_MAX_LOGN = 26;          // n and count * n are at most 2^26
constexpr uint32_t NTT_ROOT_BITS = 26;         // the two-level twiddle table holds w_{2^26}^i
constexpr uint32_t NTT_TABLE_BITS = 13;        // ... as w^lo and w^(hi 2^13), lo, hi < 2^13
// elements of one workgroup's tile in LDS: 2^10 (32 KiB, five workgroups per CU) is shipped; 2^11 and
// 2^12 are built too (KZGMI_NTT_TILE_BITS) and measured beside it: DESIGN.md 3h
constexpr uint32_t NTT_TILE_BITS = 10;
constexpr uint32_t NTT_MIN_TILE_BITS = 10, NTT_MAX_TILE_BITS = 12;
constexpr uint32_t NTT_MIN_COLS_BITS = 2;      // a tile takes at least 4 adjacent columns: 128 B runs
constexpr uint32_t NTT_MAX_BITS = NTT_TILE_BITS - NTT_MIN_COLS_BITS;  // B: the shipped most bits of a pass (8)
constexpr uint32_t NTT_WIDEST_BITS = NTT_MAX_TILE_BITS - NTT_MIN_COLS_BITS;  // ... of the largest built tile (10)
constexpr uint32_t NTT_MIN_PASS_BITS = 2;      // the least value of the test-only bound KZGMI_NTT_PASS_BITS
constexpr uint32_t NTT_MAX_PASSES = (NTT_MAX_LOGN + NTT_MIN_PASS_BITS - 1) / NTT_MIN_PASS_BITS;

// the caller's flags (include/kzgmi.h)
constexpr uint32_t NTT_F_INVERSE = 1, NTT_F_BITREV = 2;

// what a pass carries besides its sub-transforms
enum : uint32_t {
  NTT_P_READ_BE = 1,     // first pass: the input is 32 B big-endian, every value range-checked
  NTT_P_SHIFT = 2,       // forward, first pass's load: times s^i; inverse, last pass's store: times s^-i
  NTT_P_SCALE = 4,       // inverse, last pass's store: times n^-1 (one product with the shift power)
  NTT_P_BITREV_IN = 8,   // inverse, first pass: logical element i is read from bitrev(i)
  NTT_P_BITREV_OUT = 16, // forward, last pass: X[k] is written to bitrev(k)
  NTT_P_WRITE_BE = 32,   // last pass: the output is 32 B big-endian
  NTT_P_TWIDDLE = 64,    // every pass but the first: the load multiplies by w^(a tw_step kappa)
  NTT_P_LAST = 128,      // the last pass: its columns are taken in the order of kappa
  NTT_P_INVERSE = 256,   // every root is inverted
};

struct NttPass {
  uint32_t bits;      // the sub-transforms are of 2^bits points
  uint32_t lstride;   // log2 of the element stride M_p between a sub-transform's points
  uint32_t lprev;     // bits of the digits above: bits_0 + .. + bits_{p-1} (lprev + bits + lstride = logn)
  uint32_t tw_step;   // the twiddle of element a is w_{2^26}^(a kappa tw_step): 2^(26 - lprev - bits); 0 on pass 0
  uint32_t flags;     // NTT_P_*
};

struct NttPlan {
  uint32_t logn, npass;
  uint64_t count;
  NttPass pass[NTT_MAX_PASSES];
};

// bound: the most bits of a pass (NTT_MIN_PASS_BITS .. tile_bits - 2).  read_be / write_be: the
// caller's side of the data is big-endian bytes (else 8 little-endian words, canonical).  The widths
// are balanced: ceil(logn / bound) passes, the wider ones first.  Returns false on arguments out of
// range (logn > 26, count n > 2^26, a flag bit unknown, a bound out of range).
inline bool ntt_plan(uint32_t logn, uint64_t count, uint32_t flags, bool shift, uint32_t bound, bool read_be, bool write_be,
                     NttPlan* out) {
  if (logn > NTT_MAX_LOGN || (flags & ~(NTT_F_INVERSE | NTT_F_BITREV))) return false;
  if (bound < NTT_MIN_PASS_BITS || bound > NTT_WIDEST_BITS) return false;
  if (count > (uint64_t(1) << (NTT_MAX_LOGN - logn))) return false;
  const bool inv = flags & NTT_F_INVERSE, rev = flags & NTT_F_BITREV;
  NttPlan p{};
  p.logn = logn;
  p.count = count;
  p.npass = logn == 0 ? 1 : (logn + bound - 1) / bound;
  const uint32_t base = logn / p.npass, rem = logn % p.npass;
  uint32_t prev = 0;
  for (uint32_t k = 0; k < p.npass; ++k) {
    NttPass& q = p.pass[k];
    q.bits = base + (k < rem ? 1 : 0);
    q.lprev = prev;
    q.lstride = logn - prev - q.bits;
    q.tw_step = k ? 1u << (NTT_ROOT_BITS - prev - q.bits) : 0;
    q.flags = (k ? NTT_P_TWIDDLE : 0) | (inv ? NTT_P_INVERSE : 0);
    prev += q.bits;
  }
  NttPass& first = p.pass[0];
  NttPass& last = p.pass[p.npass - 1];
  if (read_be) first.flags |= NTT_P_READ_BE;
  if (write_be) last.flags |= NTT_P_WRITE_BE;
  last.flags |= NTT_P_LAST;
  if (inv) {
    if (rev) first.flags |= NTT_P_BITREV_IN;
    if (logn) last.flags |= NTT_P_SCALE;
    if (shift) last.flags |= NTT_P_SHIFT;
  } else {
    if (rev) last.flags |= NTT_P_BITREV_OUT;
    if (shift) first.flags |= NTT_P_SHIFT;
  }
  *out = p;
  return true;
}

// bytes of the ping-pong copy a plan needs beside the caller's arrays: none for one pass
inline size_t ntt_scratch_bytes(const NttPlan& p) { return p.npass > 1 ? (size_t)32 * (p.count << p.logn) : 0; }

}  // namespace kzgmi
