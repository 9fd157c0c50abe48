// What the search for a rejected batch's invalid tuples (host_find.hip) decides on the host, as plain
// data: how a suspect range splits (find_split), which failing parts a level keeps (find_next_level),
// how one grouped small-MSM launch is laid out (find_group_plan, msm_group.hpp) and which path a
// level takes at which fan-out (find_level_fanout, find_level_path, find_group_chunk).  Nothing here allocates, launches or reads the
// environment: every array is the caller's.  tests/native/find_probe.hip exposes the functions to a
// test that needs no GPU.
//
// The search is group testing over index ranges: a range [lo, hi) passes iff its randomised
// combination (A, B) satisfies e(A, [tau]_2) e(-B, [1]_2) = 1; a failing range is split into at most
// `fanout` parts, down to single tuples.  A passing range holds no invalid tuple except with
// probability ~2^-127 (the 127-bit randomisers), a failing range holds at least one.
#pragma once
#include "msm_small.hpp"

#include <cstddef>
#include <cstdint>

namespace kzgmi {

struct FindRange {
  uint64_t lo, hi;  // [lo, hi), lo < hi
};

// The search's two measured choices and its workspace bound.
struct FindTuning {
  // parts a failing range splits into: `fanout` in a grouped level (it costs by its wave-terms,
  // whatever the number of parts, plus one pairing round per 256 parts and a host round trip: few
  // levels), `bucket_fanout` in a bucket level (it costs ~1.7 ms per part: F / ln F parts per
  // halving of the range is least at F = 3 or 4); find_level_fanout
  uint32_t fanout = 16;
  uint32_t bucket_fanout = 4;
  // a level whose longest part has at most this many wave-terms (3 len + 1) runs in the grouped
  // kernel; longer parts run as bucket partial jobs, one after another (MsmTuning::small_terms' value)
  uint32_t group_terms = 4096;
  // bound on one grouped launch's tree workspace (stored nodes + arrival counters); a level with
  // more is cut into several launches, a kzgmi_batch_range_partials_device call with more is refused
  size_t group_bytes = size_t(256) << 20;
};

constexpr size_t FIND_MAX_BAD = 4096;       // most indices one search reports
constexpr size_t FIND_MAX_RANGES = 65536;   // most ranges of one kzgmi_batch_range_partials_device call

// [lo, hi) of length L into k = min(F, L) parts, part j = [lo + floor(j L / k), lo + floor((j + 1) L / k));
// out holds k ranges; returns k
inline uint32_t find_split(uint64_t lo, uint64_t hi, uint32_t F, FindRange* out) {
  const uint64_t L = hi - lo;
  const uint64_t k = L < F ? L : F;
  for (uint64_t j = 0; j < k; ++j) out[j] = {lo + j * L / k, lo + (j + 1) * L / k};
  return (uint32_t)k;
}

// One level's outcome.  parts: the level's ranges, ascending and disjoint, ok[j] != 0 where part j
// passed.  bad_in: the single tuples found so far, ascending.  Every failing part and every found
// tuple holds at least one invalid tuple and they are pairwise disjoint, so the lowest max_bad
// invalid indices lie within the lowest max_bad of them: those are kept (in ascending order: found
// tuples and failing parts of length 1 into bad_out, longer failing parts into suspects_out), the
// others are dropped and `more` is set for good.  bad_out and suspects_out hold max_bad entries;
// bad_out must not alias bad_in.
struct FindLevel {
  size_t n_suspects, n_bad;
  bool more;
};
inline FindLevel find_next_level(const FindRange* parts, const int32_t* ok, size_t nparts, size_t max_bad,
                                 const uint64_t* bad_in, size_t n_bad_in, bool more_in, uint64_t* bad_out,
                                 FindRange* suspects_out) {
  FindLevel r{0, 0, more_in};
  size_t i = 0, j = 0, kept = 0;
  while (j < nparts && ok[j]) ++j;
  while (kept < max_bad && (i < n_bad_in || j < nparts)) {
    if (j >= nparts || (i < n_bad_in && bad_in[i] < parts[j].lo)) {
      bad_out[r.n_bad++] = bad_in[i++];
    } else {
      if (parts[j].hi - parts[j].lo == 1) bad_out[r.n_bad++] = parts[j].lo;
      else suspects_out[r.n_suspects++] = parts[j];
      ++j;
      while (j < nparts && ok[j]) ++j;
    }
    ++kept;
  }
  if (i < n_bad_in || j < nparts) r.more = true;
  return r;
}

// One group of a grouped launch as the kernel reads it (device memory): tuples [lo, lo + len) of the
// resident batch, its waves [wave_base, wave_base + 3 len + T), and of its trees A (len leaves) and
// B (2 len + T leaves) the first stored node and the first arrival counter.  T is the tail: 1 for
// opening tuples (-t_g G1), 64 for EIP-7594 cells (-c_m(g) [tau^m]_1, m < 64)
struct FindGroup {
  uint32_t lo, len, wave_base;
  uint32_t node_base[2], flag_base[2];
  uint32_t pad;
};
static_assert(sizeof(FindGroup) == 32, "the group table's entries are 8 words");

// stored nodes and arrival counters of a tree with `leaves` leaves (msm_small.hpp: levels back to back)
inline void find_tree_size(uint64_t leaves, uint64_t& nodes, uint64_t& flags) {
  nodes = flags = 0;
  for (uint64_t cnt = leaves; cnt > 1; cnt = (cnt + 1) >> 1) {
    nodes += cnt;
    flags += (cnt + 1) >> 1;
  }
}
inline uint64_t find_wave_terms(uint64_t len, uint32_t tail = 1) { return 3 * len + tail; }

// The launch of G groups: group g's waves in the order r_i pi_i (A's leaves 0 .. len - 1), r_i C_i
// (B's leaves 0 .. len - 1), s_i pi_i (B's leaves len .. 2 len - 1), then the `tail` terms of the
// group's own scalars (B's leaves 2 len .. 2 len + tail - 1): -t_g G1, or the 64 of a cell range.
// ranges are relative to the resident batch.  table (G entries, may be null: sizes only).
// fits: every index stays below 2^31.
struct FindGroupPlan {
  uint64_t waves, nodes, flags;
  size_t bytes_nodes, bytes_flags, bytes_table, bytes_negt;
  size_t bytes;  // the tree workspace FindTuning::group_bytes bounds: nodes + flags
  bool fits;
};
inline FindGroupPlan find_group_plan(const FindRange* ranges, size_t G, FindGroup* table, uint32_t tail = 1) {
  FindGroupPlan p{};
  for (size_t g = 0; g < G; ++g) {
    const uint64_t len = ranges[g].hi - ranges[g].lo;
    uint64_t na, fa, nb, fb;
    find_tree_size(len, na, fa);
    find_tree_size(2 * len + tail, nb, fb);
    if (table)  // (meaningless where the plan does not fit: the caller refuses it)
      table[g] ={(uint32_t)ranges[g].lo, (uint32_t)len, (uint32_t)p.waves,
                  {(uint32_t)p.nodes, (uint32_t)(p.nodes + na)}, {(uint32_t)p.flags, (uint32_t)(p.flags + fa)}, 0};
    p.waves += find_wave_terms(len, tail);
    p.nodes += na + nb;
    p.flags += fa + fb;
  }
  p.fits = p.waves < (1ull << 31) && p.nodes < (1ull << 31) && G < (1ull << 31);
  p.bytes_nodes = (size_t)(p.nodes + 1) * SMALL_NODE_WORDS * 4;
  p.bytes_flags = (size_t)(p.flags + 1) * 4;
  p.bytes_table = (G + 1) * sizeof(FindGroup);
  p.bytes_negt = ((size_t)tail * G + 1) * 32;
  p.bytes = p.bytes_nodes + p.bytes_flags;
  return p;
}

// A level's path: 1 the grouped kernel (every part of at most group_terms wave-terms), 0 bucket
// partial jobs.  The parts of one level differ in length by at most one per level above them, and
// the longest shrinks with every level, so a search goes from bucket levels to grouped ones once.
enum FindPath { FIND_BUCKET = 0, FIND_GROUPED = 1 };
inline int find_level_path(const FindRange* parts, size_t nparts, const FindTuning& t) {
  uint64_t longest = 0;
  for (size_t j = 0; j < nparts; ++j) longest = parts[j].hi - parts[j].lo > longest ? parts[j].hi - parts[j].lo : longest;
  return find_wave_terms(longest) <= t.group_terms ? FIND_GROUPED : FIND_BUCKET;
}

// A level's fan-out.  The narrow split decides the path: where its parts are short enough for the
// grouped kernel the level is a grouped one whatever the fan-out, and takes the wide one; a level
// above that stays narrow (splitting it wide into the grouped kernel costs its suspects' whole
// length in wave-terms: 1.05 us per tuple against 1.7 ms per bucket job)
inline uint32_t find_level_fanout(const FindRange* suspects, size_t ns, const FindTuning& t) {
  uint64_t longest = 0;
  for (size_t j = 0; j < ns; ++j)
    longest = suspects[j].hi - suspects[j].lo > longest ? suspects[j].hi - suspects[j].lo : longest;
  const uint64_t part = (longest + t.bucket_fanout - 1) / t.bucket_fanout;  // the longest part of the narrow split
  return find_wave_terms(part) <= t.group_terms ? t.fanout : t.bucket_fanout;
}

// How many of ranges[0, G) one grouped launch takes within the workspace bound: at least one
inline size_t find_group_chunk(const FindRange* ranges, size_t G, const FindTuning& t, uint32_t tail = 1) {
  uint64_t nodes = 0, flags = 0, waves = 0;
  size_t g = 0;
  for (; g < G; ++g) {
    const uint64_t len = ranges[g].hi - ranges[g].lo;
    uint64_t na, fa, nb, fb;
    find_tree_size(len, na, fa);
    find_tree_size(2 * len + tail, nb, fb);
    nodes += na + nb;
    flags += fa + fb;
    waves += find_wave_terms(len, tail);
    if (g > 0 && ((nodes + 1) * SMALL_NODE_WORDS * 4 + (flags + 1) * 4 > t.group_bytes || waves >= (1ull << 31))) break;
  }
  return g;
}

}  // namespace kzgmi
