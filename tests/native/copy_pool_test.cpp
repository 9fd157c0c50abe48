// Stand-alone check of csrc/copy_pool.hpp (the pageable -> pinned staging copy of api.hip's h2d):
// every copy is compared with its source byte for byte, into a destination pre-filled with poison
// between two 64-byte guards that must stay intact.  One line per failing case, exit status 1 if
// any failed.  Built with sanitizers and run by tests/test_copy_pool_cpu.py; no GPU, no HIP.
//
//   copy_pool_test            every case
//   copy_pool_test table      only the three lengths that lost their tail at 16, 32 and 24 threads
#include "copy_pool.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

namespace {

using kzgmi::CopyPool;
constexpr size_t kMin = kzgmi::kCopyPoolMinBytes;
constexpr size_t kRing = size_t(16) << 20;  // host.hpp kRingBytes: the longest copy h2d issues
constexpr size_t kGuard = 64;
constexpr uint8_t kPoison = 0xA5, kGuardByte = 0x5A;
const int kThreads[] = {1, 2, 3, 7, 8, 9, 12, 16, 17, 24, 32, 33};
const size_t kOffsets[] = {0, 1, 3, 63};

int g_failures = 0;

// one pool per thread count, never destroyed (its workers are detached, as in the library)
CopyPool* g_pools[64];
CopyPool* pool(int threads) {
  if (!g_pools[threads]) g_pools[threads] = new CopyPool(threads);
  return g_pools[threads];
}

struct Buffers {
  std::vector<uint8_t> src, dst;
  Buffers() : src(kRing + 256), dst(kRing + 2 * kGuard + 256) {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto& b : src) {  // xorshift bytes, never the poison value: a byte left uncopied always shows
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      b = (uint8_t)(x >> 32);
      if (b == kPoison) b = 0;
    }
  }
  static uint8_t* align64(uint8_t* p) { return (uint8_t*)(((uintptr_t)p + 63) & ~uintptr_t(63)); }
  // copies len bytes through p at the given offsets from 64-byte-aligned bases; true if exact
  bool run(CopyPool* p, size_t len, size_t soff, size_t doff, std::string& why) {
    const uint8_t* s = align64(src.data()) + soff;
    uint8_t* g = align64(dst.data()) + doff;  // guard, len bytes, guard
    uint8_t* d = g + kGuard;
    memset(g, kGuardByte, kGuard);
    memset(d, kPoison, len);
    memset(d + len, kGuardByte, kGuard);
    p->copy(d, s, len);
    if (memcmp(d, s, len) != 0) {
      size_t first = 0, bad = 0;
      for (size_t i = len; i-- > 0;)
        if (d[i] != s[i]) first = i, ++bad;
      why = "dst differs from src in " + std::to_string(bad) + " bytes, first at " + std::to_string(first);
      return false;
    }
    for (size_t i = 0; i < kGuard; ++i)
      if (g[i] != kGuardByte || d[len + i] != kGuardByte) {
        why = "guard byte " + std::to_string(i) + " overwritten";
        return false;
      }
    return true;
  }
};

void check(Buffers& b, int threads, size_t len, size_t soff, size_t doff) {
  std::string why;
  if (b.run(pool(threads), len, soff, doff, why)) return;
  ++g_failures;
  printf("FAIL threads=%d len=%zu src+%zu dst+%zu: %s\n", threads, len, soff, doff, why.c_str());
}

// KZGMI_COPY_THREADS and the staged length of the three inputs that lost their tail
struct TableRow { int threads; size_t len; };
const TableRow kTable[] = {
    {16, 262145 * size_t(8)},  // 262145 uint64 indices: 2097160 B
    {32, 43691 * size_t(48)},  // 43691 compressed G1 points: 2097168 B
    {24, 2098192},             // a 16-byte-granular array
};

std::vector<size_t> lengths_for(int threads) {
  std::set<size_t> v = {kMin - 1, kMin, kRing, kRing - 16};
  for (size_t d : {1, 7, 8, 15, 16, 17, 63, 64, 65}) v.insert(kMin + d);
  const size_t step = size_t(64) * threads;
  for (size_t r = 1; r < (size_t)threads; ++r)  // the smallest 64 * parts * m + r >= the threshold
    v.insert((kMin - r + step - 1) / step * step + r);
  for (const TableRow& t : kTable) v.insert(t.len);
  return std::vector<size_t>(v.begin(), v.end());
}

// every length at every source offset and every destination offset; the pairing of the two
// rotates from one length to the next, so each thread count sees all 16 pairs several times
void all_lengths(Buffers& b) {
  for (int threads : kThreads) {
    int rot = 0;
    for (size_t len : lengths_for(threads)) {
      for (int j = 0; j < 4; ++j) check(b, threads, len, kOffsets[j], kOffsets[(j + rot) % 4]);
      ++rot;
    }
  }
}

void table_only(Buffers& b) {
  for (const TableRow& t : kTable) check(b, t.threads, t.len, 0, 0);
}

// four host threads, 200 copies each of differing lengths through one pool: the job mutex, the
// generation counter and the completion wake-up
void concurrent() {
  CopyPool* p = pool(8);
  int failed[4] = {0, 0, 0, 0};
  std::string why[4];
  std::vector<std::thread> ts;
  for (int t = 0; t < 4; ++t)
    ts.emplace_back([&, t] {
      Buffers b;
      for (int k = 0; k < 200; ++k) {
        // from just below the threshold (the plain memcpy) to ~1.5 x it, no two equal in one thread
        const size_t len = kMin - 64 + (size_t)k * 5003 + (size_t)t * 17 + (k % 3 == 0 ? 0 : (size_t)k * 257);
        std::string w;
        if (!b.run(p, len, kOffsets[(k + t) % 4], kOffsets[k % 4], w)) {
          if (!failed[t]++) why[t] = "copy " + std::to_string(k) + " len=" + std::to_string(len) + ": " + w;
        }
      }
    });
  for (auto& t : ts) t.join();
  for (int t = 0; t < 4; ++t)
    if (failed[t]) {
      ++g_failures;
      printf("FAIL concurrent host thread %d: %d of 200 copies wrong, first %s\n", t, failed[t], why[t].c_str());
    }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "all";
  {
    Buffers b;
    if (mode == "table") {
      table_only(b);
    } else if (mode == "all") {
      all_lengths(b);
    } else {
      fprintf(stderr, "usage: %s [all|table]\n", argv[0]);
      return 2;
    }
  }
  if (mode == "all") concurrent();
  printf("%s: %d failing case%s\n", g_failures ? "FAILED" : "ok", g_failures, g_failures == 1 ? "" : "s");
  return g_failures ? 1 : 0;
}
