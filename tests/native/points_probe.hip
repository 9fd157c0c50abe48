// Test-only probe of the G1 point layer (tests/test_gpu_points_ops.py): the point formulas of
// csrc/g1.hpp (32-bit XYZZ), the radix-2^29 Jacobian chain of the subgroup check and the encoding
// helpers of csrc/points.hpp, the GLV split of csrc/glv.hpp, and the launchers of csrc/launch_io.hip
// that bring points and scalars into the library.  No arithmetic lives here: a kernel loads its
// operands, calls the shipped device function and stores every output word; a stage allocates its
// buffers, calls the shipped launcher and copies everything back.  Built into
// kzgmi/libkzgmi_pointsprobe.so, one object per curve (-DKZ_CURVE=0/1); never linked into libkzgmi.so.
//
// a. Device functions, one kernel each, one case per thread (ctypes: tests/pointsprobe.py):
//   kzgmi_pointsprobe_words(curve, op, &in_words, &out_words)    words per case of an op
//   kzgmi_pointsprobe_run(curve, op, host_in, n_cases, host_out) 0, or an error code below
//   g1.*     Fp<P> values of P::N words: an affine point is x, y; an XYZZ point x, y, zz, zzz
//   jac29.*  (BLS12-381) F29 values of 14 limbs; a Jac29 is x, y, z, inf (3 x 14 + 1 words)
//   pt.*     fp_raw_gt against P::HALF; compress_encoding on the words of one encoding
//   glv.*    a scalar is 8 words, a quotient or half scalar 4
//
// b. The launchers of csrc/launch_io.hip, one stage per call.  Every buffer has its exact size and
// is followed by a guard of GUARD bytes; output buffers are filled with the caller's poison byte
// first (error words with zero: raise_err only ever raises them); after the stage each guard is read
// back: guards[buffer id] = 1 intact, 0 overwritten, 2 not used by this stage.  per_elem != 0
// enqueues the launcher once per case with n = 1 and that case's own error word (err: n words),
// otherwise one launch covers all cases (err: one word).  Everything runs on the null stream with
// one synchronise at the end.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "launch_io.hip"

#if KZ_CURVE == 0
#define PROBE_FN(name) pointsprobe_##name##_0
#else
#define PROBE_FN(name) pointsprobe_##name##_1
#endif

enum { PROBE_ERR_CURVE = -1, PROBE_ERR_OP = -2, PROBE_ERR_COUNT = -3, PROBE_ERR_ARG = -4, PROBE_ERR_HIP = 1000 };
// guard ids (tests/pointsprobe.py GUARDS)
enum { B_IN, B_IN_INF, B_PTS, B_INF, B_IMG, B_IMG_INF, B_ERR, B_OUT, B_H0, B_H1, B_COUNT };

namespace {
using namespace kzgmi;
using Cv = KZ_CURVE_T;
using L = Launch<Cv>;
using P = typename Cv::FpP;
using FpB = Fp<P>;
using XY = Xyzz<Cv>;
using AF = Affine<Cv>;
constexpr int N32 = P::N;
constexpr uint32_t MAX_CASES = 1u << 20, MAX_STAGE = 1u << 16;

#define PROBE_HIP(call)                                                \
  do {                                                                 \
    const hipError_t err_ = (call);                                    \
    if (err_ != hipSuccess && rc == 0) rc = PROBE_ERR_HIP + (int)err_; \
  } while (0)

__device__ FpB ld(const uint32_t* p) {
  FpB r;
  _Pragma("unroll") for (int i = 0; i < N32; ++i) r.v[i] = p[i];
  return r;
}
__device__ void st(uint32_t* p, const FpB& a) {
  _Pragma("unroll") for (int i = 0; i < N32; ++i) p[i] = a.v[i];
}
__device__ AF lda(const uint32_t* p) {
  AF a;
  a.x = ld(p);
  a.y = ld(p + N32);
  return a;
}
__device__ XY ldx(const uint32_t* p) { return {ld(p), ld(p + N32), ld(p + 2 * N32), ld(p + 3 * N32)}; }
__device__ void stx(uint32_t* p, const XY& a) {
  st(p, a.x); st(p + N32, a.y); st(p + 2 * N32, a.zz); st(p + 3 * N32, a.zzz);
}

// ---------------------------------------------------------------- one case per thread
template <class Op>
__global__ __launch_bounds__(64) void k_thread(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Op::run(in + (size_t)i * Op::IN, out + (size_t)i * Op::OUT);
}

#define DEFOP(NAME, NIN, NOUT, ...)                                   \
  struct NAME {                                                       \
    static constexpr int IN = (NIN), OUT = (NOUT);                    \
    static __device__ void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__; } \
  };
DEFOP(g_from_affine, 2 * N32, 4 * N32, stx(out, xyzz_from_affine(lda(in))))
DEFOP(g_dbl, 4 * N32, 4 * N32, stx(out, xyzz_dbl(ldx(in))))
DEFOP(g_dbl_affine, 2 * N32, 4 * N32, stx(out, xyzz_dbl_affine(lda(in))))
DEFOP(g_add_affine, 6 * N32, 4 * N32, stx(out, xyzz_add_affine(ldx(in), lda(in + 4 * N32))))
DEFOP(g_add, 8 * N32, 4 * N32, stx(out, xyzz_add(ldx(in), ldx(in + 4 * N32))))
DEFOP(g_neg, 4 * N32, 4 * N32, stx(out, xyzz_neg(ldx(in))))
// flag, then the point (left as the zeros it is handed in with where the function does not write it)
DEFOP(g_to_affine, 4 * N32, 1 + 2 * N32, AF a; a.x = FpB::zero(); a.y = FpB::zero();
      const bool finite = xyzz_to_affine(ldx(in), a);
      out[0] = finite ? 1u : 0u; st(out + 1, a.x); st(out + 1 + N32, a.y))
DEFOP(g_on_curve, 2 * N32, 1, out[0] = affine_on_curve(lda(in)) ? 1u : 0u)

DEFOP(p_raw_gt_half, N32, 1, out[0] = fp_raw_gt(ld(in), P::HALF) ? 1u : 0u)
DEFOP(p_compress_encoding, 2 * N32, N32, uint32_t w[2 * N32]; uint32_t o[N32];
      _Pragma("unroll") for (int k = 0; k < 2 * N32; ++k) w[k] = in[k];
      compress_encoding<Cv>(w, o);
      _Pragma("unroll") for (int k = 0; k < N32; ++k) out[k] = o[k])

#define DEF_ROUND_DIV(NAME, G)                                                    \
  DEFOP(NAME, 8, 4, uint32_t k[8]; uint32_t g[4]; uint32_t c[4];                  \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) k[i] = in[i];               \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) g[i] = Cv::K::G[i];         \
        glv_round_div<Cv>(k, g, c);                                               \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) out[i] = c[i])
DEF_ROUND_DIV(v_round_div_g1, GLV_G1)
DEF_ROUND_DIV(v_round_div_g2, GLV_G2)
DEFOP(v_split, 8, 8, uint32_t k[8]; uint32_t a[4]; uint32_t b[4];
      _Pragma("unroll") for (int i = 0; i < 8; ++i) k[i] = in[i];
      glv_split<Cv>(k, a, b);
      _Pragma("unroll") for (int i = 0; i < 4; ++i) { out[i] = a[i]; out[4 + i] = b[i]; })

#if KZ_CURVE == 0
// csrc/points.hpp runs its Jacobian chain and its square root in radix 2^29 on BLS12-381 only
constexpr int N29 = Q29::N, JW = 3 * N29 + 1;
__device__ G29 ld29(const uint32_t* p) {
  G29 r;
  _Pragma("unroll") for (int i = 0; i < N29; ++i) r.v[i] = p[i];
  return r;
}
__device__ void st29(uint32_t* p, const G29& a) {
  _Pragma("unroll") for (int i = 0; i < N29; ++i) p[i] = a.v[i];
}
__device__ Jac29 ldj(const uint32_t* p) { return {ld29(p), ld29(p + N29), ld29(p + 2 * N29), p[3 * N29] != 0}; }
__device__ void stj(uint32_t* p, const Jac29& a) {
  st29(p, a.x); st29(p + N29, a.y); st29(p + 2 * N29, a.z);
  p[3 * N29] = a.inf ? 1u : 0u;
}
DEFOP(j_dbl, JW, JW, stj(out, jac29_dbl(ldj(in))))
DEFOP(j_add_affine, JW + 2 * N29, JW, stj(out, jac29_add_affine(ldj(in), ld29(in + JW), ld29(in + JW + N29))))
DEFOP(j_add, 2 * JW, JW, stj(out, jac29_add(ldj(in), ldj(in + JW))))
// q, then the affine base qx, qy (read by the <true> form only)
DEFOP(j_mul_x_affine, JW + 2 * N29, JW,
      stj(out, mul_by_x_abs29<Cv, true>(ldj(in), ld29(in + JW), ld29(in + JW + N29))))
DEFOP(j_mul_x_jac, JW + 2 * N29, JW,
      stj(out, mul_by_x_abs29<Cv, false>(ldj(in), ld29(in + JW), ld29(in + JW + N29))))
DEFOP(j_zero, N29, 1, out[0] = zero29(ld29(in)) ? 1u : 0u)
DEFOP(j_pow_sqrt, N32, N32, st(out, fp_pow_sqrt29(ld(in))))
#endif

// ---------------------------------------------------------------- op table and host side
using LaunchFn = hipError_t (*)(const uint32_t*, uint32_t*, uint32_t);
struct Entry {
  std::string name;
  int in, out;
  LaunchFn launch;
};
template <class Op> hipError_t launch_thread(const uint32_t* in, uint32_t* out, uint32_t n) {
  k_thread<Op><<<(n + 63) / 64, 64>>>(in, out, n);
  return hipGetLastError();
}
template <class Op> void add_op(std::vector<Entry>& t, const std::string& name) {
  t.push_back({name, Op::IN, Op::OUT, &launch_thread<Op>});
}

const std::vector<Entry>& table() {
  static const std::vector<Entry> t = [] {
    std::vector<Entry> v;
    add_op<g_from_affine>(v, "g1.xyzz_from_affine");
    add_op<g_dbl>(v, "g1.xyzz_dbl");
    add_op<g_dbl_affine>(v, "g1.xyzz_dbl_affine");
    add_op<g_add_affine>(v, "g1.xyzz_add_affine");
    add_op<g_add>(v, "g1.xyzz_add");
    add_op<g_neg>(v, "g1.xyzz_neg");
    add_op<g_to_affine>(v, "g1.xyzz_to_affine");
    add_op<g_on_curve>(v, "g1.affine_on_curve");
    add_op<p_raw_gt_half>(v, "pt.fp_raw_gt_half");
    add_op<p_compress_encoding>(v, "pt.compress_encoding");
    add_op<v_round_div_g1>(v, "glv.round_div_g1");
    add_op<v_round_div_g2>(v, "glv.round_div_g2");
    add_op<v_split>(v, "glv.split");
#if KZ_CURVE == 0
    add_op<j_dbl>(v, "jac29.dbl");
    add_op<j_add_affine>(v, "jac29.add_affine");
    add_op<j_add>(v, "jac29.add");
    add_op<j_mul_x_affine>(v, "jac29.mul_by_x_affine");
    add_op<j_mul_x_jac>(v, "jac29.mul_by_x_jac");
    add_op<j_zero>(v, "jac29.zero29");
    add_op<j_pow_sqrt>(v, "jac29.fp_pow_sqrt29");
#endif
    return v;
  }();
  return t;
}

const Entry* find(const char* op) {
  for (const Entry& e : table())
    if (e.name == op) return &e;
  return nullptr;
}

// device buffers of one stage call: exact size + guard, freed on every path
constexpr size_t GUARD = 4096;
constexpr uint8_t GUARD_BYTE = 0x5C;
struct Dev {
  struct B { uint8_t* p; size_t bytes; int id; };
  std::vector<B> bufs;
  int rc = 0;
  uint8_t poison;
  explicit Dev(int poison_byte) : poison((uint8_t)poison_byte) {}
  template <class T>
  T* get(int id, size_t bytes, bool zero = false) {
    void* d = nullptr;
    PROBE_HIP(hipMalloc(&d, bytes + GUARD));
    if (!d) return nullptr;
    bufs.push_back({static_cast<uint8_t*>(d), bytes, id});
    if (bytes) PROBE_HIP(hipMemset(d, zero ? 0 : poison, bytes));
    PROBE_HIP(hipMemset(static_cast<uint8_t*>(d) + bytes, GUARD_BYTE, GUARD));
    return static_cast<T*>(d);
  }
  void put(void* dst, const void* src, size_t bytes) {
    if (rc == 0 && bytes) PROBE_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  }
  void take(void* dst, const void* src, size_t bytes) {
    if (rc == 0 && bytes) PROBE_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  }
  void finish() {
    if (rc == 0) PROBE_HIP(hipGetLastError());
    if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
  }
  void guards(uint32_t* out) {
    for (int i = 0; i < B_COUNT; ++i) out[i] = 2;
    std::vector<uint8_t> g(GUARD);
    for (const B& b : bufs) {
      take(g.data(), b.p + b.bytes, GUARD);
      bool ok = rc == 0;
      for (size_t i = 0; ok && i < GUARD; ++i) ok = g[i] == GUARD_BYTE;
      out[b.id] = ok ? 1 : 0;
    }
  }
  ~Dev() {
    for (const B& b : bufs) (void)hipFree(b.p);
  }
};

// f(first case, cases, error word): once per case, or once over all of them
template <class F>
void each(bool per_elem, uint32_t n, F f) {
  if (!per_elem) {
    f(0u, n, 0u);
    return;
  }
  for (uint32_t i = 0; i < n; ++i) f(i, 1u, i);
}
bool stage_ok(uint32_t n) { return n >= 1 && n <= MAX_STAGE; }
}  // namespace

int PROBE_FN(words)(const char* op, int* in_words, int* out_words) {
  const Entry* e = find(op);
  if (!e) return PROBE_ERR_OP;
  *in_words = e->in;
  *out_words = e->out;
  return 0;
}

int PROBE_FN(run)(const char* op, const void* host_in, uint32_t n, void* host_out) {
  const Entry* e = find(op);
  if (!e) return PROBE_ERR_OP;
  if (n == 0 || n > MAX_CASES) return PROBE_ERR_COUNT;
  const size_t ib = (size_t)n * e->in * 4, ob = (size_t)n * e->out * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  int rc = 0;
  PROBE_HIP(hipMalloc(&din, ib));
  PROBE_HIP(hipMalloc(&dout, ob));
  if (rc == 0) PROBE_HIP(hipMemcpy(din, host_in, ib, hipMemcpyHostToDevice));
  if (rc == 0) PROBE_HIP(hipMemset(dout, 0xA5, ob));  // an output word the kernel skips shows up
  if (rc == 0) PROBE_HIP(e->launch(din, dout, n));
  if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
  if (rc == 0) PROBE_HIP(hipMemcpy(host_out, dout, ob, hipMemcpyDeviceToHost));
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return rc;
}

// words of an Fp, an Affine slot and an Xyzz record
void PROBE_FN(sizes)(uint32_t* out) {
  out[0] = N32;
  out[1] = sizeof(AF) / 4;
  out[2] = sizeof(XY) / 4;
}

// form 0: 32-bit Montgomery slots; 1: radix-29 slots; 2: radix-29 slots and the GLV images.
// bytes: n uncompressed encodings; pts, img: n slots; inf, img_inf: n bytes
int PROBE_FN(convert_points)(int form, int per_elem, int poison, const uint8_t* bytes, uint32_t n, uint32_t* pts,
                             uint8_t* inf, uint32_t* img, uint8_t* img_inf, uint32_t* err, uint32_t* guards) {
  if (!stage_ok(n) || form < 0 || form > 2) return PROBE_ERR_ARG;
  constexpr size_t ENC = 8 * N32;
  const uint32_t nerr = per_elem ? n : 1;
  Dev dv(poison);
  int& rc = dv.rc;
  uint8_t* din = dv.get<uint8_t>(B_IN, n * ENC);
  AF* dpts = dv.get<AF>(B_PTS, n * sizeof(AF));
  uint8_t* dinf = dv.get<uint8_t>(B_INF, n);
  AF* dimg = form == 2 ? dv.get<AF>(B_IMG, n * sizeof(AF)) : nullptr;
  uint8_t* dimg_inf = form == 2 ? dv.get<uint8_t>(B_IMG_INF, n) : nullptr;
  uint32_t* derr = dv.get<uint32_t>(B_ERR, nerr * 4, true);
  dv.put(din, bytes, n * ENC);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t e) {
      L::convert_points(nullptr, din + i * ENC, c, dpts + i, dinf + i, derr + e, form >= 1, dimg ? dimg + i : nullptr,
                        dimg_inf ? dimg_inf + i : nullptr);
    });
    dv.finish();
  }
  dv.take(pts, dpts, n * sizeof(AF));
  dv.take(inf, dinf, n);
  if (dimg) dv.take(img, dimg, n * sizeof(AF));
  if (dimg_inf) dv.take(img_inf, dimg_inf, n);
  dv.take(err, derr, nerr * 4);
  dv.guards(guards);
  return rc;
}

// bytes: n compressed encodings
int PROBE_FN(decompress_points)(int per_elem, int poison, const uint8_t* bytes, uint32_t n, uint32_t* pts, uint8_t* inf,
                                uint32_t* err, uint32_t* guards) {
  if (!stage_ok(n)) return PROBE_ERR_ARG;
  constexpr size_t ENC = 4 * N32;
  const uint32_t nerr = per_elem ? n : 1;
  Dev dv(poison);
  int& rc = dv.rc;
  uint8_t* din = dv.get<uint8_t>(B_IN, n * ENC);
  AF* dpts = dv.get<AF>(B_PTS, n * sizeof(AF));
  uint8_t* dinf = dv.get<uint8_t>(B_INF, n);
  uint32_t* derr = dv.get<uint32_t>(B_ERR, nerr * 4, true);
  dv.put(din, bytes, n * ENC);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t e) {
      L::decompress_points(nullptr, din + i * ENC, c, dpts + i, dinf + i, derr + e);
    });
    dv.finish();
  }
  dv.take(pts, dpts, n * sizeof(AF));
  dv.take(inf, dinf, n);
  dv.take(err, derr, nerr * 4);
  dv.guards(guards);
  return rc;
}

// in: n uncompressed encodings; out: n compressed ones
int PROBE_FN(compress_points)(int per_elem, int poison, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t* guards) {
  if (!stage_ok(n)) return PROBE_ERR_ARG;
  constexpr size_t ENC = 8 * N32, CMP = 4 * N32;
  Dev dv(poison);
  int& rc = dv.rc;
  uint8_t* din = dv.get<uint8_t>(B_IN, n * ENC);
  uint8_t* dout = dv.get<uint8_t>(B_OUT, n * CMP);
  dv.put(din, in, n * ENC);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t) { L::compress_points(nullptr, din + i * ENC, c, dout + i * CMP); });
    dv.finish();
  }
  dv.take(out, dout, n * CMP);
  dv.guards(guards);
  return rc;
}

// pts: n slots in 32-bit Montgomery form; inf: n bytes (a flagged entry is skipped)
int PROBE_FN(subgroup_check)(int per_elem, int poison, const uint32_t* pts, const uint8_t* inf, uint32_t n, uint32_t* err,
                             uint32_t* guards) {
  if (!stage_ok(n)) return PROBE_ERR_ARG;
  const uint32_t nerr = per_elem ? n : 1;
  Dev dv(poison);
  int& rc = dv.rc;
  AF* dpts = dv.get<AF>(B_PTS, n * sizeof(AF));
  uint8_t* dinf = dv.get<uint8_t>(B_INF, n);
  uint32_t* derr = dv.get<uint32_t>(B_ERR, nerr * 4, true);
  dv.put(dpts, pts, n * sizeof(AF));
  dv.put(dinf, inf, n);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t e) { L::subgroup_check(nullptr, dpts + i, dinf + i, c, derr + e); });
    dv.finish();
  }
  dv.take(err, derr, nerr * 4);
  dv.guards(guards);
  return rc;
}

// scal: n scalars of 8 words at `stride` words apart (n stride words); h0, h1: 4 n words
int PROBE_FN(glv_split)(int per_elem, int poison, const uint32_t* scal, uint32_t stride, uint32_t n, uint32_t* h0,
                        uint32_t* h1, uint32_t* guards) {
  if (!stage_ok(n) || stride < 8 || stride % 4) return PROBE_ERR_ARG;  // the kernel loads 16-byte vectors
  Dev dv(poison);
  int& rc = dv.rc;
  uint32_t* din = dv.get<uint32_t>(B_IN, (size_t)n * stride * 4);
  uint32_t* dh0 = dv.get<uint32_t>(B_H0, (size_t)n * 16);
  uint32_t* dh1 = dv.get<uint32_t>(B_H1, (size_t)n * 16);
  dv.put(din, scal, (size_t)n * stride * 4);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t) {
      L::glv_split(nullptr, din + (size_t)i * stride, stride, c, dh0 + 4 * (size_t)i, dh1 + 4 * (size_t)i);
    });
    dv.finish();
  }
  dv.take(h0, dh0, (size_t)n * 16);
  dv.take(h1, dh1, (size_t)n * 16);
  dv.guards(guards);
  return rc;
}

// src: n slots (in29: already in the accumulation's radix-29 form), src_inf: n bytes
int PROBE_FN(endo_points)(int in29, int per_elem, int poison, const uint32_t* src, const uint8_t* src_inf, uint32_t n,
                          uint32_t* dst, uint8_t* dst_inf, uint32_t* guards) {
  if (!stage_ok(n)) return PROBE_ERR_ARG;
  Dev dv(poison);
  int& rc = dv.rc;
  AF* dsrc = dv.get<AF>(B_IN, n * sizeof(AF));
  uint8_t* dsrc_inf = dv.get<uint8_t>(B_IN_INF, n);
  AF* ddst = dv.get<AF>(B_PTS, n * sizeof(AF));
  uint8_t* ddst_inf = dv.get<uint8_t>(B_INF, n);
  dv.put(dsrc, src, n * sizeof(AF));
  dv.put(dsrc_inf, src_inf, n);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t) {
      L::endo_points(nullptr, dsrc + i, dsrc_inf + i, c, ddst + i, ddst_inf + i, in29 != 0);
    });
    dv.finish();
  }
  dv.take(dst, ddst, n * sizeof(AF));
  dv.take(dst_inf, ddst_inf, n);
  dv.guards(guards);
  return rc;
}

// bytes: n scalars of 32 bytes; out: 8 n words
int PROBE_FN(convert_scalars)(int per_elem, int poison, const uint8_t* bytes, uint32_t n, uint32_t* out, uint32_t* err,
                              uint32_t* guards) {
  if (!stage_ok(n)) return PROBE_ERR_ARG;
  const uint32_t nerr = per_elem ? n : 1;
  Dev dv(poison);
  int& rc = dv.rc;
  uint8_t* din = dv.get<uint8_t>(B_IN, (size_t)n * 32);
  uint32_t* dout = dv.get<uint32_t>(B_OUT, (size_t)n * 32);
  uint32_t* derr = dv.get<uint32_t>(B_ERR, nerr * 4, true);
  dv.put(din, bytes, (size_t)n * 32);
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t e) {
      L::convert_scalars(nullptr, din + (size_t)i * 32, c, dout + 8 * (size_t)i, derr + e);
    });
    dv.finish();
  }
  dv.take(out, dout, (size_t)n * 32);
  dv.take(err, derr, nerr * 4);
  dv.guards(guards);
  return rc;
}

// res: n Xyzz records (field.hpp words); out: n uncompressed encodings
int PROBE_FN(encode_points)(int per_elem, int poison, const uint32_t* res, uint32_t n, uint8_t* out, uint32_t* guards) {
  if (!stage_ok(n)) return PROBE_ERR_ARG;
  constexpr size_t ENC = 8 * N32;
  Dev dv(poison);
  int& rc = dv.rc;
  XY* dres = dv.get<XY>(B_IN, n * sizeof(XY));
  uint8_t* dout = dv.get<uint8_t>(B_OUT, n * ENC);
  dv.put(dres, res, n * sizeof(XY));
  if (rc == 0) {
    each(per_elem != 0, n, [&](uint32_t i, uint32_t c, uint32_t) { L::encode_points(nullptr, dres + i, c, dout + i * ENC); });
    dv.finish();
  }
  dv.take(out, dout, n * ENC);
  dv.guards(guards);
  return rc;
}

#if KZ_CURVE == 0
int pointsprobe_words_1(const char*, int*, int*);
int pointsprobe_run_1(const char*, const void*, uint32_t, void*);
void pointsprobe_sizes_1(uint32_t*);
int pointsprobe_convert_points_1(int, int, int, const uint8_t*, uint32_t, uint32_t*, uint8_t*, uint32_t*, uint8_t*, uint32_t*,
                                 uint32_t*);
int pointsprobe_decompress_points_1(int, int, const uint8_t*, uint32_t, uint32_t*, uint8_t*, uint32_t*, uint32_t*);
int pointsprobe_compress_points_1(int, int, const uint8_t*, uint32_t, uint8_t*, uint32_t*);
int pointsprobe_subgroup_check_1(int, int, const uint32_t*, const uint8_t*, uint32_t, uint32_t*, uint32_t*);
int pointsprobe_glv_split_1(int, int, const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*);
int pointsprobe_endo_points_1(int, int, int, const uint32_t*, const uint8_t*, uint32_t, uint32_t*, uint8_t*, uint32_t*);
int pointsprobe_convert_scalars_1(int, int, const uint8_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*);
int pointsprobe_encode_points_1(int, int, const uint32_t*, uint32_t, uint8_t*, uint32_t*);

#define PROBE_API extern "C" __attribute__((visibility("default")))
// kzgmi_pointsprobe_<name>(curve, the call's arguments): the curve's instance, or PROBE_ERR_CURVE
#define PROBE_DISPATCH(name, ...)                            \
  if (curve == 0) return pointsprobe_##name##_0(__VA_ARGS__); \
  if (curve == 1) return pointsprobe_##name##_1(__VA_ARGS__); \
  return PROBE_ERR_CURVE
PROBE_API int kzgmi_pointsprobe_guard_words() { return B_COUNT; }
PROBE_API int kzgmi_pointsprobe_words(int curve, const char* op, int* in_words, int* out_words) {
  PROBE_DISPATCH(words, op, in_words, out_words);
}
PROBE_API int kzgmi_pointsprobe_run(int curve, const char* op, const void* host_in, uint32_t n_cases, void* host_out) {
  PROBE_DISPATCH(run, op, host_in, n_cases, host_out);
}
PROBE_API int kzgmi_pointsprobe_sizes(int curve, uint32_t* out) {
  if (curve == 0) return pointsprobe_sizes_0(out), 0;
  if (curve == 1) return pointsprobe_sizes_1(out), 0;
  return PROBE_ERR_CURVE;
}
PROBE_API int kzgmi_pointsprobe_convert_points(int curve, int form, int per_elem, int poison, const uint8_t* bytes, uint32_t n,
                                               uint32_t* pts, uint8_t* inf, uint32_t* img, uint8_t* img_inf, uint32_t* err,
                                               uint32_t* guards) {
  PROBE_DISPATCH(convert_points, form, per_elem, poison, bytes, n, pts, inf, img, img_inf, err, guards);
}
PROBE_API int kzgmi_pointsprobe_decompress_points(int curve, int per_elem, int poison, const uint8_t* bytes, uint32_t n,
                                                  uint32_t* pts, uint8_t* inf, uint32_t* err, uint32_t* guards) {
  PROBE_DISPATCH(decompress_points, per_elem, poison, bytes, n, pts, inf, err, guards);
}
PROBE_API int kzgmi_pointsprobe_compress_points(int curve, int per_elem, int poison, const uint8_t* in, uint32_t n, uint8_t* out,
                                                uint32_t* guards) {
  PROBE_DISPATCH(compress_points, per_elem, poison, in, n, out, guards);
}
PROBE_API int kzgmi_pointsprobe_subgroup_check(int curve, int per_elem, int poison, const uint32_t* pts, const uint8_t* inf,
                                               uint32_t n, uint32_t* err, uint32_t* guards) {
  PROBE_DISPATCH(subgroup_check, per_elem, poison, pts, inf, n, err, guards);
}
PROBE_API int kzgmi_pointsprobe_glv_split(int curve, int per_elem, int poison, const uint32_t* scal, uint32_t stride, uint32_t n,
                                          uint32_t* h0, uint32_t* h1, uint32_t* guards) {
  PROBE_DISPATCH(glv_split, per_elem, poison, scal, stride, n, h0, h1, guards);
}
PROBE_API int kzgmi_pointsprobe_endo_points(int curve, int in29, int per_elem, int poison, const uint32_t* src,
                                            const uint8_t* src_inf, uint32_t n, uint32_t* dst, uint8_t* dst_inf,
                                            uint32_t* guards) {
  PROBE_DISPATCH(endo_points, in29, per_elem, poison, src, src_inf, n, dst, dst_inf, guards);
}
PROBE_API int kzgmi_pointsprobe_convert_scalars(int curve, int per_elem, int poison, const uint8_t* bytes, uint32_t n,
                                                uint32_t* out, uint32_t* err, uint32_t* guards) {
  PROBE_DISPATCH(convert_scalars, per_elem, poison, bytes, n, out, err, guards);
}
PROBE_API int kzgmi_pointsprobe_encode_points(int curve, int per_elem, int poison, const uint32_t* res, uint32_t n, uint8_t* out,
                                              uint32_t* guards) {
  PROBE_DISPATCH(encode_points, per_elem, poison, res, n, out, guards);
}
#endif
