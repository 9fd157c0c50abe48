// Test-only probe of the three prime-field layers (tests/test_gpu_field.py): the primitives of
// csrc/field.hpp, csrc/field29.hpp and csrc/lpfield.hpp listed in the op table below (plus the
// radix-29 record formulas of csrc/msm.hpp), each wrapped in a trivial kernel.  Helpers built
// from them (fp_dbl, fp_sqr, fp_mul3/4/8, fp_select, lp_add/sub/dbl/mul3/8/9, lp_norm64, lp_step*)
// are reached only through the ops that call them.  A kernel does no more than load the operands
// from global memory, call the shipped function and store every output word.  No arithmetic lives here: a function that
// cannot be called as it stands is not probed (acc_loop29's inline mixed addition; it is covered
// through its primitives).  Built into kzgmi/libkzgmi_fieldprobe.so, one object per curve
// (-DKZ_CURVE=0/1); never linked into libkzgmi.so.
//
// Interface (ctypes, tests/fieldprobe.py):
//   kzgmi_fieldprobe_words(curve, op, &in_words, &out_words)   words per case of an op
//   kzgmi_fieldprobe_run(curve, op, host_in, n_cases, host_out) 0, or an error code below
// Operand layouts, per case:
//   fp.* / fr.*  Fp<P> values, P::N words each (base field / scalar field of the curve)
//   f29.*        F29<Q> values, Q::N limbs each; a record is x, y, zz, zzz, inf (4 Q::N + 1 words)
//   lp.*         signed limb rows of 16 words (lane j of the row holds word j); one case per
//                16-lane row, four cases per 64-thread block, every lane active.  lp.xyzz_* take
//                Xyzz<Cv> records (4 P::N words) and use the whole wave for one case.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>
#include "field.hpp"
#include "field29.hpp"
#include "g1.hpp"
#include "lpfield.hpp"
#include "msm.hpp"

#if KZ_CURVE == 0
#define PROBE_CURVE_T ::kzgmi::Bls12_381
#define PROBE_RUN fieldprobe_run_0
#define PROBE_WORDS fieldprobe_words_0
#else
#define PROBE_CURVE_T ::kzgmi::Bn254
#define PROBE_RUN fieldprobe_run_1
#define PROBE_WORDS fieldprobe_words_1
#endif

enum { PROBE_ERR_CURVE = -1, PROBE_ERR_OP = -2, PROBE_ERR_COUNT = -3, PROBE_ERR_HIP = 1000 };

namespace {
using namespace kzgmi;
using Cv = PROBE_CURVE_T;
using Q = Fp29Of<Cv>;
using G = F29<Q>;
using LQ = LpQ<Cv>;
using FpB = Fp<typename Cv::FpP>;
constexpr int N29 = Q::N, N32 = Cv::FpP::N, REC = 4 * N29 + 1;

template <class P, class = void> struct has_mod2 : std::false_type {};
template <class P> struct has_mod2<P, std::void_t<decltype(P::MOD2)>> : std::true_type {};
template <class P, class = void> struct has_sqrt : std::false_type {};
template <class P> struct has_sqrt<P, std::void_t<decltype(P::SQRT_FIRST)>> : std::true_type {};

template <class P> __device__ Fp<P> ld(const uint32_t* p) {
  Fp<P> r;
  _Pragma("unroll") for (int i = 0; i < P::N; ++i) r.v[i] = p[i];
  return r;
}
template <class P> __device__ void st(uint32_t* p, const Fp<P>& a) {
  _Pragma("unroll") for (int i = 0; i < P::N; ++i) p[i] = a.v[i];
}
__device__ G ld29(const uint32_t* p) {
  G r;
  _Pragma("unroll") for (int i = 0; i < N29; ++i) r.v[i] = p[i];
  return r;
}
__device__ void st29(uint32_t* p, const G& a) {
  _Pragma("unroll") for (int i = 0; i < N29; ++i) p[i] = a.v[i];
}
__device__ X29<Q> ldrec(const uint32_t* p) {
  return {ld29(p), ld29(p + N29), ld29(p + 2 * N29), ld29(p + 3 * N29), p[4 * N29] != 0};
}
__device__ void strec(uint32_t* p, const X29<Q>& a) {
  st29(p, a.x); st29(p + N29, a.y); st29(p + 2 * N29, a.zz); st29(p + 3 * N29, a.zzz);
  p[4 * N29] = a.inf ? 1u : 0u;
}

// ---------------------------------------------------------------- one case per thread
template <class Op>
__global__ void k_thread(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Op::run(in + (size_t)i * Op::IN, out + (size_t)i * Op::OUT);
}

#define A(k) ld<P>(in + (k) * P::N)
#define DEF32(NAME, NIN, NOUT, ...)                                   \
  template <class P> struct NAME {                                    \
    static constexpr int IN = (NIN) * P::N, OUT = (NOUT);             \
    static __device__ void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__; } \
  };
DEF32(o_add, 2, P::N, st(out, fp_add(A(0), A(1))))
DEF32(o_sub, 2, P::N, st(out, fp_sub(A(0), A(1))))
DEF32(o_neg, 1, P::N, st(out, fp_neg(A(0))))
DEF32(o_mul, 2, P::N, st(out, fp_mul(A(0), A(1))))
DEF32(o_mul_ps, 2, P::N, st(out, fp_mul_ps(A(0), A(1))))
DEF32(o_csub_mod, 1, P::N, st(out, fp_csub<P>(A(0), P::MOD)))
DEF32(o_csub_mod2, 1, P::N, st(out, fp_csub<P>(A(0), P::MOD2)))
DEF32(o_to_mont, 1, P::N, st(out, fp_to_mont(A(0))))
DEF32(o_from_mont, 1, P::N, st(out, fp_from_mont(A(0))))
DEF32(o_raw_lt_mod, 1, 1, out[0] = fp_raw_lt_mod(A(0)) ? 1u : 0u)
DEF32(o_mul_lazy, 2, P::N, st(out, fp_mul_lazy(A(0), A(1))))
DEF32(o_mul2_lazy, 4, P::N, st(out, fp_mul2_lazy(A(0), A(1), A(2), A(3))))
DEF32(o_add_lazy, 2, P::N, st(out, fp_add_lazy(A(0), A(1))))
DEF32(o_sub_lazy, 2, P::N, st(out, fp_sub_lazy(A(0), A(1))))
DEF32(o_neg_lazy, 1, P::N, st(out, fp_neg_lazy(A(0))))
DEF32(o_rsub_mod, 1, P::N, st(out, fp_rsub_mod(A(0))))
DEF32(o_is_zero_lazy, 1, 1, out[0] = fp_is_zero_lazy(A(0)) ? 1u : 0u)
DEF32(o_canon, 1, P::N, st(out, fp_canon(A(0))))
DEF32(o_inv, 1, P::N, st(out, fp_inv(A(0))))
DEF32(o_pow_sqrt, 1, P::N, st(out, fp_pow_sqrt(A(0))))
#undef A

#define B(k) ld29(in + (k) * N29)
#define DEF29(NAME, NIN, NOUT, ...)                                   \
  struct NAME {                                                       \
    static constexpr int IN = (NIN), OUT = (NOUT);                    \
    static __device__ void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__; } \
  };
DEF29(q_mul, 2 * N29, N29, st29(out, mul29(B(0), B(1))))
DEF29(q_sqr, N29, N29, st29(out, sqr29(B(0))))
DEF29(q_mul2, 4 * N29, N29, st29(out, mul2_29(B(0), B(1), B(2), B(3))))
// the accumulation's Y3: R (Q - X3) - Y1 PPP with -PPP = neg_lazy29(PPP, ACC_PPP); operands R, D, y, PPP
DEF29(q_mul2_neg, 4 * N29, N29, st29(out, mul2_29(B(0), B(1), B(2), neg_lazy29(B(3), Q::ACC_PPP))))
#define DEF_SUB(NAME, BIAS) DEF29(NAME, 2 * N29, N29, st29(out, sub29(B(0), B(1), Q::BIAS)))
DEF_SUB(q_sub_B2, B2) DEF_SUB(q_sub_B4, B4) DEF_SUB(q_sub_B8, B8) DEF_SUB(q_sub_B16, B16)
DEF_SUB(q_sub_ACC_NEG, ACC_NEG) DEF_SUB(q_sub_ACC_P, ACC_P) DEF_SUB(q_sub_ACC_R, ACC_R)
DEF_SUB(q_sub_ACC_QX, ACC_QX) DEF_SUB(q_sub_DBL_X, DBL_X) DEF_SUB(q_sub_DBL_QX, DBL_QX)
DEF_SUB(q_sub_DBL_Y, DBL_Y)
DEF_SUB(q_sub_B32, B32) DEF_SUB(q_sub_B64, B64)  // csrc/points.hpp's Jacobian formulas (BLS12-381)
DEF29(q_sub3_ACC_X3, 3 * N29, N29, st29(out, sub3_29(B(0), B(1), B(2), Q::ACC_X3)))
DEF29(q_add3, 3 * N29, N29, st29(out, add3_29(B(0), B(1), B(2))))
DEF29(q_canon, N29, N29, st29(out, canon29(B(0))))
DEF29(q_is_zero, N29, 1, out[0] = is_zero29(B(0)) ? 1u : 0u)
DEF29(q_is_zero_mf, N29, 1, out[0] = is_zero29_mf(B(0)) ? 1u : 0u)
DEF29(q_limbs29, N32, N29, st29(out, limbs29<Q>(ld<typename Cv::FpP>(in).v)))
DEF29(q_words32, N29, N32, FpB r; words32<Q>(B(0), r.v); st(out, r))
DEF29(q_fp_to29, N32, N29, st29(out, fp_to29<Q>(ld<typename Cv::FpP>(in))))
DEF29(q_fp_from29, N29, N32, st(out, fp_from29<Q, typename Cv::FpP>(B(0))))
DEF29(q_x29_add, 2 * REC, REC, strec(out, x29_add<Cv, Q>(ldrec(in), ldrec(in + REC))))
DEF29(q_x29_dbl, REC, REC, strec(out, x29_dbl<Q>(ldrec(in))))
#undef B

// dbl_affine29 writes ZZ, ZZZ to the caller's LDS columns at stride 256 words, as in acc_loop29
struct q_dbl_affine {
  static constexpr int IN = 2 * N29, OUT = 4 * N29;
};
__global__ __launch_bounds__(256) void k_dbl_affine(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  __shared__ uint32_t s_zz[N29][256], s_zzz[N29][256];
  const uint32_t tx = threadIdx.x, i = blockIdx.x * 256 + tx;
  if (i >= n) return;
  const uint32_t* a = in + (size_t)i * q_dbl_affine::IN;
  uint32_t* o = out + (size_t)i * q_dbl_affine::OUT;
  const Xy29<Q> d = dbl_affine29<Q>(ld29(a), ld29(a + N29), &s_zz[0][tx], &s_zzz[0][tx]);
  st29(o, d.x);
  st29(o + N29, d.y);
  _Pragma("unroll") for (int k = 0; k < N29; ++k) {
    o[2 * N29 + k] = s_zz[k][tx];
    o[3 * N29 + k] = s_zzz[k][tx];
  }
}

// ---------------------------------------------------------------- lane-parallel: whole waves
template <class Op>
__global__ __launch_bounds__(64) void k_lp(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const LpCtx<Cv> c = lp_ctx<Cv>();
  const size_t cs = Op::WAVE ? (size_t)blockIdx.x : (size_t)4 * blockIdx.x + c.row;
  Op::run(c, in + cs * Op::IN, out + cs * Op::OUT, (int)(threadIdx.x & 15));
}
#define L(k) ((int32_t)in[(k) * 16 + j])
#define DEFLP(NAME, WHOLE, NIN, NOUT, ...)                            \
  struct NAME {                                                       \
    static constexpr bool WAVE = (WHOLE);                             \
    static constexpr int IN = (NIN), OUT = (NOUT);                    \
    static __device__ void run(const LpCtx<Cv>& c, const uint32_t* in, uint32_t* out, int j) { __VA_ARGS__; } \
  };
DEFLP(l_norm, false, 16, 16, out[j] = (uint32_t)lp_norm(c, L(0)))
DEFLP(l_mul, false, 32, 16, out[j] = (uint32_t)lp_mul(c, L(0), L(1)))
DEFLP(l_reduce, false, 16, 16, out[j] = (uint32_t)lp_reduce(c, L(0)))
DEFLP(l_row_is_zero, false, 16, 1, const bool z = lp_row_is_zero(c, L(0)); if (j == 0) out[0] = z ? 1u : 0u)
// lp_canon reads row 0: each row's value is handed to every row in turn (ds_bpermute, lp_row)
DEFLP(l_to_fp, false, 16, N32, const int32_t v = L(0);
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {
        const FpB f = lp_to_fp(c, lp_row(c, v, r));
        if (c.row == r && j == 0) st(out, f);
      })
// lp_canon + lp_pack on the row itself: v mod p as words
DEFLP(l_canon, false, 16, N32, const int32_t v = L(0);
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {
        int64_t l[LQ::N];
        lp_canon<Cv>(lp_row(c, v, r), l);
        const FpB f = lp_pack<Cv>(l);
        if (c.row == r && j == 0) st(out, f);
      })
DEFLP(l_raw_from_words, false, N32, 16, out[j] = (uint32_t)lp_raw_from_words<Cv>(in))
DEFLP(l_xyzz_dbl, true, 4 * N32, 4 * N32, (void)j;
      lp_store_xyzz(c, reinterpret_cast<Xyzz<Cv>*>(out),
                    lp_xyzz_dbl(c, lp_load_xyzz(c, reinterpret_cast<const Xyzz<Cv>*>(in)))))
DEFLP(l_xyzz_add, true, 8 * N32, 4 * N32, (void)j;
      lp_store_xyzz(c, reinterpret_cast<Xyzz<Cv>*>(out),
                    lp_xyzz_add(c, lp_load_xyzz(c, reinterpret_cast<const Xyzz<Cv>*>(in)),
                                lp_load_xyzz(c, reinterpret_cast<const Xyzz<Cv>*>(in) + 1))))
#undef L

// ---------------------------------------------------------------- op table and host side
using LaunchFn = hipError_t (*)(const uint32_t*, uint32_t*, uint32_t);
struct Entry {
  std::string name;
  int in, out;
  int group;  // cases per launch unit: 1, or 4 (row ops: n must be a multiple of 4)
  LaunchFn launch;
};

template <class Op> hipError_t launch_thread(const uint32_t* in, uint32_t* out, uint32_t n) {
  k_thread<Op><<<(n + 63) / 64, 64>>>(in, out, n);
  return hipGetLastError();
}
hipError_t launch_dbl_affine(const uint32_t* in, uint32_t* out, uint32_t n) {
  k_dbl_affine<<<(n + 255) / 256, 256>>>(in, out, n);
  return hipGetLastError();
}
template <class Op> hipError_t launch_lp(const uint32_t* in, uint32_t* out, uint32_t n) {
  k_lp<Op><<<Op::WAVE ? n : n / 4, 64>>>(in, out);
  return hipGetLastError();
}

template <class Op> void add_thread(std::vector<Entry>& t, const std::string& name) {
  t.push_back({name, Op::IN, Op::OUT, 1, &launch_thread<Op>});
}
template <class Op> void add_lp(std::vector<Entry>& t, const std::string& name) {
  t.push_back({name, Op::IN, Op::OUT, Op::WAVE ? 1 : 4, &launch_lp<Op>});
}

template <class P> void add_fp_ops(std::vector<Entry>& t, const std::string& pre) {
  add_thread<o_add<P>>(t, pre + "add");
  add_thread<o_sub<P>>(t, pre + "sub");
  add_thread<o_neg<P>>(t, pre + "neg");
  add_thread<o_mul<P>>(t, pre + "mul");
  add_thread<o_mul_ps<P>>(t, pre + "mul_ps");
  add_thread<o_csub_mod<P>>(t, pre + "csub_mod");
  add_thread<o_to_mont<P>>(t, pre + "to_mont");
  add_thread<o_from_mont<P>>(t, pre + "from_mont");
  add_thread<o_raw_lt_mod<P>>(t, pre + "raw_lt_mod");
  add_thread<o_inv<P>>(t, pre + "inv");
  if constexpr (has_mod2<P>::value) {  // the lazy [0, 2p) forms exist for the base fields only
    add_thread<o_csub_mod2<P>>(t, pre + "csub_mod2");
    add_thread<o_mul_lazy<P>>(t, pre + "mul_lazy");
    add_thread<o_mul2_lazy<P>>(t, pre + "mul2_lazy");
    add_thread<o_add_lazy<P>>(t, pre + "add_lazy");
    add_thread<o_sub_lazy<P>>(t, pre + "sub_lazy");
    add_thread<o_neg_lazy<P>>(t, pre + "neg_lazy");
    add_thread<o_rsub_mod<P>>(t, pre + "rsub_mod");
    add_thread<o_is_zero_lazy<P>>(t, pre + "is_zero_lazy");
    add_thread<o_canon<P>>(t, pre + "canon");
  }
  if constexpr (has_sqrt<P>::value) add_thread<o_pow_sqrt<P>>(t, pre + "pow_sqrt");
}

const std::vector<Entry>& table() {
  static const std::vector<Entry> t = [] {
    std::vector<Entry> v;
    add_fp_ops<typename Cv::FpP>(v, "fp.");
    add_fp_ops<typename Cv::FrP>(v, "fr.");
    add_thread<q_mul>(v, "f29.mul");
    add_thread<q_sqr>(v, "f29.sqr");
    add_thread<q_mul2>(v, "f29.mul2");
    add_thread<q_mul2_neg>(v, "f29.mul2_neg");
    add_thread<q_sub_B2>(v, "f29.sub_B2");
    add_thread<q_sub_B4>(v, "f29.sub_B4");
    add_thread<q_sub_B8>(v, "f29.sub_B8");
    add_thread<q_sub_B16>(v, "f29.sub_B16");
    add_thread<q_sub_ACC_NEG>(v, "f29.sub_ACC_NEG");
    add_thread<q_sub_ACC_P>(v, "f29.sub_ACC_P");
    add_thread<q_sub_ACC_R>(v, "f29.sub_ACC_R");
    add_thread<q_sub_ACC_QX>(v, "f29.sub_ACC_QX");
    add_thread<q_sub_DBL_X>(v, "f29.sub_DBL_X");
    add_thread<q_sub_DBL_QX>(v, "f29.sub_DBL_QX");
    add_thread<q_sub_DBL_Y>(v, "f29.sub_DBL_Y");
    if constexpr (Cv::ID == 0) {
      add_thread<q_sub_B32>(v, "f29.sub_B32");
      add_thread<q_sub_B64>(v, "f29.sub_B64");
    }
    add_thread<q_sub3_ACC_X3>(v, "f29.sub3_ACC_X3");
    add_thread<q_add3>(v, "f29.add3");
    add_thread<q_canon>(v, "f29.canon");
    add_thread<q_is_zero>(v, "f29.is_zero");
    add_thread<q_is_zero_mf>(v, "f29.is_zero_mf");
    add_thread<q_limbs29>(v, "f29.limbs29");
    add_thread<q_words32>(v, "f29.words32");
    add_thread<q_fp_to29>(v, "f29.fp_to29");
    add_thread<q_fp_from29>(v, "f29.fp_from29");
    add_thread<q_x29_add>(v, "f29.x29_add");
    add_thread<q_x29_dbl>(v, "f29.x29_dbl");
    v.push_back({"f29.dbl_affine", q_dbl_affine::IN, q_dbl_affine::OUT, 1, &launch_dbl_affine});
    add_lp<l_norm>(v, "lp.norm");
    add_lp<l_mul>(v, "lp.mul");
    add_lp<l_reduce>(v, "lp.reduce");
    add_lp<l_row_is_zero>(v, "lp.row_is_zero");
    add_lp<l_to_fp>(v, "lp.to_fp");
    add_lp<l_canon>(v, "lp.canon");
    add_lp<l_raw_from_words>(v, "lp.raw_from_words");
    add_lp<l_xyzz_dbl>(v, "lp.xyzz_dbl");
    add_lp<l_xyzz_add>(v, "lp.xyzz_add");
    return v;
  }();
  return t;
}

const Entry* find(const char* op) {
  for (const Entry& e : table())
    if (e.name == op) return &e;
  return nullptr;
}
}  // namespace

int PROBE_WORDS(const char* op, int* in_words, int* out_words) {
  const Entry* e = find(op);
  if (!e) return PROBE_ERR_OP;
  *in_words = e->in;
  *out_words = e->out;
  return 0;
}

#define PROBE_HIP(call)                                  \
  do {                                                   \
    const hipError_t err_ = (call);                      \
    if (err_ != hipSuccess && rc == 0) rc = PROBE_ERR_HIP + (int)err_; \
  } while (0)

int PROBE_RUN(const char* op, const void* host_in, uint32_t n, void* host_out) {
  const Entry* e = find(op);
  if (!e) return PROBE_ERR_OP;
  if (n == 0 || n > (1u << 20) || n % e->group) return PROBE_ERR_COUNT;
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

#if KZ_CURVE == 0
int fieldprobe_run_1(const char* op, const void* host_in, uint32_t n, void* host_out);
int fieldprobe_words_1(const char* op, int* in_words, int* out_words);

extern "C" __attribute__((visibility("default"))) int kzgmi_fieldprobe_run(int curve, const char* op, const void* host_in,
                                                                             uint32_t n_cases, void* host_out) {
  if (curve == 0) return fieldprobe_run_0(op, host_in, n_cases, host_out);
  if (curve == 1) return fieldprobe_run_1(op, host_in, n_cases, host_out);
  return PROBE_ERR_CURVE;
}
extern "C" __attribute__((visibility("default"))) int kzgmi_fieldprobe_words(int curve, const char* op, int* in_words,
                                                                               int* out_words) {
  if (curve == 0) return fieldprobe_words_0(op, in_words, out_words);
  if (curve == 1) return fieldprobe_words_1(op, in_words, out_words);
  return PROBE_ERR_CURVE;
}
#endif
