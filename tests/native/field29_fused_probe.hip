// Test-only probe of the fused product-and-subtract forms of csrc/field29.hpp
// (tests/test_gpu_field29_fused.py): mulsub29 and sqrsub3_29 with each bias constant csrc/msm.hpp
// passes them (acc_loop29: ACC_P, ACC_R, ACC_X3; x29_add: B2, C8), each wrapped in a trivial
// kernel.  A kernel does no more than load the operands from global memory, call the shipped
// function and store every output limb; no arithmetic lives here.  Built into
// kzgmi/libkzgmi_fusedprobe.so, one object per curve (-DKZ_CURVE=0/1); never linked into
// libkzgmi.so.
//
// Interface (ctypes, tests/fusedprobe.py):
//   kzgmi_fusedprobe_run(curve, op, host_in, n_cases, host_out)   0, or an error code below
// A case is three F29<Q> operands (3 Q::N limbs: a, b, x or a, s, t), the output one (Q::N limbs).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "field29.hpp"
#include "tower.hpp"

#if KZ_CURVE == 0
#define PROBE_CURVE_T ::kzgmi::Bls12_381
#define PROBE_RUN fusedprobe_run_0
#else
#define PROBE_CURVE_T ::kzgmi::Bn254
#define PROBE_RUN fusedprobe_run_1
#endif

enum { PROBE_ERR_CURVE = -1, PROBE_ERR_OP = -2, PROBE_ERR_COUNT = -3, PROBE_ERR_HIP = 1000 };

namespace {
using namespace kzgmi;
using Cv = PROBE_CURVE_T;
using Q = Fp29Of<Cv>;
using G = F29<Q>;
constexpr int N29 = Q::N;

__device__ G ld29(const uint32_t* p) {
  G r;
  _Pragma("unroll") for (int i = 0; i < N29; ++i) r.v[i] = p[i];
  return r;
}
__device__ void st29(uint32_t* p, const G& a) {
  _Pragma("unroll") for (int i = 0; i < N29; ++i) p[i] = a.v[i];
}

template <class Op>
__global__ void k_thread(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* a = in + (size_t)i * 3 * N29;
  st29(out + (size_t)i * N29, Op::run(ld29(a), ld29(a + N29), ld29(a + 2 * N29)));
}

#define DEF_OP(NAME, CALL)                                                     \
  struct NAME {                                                                \
    static __device__ G run(const G& a, const G& b, const G& c) { return CALL; } \
  };
DEF_OP(q_mulsub_ACC_P, mulsub29(a, b, c, Q::ACC_P))
DEF_OP(q_mulsub_ACC_R, mulsub29(a, b, c, Q::ACC_R))
DEF_OP(q_mulsub_B2, mulsub29(a, b, c, Q::B2))
DEF_OP(q_sqrsub3_ACC_X3, sqrsub3_29(a, b, c, Q::ACC_X3))
DEF_OP(q_sqrsub3_C8, sqrsub3_29(a, b, c, Q::C8))

using LaunchFn = hipError_t (*)(const uint32_t*, uint32_t*, uint32_t);
template <class Op> hipError_t launch_thread(const uint32_t* in, uint32_t* out, uint32_t n) {
  k_thread<Op><<<(n + 63) / 64, 64>>>(in, out, n);
  return hipGetLastError();
}
struct Entry {
  const char* name;
  LaunchFn launch;
};
const Entry kTable[] = {
    {"mulsub_ACC_P", &launch_thread<q_mulsub_ACC_P>},     {"mulsub_ACC_R", &launch_thread<q_mulsub_ACC_R>},
    {"mulsub_B2", &launch_thread<q_mulsub_B2>},           {"sqrsub3_ACC_X3", &launch_thread<q_sqrsub3_ACC_X3>},
    {"sqrsub3_C8", &launch_thread<q_sqrsub3_C8>},
};
}  // namespace

#define PROBE_HIP(call)                                  \
  do {                                                   \
    const hipError_t err_ = (call);                      \
    if (err_ != hipSuccess && rc == 0) rc = PROBE_ERR_HIP + (int)err_; \
  } while (0)

int PROBE_RUN(const char* op, const void* host_in, uint32_t n, void* host_out) {
  const Entry* e = nullptr;
  for (const Entry& t : kTable)
    if (std::strcmp(t.name, op) == 0) e = &t;
  if (!e) return PROBE_ERR_OP;
  if (n == 0 || n > (1u << 20)) return PROBE_ERR_COUNT;
  const size_t ib = (size_t)n * 3 * N29 * 4, ob = (size_t)n * N29 * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  int rc = 0;
  PROBE_HIP(hipMalloc(&din, ib));
  if (rc == 0) PROBE_HIP(hipMalloc(&dout, ob));
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
int fusedprobe_run_1(const char* op, const void* host_in, uint32_t n, void* host_out);

extern "C" __attribute__((visibility("default"))) int kzgmi_fusedprobe_run(int curve, const char* op, const void* host_in,
                                                                             uint32_t n_cases, void* host_out) {
  if (curve == 0) return fusedprobe_run_0(op, host_in, n_cases, host_out);
  if (curve == 1) return fusedprobe_run_1(op, host_in, n_cases, host_out);
  return PROBE_ERR_CURVE;
}
#endif
