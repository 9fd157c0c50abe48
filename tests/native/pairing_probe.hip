// Test-only probe of the workgroup-parallel pairing interpreter (tests/test_gpu_pairing.py):
// csrc/pairing_par.hpp's par_load_consts / par_run / par_load_point and csrc/pairing.hpp's
// k_precompute_lines, run as shipped on a caller-supplied program and register image.  A probe
// kernel does no more than load, call the shipped device functions and store; no field
// arithmetic lives here.  Built into kzgmi/libkzgmi_pairingprobe.so, one object per curve
// (-DKZ_CURVE=0/1); never linked into libkzgmi.so.
//
// Interface (ctypes, tests/pairingprobe.py); every function returns 0 or an error code below:
//   kzgmi_pairingprobe_info_words()                  the length of info's output, in ints
//   kzgmi_pairingprobe_info(curve, out)
//       NPROG, NR, R_K, R_E, R_P, R_SCAL, R_G, R_RES, OP_COUNT, PAR_THREADS, num_lines, then NP of
//       every op and NO of every op, as compiled (no GPU needed)
//   kzgmi_pairingprobe_run_program(curve, force_generic, poison, program, n_ins, n_cases, rows_in,
//                                  rows_out, fast_ok_out)
//       One 1024-thread block per case: every LDS word set to `poison`, par_load_consts, the
//       case's image of rows [R_P, NR) (16 signed limbs a row) into S.R, the program (n_ins instructions of 10 uint16, padded here to
//       NPROG with the self-copy K_COPY R_G -> R_G) into S.prog, S.fast_ok cleared if
//       force_generic, par_run with both pairs skipped (it initialises only the E registers),
//       rows [R_P, NR) and S.fast_ok out.  The bytecode is validated on the host first
//       (check_program): a program that fails is not launched.
//   kzgmi_pairingprobe_run_pairing(curve, force_generic, poison, n_cases, xyzz_pairs, g2_pairs, q_inf,
//                                  verdict_out, rows_out)
//       Per case two Xyzz records (field.hpp words), two affine G2 points (Montgomery words) and
//       two q_inf bytes: k_precompute_lines, then the LDS poison and the body of
//       k_pairing_check_par; the verdict and the twelve R_RES rows out.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "pairing_par.hpp"

#if KZ_CURVE == 0
#define PROBE_CURVE_T ::kzgmi::Bls12_381
#define PROBE_FN(name) pairingprobe_##name##_0
#else
#define PROBE_CURVE_T ::kzgmi::Bn254
#define PROBE_FN(name) pairingprobe_##name##_1
#endif

enum { PROBE_ERR_CURVE = -1, PROBE_ERR_PROGRAM = -2, PROBE_ERR_COUNT = -3, PROBE_ERR_HIP = 1000 };
constexpr int INFO_HEAD = 11;
constexpr int MAX_CASES = 4096, MAX_PAIRINGS = 64;

namespace {
using namespace kzgmi;
using Cv = PROBE_CURVE_T;
using I = typename ProgInfo<Cv>::I;
constexpr int NIMG = I::NR - I::R_P;  // rows of the image: P, scalars, G0..G15
constexpr int kNP[OP_COUNT] = {I::MUL_NP, I::SQR_NP, I::CYC_NP, I::CONJ_NP, I::LINE_NP, I::LL_NP, I::FROB1_NP,
                               I::FROB2_NP, I::FROB3_NP, I::INV_NORM_NP, I::INV6_T_NP, I::INV6_D_NP, I::INV2_N_NP,
                               I::INV2_FIN_NP, I::INV6_FIN_NP, I::INV12_FIN_NP, I::LEVAL_NP};
constexpr int kNO[OP_COUNT] = {I::MUL_NO, I::SQR_NO, I::CYC_NO, I::CONJ_NO, I::LINE_NO, I::LL_NO, I::FROB1_NO,
                               I::FROB2_NO, I::FROB3_NO, I::INV_NORM_NO, I::INV6_T_NO, I::INV6_D_NO, I::INV2_N_NO,
                               I::INV2_FIN_NO, I::INV6_FIN_NO, I::INV12_FIN_NO, I::LEVAL_NO};

// rows an op reads from its A and B blocks and its sizes, from the compiled tables: the widest
// index of source 0 / 1 over every factor and output list
__global__ void k_op_shapes(int* __restrict__ shapes) {  // [OP_COUNT][4]: wa, wb, np, no
  const int op = threadIdx.x;
  if (op >= OP_COUNT) return;
  const OpDesc d = OpTables<Cv>::get(op);
  const uint8_t* code = OpTables<Cv>::code();
  int w[2] = {0, 0};
  for (int l = 0; l < 2 * d.np + d.no; ++l) {
    for (int t = l < 2 * d.np ? d.P[l] : d.O[l - 2 * d.np]; code[t] != 255; ++t) {
      const int src = code[t] >> 6, i = code[t] & 63;
      if (src < 2 && i + 1 > w[src]) w[src] = i + 1;
    }
  }
  shapes[4 * op] = w[0];
  shapes[4 * op + 1] = w[1];
  shapes[4 * op + 2] = d.np;
  shapes[4 * op + 3] = d.no;
}

// Every word of the kernel's LDS set to `poison` before anything runs: the shipped kernel starts on
// whatever the previous workgroup left there, so a result that depends on a word nothing wrote
// shows up as a difference between two poisons instead of once in a while.
__device__ void poison_lds(ParShared<Cv>& S, uint32_t poison) {
  static_assert(sizeof(ParShared<Cv>) % sizeof(uint32_t) == 0, "ParShared is a whole number of words");
  uint32_t* w = reinterpret_cast<uint32_t*>(&S);
  for (int i = threadIdx.x; i < (int)(sizeof(ParShared<Cv>) / sizeof(uint32_t)); i += PAR_THREADS) w[i] = poison;
  __syncthreads();
}

__global__ void __launch_bounds__(PAR_THREADS) k_run_program(const uint16_t* __restrict__ prog, int force_generic,
                                                             uint32_t poison,
                                                             const int32_t* __restrict__ rows_in,
                                                             int32_t* __restrict__ rows_out,
                                                             int* __restrict__ fast_ok_out) {
  __shared__ ParShared<Cv> S;
  poison_lds(S, poison);
  const LpCtx<Cv> c = lp_ctx<Cv>();
  par_load_consts(S, c);
  const int32_t* in = rows_in + (size_t)blockIdx.x * NIMG * 16;
  int32_t* out = rows_out + (size_t)blockIdx.x * NIMG * 16;
  for (int i = threadIdx.x; i < NIMG * 16; i += PAR_THREADS) S.R[I::R_P + (i >> 4)][i & 15] = in[i];
  for (int i = threadIdx.x; i < I::NPROG * 10; i += PAR_THREADS) S.prog[i] = prog[i];
  if (force_generic && threadIdx.x == 0) S.fast_ok = 0;
  __syncthreads();
  (void)par_run(S, c, static_cast<const Line<Cv>*>(nullptr), true, true);  // skipped pairs read no line
  for (int i = threadIdx.x; i < NIMG * 16; i += PAR_THREADS) out[i] = S.R[I::R_P + (i >> 4)][i & 15];
  if (threadIdx.x == 0) fast_ok_out[blockIdx.x] = S.fast_ok;
}

// the body of k_pairing_check_par, one case per block
__global__ void __launch_bounds__(PAR_THREADS) k_run_pairing(const Xyzz<Cv>* __restrict__ res_all,
                                                             const Line<Cv>* __restrict__ lines_all,
                                                             const uint8_t* __restrict__ q_inf_all, int force_generic,
                                                             uint32_t poison, int* __restrict__ ok,
                                                             int32_t* __restrict__ rows_out) {
  __shared__ ParShared<Cv> S;
  const Xyzz<Cv>* res = res_all + 2 * (size_t)blockIdx.x;
  const Line<Cv>* lines = lines_all + 2 * (size_t)num_lines<Cv>() * blockIdx.x;
  const uint8_t* q_inf = q_inf_all + 2 * (size_t)blockIdx.x;
  poison_lds(S, poison);
  const LpCtx<Cv> c = lp_ctx<Cv>();
  par_load_consts(S, c);
  if (force_generic && threadIdx.x == 0) S.fast_ok = 0;
  const int row = threadIdx.x >> 4;
  if (row < 2) par_load_point(S, c, &res[row], row, row == 1);
  __syncthreads();
  const bool s0 = q_inf[0] != 0 || res[0].zz.is_zero();
  const bool s1 = q_inf[1] != 0 || res[1].zz.is_zero();
  const bool r = par_run(S, c, lines, s0, s1);
  if (threadIdx.x == 0) ok[blockIdx.x] = r ? 1 : 0;
  int32_t* out = rows_out + (size_t)blockIdx.x * 12 * 16;
  for (int i = threadIdx.x; i < 12 * 16; i += PAR_THREADS) out[i] = S.R[I::R_RES + (i >> 4)][i & 15];
}

#define PROBE_HIP(call)                                                \
  do {                                                                 \
    const hipError_t err_ = (call);                                    \
    if (err_ != hipSuccess && rc == 0) rc = PROBE_ERR_HIP + (int)err_; \
  } while (0)

struct Bufs {  // device allocations of one call, freed on every path
  std::vector<void*> p;
  template <class T> T* get(size_t bytes, int& rc) {
    void* d = nullptr;
    PROBE_HIP(hipMalloc(&d, bytes ? bytes : 1));
    if (d) p.push_back(d);
    return static_cast<T*>(d);
  }
  ~Bufs() {
    for (void* d : p) (void)hipFree(d);
  }
};

int op_shapes(int (&shapes)[OP_COUNT][4]) {
  static int cached[OP_COUNT][4];
  static bool have = false;
  int rc = 0;
  if (!have) {
    Bufs b;
    int* d = b.get<int>(sizeof(cached), rc);
    if (rc == 0) {
      k_op_shapes<<<1, 64>>>(d);
      PROBE_HIP(hipGetLastError());
    }
    if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
    if (rc == 0) PROBE_HIP(hipMemcpy(cached, d, sizeof(cached), hipMemcpyDeviceToHost));
    if (rc) return rc;
    have = true;
  }
  for (int op = 0; op < OP_COUNT; ++op)
    for (int k = 0; k < 4; ++k) shapes[op][k] = cached[op][k];
  return 0;
}

// a round's products fit S.prod (two per row at most) and its outputs the rows, one each
bool round_fits(const int* s1, const int* s2) {
  const int np = s1[2] + (s2 ? s2[2] : 0), no = s1[3] + (s2 ? s2[3] : 0);
  return np <= 2 * PAR_ROWS && np <= 128 && no <= PAR_ROWS;
}

bool block_ok(int start, int width) { return width == 0 || (start >= 0 && start + width <= I::NR); }

// every register block an instruction touches, as a range of the op's compiled widths, lies in [0, NR)
bool check_program(const uint16_t* prog, int n_ins, const int (&shapes)[OP_COUNT][4]) {
  if (n_ins < 0 || n_ins > I::NPROG) return false;
  auto half = [&](const uint16_t* h) {  // op, a, b, out
    if (h[0] >= OP_COUNT) return false;
    const int* s = shapes[h[0]];
    if (s[1] > 0 && h[2] == R_NONE) return false;
    return block_ok(h[1], s[0]) && block_ok(h[2] == R_NONE ? 0 : h[2], s[1]) && block_ok(h[3], s[3]);
  };
  for (int k = 0; k < n_ins; ++k) {
    const uint16_t* ins = prog + 10 * k;
    switch (ins[0]) {
      case K_ROUND:  // (half: op in range, so shapes[] may be indexed after it)
        if (!half(ins + 1) || !round_fits(shapes[ins[1]], nullptr)) return false;
        break;
      case K_ROUND2:
        if (!half(ins + 1) || !half(ins + 5) || !round_fits(shapes[ins[1]], shapes[ins[5]])) return false;
        break;
      case K_COPY:
        if (!block_ok(ins[2], 12) || !block_ok(ins[4], 12)) return false;
        break;
      case K_INV:
        if (!block_ok(ins[2], 1) || !block_ok(ins[4], 1)) return false;
        break;
      case K_CYCRUN: {
        const int* s = shapes[OP_CYC];
        if (ins[1] < 1 || ins[1] > 64 || !round_fits(s, nullptr)) return false;
        if (!block_ok(ins[2], s[0]) || !block_ok(ins[2], s[3])) return false;  // s0 is read; u, v read and written
        if (!block_ok(ins[3], s[0]) || !block_ok(ins[3], s[3])) return false;
        if (!block_ok(ins[4], s[0]) || !block_ok(ins[4], s[3])) return false;
        break;
      }
      default:
        return false;
    }
  }
  return true;
}
}  // namespace

int PROBE_FN(info)(int* out) {
  const int head[INFO_HEAD] = {I::NPROG, I::NR, I::R_K, I::R_E, I::R_P, I::R_SCAL, I::R_G, I::R_RES,
                               OP_COUNT, PAR_THREADS, num_lines<Cv>()};
  for (int k = 0; k < INFO_HEAD; ++k) out[k] = head[k];
  for (int k = 0; k < OP_COUNT; ++k) {
    out[INFO_HEAD + k] = kNP[k];
    out[INFO_HEAD + OP_COUNT + k] = kNO[k];
  }
  return 0;
}

int PROBE_FN(run_program)(int force_generic, uint32_t poison, const uint16_t* program, int n_ins, int n_cases,
                          const int32_t* rows_in,
                          int32_t* rows_out, int* fast_ok_out) {
  if (n_cases < 1 || n_cases > MAX_CASES) return PROBE_ERR_COUNT;
  int shapes[OP_COUNT][4];
  int rc = op_shapes(shapes);
  if (rc) return rc;
  for (int op = 0; op < OP_COUNT; ++op)  // the widths came from the same tables as the compiled sizes
    if (shapes[op][2] != kNP[op] || shapes[op][3] != kNO[op])
      return PROBE_ERR_PROGRAM;
  if (!check_program(program, n_ins, shapes)) return PROBE_ERR_PROGRAM;
  std::vector<uint16_t> prog((size_t)I::NPROG * 10, 0);
  for (int k = 0; k < I::NPROG; ++k) {
    uint16_t* ins = &prog[10 * (size_t)k];
    if (k < n_ins) {
      for (int j = 0; j < 10; ++j) ins[j] = program[10 * (size_t)k + j];
    } else {  // no-op: a register block copied onto itself
      ins[0] = K_COPY; ins[2] = I::R_G; ins[3] = R_NONE; ins[4] = I::R_G;
    }
  }
  const size_t img = (size_t)n_cases * NIMG * 16 * sizeof(int32_t);
  Bufs b;
  uint16_t* dprog = b.get<uint16_t>(prog.size() * sizeof(uint16_t), rc);
  int32_t* din = b.get<int32_t>(img, rc);
  int32_t* dout = b.get<int32_t>(img, rc);
  int* dfast = b.get<int>((size_t)n_cases * sizeof(int), rc);
  if (rc == 0) PROBE_HIP(hipMemcpy(dprog, prog.data(), prog.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  if (rc == 0) PROBE_HIP(hipMemcpy(din, rows_in, img, hipMemcpyHostToDevice));
  if (rc == 0) PROBE_HIP(hipMemset(dout, 0xA5, img));  // an output word the kernel skips shows up
  if (rc == 0) PROBE_HIP(hipMemset(dfast, 0xA5, (size_t)n_cases * sizeof(int)));
  if (rc == 0) {
    k_run_program<<<n_cases, PAR_THREADS>>>(dprog, force_generic, poison, din, dout, dfast);
    PROBE_HIP(hipGetLastError());
  }
  if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
  if (rc == 0) PROBE_HIP(hipMemcpy(rows_out, dout, img, hipMemcpyDeviceToHost));
  if (rc == 0) PROBE_HIP(hipMemcpy(fast_ok_out, dfast, (size_t)n_cases * sizeof(int), hipMemcpyDeviceToHost));
  return rc;
}

int PROBE_FN(run_pairing)(int force_generic, uint32_t poison, int n_cases, const void* xyzz_pairs, const void* g2_pairs,
                          const uint8_t* q_inf, int* verdict_out, int32_t* rows_out) {
  if (n_cases < 1 || n_cases > MAX_PAIRINGS) return PROBE_ERR_COUNT;
  constexpr int NL = num_lines<Cv>();
  const size_t n = (size_t)n_cases, rows = n * 12 * 16 * sizeof(int32_t);
  int rc = 0;
  Bufs b;
  Xyzz<Cv>* dres = b.get<Xyzz<Cv>>(2 * n * sizeof(Xyzz<Cv>), rc);
  G2Aff<Cv>* dq = b.get<G2Aff<Cv>>(2 * n * sizeof(G2Aff<Cv>), rc);
  Line<Cv>* dlines = b.get<Line<Cv>>(2 * n * NL * sizeof(Line<Cv>), rc);
  uint8_t* dinf = b.get<uint8_t>(2 * n, rc);
  int* dok = b.get<int>(n * sizeof(int), rc);
  int32_t* dout = b.get<int32_t>(rows, rc);
  if (rc == 0) PROBE_HIP(hipMemcpy(dres, xyzz_pairs, 2 * n * sizeof(Xyzz<Cv>), hipMemcpyHostToDevice));
  if (rc == 0) PROBE_HIP(hipMemcpy(dq, g2_pairs, 2 * n * sizeof(G2Aff<Cv>), hipMemcpyHostToDevice));
  if (rc == 0) PROBE_HIP(hipMemcpy(dinf, q_inf, 2 * n, hipMemcpyHostToDevice));
  if (rc == 0) PROBE_HIP(hipMemset(dok, 0xA5, n * sizeof(int)));
  if (rc == 0) PROBE_HIP(hipMemset(dout, 0xA5, rows));
  for (size_t k = 0; k < n && rc == 0; ++k) {
    k_precompute_lines<Cv><<<1, 64>>>(dq + 2 * k, dlines + 2 * k * NL);
    PROBE_HIP(hipGetLastError());
  }
  if (rc == 0) {
    k_run_pairing<<<n_cases, PAR_THREADS>>>(dres, dlines, dinf, force_generic, poison, dok, dout);
    PROBE_HIP(hipGetLastError());
  }
  if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
  if (rc == 0) PROBE_HIP(hipMemcpy(verdict_out, dok, n * sizeof(int), hipMemcpyDeviceToHost));
  if (rc == 0) PROBE_HIP(hipMemcpy(rows_out, dout, rows, hipMemcpyDeviceToHost));
  return rc;
}

#if KZ_CURVE == 0
int pairingprobe_info_1(int* out);
int pairingprobe_run_program_1(int force_generic, uint32_t poison, const uint16_t* program, int n_ins, int n_cases,
                               const int32_t* rows_in, int32_t* rows_out, int* fast_ok_out);
int pairingprobe_run_pairing_1(int force_generic, uint32_t poison, int n_cases, const void* xyzz_pairs, const void* g2_pairs,
                               const uint8_t* q_inf, int* verdict_out, int32_t* rows_out);

#define PROBE_API extern "C" __attribute__((visibility("default")))
PROBE_API int kzgmi_pairingprobe_info_words() { return INFO_HEAD + 2 * kzgmi::OP_COUNT; }
PROBE_API int kzgmi_pairingprobe_info(int curve, int* out) {
  if (curve == 0) return pairingprobe_info_0(out);
  if (curve == 1) return pairingprobe_info_1(out);
  return PROBE_ERR_CURVE;
}
PROBE_API int kzgmi_pairingprobe_run_program(int curve, int force_generic, uint32_t poison, const uint16_t* program, int n_ins,
                                             int n_cases, const int32_t* rows_in, int32_t* rows_out,
                                             int* fast_ok_out) {
  if (curve == 0) return pairingprobe_run_program_0(force_generic, poison, program, n_ins, n_cases, rows_in, rows_out, fast_ok_out);
  if (curve == 1) return pairingprobe_run_program_1(force_generic, poison, program, n_ins, n_cases, rows_in, rows_out, fast_ok_out);
  return PROBE_ERR_CURVE;
}
PROBE_API int kzgmi_pairingprobe_run_pairing(int curve, int force_generic, uint32_t poison, int n_cases, const void* xyzz_pairs,
                                             const void* g2_pairs, const uint8_t* q_inf, int* verdict_out,
                                             int32_t* rows_out) {
  if (curve == 0) return pairingprobe_run_pairing_0(force_generic, poison, n_cases, xyzz_pairs, g2_pairs, q_inf, verdict_out, rows_out);
  if (curve == 1) return pairingprobe_run_pairing_1(force_generic, poison, n_cases, xyzz_pairs, g2_pairs, q_inf, verdict_out, rows_out);
  return PROBE_ERR_CURVE;
}
#endif
