// Power-of-two transforms over Fr (kzgmi_fr_ntt*): the plan of ntt_plan.hpp run pass by pass with
// the kernels of ntt.hpp.  One pass goes straight from the input to the output; more go input ->
// scratch, in place there, scratch -> output, so an in-place call needs no further copy.  DESIGN.md 3h.
#include "host.hpp"

namespace kzgmi {

int ntt_check_args(int curve, unsigned logn, size_t count, uint32_t flags, const uint8_t* shift32, Seed* shift_out,
                   bool* has_shift) {
  if (curve != KZGMI_BLS12_381 && curve != KZGMI_BN254) return fail(KZGMI_ERR_ARG, "unknown curve");
  if (logn > NTT_MAX_LOGN) return fail(KZGMI_ERR_ARG, "transform too large (max 2^26 points)");
  if (flags & ~(uint32_t)(KZGMI_NTT_INVERSE | KZGMI_NTT_BITREV)) return fail(KZGMI_ERR_ARG, "unknown transform flag");
  if (count > (size_t(1) << (NTT_MAX_LOGN - logn))) return fail(KZGMI_ERR_ARG, "too many values (count * n is at most 2^26)");
  *has_shift = shift32 != nullptr;
  if (!shift32) return 0;
  uint8_t buf[32];
  *shift_out = make_seed(shift32, buf);
  const uint32_t* mod = curve == KZGMI_BLS12_381 ? Bls12_381::FrP::MOD : Bn254::FrP::MOD;
  bool below = false, zero = true;
  for (int k = 0; k < 8; ++k) zero = zero && shift_out->w[k] == 0;
  for (int k = 0; k < 8; ++k) {  // word 0 is the most significant
    const uint32_t m = mod[7 - k];
    if (shift_out->w[k] != m) {
      below = shift_out->w[k] < m;
      break;
    }
  }
  if (!below) return fail(KZGMI_ERR_SCALAR, "shift is not below the scalar modulus");
  if (zero) return fail(KZGMI_ERR_ARG, "shift is zero");
  return 0;
}

template <class Cv>
int HostNtt<Cv>::enqueue(kzgmi_ctx* c, Slot& s, const void* d_in, unsigned logn, size_t count, uint32_t flags,
                         const Seed* shift, bool read_be, bool write_be, void* d_out, uint32_t* err) {
  using L = Launch<Cv>;
  if (count == 0) return 0;
  NttPlan plan;
  const uint32_t bound = std::min(c->ntt_pass_bits, c->ntt_tile_bits - NTT_MIN_COLS_BITS);
  if (!ntt_plan(logn, count, flags, shift != nullptr, bound, read_be, write_be, &plan))
    return fail(KZGMI_ERR_ARG, "bad transform arguments");
  hipStream_t st = s.stream;
  CHK(ensure_once(c->fr_ntt_table_ready[Cv::ID], c->fr_ntt_table[Cv::ID], L::ntt_table_bytes(), st,
                  [&] { L::ntt_roots(st, c->fr_ntt_table[Cv::ID].p); }));
  const void* roots = c->fr_ntt_table[Cv::ID].p;
  const bool call_table = shift || (plan.pass[plan.npass - 1].flags & NTT_P_SCALE);
  if (call_table) {
    CHK(s.ntt_call.ensure(L::ntt_call_bytes()));
    L::ntt_call_table(st, shift, flags & KZGMI_NTT_INVERSE, logn, s.ntt_call.p);
  }
  if (plan.npass > 1) CHK(s.ntt_tmp.ensure(ntt_scratch_bytes(plan)));
  for (uint32_t k = 0; k < plan.npass; ++k) {
    const void* in = k == 0 ? d_in : s.ntt_tmp.p;
    void* out = k + 1 == plan.npass ? d_out : s.ntt_tmp.p;
    L::ntt_pass(st, c->ntt_tile_bits, plan.pass[k], logn, count, in, out, roots, s.ntt_call.p, err);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

template struct HostNtt<Bls12_381>;
template struct HostNtt<Bn254>;

}  // namespace kzgmi

namespace {

int check_ntt_arrays(const void* in, const void* out, unsigned logn, size_t count, bool device) {
  if (count == 0) return 0;
  if (!in || !out) return fail(KZGMI_ERR_ARG, "null argument");
  if (!device) return 0;
  const uintptr_t x = (uintptr_t)in, y = (uintptr_t)out;
  if ((x | y) & 15) return fail(KZGMI_ERR_ARG, "device arrays must be 16-byte aligned");
  const size_t bytes = (size_t)32 * (count << logn);
  if (x != y && x < y + bytes && y < x + bytes) return fail(KZGMI_ERR_ARG, "the output overlaps the input (in place: the same pointer)");
  return 0;
}

}  // namespace

extern "C" {

int kzgmi_fr_ntt_device_async(kzgmi_ctx* c, kzgmi_curve curve, int slot, const void* d_in, unsigned logn, size_t count,
                              uint32_t flags, const uint8_t* shift32, void* d_out) {
  KZ_ROUTE(c, nullptr, slot);
  CHK(check_ctx(c, slot));
  Seed shift;
  bool has_shift = false;
  CHK(ntt_check_args(curve, logn, count, flags, shift32, &shift, &has_shift));
  CHK(check_ntt_arrays(d_in, d_out, logn, count, true));
  Slot& s = c->slots[slot];
  if (s.pending) return fail(KZGMI_ERR_ARG, "slot busy: call kzgmi_slot_wait first");
  if (count == 0) return arm_empty(s, JobKind::Utility, curve);  // succeeds, writes nothing
  Roctx rx("kzgmi_fr_ntt_device_async");
  return dispatch(curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    CHK(s.flags.ensure(16));
    CHK(begin_job(s));
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
    uint32_t* err = s.flags.template as<uint32_t>() + 1;
    // (a failed enqueue leaves the stream with nothing of this call that the slot's next job could see)
    CHK(HostNtt<Cv>::enqueue(c, s, d_in, logn, count, flags, has_shift ? &shift : nullptr, true, true, d_out, err));
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
    CHK(end_job(s));
    arm(s, JobKind::Utility, Cv::ID);
    return 0;
  });
}

int kzgmi_fr_ntt_device(kzgmi_ctx* c, kzgmi_curve curve, const void* d_in, unsigned logn, size_t count, uint32_t flags,
                        const uint8_t* shift32, void* d_out) {
  CHK(check_ctx(c));
  CHK(slot0_idle(c));
  CHK(kzgmi_fr_ntt_device_async(c, curve, 0, d_in, logn, count, flags, shift32, d_out));
  return kzgmi_slot_wait(c, 0, nullptr);
}

// The host form: the values in slot 0's stage buffer, transformed in place there and copied back
int kzgmi_fr_ntt(kzgmi_ctx* c, kzgmi_curve curve, const uint8_t* in, unsigned logn, size_t count, uint32_t flags,
                 const uint8_t* shift32, uint8_t* out) {
  CHK(check_ctx(c));
  Seed shift;
  bool has_shift = false;
  CHK(ntt_check_args(curve, logn, count, flags, shift32, &shift, &has_shift));
  CHK(check_ntt_arrays(in, out, logn, count, false));
  CHK(slot0_idle(c));
  if (count == 0) return 0;
  const size_t bytes = (size_t)32 * (count << logn);
  const StageItem item{in, bytes};
  uint8_t* d = nullptr;
  CHK(stage_host(c, c->slots[0], &item, 1, &d));
  CHK(kzgmi_fr_ntt_device_async(c, curve, 0, d, logn, count, flags, shift32, d));
  CHK(kzgmi_slot_wait(c, 0, nullptr));
  HIPCHK(hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
