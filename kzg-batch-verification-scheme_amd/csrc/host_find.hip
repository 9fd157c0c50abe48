// Locating the invalid tuples of a rejected batch: the verdicts of gathered record pairs, the
// combinations of index ranges of a resident batch (grouped small MSMs, msm_group.hpp) and the search
// by group testing over index ranges that uses both (find_plan.hpp), for opening tuples,
// EIP-4844 blob batches and EIP-7594 cell batches (whose ranges end in 64 tail terms over the cell
// SRS, from the cells' own interpolation coefficients: cell.hpp k_cell_coeffs).  Synchronous, on
// slot 0 of the primary device.
#include "host.hpp"

#include <vector>

namespace {
constexpr uint32_t kFindFlags = KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK | KZGMI_FLAG_TRUSTED_G1;
constexpr size_t kBlobMax = size_t(1) << 20;  // blobs per call (host_eip.hip)

int check_find_flags(uint32_t flags) {
  if (flags & (KZGMI_FLAG_POWERS | KZGMI_FLAG_FIAT_SHAMIR))
    return fail(KZGMI_ERR_ARG, "the search uses counter-mode randomisers: KZGMI_FLAG_POWERS and KZGMI_FLAG_FIAT_SHAMIR do not apply");
  if (flags & ~kFindFlags) return fail(KZGMI_ERR_ARG, "unknown flags");
  return 0;
}

// whatever a failed call enqueued drains before its error returns, and the slot is left idle
int drain(Slot& s, int r) {
  if (!r) return 0;
  const std::string msg = g_err;
  (void)hipStreamSynchronize(s.stream);
  s.ndep = 0;
  s.pending = false;
  return fail(r, msg);
}

// The batch's front end for the grouped kernel, once per call: decode and validate the 2 n points into
// the slot's radix-29 slots [pi | C | G1], r_i (scal_r) and s_i (scal_s) for global indices offset + i.
// Errors land in the slot's error word.
template <class Cv>
int enqueue_front(Slot& s, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy, const void* dpi,
                  size_t n, const Seed& seed, uint64_t offset, uint32_t flags) {
  using L = Launch<Cv>;
  using AF = Affine<Cv>;
  CHK(s.pts.ensure((2 * n + 1) * sizeof(AF)));
  CHK(s.inf.ensure(2 * n + 1));
  CHK(s.scal_r.ensure(n * 16));
  CHK(s.scal_s.ensure(n * 32));
  CHK(s.scal_t.ensure(32));
  CHK(s.tpart.ensure(L::tpart_bytes((uint32_t)n)));
  hipStream_t st = s.stream;
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  AF* pts = s.pts.template as<AF>();
  uint8_t* inf = s.inf.template as<uint8_t>();
  // decompression and the subgroup check work in the 32-bit form, converted afterwards (enqueue_batch)
  const bool pts29 = !(flags & (KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK));
  if (flags & KZGMI_FLAG_COMPRESSED) {
    L::decompress_points(st, (const uint8_t*)dpi, (uint32_t)n, pts, inf, err);
    L::decompress_points(st, (const uint8_t*)dC, (uint32_t)n, pts + n, inf + n, err);
  } else {
    L::convert_points(st, (const uint8_t*)dpi, (uint32_t)n, pts, inf, err, pts29);
    L::convert_points(st, (const uint8_t*)dC, (uint32_t)n, pts + n, inf + n, err, pts29);
  }
  if (flags & KZGMI_FLAG_SUBGROUP_CHECK) L::subgroup_check(st, pts, inf, (uint32_t)(2 * n), err);
  HIPCHK(hipMemcpyAsync(pts + 2 * n, pts29 ? srs->g1_29() : srs->g1.p, sizeof(AF), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(inf + 2 * n, srs->g1.template as<uint8_t>() + sizeof(AF), 1, hipMemcpyDeviceToDevice, st));
  if (!pts29) L::pts_to29(st, pts, (uint32_t)(2 * n + 1));
  L::scalar_prep(st, seed, nullptr, offset, (const uint8_t*)dz, (const uint8_t*)dy, (uint32_t)n,
                 s.scal_r.template as<uint32_t>(), s.scal_s.template as<uint32_t>(), s.tpart.p,
                 s.scal_t.template as<uint32_t>(), err);
  HIPCHK(hipGetLastError());
  return 0;
}

// An EIP-7594 cell batch as the search takes it (device arrays, include/kzgmi.h): m unique commitments,
// n commitment indices, cell indices, cells and proofs
struct CellBatch {
  const kzgmi_cell_srs* srs;
  const void* dC;
  size_t m;
  const void* cidx;
  const void* eidx;
  const void* cells;
  const void* dpi;
};
constexpr uint32_t kCellTail = CellLaunch::TERMS;  // a cell range's tail terms: -c_m(g) [tau^m]_1
// cells per search: every level runs in the grouped kernel, and level 0 of 65 536 cells holds ~105 MB of trees
constexpr size_t kCellFindMax = size_t(1) << 16;

// The cell batch's front end for the grouped kernel, once per call (enqueue_front plus the cell part of
// enqueue_batch): the n proofs and, behind the slots the kernel reads, the m unique commitments are
// decoded and checked, the commitments gathered to n slots and the cell SRS's 64 points put behind
// them: radix-29 slots [pi (n) | C (n) | tau^m (64)].  z_k = h_k^64 with y_k = 0 (both index arrays
// checked there), r_k and s_k = r_k z_k in counter mode, and the coefficients of every I_k.
int enqueue_cell_front(kzgmi_ctx* c, Slot& s, const CellBatch& cb, size_t n, const Seed& seed, uint64_t offset) {
  using Cv = Bls12_381;
  using L = Launch<Cv>;
  using AF = Affine<Cv>;
  const size_t TB = 2 * n, UB = TB + kCellTail;  // the first tail point, the first unique commitment
  const uint32_t nn = (uint32_t)n, mm = (uint32_t)cb.m;
  CHK(s.pts.ensure((UB + cb.m) * sizeof(AF)));
  CHK(s.inf.ensure(UB + cb.m));
  CHK(s.scal_r.ensure(n * 16));
  CHK(s.scal_s.ensure(n * 32));
  CHK(s.scal_t.ensure(32));
  CHK(s.tpart.ensure(L::tpart_bytes(nn)));
  CHK(s.blob_z.ensure(n * 32));
  CHK(s.blob_y.ensure(n * 32));
  CHK(s.cell_tab.ensure(n * CellLaunch::BYTES));
  hipStream_t st = s.stream;
  uint32_t* err = s.flags.template as<uint32_t>() + 1;
  AF* pts = s.pts.template as<AF>();
  uint8_t* inf = s.inf.template as<uint8_t>();
  L::decompress_points(st, (const uint8_t*)cb.dpi, nn, pts, inf, err);
  L::decompress_points(st, (const uint8_t*)cb.dC, mm, pts + UB, inf + UB, err);
  L::subgroup_check(st, pts, inf, nn, err);
  L::subgroup_check(st, pts + UB, inf + UB, mm, err);
  CellLaunch::gather(st, cb.cidx, nn, mm, pts, inf, (uint32_t)UB, nn);
  HIPCHK(hipMemcpyAsync(pts + TB, cb.srs->pts.p, kCellTail * sizeof(AF), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(inf + TB, cb.srs->inf.p, kCellTail, hipMemcpyDeviceToDevice, st));
  L::pts_to29(st, pts, (uint32_t)UB);
  uint8_t* bz = s.blob_z.template as<uint8_t>();
  uint8_t* by = s.blob_y.template as<uint8_t>();
  CellLaunch::z(st, cb.eidx, cb.cidx, nn, mm, c->cell_table.p, bz, by, err);
  L::scalar_prep(st, seed, nullptr, offset, bz, by, nn, s.scal_r.template as<uint32_t>(),
                 s.scal_s.template as<uint32_t>(), s.tpart.p, s.scal_t.template as<uint32_t>(), err);
  CellLaunch::coeffs(st, cb.eidx, (const uint8_t*)cb.cells, nn, c->cell_table.p, s.cell_tab.template as<uint32_t>(),
                     nullptr, err);
  HIPCHK(hipGetLastError());
  return 0;
}

// One grouped launch: the combinations of ranges[0, G) (relative to the resident batch of n tuples
// whose first has global index offset) -> out[2 g], out[2 g + 1].  table: G entries of host scratch,
// kept by the caller until the slot has been waited for.  cells: the batch is a cell batch (64 tail
// terms per range, from the slot's coefficient table); dy is not read then.
template <class Cv>
int enqueue_groups(Slot& s, const FindRange* ranges, size_t G, FindGroup* table, size_t table_at, size_t n,
                   const Seed& seed, uint64_t offset, const void* dy, Xyzz<Cv>* out, uint64_t* wave_terms,
                   bool cells = false) {
  const uint32_t tail = cells ? kCellTail : 1;
  const FindGroupPlan p = find_group_plan(ranges, G, table, tail);
  if (!p.fits) return fail(KZGMI_ERR_ARG, "too many terms for one grouped launch");
  CHK(s.find_nodes.ensure(p.bytes_nodes));
  CHK(s.find_flags.ensure(p.bytes_flags));
  FindGroup* dtab = s.find_tab.template as<FindGroup>() + table_at;
  HIPCHK(hipMemcpyAsync(dtab, table, G * sizeof(FindGroup), hipMemcpyHostToDevice, s.stream));
  uint32_t* negt = s.find_negt.template as<uint32_t>() + 8 * (size_t)tail * table_at;
  if (cells) {
    if constexpr (Cv::ID == 0)
      Launch<Cv>::group_msm_cells(s.stream, dtab, (uint32_t)G, (uint32_t)p.waves, (uint32_t)n, seed, offset,
                                  s.cell_tab.template as<uint32_t>(), s.scal_r.template as<uint32_t>(),
                                  s.scal_s.template as<uint32_t>(), negt, s.pts.template as<Affine<Cv>>(),
                                  s.inf.template as<uint8_t>(), s.find_nodes.template as<uint32_t>(),
                                  s.find_flags.template as<uint32_t>(), (size_t)p.flags + 1, out);
    else
      return fail(KZGMI_ERR_ARG, "cells are BLS12-381 only");
  } else {
    Launch<Cv>::group_msm(s.stream, dtab, (uint32_t)G, (uint32_t)p.waves, (uint32_t)n, seed, offset, (const uint8_t*)dy,
                          s.scal_r.template as<uint32_t>(), s.scal_s.template as<uint32_t>(), negt,
                          s.pts.template as<Affine<Cv>>(), s.inf.template as<uint8_t>(),
                          s.find_nodes.template as<uint32_t>(), s.find_flags.template as<uint32_t>(), (size_t)p.flags + 1,
                          out);
  }
  HIPCHK(hipGetLastError());
  if (wave_terms) *wave_terms += p.waves;
  return 0;
}

// The verdicts of G record pairs -> ok (host), behind whatever the slot's stream holds; a marked record
// is the call's error.  The slot is waited for.
template <class Cv>
int check_pairs(Slot& s, const kzgmi_srs* srs, const Xyzz<Cv>* recs, size_t G, std::vector<int32_t>& ok) {
  using L = Launch<Cv>;
  CHK(s.find_ok.ensure(G * 4));
  hipStream_t st = s.stream;
  HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, st));
  L::check_marks(st, recs, (uint32_t)(2 * G), s.flags.template as<uint32_t>() + 1);
  L::pairing_check(st, recs, srs->lines.template as<Line<Cv>>(), srs->q_inf.template as<uint8_t>(),
                   s.find_ok.template as<int>(), (uint32_t)G);
  HIPCHK(hipGetLastError());
  ok.resize(G);
  HIPCHK(hipMemcpyAsync(ok.data(), s.find_ok.p, G * 4, hipMemcpyDeviceToHost, st));  // 4 bytes per pair
  HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, st));
  CHK(sync_job(s));
  return map_device_err((uint32_t)s.host_flags[1]);
}

// The search.  Level by level: every suspect range is split (find_split, at the level's fan-out:
// find_level_fanout), every part's (A, B) is
// computed -- long parts as bucket partial jobs of the existing pipeline, one after another, each with
// its own front end over its range; short parts in the grouped kernel over the batch's front end, run
// once before the first such level --, one batched pairing launch decides all parts, and
// find_next_level keeps the lowest failing ones.  dz / dy: n x 32 B on the device.
// cell: the batch is an EIP-7594 cell batch (dC .. dpi are not read; srs is the cell SRS's inner one).
// Every level is then a grouped level at the wide fan-out, whatever its parts' lengths, over the cell
// front end: the bucket pipeline's cell mode is tied to powers-of-r weights (enqueue_batch), and a
// cell batch is short (at most kCellFindMax).
template <class Cv>
int find_invalid(kzgmi_ctx* c, Slot& s, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                 const void* dpi, size_t n, const Seed& seed, uint32_t flags, uint64_t* bad_out, size_t max_bad,
                 size_t* n_bad_out, int* more_out, const CellBatch* cell = nullptr) {
  using XY = Xyzz<Cv>;
  const FindTuning& t = c->find_tune;
  const size_t gb = (flags & KZGMI_FLAG_COMPRESSED) ? g1_bytes(Cv::ID) / 2 : g1_bytes(Cv::ID);
  uint64_t* st = c->find_stats;
  st[0] = st[1] = st[2] = st[3] = 0;
  std::vector<FindRange> suspects{{0, n}}, parts, next(max_bad);
  std::vector<uint64_t> bad(max_bad), bad_next(max_bad);
  std::vector<FindGroup> table;
  std::vector<int32_t> ok;
  size_t n_bad = 0;
  bool more = false, front_done = false;
  bool front_read = false;  // the cell front end's error word is on its way to host_flags[2] (pinned: ok, err, this)
  s.host_flags[2] = 0;
  CHK(s.flags.ensure(16));
  CHK(begin_job(s));
  while (!suspects.empty()) {
    const uint32_t F = cell ? t.fanout : find_level_fanout(suspects.data(), suspects.size(), t);
    parts.resize(suspects.size() * F);
    size_t P = 0;
    for (const FindRange& r : suspects) P += find_split(r.lo, r.hi, F, parts.data() + P);
    parts.resize(P);
    CHK(s.find_rec.ensure(2 * P * sizeof(XY)));
    XY* rec = s.find_rec.template as<XY>();
    if (!cell && find_level_path(parts.data(), P, t) == FIND_BUCKET) {
      for (size_t g = 0; g < P; ++g) {
        const uint64_t lo = parts[g].lo, len = parts[g].hi - lo;
        CHK(HostCore<Cv>::enqueue_batch(c, s, srs, (const uint8_t*)dC + lo * gb, (const uint8_t*)dz + lo * 32,
                                        (const uint8_t*)dy + lo * 32, (const uint8_t*)dpi + lo * gb, (size_t)len, seed, lo,
                                        rec + 2 * g, flags));
        s.pending = false;  // this call waits for the slot itself
        st[1] += 1;
      }
    } else {
      CHK(s.find_tab.ensure((P + 1) * sizeof(FindGroup)));
      const uint32_t tail = cell ? kCellTail : 1;
      CHK(s.find_negt.ensure(((size_t)tail * P + 1) * 32));
      HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
      if (!front_done) {
        if (cell) CHK(enqueue_cell_front(c, s, *cell, n, seed, 0));
        else CHK(enqueue_front<Cv>(s, srs, dC, dz, dy, dpi, n, seed, 0, flags));
      }
      table.resize(P);
      for (size_t g0 = 0; g0 < P;) {  // launches within the workspace bound
        const size_t G = find_group_chunk(parts.data() + g0, P - g0, t, tail);
        CHK(enqueue_groups<Cv>(s, parts.data() + g0, G, table.data() + g0, g0, n, seed, 0, dy, rec + 2 * g0, &st[2],
                               cell != nullptr));
        g0 += G;
      }
      // a front-end error marks every record, as a bucket job marks its own
      if (!front_done) {
        uint32_t* err = s.flags.template as<uint32_t>() + 1;
        Launch<Cv>::mark_records(s.stream, rec, (uint32_t)(2 * P), err);
        // (a marked record does not carry DERR_ARG, the cell front end's index error: kernels.hpp partial_mark)
        if (cell) {
          HIPCHK(hipMemcpyAsync(s.host_flags + 2, err, 4, hipMemcpyDeviceToHost, s.stream));
          front_read = true;
        }
      }
      front_done = true;
    }
    const int pr = check_pairs<Cv>(s, srs, rec, P, ok);
    if (front_read && pr != KZGMI_ERR_DEVICE && s.host_flags[2])  // the front end's error by its own code
      return map_device_err((uint32_t)s.host_flags[2]);
    front_read = false;
    CHK(pr);
    st[0] += 1;
    st[3] += P;
    const FindLevel lv = find_next_level(parts.data(), ok.data(), P, max_bad, bad.data(), n_bad, more, bad_next.data(),
                                         next.data());
    bad.swap(bad_next);
    n_bad = lv.n_bad;
    more = lv.more;
    suspects.assign(next.begin(), next.begin() + lv.n_suspects);
  }
  for (bool& u : s.ev_used) u = false;  // the bucket jobs' phase marks belong to no batch
  for (size_t k = 0; k < n_bad; ++k) bad_out[k] = bad[k];
  *n_bad_out = n_bad;
  *more_out = more ? 1 : 0;
  return 0;
}

int check_find_args(kzgmi_ctx* c, const kzgmi_srs* srs, size_t n, uint32_t flags, const uint64_t* bad_out, size_t max_bad,
                    const size_t* n_bad_out, const int* more_out) {
  if (!srs || srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (!bad_out || !n_bad_out || !more_out) return fail(KZGMI_ERR_ARG, "null output");
  if (max_bad < 1 || max_bad > FIND_MAX_BAD) return fail(KZGMI_ERR_ARG, "max_bad must be in 1 .. 4096");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "batch too large (max 2^26 tuples per call)");
  return check_find_flags(flags);
}

// ... of a cell search: nothing is read from the batch before they pass
int check_cell_find_args(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, size_t m, size_t n, const uint64_t* bad_out,
                         size_t max_bad, const size_t* n_bad_out, const int* more_out) {
  if (!is_cell_srs(c, csrs)) return fail(KZGMI_ERR_ARG, "not a cell srs of this context (kzgmi_cell_srs_load)");
  if (!bad_out || !n_bad_out || !more_out) return fail(KZGMI_ERR_ARG, "null output");
  if (max_bad < 1 || max_bad > FIND_MAX_BAD) return fail(KZGMI_ERR_ARG, "max_bad must be in 1 .. 4096");
  if (n > kCellFindMax)
    return fail(KZGMI_ERR_ARG, "too many cells for one search (max 65536 per call: every level runs in the grouped kernel)");
  if (m > kCellFindMax) return fail(KZGMI_ERR_ARG, "too many commitments (max 65536 per call)");
  if (n && !m) return fail(KZGMI_ERR_ARG, "cells without commitments");
  return 0;
}
}  // namespace

extern "C" {

int kzgmi_batch_check_partials_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* d_partials, size_t n_groups,
                                      uint8_t* ok_out) {
  CHK(check_ctx(c));
  if (!srs || srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  if (n_groups && (!d_partials || !ok_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n_groups > (size_t(1) << 24)) return fail(KZGMI_ERR_ARG, "too many record pairs (max 2^24 per call)");
  CHK(slot0_idle(c));
  if (n_groups == 0) return 0;
  Slot& s = c->slots[0];
  Roctx rx("kzgmi_batch_check_partials_device");
  return dispatch(srs->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    std::vector<int32_t> ok;
    CHK(s.flags.ensure(16));
    CHK(begin_job(s));
    CHK(drain(s, check_pairs<Cv>(s, srs, (const Xyzz<Cv>*)d_partials, n_groups, ok)));
    for (size_t g = 0; g < n_groups; ++g) ok_out[g] = ok[g] ? 1 : 0;
    return 0;
  });
}

int kzgmi_batch_range_partials_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                                      const void* dpi, size_t n, uint64_t index_offset, const uint8_t* seed32,
                                      uint32_t flags, const uint64_t* ranges, size_t n_ranges, void* d_partials_out) {
  CHK(check_ctx(c));
  if (!srs || srs->ctx != c) return fail(KZGMI_ERR_ARG, "srs does not belong to this context");
  CHK(check_find_flags(flags));
  if (n_ranges > FIND_MAX_RANGES) return fail(KZGMI_ERR_ARG, "too many ranges (max 65536 per call)");
  if (n_ranges && (!ranges || !d_partials_out || !dC || !dz || !dy || !dpi)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > (1u << 26)) return fail(KZGMI_ERR_ARG, "batch too large (max 2^26 tuples per call)");
  std::vector<FindRange> rs(n_ranges);
  for (size_t g = 0; g < n_ranges; ++g) {
    rs[g] = {ranges[2 * g], ranges[2 * g + 1]};
    if (rs[g].lo >= rs[g].hi || rs[g].hi > n) return fail(KZGMI_ERR_ARG, "a range is empty or ends past the batch");
  }
  const FindGroupPlan p = find_group_plan(rs.data(), n_ranges, nullptr);
  if (!p.fits || p.bytes > c->find_tune.group_bytes)
    return fail(KZGMI_ERR_ARG, "the ranges' trees pass the grouped kernel's workspace bound (" +
                                   std::to_string(c->find_tune.group_bytes >> 20) + " MiB): pass fewer or shorter ranges");
  CHK(slot0_idle(c));
  if (n_ranges == 0) return 0;
  Slot& s = c->slots[0];
  uint8_t sb[32];
  const Seed seed = make_seed(seed32, sb);
  Roctx rx("kzgmi_batch_range_partials_device");
  return dispatch(srs->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    using XY = Xyzz<Cv>;
    std::vector<FindGroup> table(n_ranges);
    auto run = [&]() -> int {
      CHK(s.flags.ensure(16));
      CHK(s.find_tab.ensure((n_ranges + 1) * sizeof(FindGroup)));
      CHK(s.find_negt.ensure((n_ranges + 1) * 32));
      CHK(begin_job(s));
      HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
      CHK(enqueue_front<Cv>(s, srs, dC, dz, dy, dpi, n, seed, index_offset, flags));
      CHK(enqueue_groups<Cv>(s, rs.data(), n_ranges, table.data(), 0, n, seed, index_offset, dy, (XY*)d_partials_out,
                             nullptr));
      Launch<Cv>::mark_records(s.stream, (XY*)d_partials_out, (uint32_t)(2 * n_ranges), s.flags.template as<uint32_t>() + 1);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
      CHK(sync_job(s));
      s.curve = Cv::ID;
      return map_device_err((uint32_t)s.host_flags[1]);
    };
    return drain(s, run());
  });
}

int kzgmi_batch_find_invalid_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* dC, const void* dz, const void* dy,
                                    const void* dpi, size_t n, const uint8_t* seed32, uint32_t flags, uint64_t* bad_out,
                                    size_t max_bad, size_t* n_bad_out, int* more_out) {
  CHK(check_ctx(c));
  CHK(check_find_args(c, srs, n, flags, bad_out, max_bad, n_bad_out, more_out));
  if (n && (!dC || !dz || !dy || !dpi)) return fail(KZGMI_ERR_ARG, "null input");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  if (n == 0) {
    s.ndep = 0;
    *n_bad_out = 0;
    *more_out = 0;
    return 0;
  }
  uint8_t sb[32];
  const Seed seed = make_seed(seed32, sb);
  Roctx rx("kzgmi_batch_find_invalid_device");
  return dispatch(srs->curve, [&](auto cv) -> int {
    using Cv = decltype(cv);
    const int r = drain(s, find_invalid<Cv>(c, s, srs, dC, dz, dy, dpi, n, seed, flags, bad_out, max_bad, n_bad_out, more_out));
    s.curve = Cv::ID;
    return r;
  });
}

int kzgmi_batch_find_invalid(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* commitments, const uint8_t* zs,
                             const uint8_t* ys, const uint8_t* proofs, size_t n, const uint8_t* seed32, uint32_t flags,
                             uint64_t* bad_out, size_t max_bad, size_t* n_bad_out, int* more_out) {
  CHK(check_ctx(c));
  CHK(check_find_args(c, srs, n, flags, bad_out, max_bad, n_bad_out, more_out));
  if (n && (!commitments || !zs || !ys || !proofs)) return fail(KZGMI_ERR_ARG, "null input");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  const size_t gb = (flags & KZGMI_FLAG_COMPRESSED) ? g1_bytes(srs->curve) / 2 : g1_bytes(srs->curve);
  uint8_t* d[4] = {};  // the host arrays in the slot's stage buffer, as kzgmi_batch_verify_ex stages them
  const StageItem items[4] = {{commitments, n * gb}, {proofs, n * gb}, {zs, n * 32}, {ys, n * 32}};
  if (n) CHK(stage_host(c, s, items, 4, d));
  return kzgmi_batch_find_invalid_device(c, srs, d[0], d[2], d[3], d[1], n, seed32, flags, bad_out, max_bad, n_bad_out,
                                         more_out);
}

int kzgmi_verify_blob_batch_find_invalid_device(kzgmi_ctx* c, const kzgmi_srs* srs, const void* d_blobs, const void* dC48,
                                                const void* dpi48, size_t n, uint64_t* bad_out, size_t max_bad,
                                                size_t* n_bad_out, int* more_out) {
  CHK(check_ctx(c));
  CHK(check_find_args(c, srs, n, 0, bad_out, max_bad, n_bad_out, more_out));
  if (srs->curve != 0) return fail(KZGMI_ERR_ARG, "blob verification is BLS12-381 only");
  if (n && (!d_blobs || !dC48 || !dpi48)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  if (n == 0) {
    s.ndep = 0;
    *n_bad_out = 0;
    *more_out = 0;
    return 0;
  }
  Roctx rx("kzgmi_verify_blob_batch_find_invalid_device");
  // z_i and y_i = p_i(z_i) by the blob stages into the slot's blob_z / blob_y, then the search on
  // (C_i, z_i, y_i, pi_i); a blob element >= r is the call's error
  CHK(s.blob_z.ensure(n * 32));
  CHK(s.blob_y.ensure(n * 32));
  CHK(s.flags.ensure(16));
  CHK(ensure_once(c->blob_table_ready, c->blob_table, BlobLaunch::table_bytes(), s.stream,
                  [&] { BlobLaunch::domain(s.stream, c->blob_table.p); }));
  auto derive = [&]() -> int {
    CHK(begin_job(s));
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
    uint32_t* err = s.flags.template as<uint32_t>() + 1;
    uint8_t* bz = s.blob_z.template as<uint8_t>();
    BlobLaunch::challenges(s.stream, blob_mapping(c, n), (const uint8_t*)d_blobs, (const uint8_t*)dC48, (uint32_t)n, bz, err);
    BlobLaunch::eval(s.stream, (const uint8_t*)d_blobs, bz, c->blob_table.p, (uint32_t)n, false,
                     s.blob_y.template as<uint8_t>(), err);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
    CHK(sync_job(s));
    return map_device_err((uint32_t)s.host_flags[1]);
  };
  CHK(drain(s, derive()));
  uint8_t sb[32];
  const Seed seed = make_seed(nullptr, sb);  // verifier-private randomisers
  const int r = drain(s, find_invalid<Bls12_381>(c, s, srs, dC48, s.blob_z.p, s.blob_y.p, dpi48, n, seed,
                                                 KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK, bad_out, max_bad,
                                                 n_bad_out, more_out));
  s.curve = 0;
  return r;
}

int kzgmi_verify_blob_batch_find_invalid(kzgmi_ctx* c, const kzgmi_srs* srs, const uint8_t* blobs,
                                         const uint8_t* commitments48, const uint8_t* proofs48, size_t n,
                                         uint64_t* bad_out, size_t max_bad, size_t* n_bad_out, int* more_out) {
  CHK(check_ctx(c));
  CHK(check_find_args(c, srs, n, 0, bad_out, max_bad, n_bad_out, more_out));
  if (n && (!blobs || !commitments48 || !proofs48)) return fail(KZGMI_ERR_ARG, "null input");
  if (n > kBlobMax) return fail(KZGMI_ERR_ARG, "too many blobs (max 2^20 per call)");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  uint8_t* d[3] = {};  // blobs, commitments, proofs in the slot's stage buffer
  const StageItem items[3] = {{blobs, n * BlobLaunch::BYTES}, {commitments48, n * 48}, {proofs48, n * 48}};
  if (n) CHK(stage_host(c, s, items, 3, d));
  return kzgmi_verify_blob_batch_find_invalid_device(c, srs, d[0], d[1], d[2], n, bad_out, max_bad, n_bad_out, more_out);
}

// ------------------------------------------------------------------------------ EIP-7594 cells
int kzgmi_cell_coeffs_device(kzgmi_ctx* c, const void* d_cell_indices, const void* d_cells, size_t n,
                             void* d_coeffs_out) {
  CHK(check_ctx(c));
  if (n && (!d_cell_indices || !d_cells || !d_coeffs_out)) return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kCellFindMax) return fail(KZGMI_ERR_ARG, "too many cells (max 65536 per call)");
  if (n == 0) return 0;
  return slot0_utility_job(
      c,
      [&](Slot& s) -> int {
        CHK(ensure_cell_table(c, s.stream));
        CHK(s.blob_z.ensure(n * 32));
        CHK(s.blob_y.ensure(n * 32));
        return s.cell_tab.ensure(n * CellLaunch::BYTES);
      },
      [&](Slot& s, uint32_t* err) -> int {
        // the cell indices are checked where the batch checks them
        CellLaunch::z(s.stream, d_cell_indices, nullptr, (uint32_t)n, 0, c->cell_table.p, s.blob_z.template as<uint8_t>(),
                      s.blob_y.template as<uint8_t>(), err);
        CellLaunch::coeffs(s.stream, d_cell_indices, (const uint8_t*)d_cells, (uint32_t)n, c->cell_table.p,
                           s.cell_tab.template as<uint32_t>(), (uint8_t*)d_coeffs_out, err);
        return 0;
      });
}

int kzgmi_cell_range_partials_device(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, const void* dC48, size_t m,
                                     const void* d_cidx, const void* d_eidx, const void* d_cells, const void* dpi48,
                                     size_t n, uint64_t index_offset, const uint8_t* seed32, const uint64_t* ranges,
                                     size_t n_ranges, void* d_partials_out) {
  CHK(check_ctx(c));
  if (!is_cell_srs(c, csrs)) return fail(KZGMI_ERR_ARG, "not a cell srs of this context (kzgmi_cell_srs_load)");
  if (n_ranges > FIND_MAX_RANGES) return fail(KZGMI_ERR_ARG, "too many ranges (max 65536 per call)");
  if (n_ranges && (!ranges || !d_partials_out || !dC48 || !d_cidx || !d_eidx || !d_cells || !dpi48))
    return fail(KZGMI_ERR_ARG, "null argument");
  if (n > kCellFindMax) return fail(KZGMI_ERR_ARG, "too many cells (max 65536 per call)");
  if (m > kCellFindMax) return fail(KZGMI_ERR_ARG, "too many commitments (max 65536 per call)");
  if (n && !m) return fail(KZGMI_ERR_ARG, "cells without commitments");
  std::vector<FindRange> rs(n_ranges);
  for (size_t g = 0; g < n_ranges; ++g) {
    rs[g] = {ranges[2 * g], ranges[2 * g + 1]};
    if (rs[g].lo >= rs[g].hi || rs[g].hi > n) return fail(KZGMI_ERR_ARG, "a range is empty or ends past the batch");
  }
  const FindGroupPlan p = find_group_plan(rs.data(), n_ranges, nullptr, kCellTail);
  if (!p.fits || p.bytes > c->find_tune.group_bytes)
    return fail(KZGMI_ERR_ARG, "the ranges' trees pass the grouped kernel's workspace bound (" +
                                   std::to_string(c->find_tune.group_bytes >> 20) + " MiB): pass fewer or shorter ranges");
  CHK(slot0_idle(c));
  if (n_ranges == 0) return 0;
  Slot& s = c->slots[0];
  uint8_t sb[32];
  const Seed seed = make_seed(seed32, sb);
  Roctx rx("kzgmi_cell_range_partials_device");
  using Cv = Bls12_381;
  using XY = Xyzz<Cv>;
  const CellBatch cb{csrs, dC48, m, d_cidx, d_eidx, d_cells, dpi48};
  std::vector<FindGroup> table(n_ranges);
  auto run = [&]() -> int {
    CHK(s.flags.ensure(16));
    CHK(s.find_tab.ensure((n_ranges + 1) * sizeof(FindGroup)));
    CHK(s.find_negt.ensure(p.bytes_negt));
    CHK(ensure_cell_table(c, s.stream));
    CHK(begin_job(s));
    HIPCHK(hipMemsetAsync(s.flags.p, 0, 16, s.stream));
    CHK(enqueue_cell_front(c, s, cb, n, seed, index_offset));
    CHK(enqueue_groups<Cv>(s, rs.data(), n_ranges, table.data(), 0, n, seed, index_offset, nullptr, (XY*)d_partials_out,
                           nullptr, true));
    Launch<Cv>::mark_records(s.stream, (XY*)d_partials_out, (uint32_t)(2 * n_ranges), s.flags.template as<uint32_t>() + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.host_flags, s.flags.p, 8, hipMemcpyDeviceToHost, s.stream));
    CHK(sync_job(s));
    s.curve = Cv::ID;
    return map_device_err((uint32_t)s.host_flags[1]);
  };
  return drain(s, run());
}

int kzgmi_verify_cell_batch_find_invalid_device(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, const void* dC48, size_t m,
                                                const void* d_cidx, const void* d_eidx, const void* d_cells,
                                                const void* dpi48, size_t n, const uint8_t* seed32, uint64_t* bad_out,
                                                size_t max_bad, size_t* n_bad_out, int* more_out) {
  CHK(check_ctx(c));
  CHK(check_cell_find_args(c, csrs, m, n, bad_out, max_bad, n_bad_out, more_out));
  if (n && (!dC48 || !d_cidx || !d_eidx || !d_cells || !dpi48)) return fail(KZGMI_ERR_ARG, "null input");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  if (n == 0) {
    s.ndep = 0;
    *n_bad_out = 0;
    *more_out = 0;
    return 0;
  }
  uint8_t sb[32];
  const Seed seed = make_seed(seed32, sb);
  Roctx rx("kzgmi_verify_cell_batch_find_invalid_device");
  CHK(ensure_cell_table(c, s.stream));
  const CellBatch cb{csrs, dC48, m, d_cidx, d_eidx, d_cells, dpi48};
  const int r = drain(s, find_invalid<Bls12_381>(c, s, csrs->srs, nullptr, nullptr, nullptr, nullptr, n, seed,
                                                 KZGMI_FLAG_COMPRESSED | KZGMI_FLAG_SUBGROUP_CHECK, bad_out, max_bad,
                                                 n_bad_out, more_out, &cb));
  s.curve = 0;
  return r;
}

int kzgmi_verify_cell_batch_find_invalid(kzgmi_ctx* c, const kzgmi_cell_srs* csrs, const uint8_t* commitments48, size_t m,
                                         const uint64_t* commitment_indices, const uint64_t* cell_indices,
                                         const uint8_t* cells, const uint8_t* proofs48, size_t n, const uint8_t* seed32,
                                         uint64_t* bad_out, size_t max_bad, size_t* n_bad_out, int* more_out) {
  CHK(check_ctx(c));
  CHK(check_cell_find_args(c, csrs, m, n, bad_out, max_bad, n_bad_out, more_out));
  if (n && (!commitments48 || !commitment_indices || !cell_indices || !cells || !proofs48))
    return fail(KZGMI_ERR_ARG, "null input");
  CHK(slot0_idle(c));
  Slot& s = c->slots[0];
  uint8_t* d[6] = {};  // the five arrays in the slot's stage buffer, then 16 bytes of slack (kzgmi_verify_cell_batch)
  const StageItem items[6] = {{commitments48, 48 * m}, {commitment_indices, 8 * n}, {cell_indices, 8 * n},
                              {cells, n * CellLaunch::BYTES}, {proofs48, 48 * n}, {nullptr, 16}};
  if (n) CHK(stage_host(c, s, items, 6, d));
  return kzgmi_verify_cell_batch_find_invalid_device(c, csrs, d[0], m, d[1], d[2], d[3], d[4], n, seed32, bad_out, max_bad,
                                                     n_bad_out, more_out);
}

int kzgmi_find_invalid_stats(kzgmi_ctx* c, uint64_t out[4]) {
  if (!c) return fail(KZGMI_ERR_ARG, "null context");
  if (!out) return fail(KZGMI_ERR_ARG, "null output");
  for (int k = 0; k < 4; ++k) out[k] = c->find_stats[k];
  return 0;
}

}  // extern "C"
