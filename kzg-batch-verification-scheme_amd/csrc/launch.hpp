// Host-side launchers for every kernel, one set per curve.  Each group of launchers is
// defined in its own translation unit (launch_*.hip) compiled once per curve (-DKZ_CURVE=0
// BLS12-381, 1 BN254), so the device code builds in parallel; the host units (api.hip,
// host_*.hip) only call these.
#pragma once
#include "kernels.hpp"
#include "msm_small.hpp"
#include "find_plan.hpp"
#include "ntt_plan.hpp"

namespace kzgmi {

constexpr int G1NTT_FORM_AUTO = 0, G1NTT_FORM_THREAD = 1, G1NTT_FORM_WAVE = 2;  // the stage forms of g1ntt.hpp
constexpr unsigned G1NTT_MAX_LOGN = 20;     // kzgmi_g1_ntt: count * n <= 2^20 points per call
constexpr unsigned OPEN_ALL_MAX_LOGN = 19;  // kzgmi_open_all: its 2n-point transforms stay within that
static_assert(OPEN_ALL_MAX_LOGN + 1 <= G1NTT_MAX_LOGN, "open_all's 2n-point transform is a transform the library runs");
// kzgmi_open_cosets: count * N <= 2^19 coefficients (the call's count * 2N terms and the records of its
// inverse transforms stay within a G1 transform call) and count * K * l <= 2^20 evaluations
constexpr unsigned OPEN_COSETS_MAX_LOG_COEFFS = OPEN_ALL_MAX_LOGN, OPEN_COSETS_MAX_LOG_POINTS = G1NTT_MAX_LOGN;

template <class Cv>
struct Launch {
  using XY = Xyzz<Cv>;
  using AF = Affine<Cv>;
  // ---- MSM (launch_msm.hip)
  // digits: sum_k count_k * nwin_k u32 (tl.c[k].dig_base set), coarse: 3 * nsets * 256 u32
  // (counts, offsets, cursors), ent: emax x 8 B (coarse-pass entries: msm.hpp EntPacked / EntSplit)
  // sort_flags: SORT_SPLIT (split coarse-pass entries at every size), SORT_FULL_BINS (every set at
  // full-width coarse bins, the fallback of a set table overflow) -- test knobs
  static constexpr int SORT_SPLIT = 1, SORT_FULL_BINS = 2;
  static void sort(hipStream_t st, const TermList& tl, uint32_t nsets, const uint8_t* inf, uint32_t* digits,
                   uint32_t* coarse, uint64_t* ent, size_t emax, int sort_flags, uint32_t* off, uint32_t* cnt, uint32_t* total, uint32_t* sval,
                   uint32_t* skey, int wbits = WBITS);
  // both curves accumulate in radix 2^29: pts in that format (convert_points(to29) or
  // pts_to29), acc29 = (nb + 2 x launched threads) records of W29 words that stay the bucket
  // store (k_fixup joins pieces into them; reduce reads them).  The sorted entries [*lo, *total)
  // (lo nullptr: from 0), whole buckets
  static void accumulate(hipStream_t st, size_t nchunks, const uint32_t* total, const uint32_t* sval,
                         const uint32_t* skey, const uint32_t* off, const uint32_t* cnt, const AF* pts,
                         uint32_t* acc29, uint32_t nb, size_t acc_threads, uint32_t* next_chunk, uint32_t* crowd,
                         const uint32_t* lo, hipStream_t fix_st);
  // the piece joins of an accumulation launch (k_fixup, k_fixup_crowded: same nchunks, nb, lo);
  // accumulate issues them itself on fix_st (nullptr: the caller does, e.g. on another stream,
  // always behind the accumulation launch with the same crowd list, which zeroes it).
  // nb: the record index of the launch's first piece (its pieces follow the nb bucket records)
  static void fixup(hipStream_t st, size_t nchunks, const uint32_t* total, const uint32_t* skey, const uint32_t* off,
                    const uint32_t* cnt, uint32_t* acc29, uint32_t nb, uint32_t* crowd, const uint32_t* lo);
  // Row accumulation (msm.hpp k_accumulate_rows) of the whole sorted list.  row_items: the items
  // of off / cnt (buckets of more than L entries cut), sorted by length, longest first, into
  // `items` (3 x cap words) with the cut buckets' join list in `cuts` (cut_cap lines); rowq
  // (RQ_WORDS words) is zeroed here and carries the counts to accumulate_rows, which walks the rows with `threads`
  // threads (whole blocks of a resident round) and then joins the cut buckets' pieces (records
  // nb + slot) into their records.  Both on st, row_items any time after the sort.
  static void row_items(hipStream_t st, const uint32_t* off, const uint32_t* cnt, uint32_t nb, uint32_t L, uint32_t* rowq,
                        uint32_t* items, uint32_t cap, uint32_t* cuts, uint32_t cut_cap);
  static void accumulate_rows(hipStream_t st, size_t threads, const uint32_t* sval, const AF* pts, uint32_t* acc29,
                              uint32_t nb, uint32_t* rowq, const uint32_t* items, uint32_t cap, const uint32_t* cuts,
                              uint32_t cut_cap);
  static void pts_to29(hipStream_t st, AF* pts, uint32_t n);  // in place
  // acc29[b] += acc29b[b] for the buckets with cntb[b] != 0, cnt[b] += cntb[b] (chunked batches)
  static void merge_buckets(hipStream_t st, uint32_t nb, uint32_t* acc29, uint32_t* cnt, const uint32_t* acc29b,
                            const uint32_t* cntb);
  // low_prio: the kernels run at normal issue priority instead of the tail's raised one (the
  // side stream of a split accumulation)
  // seg4_waves: 4 threads per reduction segment when that grid stays within seg4_waves waves per
  // SIMD of the device's `simds` (0: always 2 threads)
  static void reduce(hipStream_t st, uint32_t nsets, const uint32_t* cnt, const uint32_t* acc29, XY* R, XY* U,
                     XY* scratch, XY* winsum, int wbits = WBITS, bool low_prio = false, int seg4_waves = 0,
                     int simds = 1024);
  static void window_combine(hipStream_t st, const MsmWindows& mw, const XY* winsum, XY* res, int wbits = WBITS,
                             bool low_prio = false);
  // small calls (msm_small.hpp): one wave per term + a counter tree; res (nmsm records)
  // and flags are cleared here; nodes: small_node_words() words, flags: small_flag_words() words
  static void small_msm(hipStream_t st, const TermList& tl, const SmallPlan& sp, uint32_t terms, const AF* pts,
                        const uint8_t* inf, uint32_t* nodes, uint32_t* flags, uint32_t flag_words, XY* res);
  // ---- I/O and scalars (launch_io.hip)
  // to29: store in the accumulation's radix-29 format, for
  // points that go straight into run_msm_core(..., pts29 = true)
  static void convert_points(hipStream_t st, const uint8_t* bytes, uint32_t n, AF* pts, uint8_t* inf, uint32_t* err,
                             bool to29 = false, AF* img = nullptr, uint8_t* img_inf = nullptr);
  static void set_generator(hipStream_t st, AF* pt, uint8_t* inf);
  static void decompress_points(hipStream_t st, const uint8_t* bytes, uint32_t n, AF* pts, uint8_t* inf,
                                uint32_t* err);
  static void compress_points(hipStream_t st, const uint8_t* in, uint32_t n, uint8_t* out);
  static void subgroup_check(hipStream_t st, const AF* pts, const uint8_t* inf, uint32_t n, uint32_t* err);
  static void convert_scalars(hipStream_t st, const uint8_t* bytes, uint32_t n, uint32_t* out, uint32_t* err);
  // GLV (glv.hpp): n scalars of 8 words, `stride` words apart -> half scalars h0, h1 (4 words each)
  static void glv_split(hipStream_t st, const uint32_t* scal, uint32_t stride, uint32_t n, uint32_t* h0, uint32_t* h1);
  // in29: src is in the accumulation's radix-29 format (and dst is written in it)
  static void endo_points(hipStream_t st, const AF* src, const uint8_t* src_inf, uint32_t n, AF* dst, uint8_t* dst_inf,
                          bool in29 = false);
  static void convert_g2(hipStream_t st, const uint8_t* bytes, uint32_t n, G2Aff<Cv>* out, uint8_t* inf,
                         uint32_t* err);
  static void tsum(hipStream_t st, const void* tpart, uint32_t nblocks, uint32_t* negt);  // negt = -(sum) mod r
  static void scalar_prep(hipStream_t st, const Seed& seed, const uint32_t* seed_dev, uint64_t index_offset,
                          const uint8_t* zs,
                          const uint8_t* ys, uint32_t n, uint32_t* r_out, uint32_t* s_out, void* tpart,
                          uint32_t* negt, uint32_t* err, uint32_t* h0 = nullptr, uint32_t* h1 = nullptr);
  static size_t tpart_bytes(uint32_t n);
  // ---- Fiat-Shamir / powers-of-r randomisers (fs.hpp)
  static void fs_leaves(hipStream_t st, const uint8_t* dC, const uint8_t* dpi, const uint8_t* dz, const uint8_t* dy,
                        uint32_t n, uint64_t offset, bool compressed, uint32_t* leaves);
  // Merkle-reduce `count` 32-byte nodes to `target` (count / target a power of two; each
  // result node covers count / target consecutive inputs); tmp holds 3 count / 4 nodes;
  // returns the buffer holding the result
  static const uint32_t* fs_reduce(hipStream_t st, const uint32_t* in, uint32_t count, uint32_t target, uint32_t* tmp);
  static void fs_pad(hipStream_t st, uint32_t* digests, uint32_t nchunks, uint32_t p2);
  static void fs_challenge(hipStream_t st, const uint32_t* root, uint64_t n, void* pow, uint32_t* chal_out);
  static void pow_table(hipStream_t st, const Seed& r_be, void* pow, uint32_t* err);
  static void scalar_prep_pow(hipStream_t st, const void* pow, uint64_t index_offset, const uint8_t* zs,
                              const uint8_t* ys, uint32_t n, uint32_t* r_out, uint32_t* s_out, void* tpart,
                              uint32_t* negt, uint32_t* err);
  static void encode_points(hipStream_t st, const XY* res, uint32_t count, uint8_t* out);
  // sum of gathered partial records; a record marked failed raises its code into *err
  static void sum_partials(hipStream_t st, const XY* parts, uint32_t nparts, uint32_t stride, uint32_t nout, XY* out,
                           uint32_t* err);
  // count partial records out = res, marked failed (kernels.hpp partial_mark) when *err != 0
  static void partial_out(hipStream_t st, const XY* res, uint32_t count, const uint32_t* err, XY* out);
  // ---- pairing (launch_pairing.hip)
  static int num_lines();
  static void precompute_lines(hipStream_t st, const G2Aff<Cv>* q, Line<Cv>* lines);
  // G record pairs (res[2 g], res[2 g + 1]) -> ok[g], one workgroup each
  static void pairing_check(hipStream_t st, const XY* res, const Line<Cv>* lines, const uint8_t* q_inf, int* ok,
                            uint32_t G = 1);
  static void pairing_one(hipStream_t st, const AF* p, const uint8_t* p_inf, const Line<Cv>* lines,
                          const uint8_t* q_inf, uint8_t* out);
  // ---- grouped small MSMs (msm_group.hpp, launch_find.hip): the (A_g, B_g) of G index ranges of the resident
  // batch of n tuples (points [pi | C | G1] in the radix-29 slots, scal_r, scal_s) -> res[2 g], res[2 g + 1].
  // table: the G groups of find_group_plan (device); negt: G x 8 words of scratch, filled here from ys and
  // the seed (global index = index_offset + position in the batch); flags (flag_words) are zeroed here
  static void group_msm(hipStream_t st, const FindGroup* table, uint32_t G, uint32_t waves, uint32_t n,
                        const Seed& seed, uint64_t index_offset, const uint8_t* ys, const uint32_t* scal_r,
                        const uint32_t* scal_s, uint32_t* negt, const AF* pts, const uint8_t* inf, uint32_t* nodes,
                        uint32_t* flags, size_t flag_words, XY* res);
  // ... of G index ranges of a resident batch of n EIP-7594 cells (BLS12-381 only): points
  // [pi | C | tau^m (64)], coef: CellLaunch::coeffs' table; negt: G x 64 x 8 words of scratch, filled here
  static void group_msm_cells(hipStream_t st, const FindGroup* table, uint32_t G, uint32_t waves, uint32_t n,
                              const Seed& seed, uint64_t index_offset, const uint32_t* coef, const uint32_t* scal_r,
                              const uint32_t* scal_s, uint32_t* negt, const AF* pts, const uint8_t* inf,
                              uint32_t* nodes, uint32_t* flags, size_t flag_words, XY* res);
  // count records become marked when *err != 0; a marked record among them raises its code into *err
  static void mark_records(hipStream_t st, XY* recs, uint32_t count, const uint32_t* err);
  static void check_marks(hipStream_t st, const XY* recs, uint32_t count, uint32_t* err);
  // ---- prover commit key (launch_gen.hip): row out = 2^16 * row in, affine
  static void shift_points(hipStream_t st, const AF* in, const uint8_t* inf_in, uint32_t n, AF* out, uint8_t* inf_out);
  // ---- KZG openings in coefficient form (open.hpp, launch_open.hip)
  static uint32_t open_tiles(size_t m);  // tiles of m coefficients
  // k points (32 B big-endian; >= r raises DERR_SCALAR) -> zp: open_power_bytes() each
  static size_t open_power_bytes();
  static void open_points(hipStream_t st, const uint8_t* zs, uint32_t k, uint32_t* zp, uint32_t* err);
  // The scan of m >= 1 coefficients (8 LE words each, canonical) at the g points whose powers start at
  // zp: y -> ys (g x 32 B big-endian) and, for m >= 2, Q_1 .. Q_{m-1} of point p -> q + 32 (m - 1) p
  // bytes, 8 LE words each (be: 32 big-endian bytes).  Scratch, 32 B per value: runv g x tiles x 256,
  // tilev and tilec g x tiles
  static void open_quotients(hipStream_t st, const uint32_t* coef, uint32_t m, const uint32_t* zp, uint32_t g, uint32_t* runv,
                        uint32_t* tilev, uint32_t* tilec, uint8_t* ys, void* q, bool be);
  // ---- power-of-two transforms over Fr (ntt.hpp, launch_ntt.hip)
  static size_t ntt_table_bytes();  // the curve's root tables
  static size_t ntt_call_bytes();   // a call's shift and scale table
  static void ntt_roots(hipStream_t st, void* table);
  // shift: s as a Seed (canonical, nonzero), or nullptr: s = 1 (then only the scale is written)
  static void ntt_call_table(hipStream_t st, const Seed* shift, bool inverse, uint32_t logn, void* tab);
  // one pass of a plan over count transforms of 2^logn, tiles of 2^tile_bits elements
  // (NTT_MIN_TILE_BITS .. NTT_MAX_TILE_BITS, at least pass.bits + 2); a value >= r read by a
  // NTT_P_READ_BE pass raises DERR_SCALAR
  static void ntt_pass(hipStream_t st, uint32_t tile_bits, const NttPass& pass, uint32_t logn, uint64_t count, const void* in,
                       void* out, const void* roots, const void* call, uint32_t* err);
  // ---- power-of-two transforms over G1 and kzgmi_open_all (g1ntt.hpp, launch_g1ntt.hip)
  // validated points -> records; rev: every transform of 2^logn gathered through the bit reversal
  static void g1ntt_from_affine(hipStream_t st, const AF* pts, const uint8_t* inf, uint32_t total, uint32_t logn, bool rev,
                                XY* out);
  // the logn stages of count transforms in place: natural order in, bit-reversed order out, the
  // inverse not scaled by 1 / n.  roots: the curve's table of ntt_roots.  form: G1NTT_FORM_AUTO takes a wave per
  // butterfly where a stage has few of them and a thread per butterfly above (g1ntt.hpp), the others force one
  static void g1ntt_stages(hipStream_t st, XY* data, uint32_t logn, uint32_t count, bool inverse, const void* roots,
                           int form);
  // out[i] = [scal[i]] in[i] (8 canonical LE words each), or [2^-logn] in[i] with scal == nullptr; in == out allowed
  static void g1ntt_mul(hipStream_t st, const XY* in, const uint32_t* scal, uint32_t logn, uint32_t total, XY* out);
  static void g1ntt_rev(hipStream_t st, const XY* in, uint32_t logn, uint32_t total, XY* out);  // in != out
  // kzgmi_open_all: the key's vector x (2n records) from a commit key's resident row of powers; the shift
  // (h_0 .. h_{n-2}, infinity) out of the inverse 2n-point transform's output; a = (c_0 .. c_{m-1}, 0 ..) / 2^halvings
  // of 2^lg scalars (8 LE words each)
  static void g1ntt_key_x(hipStream_t st, const AF* srs29, const uint8_t* srs_inf, uint32_t logn, XY* x);
  static void g1ntt_shift(hipStream_t st, const XY* ihat, uint32_t logn, XY* d);
  static void g1ntt_pad(hipStream_t st, const uint32_t* coef, uint32_t m, uint32_t lg, uint32_t halvings, uint32_t* a);
  // ---- FK20 multi-proofs on every coset of a domain, kzgmi_open_cosets (cosets.hpp, launch_cosets.hip)
  // the key's l vectors x^(b) ([b][i], 2N records) from a commit key's resident row of powers; their staged
  // transforms xs (bit-reversed order) -> the key as the products read it, [pos][b]
  static void cosets_key_x(hipStream_t st, const AF* srs29, const uint8_t* srs_inf, uint32_t logN, uint32_t logl, XY* x);
  static void cosets_key_gather(hipStream_t st, const XY* xs, uint32_t logN, uint32_t logl, XY* out);
  // a[(t l + b) 2^loglen + u] = c_t[l u + b] / 2^halvings (u < ulim, l u + b < m; else 0), count polynomials of m
  static void cosets_pad(hipStream_t st, const uint32_t* coef, uint32_t m, uint32_t count, uint32_t logl, uint32_t loglen,
                         uint32_t ulim, uint32_t halvings, uint32_t* a);
  // records a launch of cosets_products may write into each of its two buffers
  static size_t cosets_scratch_records(uint32_t logN, uint32_t logl, uint32_t count, int form);
  // the scalars in term order: out[(t 2R + pos) l + b] = ahat[(t l + b) 2R + pos], count 2N values of 8 LE words (ahat != out)
  static void cosets_scal(hipStream_t st, const uint32_t* ahat, uint32_t logN, uint32_t logl, uint32_t count, uint32_t* out);
  // hhat[t 2R + pos] = sum_b [scal[(t 2R + pos) l + b]] key[pos l + b] for count polynomials: the products
  // and their sums, in the thread or the wave form (form as g1ntt_stages takes it, decided by the
  // call's count * 2N terms); a and b: cosets_scratch_records each, distinct.  Returns the one that holds hhat
  static XY* cosets_products(hipStream_t st, const XY* key, const uint32_t* scal, uint32_t logN, uint32_t logl, uint32_t count,
                             int form, XY* a, XY* b);
  // d[t K + j] = H_j (j <= R - 2) or infinity, out of count inverse 2R-point transforms' bit-reversed output
  static void cosets_shift(hipStream_t st, const XY* ihat, uint32_t logr2, uint32_t logk, uint32_t count, XY* d);
  // 32-byte values, count x K l: out[t n + e l + j] = y[t n + e + K j] (y != out)
  static void cosets_ys(hipStream_t st, const void* y, uint32_t logk, uint32_t logl, uint32_t count, void* out);
  // ---- generators (launch_gen.hip)
  static void gen_table(hipStream_t st, XY* base, AF* table);
  static void gen_g1(hipStream_t st, const uint8_t* scalars, uint32_t n, const AF* table, uint8_t* out, uint32_t* err);
  static void g2_mul(hipStream_t st, const G2Aff<Cv>* q, const uint8_t* q_inf, const uint32_t (&k_le)[8], uint8_t* out);
  static void fpmul_probe(hipStream_t st, uint32_t blocks, uint32_t iters, uint32_t* out);
  static void gen_tuples(hipStream_t st, const Seed& seed, const uint32_t (&tau_le)[8], uint32_t n, const AF* table,
                         uint8_t* cm, uint8_t* zs, uint8_t* ys, uint8_t* pf);
};

// ---- EIP-4844 blob front end (blob.hpp, launch_blob.hip): BLS12-381 only, 4096-element blobs
struct BlobLaunch {
  // the blob hash's mapping: a lane per blob, or a wave per blob on wave-uniform values
  static constexpr int HASH_LANE = 1, HASH_WAVE = 2;
  static constexpr size_t BYTES = 4096 * 32;        // one blob
  static size_t table_bytes();                      // the domain table: dom[0 .. 4096), 4096^-1
  static void domain(hipStream_t st, void* table);
  // z_i = H(tag || blob_i || C_i) mod r -> zs (n x 32 B); every blob element range-checked
  static void challenges(hipStream_t st, int mapping, const uint8_t* blobs, const uint8_t* commitments, uint32_t n,
                         uint8_t* zs, uint32_t* err);
  // y_i = p_i(z_i) -> ys; range_check: the blob elements are checked here (else they were already)
  static void eval(hipStream_t st, const uint8_t* blobs, const uint8_t* zs, const void* table, uint32_t n,
                   bool range_check, uint8_t* ys, uint32_t* err);
  // r of the batch -> chal_out (8 big-endian words) and the power table of scalar_prep_pow
  static void batch_challenge(hipStream_t st, const uint8_t* commitments, const uint8_t* zs, const uint8_t* ys,
                              const uint8_t* proofs, uint32_t n, void* pow, uint32_t* chal_out);
};

// ---- EIP-7594 cell front end (cell.hpp, launch_cell.hip): BLS12-381 only, 64-element cells on 128 cosets
struct CellLaunch {
  static constexpr size_t BYTES = 64 * 32;          // one cell
  static constexpr uint32_t TERMS = 64;             // [tau^m]_1, m < 64: MSM#1's tail class
  static size_t table_bytes();                      // the coset table
  static size_t part_bytes();                       // per-coset coefficients: 128 x 64 Fr
  static void table(hipStream_t st, void* table);
  // z_k = h_k^64 -> zs, y_k = 0 -> ys (n x 32 B each); indices out of range raise DERR_ARG
  // (commitment_indices may be null: not checked)
  static void z(hipStream_t st, const void* cell_indices, const void* commitment_indices, uint32_t n, uint32_t m,
                const void* table, uint8_t* zs, uint8_t* ys, uint32_t* err);
  // pts[dst + k] = pts[src + commitment_indices[k]] (with the infinity flags)
  static void gather(hipStream_t st, const void* commitment_indices, uint32_t n, uint32_t m, Affine<Bls12_381>* pts,
                     uint8_t* inf, uint32_t src, uint32_t dst);
  // c_m of sum_k r^k I_k (rk: r^k as 8 LE words each): -c_m as LE words -> neg_le (64 x 8 words),
  // c_m as 32 B big-endian -> coeffs_be (may be null); every cell element range-checked
  static void interp(hipStream_t st, const void* cell_indices, const uint8_t* cells, const uint32_t* rk, uint32_t n,
                     const void* table, void* part, uint32_t* neg_le, uint8_t* coeffs_be, uint32_t* err);
  // c_m of every cell's own I_k: 8 LE words each in standard form -> coef_le (n x 64 x 8 words), and as
  // 32 B big-endian -> coeffs_be (may be null); every cell element range-checked
  static void coeffs(hipStream_t st, const void* cell_indices, const uint8_t* cells, uint32_t n, const void* table,
                     uint32_t* coef_le, uint8_t* coeffs_be, uint32_t* err);
  // r of the batch -> chal_out (8 big-endian words) and the power table of scalar_prep_pow
  static void batch_challenge(hipStream_t st, const uint8_t* commitments, uint32_t m, const void* commitment_indices,
                              const void* cell_indices, const uint8_t* cells, const uint8_t* proofs, uint32_t n,
                              void* pow, uint32_t* chal_out);
};

// ---- EIP-7594 cell extension and recovery (recover.hpp, launch_recover.hip): BLS12-381 only
struct RecoverLaunch {
  static constexpr size_t OUT_BYTES = 8192 * 32;    // one extended blob: 128 cells
  static constexpr uint32_t MIN_CELLS = 64, MAX_CELLS = 128;
  static size_t table_bytes();                      // the transform table: twiddles and scale factors
  static size_t z_bytes();                          // recover's per-call table (vanishing polynomial values, cell places)
  static void table(hipStream_t st, void* table);
  // blob b -> its 128 cells at out + b * OUT_BYTES; every element range-checked
  static void compute(hipStream_t st, const uint8_t* blobs, uint32_t nb, const void* table, uint8_t* out, uint32_t* err);
  // the k given cells of every blob (cells: nb x k x 2048 B, in the order of the k shared indices)
  // -> all 128; an index >= 128, a duplicate or an inconsistent blob raises DERR_ARG, an element
  // >= r DERR_SCALAR.  cell_table: CellLaunch's coset table; z: z_bytes() of scratch
  static void recover(hipStream_t st, const void* cell_indices, uint32_t k, const uint8_t* cells, uint32_t nb,
                      const void* cell_table, const void* table, void* z, uint8_t* out, uint32_t* err);
};

// ---- EIP-7594 cell proof generation, FK20 (fk20.hpp, launch_fk20.hip): BLS12-381 only
struct Fk20Launch {
  using XY = Xyzz<Bls12_381>;
  using AF = Affine<Bls12_381>;
  static constexpr uint32_t SRS_POINTS = 4096;      // [tau^m]_1, m < 4096 (m < 4032 is used)
  static constexpr uint32_t N = 128;                // transform size = proofs per blob
  static constexpr uint32_t KEY_TRANSFORMS = 64;    // xhat: one transform per column b
  static constexpr size_t PROOFS_BYTES = 128 * 48;  // one blob's proofs, compressed
  static size_t table_bytes();                      // the key's window table (affine rows)
  static size_t table_flags();                      // its infinity flags: one byte per base
  static size_t coef_bytes(uint32_t nb);            // c_m / 2^k, standard form
  static size_t scal_bytes(uint32_t nb);            // ahat: 8192 x 32 B per blob
  // the validated monomial SRS -> table, tab_inf; x: KEY_TRANSFORMS * N records of scratch
  static void key(hipStream_t st, const AF* srs, const void* ntt_table, XY* x, void* table, uint8_t* tab_inf);
  // ahat of nb blobs `stride` bytes apart -> scal (32 B big-endian at 32 ((128 blob + pos) 64 + b)),
  // times 1 / 128 if fold128 (the pipeline's inverse transform is then unscaled); every element
  // range-checked
  static void scalars(hipStream_t st, const uint8_t* blobs, size_t stride, uint32_t nb, const void* ntt_table,
                      bool fold128, void* coef, uint8_t* scal, uint32_t* err);
  static void msm(hipStream_t st, const uint8_t* scal, uint32_t nb, const void* table, const uint8_t* tab_inf, XY* out);
  // count transforms of 128 records in place, natural order in, bit-reversed order out; the
  // inverse is not scaled by 1 / 128
  static void fft(hipStream_t st, XY* data, uint32_t count, const void* ntt_table, bool inverse);
  static void scale128(hipStream_t st, XY* data, uint32_t n);
  static void shift(hipStream_t st, const XY* h, uint32_t count, XY* d);
  static void unrev(hipStream_t st, const XY* in, uint32_t count, XY* out);
  static void from_affine(hipStream_t st, const AF* pts, const uint8_t* inf, uint32_t n, XY* out);
  // out = in (bytes: a multiple of 16) unless *err is set
  static void emit(hipStream_t st, const void* in, size_t bytes, const uint32_t* err, void* out);
};

// ---- EIP-4844 commitments and proofs (blobproof.hpp, launch_blobproof.hip): BLS12-381 only
struct BlobProofLaunch {
  using XY = Xyzz<Bls12_381>;
  using AF = Affine<Bls12_381>;
  static constexpr uint32_t POINTS = 4096;          // the key: [L_j(tau)]_1, j < 4096
  static constexpr uint32_t PARTS = 64;             // partial sums per blob: one per 64 bases
  static size_t table_bytes();                      // the key's window table (affine rows)
  static size_t table_flags();                      // its infinity flags: one byte per base
  // the validated points -> table, tab_inf
  static void key(hipStream_t st, const AF* pts, const uint8_t* inf, void* table, uint8_t* tab_inf);
  // y_i = p_i(z_i) -> ys (nb x 32 B) and the quotient's evaluations q_i -> q (nb x 128 KiB, blob layout);
  // domain: BlobLaunch's table; range_check: the blob elements are checked here (else they were already)
  static void quotient(hipStream_t st, const uint8_t* blobs, const uint8_t* zs, const void* domain, uint32_t nb,
                       bool range_check, uint8_t* ys, uint8_t* q, uint32_t* err);
  // out[i] = sum_j scal[i][j] L_j for nb vectors of 4096 x 32 B big-endian scalars (q, or blobs);
  // parts: nb * PARTS records of scratch; range_check: a scalar >= r raises DERR_SCALAR
  static void msm(hipStream_t st, const uint8_t* scal, uint32_t nb, bool range_check, const void* table,
                  const uint8_t* tab_inf, XY* parts, XY* out, uint32_t* err);
};

inline unsigned grid_for(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

}  // namespace kzgmi

#if defined(KZ_CURVE)
#if KZ_CURVE == 0
#define KZ_CURVE_T ::kzgmi::Bls12_381
#else
#define KZ_CURVE_T ::kzgmi::Bn254
#endif
#endif
