// Internal declarations shared by the kernel units (vs_*.hip: device code +
// launchers) and the host units (vs_host.h).  Nothing here is part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

namespace vs {

// Score modes of the fused kernels.  Every mode is reduced to a "key" where
// smaller is better, so one list discipline serves all of them:
//   IP : key = -<q,x>                        (faiss knn_inner_product, CMin heap)
//   L2 : key = (|q|^2 + |x|^2) - 2<q,x>, <0 -> 0 (faiss knn_L2sqr BLAS branch)
//   L2D: key = sum (x-q)^2                   (faiss knn_L2sqr sequential branch, nq < 20)
//   COS: key = -(<q,x> * rq * rx)             (pgvector 1 - (a <=> b))
enum Mode : int { MODE_IP = 0, MODE_L2 = 1, MODE_COS = 2, MODE_L2D = 3 };

// GEMM tile geometry (fp32 MFMA path): 128 database rows x 128 queries per
// workgroup, K staged 32 floats at a time through LDS.
constexpr int kBN = 128;
constexpr int kBQ = 128;
constexpr int kBK = 32;
// Row storage stride (floats) is a multiple of kBK; capacity keeps >= kBQ rows of
// zeroed slack past ntotal and is a multiple of kRowPad, so every tile load of
// the GEMM (database tiles and self-join query tiles) stays inside the buffer.
constexpr int kRowPad = 256;
// The GEMV (small batch) path handles up to this many queries per launch.
constexpr int kGemvMaxQ = 8;
// faiss's distance_compute_blas_threshold: a search CALL with fewer queries runs
// the sequential branch (L2 as the direct sum of squares).
constexpr int kBlasThreshold = 20;
// The skinny MFMA (small batch) path handles up to this many queries per launch.
constexpr int kSkinnyMaxQ = 32;

__host__ __device__ inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu))  // NaN stays a (quiet) NaN
    return (uint16_t)((u >> 16) | 0x0040u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// Merge-buffer record: key + local row id (int32; a shard never holds 2^31 rows).
struct Partials {
  float* key = nullptr;
  int* id = nullptr;
  int P = 0;   // lists per query
  int KP = 0;  // entries per list
  int KL = 0;  // for launch_merge_partials: entries stored per list when fewer
               // than the merge keeps (0 = KP; a multiple of 4)
};

// ---- launchers (return the launch status; all asynchronous on `st`) -------
// Fused MFMA distance + top-k over database tiles, writing 2*nsplit lists/query.
// X / Q are fp32 (esize 4) or bf16 (esize 2) rows of stride ld elements.
// With `qlist`, query slot s of the (nq_pad-row) batch is row qlist[s] of Q (and
// of qaux; self row self0 + qlist[s]), only slots s < *qcount are computed
// (query tiles past the device-side count return at once), lists indexed by slot.
// With fkey/fid (inner product, KP = 64): only rows strictly after the query's
// floor (fkey, fid) in (key, row) order enter (floors indexed like qaux).
hipError_t launch_gemm_topk(int KP, int mode, const void* X, const float* xaux, const void* Q,
                            const float* qaux, int64_t ld, int esize, int ntotal, int nq_pad,
                            int nsplit, int64_t self0, Partials part, hipStream_t st,
                            const int* qlist = nullptr, const int* qcount = nullptr,
                            const float* fkey = nullptr, const int* fid = nullptr);
// Streaming (HBM-bound) distance + top-k for nq <= kGemvMaxQ.
// X fp32 or bf16 rows; Q always fp32 (values already rounded for bf16 indexes).
// With fkey/fid (inner product, KP = 64): the floor of each query, as in
// launch_gemm_topk; `run` (device, optional): every block exits when *run == 0.
hipError_t launch_gemv_topk(int KP, int mode, int nq, const void* X, int esize, const float* Q,
                            int64_t ld, int ntotal, int nblocks, Partials part, hipStream_t st,
                            const float* fkey = nullptr, const int* fid = nullptr,
                            const int* run = nullptr);
// Small-batch MFMA path (nq <= kSkinnyMaxQ, KP <= 32, IP or L2 via norms):
// one list per query per block, part.P == nblocks.
// The deep bf16 stage for a few gathered queries (device-side count; the
// kernel exits when it is 0 or above skinny_plane_max_queries()): lane lists
// of 8 in the x1 layout [slot][part.P][part.KP] from the tile-major bf16 plane
// (ld = the plane's K in elements) and the gathered query plane's tile 0.
// filter FILTER_I8: the int8 plane with the x1 pass's keys (qs: the queries'
// scales, xs: the rows' factors).
hipError_t launch_skinny_plane(int filter, const void* XH, const void* QH, int64_t ld, int ntotal,
                               const int* qcount, const float* qs, const float* xs, Partials part,
                               hipStream_t st, int nq_hint = 0);
int skinny_plane_max_queries();
// qcount (optional, device): the kernel does nothing when *qcount is 0 (the
// staged engine's last stage over a gathered batch, usually empty)
hipError_t launch_skinny_topk(int KP, int mode, int nq, const void* X, int esize,
                              const float* xaux, const void* Q, const float* qaux, int64_t ld,
                              int ntotal, int nblocks, Partials part, hipStream_t st,
                              const int* qcount = nullptr);
// The filter pass of the filter-and-verify engine (vs_gemm_x1.hip): one MFMA
// product per fp32 product over a low-precision "filter plane" of rows and
// queries: bf16 (RNE) on v_mfma_f32_32x32x16_bf16, or int8 with one fp32 scale
// per row (code = rint(x / s), s = max|x| / 127) on v_mfma_i32_32x32x32_i8
// (twice the bf16 rate, exact int32 sums, half the bytes per element; the
// inner-product dump launches on v_mfma_i32_16x16x64_i8, the same sums).
enum Filter : int { FILTER_BF16 = 0, FILTER_I8 = 1 };
inline int filter_bytes(int filter) { return filter == FILTER_I8 ? 1 : 2; }
// Filter planes are stored TILE-MAJOR: [tile of 256 rows][64-B step][256
// rows][64 B], so the bytes one filter-pass step reads from a tile (256 rows x
// 64 B) are one contiguous 16-KB block and every DMA piece is 1 KB of
// consecutive bytes (whole 128-B lines; cdna_hip_programming.md: fragment-
// shaped pieces of half lines cost the TA twice).  `ldb` = bytes per row, a
// multiple of 64.  Any row range of a capacity that is a multiple of 256 rows
// lives inside the same prefix of tiles whatever the capacity.
__host__ __device__ inline int64_t plane_offset(int64_t row, int64_t byte, int64_t ldb) {
  return ((row >> 8) * (ldb >> 6) + (byte >> 6)) * 16384 + (row & 255) * 64 + (byte & 63);
}
// Per-launch timing hook of the filter pass (vs_host.h X1SpanTimer): x1_launch brackets
// every pass launch with begin/end; `dominant` is false for the list launch of
// a pass that dumps (its spans are named apart from the dump launches').
struct X1Timing {
  // share: the launch's part of the pass's database tiles
  virtual void begin(hipStream_t st, bool dominant, double share) = 0;
  virtual void end(hipStream_t st) = 0;
  virtual ~X1Timing() = default;
};
struct X1Args {
  X1Timing* timing = nullptr;
  int qskip = 0;  // gathered stage: counts <= qskip are skinny_plane_topk's (x1 exits)
  int filter = FILTER_BF16;
  const void* XH = nullptr;      // database plane, tile-major (plane_offset)
  const float* xs = nullptr;     // int8: per-row factor s_x (IP) or s_x / |x| (COS)
  const float* xgmax = nullptr;  // int8: launch_group_max of xs (capacity rows)
  const float* xgmin = nullptr;  // int8: the group minima of xs over rows < ntotal
  // Dump launches (vs_gemm_x1.hip header): after the pass's first launch the
  // cuts are set and the later launches store the blocks below them
  bool dump = false;
  bool dump32 = false;           // int8 dump launches on the 32x32x32 MFMA form (A/B; default 16x16x64)
  float* qcut = nullptr;         // per query (nqa): the cut, set after the first launch
  const double* qbkey = nullptr; // per query: the verification's bound B (x1_qcut)
  int qcut_m = 0;                // the M of the verification
  int recut = 1;                 // cuts after every replay: 0 set once, 1 fused, 2 replay + x1_qcut
  // Exact-key cuts (vs_x1_cuts.hip "Exact-key cuts"; int8 inner-product passes
  // over fp32 rows): every cut is also lowered to e_M + 1.000001 B.  ecut_x = the
  // fp32 rows (null: a_M + 2B alone), ecut_q = the stage's fp32 queries, both of
  // stride ecut_ld; qam / ecut_key / ecut_id = scratch (per query: the last
  // a_M; the kEcutMaxM best exact keys scored so far and their rows)
  const float* ecut_x = nullptr;
  const float* ecut_q = nullptr;
  int64_t ecut_ld = 0;
  float* qam = nullptr;
  float* ecut_key = nullptr;
  int* ecut_id = nullptr;
  int* dcount = nullptr;         // [nq_pad][P] dumps per lane list (zeroed before the pass)
  int* dslot = nullptr;          // [nq_pad][P][dR][2] dumped (row, raw sum) pairs
  int dR = 0;                    // dump slots per lane list and segment
  unsigned long long* dstats = nullptr;  // [2] dumps replayed, lists out of slots
  const float* xaux = nullptr;   // per-row norms (L2) or 1/|x| (COS)
  const void* QH = nullptr;      // query plane, tile-major (self-join: the stored plane)
  int qtile0 = 0;                // QH's tile of query tile 0 (self-join: self0 / 256)
  const float* qs = nullptr;     // int8: per-query factor s_q (IP) or s_q / |q| (COS)
  const float* qaux = nullptr;   // per-query aux, nqa entries (padding queries read 0)
  int nqa = 0;
  int64_t ld = 0;                // elements per row, a multiple of 64
  int ntotal = 0;
  int nq_pad = 0;                // multiple of kX1Q
  int nsplit = 1;
  int64_t self0 = -1;
  const int* qrow = nullptr;     // per-query excluded row (-1 none), else self0 + q
  const int* qcount = nullptr;   // gathered batch: device-side query count
};
constexpr int kX1Q = 256;  // queries (and database rows) per x1 tile
constexpr int kEcutMaxM = 32;  // exact-key cuts: the largest M (inner product: k <= 16)
// int8 sums stay exact in int32 up to this many elements per row.
constexpr int64_t kI8MaxLd = 131072;
// Candidates merged from the lane lists for `need` exact entries (24, 32, 64 or
// 128; 0 = not served by the filter engine).
int x1_list_len(int need);
// Entries per lane list of the filter pass (8).
int x1_lane_len();
// Diagnostic: the per-segment cycle sums of a VS_X1_STAMP build (58 values:
// [2 groups][9 segments + 3 epilogue counts] + steps per group + two
// histograms of dump events per lane and launch); zeros in a real build.
hipError_t x1_stamps(unsigned long long* out, int reset);
// Diagnostic: the launch plan of a pass (x1_plan, vs_gemm_x1.hip) in
// vs_x1_plan's layout (include/vsearch.h: out[2] is always 0 and launch kind 1
// is never produced, both left from a removed launch form so that readers keep
// their indices and values); touches no device.  dump32 as in X1Args.  False
// for arguments no pass can have.
bool x1_plan_describe(int mode, int filter, int64_t ntotal, int nsplit, bool can_dump, bool ecut,
                      bool gathered, int recut, bool dump32, int32_t* out, int cap, int* nlaunch);
// Writes 4*nsplit lists of part.KP entries per query (nq_pad queries), each holding
// x1_lane_len() entries and empty padding.  *ndispatch = kernel launches used.
hipError_t launch_gemm_topk_x1(int mode, const X1Args& a, Partials part, hipStream_t st,
                               int* ndispatch);
// Bound constants of the verification (vs_x1_verify.hip).
struct BoundArgs {
  int filter = FILTER_BF16;
  double gam = 0.0;       // relative error of the filter's own arithmetic (bf16: fp32
                          // accumulation of ld + 1 terms, n u / (1 - n u), u = 2^-23;
                          // int8: exact int32 sum, three fp32 roundings of the scaling)
  double norm_inf = 0.0;  // relative undercount of the stored fp32 norms
  // L2 on the int8 plane (the augmented inner product, launch_quantize_i8_l2aug):
  // the bound is the inner-product bound of the augmented vectors, mapped to
  // the L2 key; aug_q2 = m C^2, what the augmentation adds to every |q|^2
  int l2aug = 0;
  double aug_q2 = 0.0;
  double aug_nref = 0.0;  // the augmentation's reference norm (launch_l2aug_map)
  // the pass multiplied the fp32 rows and queries themselves (the exact
  // engine's fp32 GEMM, the staged engine's last stage): no residuals, only the
  // fp32 accumulation (gam as for bf16 products) and the key's own roundings
  int rows_exact = 0;
};
BoundArgs make_bound_args(int64_t ld, int filter);
// What the two verification launchers share (launch_verify_rescore,
// launch_verify_wide): one stage's candidates, rows, queries and outputs.
struct VerifyArgs {
  int mode = MODE_IP;  // the exact keys' metric (MODE_L2D: faiss's sequential L2 formula)
  int KF = 0;          // approximate candidates per query
  int M = 0;           // exact entries the answer needs (the bound is checked at the M-th)
  const void* X = nullptr;    // the index's rows: fp32 (xesize 4) or bf16 (xesize 2)
  int xesize = 4;
  const float* xn = nullptr;  // |x|^2 per row
  const float* Q = nullptr;   // the stage's fp32 query rows (stride ld)
  const float* qn = nullptr;  // the queries' aux values (|q|^2 for L2)
  int64_t ld = 0;
  BoundArgs ba;
  const unsigned* stats = nullptr;  // the plane's index maxima (launch_bound_stats)
  Partials lists;  // the filter pass's lane lists (L entries each), for their floors
  int L = 0;
  float* okey = nullptr;  // sorted exact lists of KP entries per query
  int* oid = nullptr;
  int KP = 0;
  int* fail = nullptr;  // fail[q] = 1: the next stage must redo query q
  const float* qinv = nullptr;   // cosine: 1/|q|
  const float* xinv = nullptr;   // cosine: 1/|x|
  const float* qr2i8 = nullptr;  // int8 plane: the queries' residual norms (null for bf16)
  const float* qcut = nullptr;   // the pass's query cuts (dump launches; null: none)
};
// The augmentation of an L2 index's int8 plane (launch_quantize_i8_l2aug).
struct L2Aug {
  int m = 0;          // int8 extra columns (a multiple of 64)
  float C = 0.0f;     // the queries' extra entry (int8 plane)
  float nref = 0.0f;  // reference norm: the rows' extra entries sum to (nref - n_x) / (2 C)
  float Cb = 0.0f;    // bf16 plane: the queries' extra entry (C's power of two, exact in bf16)
};
// Extra columns of an L2 index's augmented bf16 plane (bf16 has no per-row
// scale to keep the extra entries within: one 64-element block).
constexpr int kAugBf16 = 64;
// The bound constants for an L2 index's augmented int8 / bf16 plane.
BoundArgs make_bound_args_l2aug(int64_t ld, const L2Aug& g, int filter = FILTER_I8);
// out[0..3) = bits of max norms, max rn2, max rn2/norms over rows [0, n).
// accumulate: fold rows [0, n) into the maxima already in out (no reset).
hipError_t launch_bound_stats(const float* norms, const float* rn2, int64_t n, unsigned* out,
                              hipStream_t st, bool accumulate = false);
// rn2[r] = |x_r - bf16_rne(x_r)|^2 (rounded up) for fp32 rows [r0, r0+n).
hipError_t launch_resid_norms(const float* X, int64_t ld, int64_t r0, int64_t n, float* out,
                              hipStream_t st);
// int8 filter plane of fp32 rows [r0, r0+n) (stride ld): codes (int8,
// tile-major plane rows r0..), scale[r] = max|x_r| / 127 and, when rn2 != nullptr, rn2[r] = |x_r - scale
// * code_r|^2 rounded up (+inf for a row with a non-finite element).
// X: fp32 rows (xesize 4) or bf16 rows (xesize 2: a bf16 index's int8 plane).
hipError_t launch_quantize_i8(const void* X, int64_t ld, int64_t r0, int64_t n, int8_t* codes,
                              float* scale, float* rn2, hipStream_t st, int xesize = 4);
// L2 as an inner product ("int8 L2"): ranking rows by the faiss
// L2 key |q|^2 + |x|^2 - 2 q.x is ranking them by q.x + (nref - n_x) / 2 =
// x'.q' with x' = [x, e_1 .. e_m], sum_j C e_j = (nref - n_x) / 2 (n_x the
// stored norm, nref a constant of the index: the largest norm of its first
// rows, so the scores of the best rows stay positive and the extra entries
// small), and q' = [q, C .. C].  Rows (norms != nullptr): the codes of x'
// (plane rows of ld + m bytes, the extra columns at [ld, ld + m)), s =
// max(max|x|, |E| / m) / 127 with E = (nref - n_x) / (2 C), the extra codes an
// even split of T = rint(E / s) (the conceptual e_j are those codes' values
// plus an even share of the remainder, so the residual of the extra block is
// |E - s T|^2 / m), rn2 = |x' - plane(x')|^2 and anorm = |x'|^2, both rounded
// up.  Queries (norms == nullptr): extra codes c and s = C / c with c =
// min(127, floor(127 C / max|q|)) (so s * c = C up to one rounding), rn2 =
// |q' - plane(q')|^2 rounded up.
hipError_t launch_quantize_i8_l2aug(const float* X, int64_t ld, int64_t r0, int64_t n,
                                    const L2Aug& g, const float* norms, int8_t* codes,
                                    float* scale, float* rn2, float* anorm, hipStream_t st);
// The same augmentation on the bf16 plane (plane rows of ld + kAugBf16
// elements): rows (norms != nullptr) get kAugBf16 equal extra entries
// bf16(E / kAugBf16), E = (nref - n_x) / (2 Cb) (the conceptual entries add an
// even share of E minus their sum: residual |E - sum|^2 / kAugBf16), rn2 =
// |x' - plane(x')|^2 and anorm = |x'|^2 rounded up; queries (norms == nullptr)
// get Cb (exact: a power of two).
hipError_t launch_bf16_plane_l2aug(const float* X, int64_t ld, int64_t r0, int64_t n,
                                   const L2Aug& g, const float* norms, uint16_t* plane, float* rn2,
                                   float* anorm, hipStream_t st);
// The augmentation's parameters from fp32 rows [r0, r0+n): C = the mean of
// max|x| over the nonzero rows, nref = the largest norm, m = the extra columns
// that keep every row's extra entries within its own max|x|
// (|nref - n_x| / (2 C max|x|) at most), rounded up to 64, at least 64 (no
// nonzero row: C = 1).  Synchronises `st`.
hipError_t l2aug_params(const float* X, int64_t ld, int64_t r0, int64_t n, const float* norms,
                        L2Aug* out, hipStream_t st);
// Lane lists of an augmented pass -> L2 keys: key = max(0, fl(fl(|q|^2 + nref)
// + 2 key)) for every entry with a row (the map is monotone, so the lists stay
// sorted and every floor stays a floor), and the cuts likewise (-FLT_MAX kept).
hipError_t launch_l2aug_map(float* key, const int* id, int64_t per_query, int nq,
                            const float* qn, float nref, float* qcut, hipStream_t st);
// A later filter stage's gathered batch: dst[s] = src[gl[s]] (rows of stride
// ld), daux[s] = aux[gl[s]], drow[s] = self0 + gl[s] (or -1) for s < *count,
// zero rows / 0 / -1 for the other slots of [0, nslot).
hipError_t launch_gather_queries(const float* src, int64_t ld, const float* aux, const int* gl,
                                 const int* count, int nslot, int64_t self0, float* dst,
                                 float* daux, int* drow, hipStream_t st);
// acc[0] += n, acc[1] += *count.
hipError_t launch_add_counts(const int* count, int n, unsigned long long* acc, hipStream_t st);
// out[j] = outer[inner[j]] for j < *count (j < n).
hipError_t launch_compose_list(const int* outer, const int* inner, const int* count, int n,
                               int* out, hipStream_t st);
// *out = clamp(*count - w0, 0, cap): the device-side count of one slot window
// [w0, w0 + cap) of a gathered batch.
hipError_t launch_window_count(const int* count, int w0, int cap, int* out, hipStream_t st);
// out[2 g + b] = max of f over the rows of 32-row group g whose bit 2 is b
// (the int8 filter's per-lane factor bound), n a multiple of 32.
hipError_t launch_group_max(const float* f, int64_t n, float* out, hipStream_t st,
                            int64_t nvalid = 0, float* outmin = nullptr);
// out[i] = a[i] * b[i] (the int8 cosine's folded factors s / |x|).
hipError_t launch_mul_arrays(const float* a, const float* b, int64_t n, float* out,
                             hipStream_t st);
// Checks and rescores the filter candidates: Dk/Ik hold the KF best approximate
// keys of each query (ascending, local rows), `lists` the filter pass's lane
// lists (L entries each) for their floors; writes sorted exact lists of KP
// entries (okey/oid) and fail[q] = 1 where the exact engine must redo query q.
// qcount (optional): only the queries q < *qcount (device-side count).
hipError_t launch_verify_rescore(const VerifyArgs& v, int nq, const float* Dk, const int64_t* Ik,
                                 const int* qcount, hipStream_t st);
// Flagged queries (flags[i] != 0) -> ascending qlist[0 .. *count), all on the
// device; *total += count and *total_n += n when not null.
hipError_t launch_compact_flags(const int* flags, int n, int* list, int* count,
                                unsigned long long* total, unsigned long long* total_n,
                                hipStream_t st);
// Second verification of the queries qlist[0 .. *count) (device count, fixed
// grid): every lane-list entry below the smallest full-list floor (or below
// Dk's M-th key + 2 B when that is smaller; Dk = the merged approximate keys,
// [nq][KF], Ik its rows) is rescored
// exactly (up to kWideCap per query) and the condition re-checked on that wider
// set; passing queries get their sorted exact list in okey/oid and fail[q] = 0.
// okey/oid hold on entry the first check's exact keys of Ik (KP <= 64), which
// are reused instead of read again.  sizes (optional): += the wide-set entries
// and the rescored ones.
constexpr int kWideCap = 4096;
hipError_t launch_verify_wide(const VerifyArgs& v, int nq_max, const int* qlist, const int* count,
                              const float* Dk, const int64_t* Ik, unsigned long long* sizes,
                              hipStream_t st);
// The most candidates (KF) the verification rescores per query, and the longest
// exact list (KP) it writes: 1024 holds inner product's 2k - 1 for k <= 512
// (and k <= 1023 for L2 / cosine); past it the paged exact engine answers.
constexpr int kVerifyMaxKF = 1024;
// The KF (<= kVerifyMaxKF) lexicographically best (key, row) entries of every
// query's P lane lists of L entries (stride part.KP), ascending, into Dk/Ik
// [nq][KF] (the approximate merge when KF > 64; launch_merge_partials below).
hipError_t launch_select_lists(Partials part, int L, int nq, int KF, float* Dk, int64_t* Ik,
                               hipStream_t st, const int* qcount = nullptr);
// The same for KF <= 64 from lane lists of L = 8 (stride 8) by a bound from the
// lists' heads (P >= KF, P <= 512; select_heads_applies), else the list merge.
bool select_heads_applies(const Partials& part, int L, int KF);
hipError_t launch_select_heads(Partials part, int nq, int KF, float* Dk, int64_t* Ik,
                               hipStream_t st, const int* qcount = nullptr);

// Scratch chunks (vs_runtime.hip): device memory of at least `bytes` whose previous
// use the taker's stream `st` waits for; put records the chunk's last use on
// `st` and keeps it for the next taker.  scratch_trim frees the idle chunks of
// the current device (synchronising it).
struct ScratchChunk {
  void* p = nullptr;
  size_t size = 0;
  int dev = 0;
  hipEvent_t ev = nullptr;
  hipStream_t st = nullptr;  // the stream of its last use
};
hipError_t scratch_chunk_get(size_t bytes, hipStream_t st, ScratchChunk* out);
void scratch_chunk_put(const ScratchChunk& c, hipStream_t st);
void scratch_trim();
// Query cuts and dump launches of the filter pass (vs_x1_cuts.hip, "Query
// cuts"): bkey[q] = the verification's bound B of query q; x1_dump_applies:
// the pass of this mode and plane has a dump form: inner product on either
// plane, the augmented L2 among them, never the cosine (launch_gemm_topk_x1 then
// sets the cuts after its first launch and dumps in the others; the host runs
// launch_x1_replay after it, and the verification must get the same cuts).
hipError_t launch_qbound(int mode, const float* Q, int64_t ld, const float* qn, int filter,
                         const unsigned* stats, const float* qr2i8, int nq, double* bkey,
                         hipStream_t st, const BoundArgs* ba = nullptr);
bool x1_dump_applies(int mode, int filter);
int x1_dump_slots();  // the most dump slots per lane list worth allocating
bool x1_pass_dumps(int ntotal, int nsplit);  // a pass this long has dump launches
// a.dstats[0] += dumps replayed, a.dstats[1] += lane lists out of slots
// (launch_gemm_topk_x1 calls it between its segments of dump launches)
hipError_t launch_x1_replay(const X1Args& a, Partials part, hipStream_t st);
// Lists -> final (D, I) rows of k entries each (row stride ldo), labels offset by id_base.
// Inner product applies faiss's tie rule unless `raw` (plain lexicographic
// (key, label) order, the per-shard half of an exact sharded merge).  With
// `qlist`, list q belongs to query qlist[q] (emitted to that row) and only
// q < *qcount are merged (device-side count; the grid covers nq).
hipError_t launch_merge_partials(int mode, Partials part, int nq, int k, int64_t id_base,
                                 float min_score, float* D, int64_t* I, int64_t ldo,
                                 hipStream_t st, int raw = 0, const int* qlist = nullptr,
                                 const int* qcount = nullptr);
// Shard lists [nparts][nq][k_in] (scores, int64 labels) -> [nq][k].
hipError_t launch_merge_parts(int mode, const float* Dp, const int64_t* Ip, int nparts,
                              int nq, int k_in, int k, float* D, int64_t* I, hipStream_t st);
// The exact-key stream (vs_exact.hip): for the gathered slots
// slots[s0 .. s0 + min(*count - s0, nslot)) of a query batch whose rows sit at
// Q + slot * ld (aux values qaux[slot]: |q|^2 for L2, 1/|q| for cosine; qrow[slot]:
// the row to exclude, or -1; qrow may be null), the top-KP of every row by the
// rescoring's exact key (fp64 sums, vs_x1_device.h exact_key), as part.P lists
// per slot (part.P row blocks).  NQ queries per group: exact_stream_nq(ld)
// (0: ld too large for the LDS staging).
struct ExactStreamArgs {
  const float* X = nullptr;     // fp32 rows [ntotal][ld]
  const float* xn = nullptr;    // |x|^2 (L2)
  const float* xinv = nullptr;  // 1/|x| (cosine)
  int64_t ld = 0;
  int ntotal = 0;
  const float* Q = nullptr;
  const float* qaux = nullptr;
  const int* qrow = nullptr;
  const int* slots = nullptr;
  const int* count = nullptr;
  int s0 = 0, nslot = 0;
  // per query (indexed like slots' entries): only entries lexicographically
  // after (fkey, fid) enter (a page of the paged engine); null: no floor
  const float* fkey = nullptr;
  const int* fid = nullptr;
};
int exact_stream_nq(int64_t ld);
hipError_t launch_exact_stream(int KP, int mode, const ExactStreamArgs& a, Partials part,
                               hipStream_t st);
// The paged exact engine (vs_support.hip, "paged exact engine"; vs_engines.hip
// run_paged).  Dacc/Iacc [n][KA]: the pages side by side (scores, local rows).
// page_init: member/active flags (every q < n, or gl[0 .. *gc) of zeroed rows)
// and the first page's floor (-inf, -1) for fkey/fid[0 .. nfloor).
hipError_t launch_page_init(int n, int nfloor, const int* gl, const int* gc, int* member,
                            int* active, float* fkey, int* fid, hipStream_t st);
// After page `page`: active[q] = query q needs the next page (its page was full
// and it has fewer than k entries, or `rule` and the k-th key's run of ties
// reaches the page's end below 2k - 1), fkey/fid = its floor (+inf when not).
hipError_t launch_page_step(const float* Dacc, const int64_t* Iacc, int64_t KA, int page, int n,
                            int64_t k, int rule, int mode, int* active, float* fkey, int* fid,
                            hipStream_t st);
// *out = *count > 0 ? n : 0 (the device-side count of a GEMV page's lists).
hipError_t launch_page_gate(const int* count, int n, int* out, hipStream_t st);
// The member queries' k outputs (faiss's inner-product rule when `rule`), rows
// q * k of D / I, labels + id_base, min_score applied as merge_partials does.
hipError_t launch_page_finish(int mode, float* Dacc, int64_t* Iacc, int64_t KA, int n, int64_t k,
                              int rule, const int* member, int64_t id_base, float min_score,
                              float* D, int64_t* I, hipStream_t st);
// out[r] = sum_j X[r][j]^2 for rows [r0, r0+n) (fp32 or bf16 rows).
hipError_t launch_row_norms(const void* X, int esize, int64_t ld, int64_t r0, int64_t n,
                            float* out, hipStream_t st);
// Pitched conversions: fp32 -> bf16 (round to nearest even, NaN kept) with zero
// padding of columns [cols, ldo); bf16 -> fp32 (exact widening); fp32 -> fp32
// rounded through bf16 (the value a bf16 index stores).
hipError_t launch_f32_to_bf16(const float* in, int64_t ldi, uint16_t* out, int64_t ldo,
                              int64_t rows, int64_t cols, hipStream_t st);
// bf16 plane (tile-major) of fp32 rows [r0, r0+n) of stride ld (ld elements
// per plane row, RNE).
hipError_t launch_bf16_plane(const float* X, int64_t ld, int64_t r0, int64_t n, uint16_t* plane,
                             hipStream_t st);
// Zeroes plane rows [r0, r0+n) of a tile-major plane with ldb bytes per row.
hipError_t launch_plane_zero_rows(char* plane, int64_t ldb, int64_t r0, int64_t n, hipStream_t st);
hipError_t launch_bf16_to_f32(const uint16_t* in, int64_t ldi, float* out, int64_t ldo,
                              int64_t rows, int64_t cols, hipStream_t st);
hipError_t launch_round_bf16(float* x, int64_t n, hipStream_t st);
// out[r] = 1/sqrt(norm[r]) (double-precision rsqrt rounded to float).
hipError_t launch_rsqrt(const float* norm, int64_t n, float* out, hipStream_t st);
// Counter-based synthetic rows into a pitched fp32 or bf16 buffer (zero padding d..ldo).
hipError_t launch_fill_synthetic(void* out, int esize, int64_t rows, int64_t d, int64_t ldo,
                                 uint64_t seed, int64_t row0, hipStream_t st);
// Same generator for an explicit list of generator row numbers (device int64).
hipError_t launch_fill_synthetic_ids(void* out, int esize, const int64_t* ids, int64_t rows,
                                     int64_t d, int64_t ldo, uint64_t seed, hipStream_t st);
// Fill n (D, I) pairs with the empty-result sentinel of `mode`.
hipError_t launch_fill_empty(int mode, float* D, int64_t* I, int64_t n, hipStream_t st);
// out[0 .. n) = 0 .. n-1 and *count = n (device): a gathered batch of every query.
hipError_t launch_iota(int* out, int n, int* count, hipStream_t st);
// Tombstones: rows[0 .. n) (device) filled with NaN elements and a NaN norm;
// the labels I[0 .. n) of a search (kernel rows + id_base) mapped to positions
// among the live rows (dead: the sorted tombstoned rows, ndead of them).
// scale (optional): the int8 plane's row factors, set to NaN too (the plane's
// keys of a tombstoned row are NaN and never enter a list).
hipError_t launch_fill_nan_rows(void* X, int64_t rowbytes, float* norms, int esize,
                                const int64_t* rows, int64_t n, hipStream_t st,
                                float* scale = nullptr);
hipError_t launch_label_map(int64_t* I, int64_t n, const int64_t* dead, int64_t ndead,
                            int64_t id_base, hipStream_t st);
// Stable compaction helper: copy the kept rows of [src0, src0+n) into tmp,
// given the sorted removed-row list (device).  Also moves the norms.
// Rows are `rowbytes` long (multiple of 16).
hipError_t launch_gather_kept(const void* X, const float* norms, int64_t rowbytes, int64_t src0,
                              int64_t n, const int64_t* removed, int64_t nrem, void* tmp,
                              float* tmp_norms, hipStream_t st);

// In-place updates (vs_update.hip; vs_api_update.hip vs_update_rows): staged
// row i of every array an index holds -> row rows[i] (device, n distinct rows
// inside the destination arrays).  The staged planes are tile-major over rows
// [0, n) (plane_offset) like the index's, ldb bytes per row; a null
// destination leaves that array out.  Scalars: norms, fscale, rn2[2], anorm,
// anorm_b, one float per row each.
struct UpdateScatter {
  const char* s_codes = nullptr;  // [n][rowbytes]
  char* codes = nullptr;
  int64_t rowbytes = 0;           // a multiple of 16
  const char* s_plane[2] = {nullptr, nullptr};
  char* plane[2] = {nullptr, nullptr};
  int64_t ldb[2] = {0, 0};        // multiples of 64
  static constexpr int kScalars = 6;
  const float* s_scal[kScalars] = {};
  float* scal[kScalars] = {};
};
hipError_t launch_update_scatter(const UpdateScatter& a, const int64_t* rows, int64_t n,
                                 hipStream_t st);

// Selector searches (vs_select.hip; vs_api_select.hip vs_selector_create / vs_search_sel).
// A selector is a bitmap over the rows in place (word r >> 5, bit r & 31) and
// the ascending list of the selected rows.
// Rows per compaction block: 256 words of 32 rows.
constexpr int kSelBlockRows = 8192;
// rbits[0 .. nwords) from the label bitmap (faiss IDSelectorBitmap layout over
// labels - id_base, nbits of them): row r is selected iff it is live (not in
// the sorted dead list) and the bit of its position among the live rows is set.
// nwords covers whole compaction blocks; bits of rows >= ntotal are clear.
hipError_t launch_sel_row_bits(const uint8_t* lbits, int64_t nbits, const int64_t* dead,
                               int64_t ndead, int ntotal, uint32_t* rbits, int64_t nwords,
                               hipStream_t st);
// Compaction of the set bits: bsum[b] = the set bits of block b, then the
// exclusive scan of bsum in place and *count = their total, then the scatter
// of the set rows, ascending, to list[0 .. *count) and the padding of the list
// to a multiple of kBN with its last row.
hipError_t launch_sel_block_counts(const uint32_t* rbits, int nblocks, int* bsum, hipStream_t st);
hipError_t launch_sel_scan(int* bsum, int nblocks, int* count, hipStream_t st);
hipError_t launch_sel_scatter(const uint32_t* rbits, int nblocks, const int* boff,
                              const int* count, int* list, hipStream_t st);
// Route (b): the entries of Din / Iin ([nq][k_in], labels = row + id_base, -1
// empty) whose row bit is set, in order, as the first k_out entries of every
// query's row of Dout / Iout (padded with the empty result of `mode`).
hipError_t launch_sel_drop(int mode, const float* Din, const int64_t* Iin, int nq, int k_in,
                           const uint32_t* rbits, int64_t id_base, float* Dout, int64_t* Iout,
                           int k_out, hipStream_t st);
// gemm_topk over the rows list[0 .. count) (list padded to a multiple of kBN
// with a valid row): the lists hold rows in place, 2 * nsplit lists per query.
// Modes IP and L2 (norm expansion), fp32 or bf16 rows.
hipError_t launch_gemm_topk_rows(int KP, int mode, const void* X, const float* xaux,
                                 const void* Q, const float* qaux, int64_t ld, int esize,
                                 const int* list, int count, int nq_pad, int nsplit,
                                 Partials part, hipStream_t st);
// gemv_topk over the rows list[0 .. count): modes IP and L2D, nq <= kGemvMaxQ,
// one list per query per block (part.P == nblocks).
hipError_t launch_gemv_topk_rows(int KP, int mode, int nq, const void* X, int esize,
                                 const float* Q, int64_t ld, const int* list, int count,
                                 int nblocks, Partials part, hipStream_t st);

// Range search (vs_range.hip; vs_api_range.hip vs_range_search).
// The candidate passes: gemm_topk's loop with a threshold epilogue.  A row is
// a candidate of query q iff row < ntotal and its GEMM key (IP: -score, L2: the
// norm expansion) is <= thr[q] (nq_pad entries; NaN admits nothing).  fill =
// false: cnt[q * nsplit + split] = the query's candidates among the split's
// rows.  fill = true, with off = the exclusive scan of cnt (nq_pad * nsplit + 1
// entries): the candidates' rows, ascending, at cand[off[q * nsplit + split] ..);
// nothing is written outside a segment, and *err = 1 if a segment does not
// come out as counted.  MODE_COS (the range self-join): Q = the stored rows
// from the first query row on, qaux / xaux = 1/|row| (qaux from that row on),
// key -(ip * (qaux[q] * xaux[row])).  upper_q0 >= 0 (MODE_COS only; the first
// query's row): query tile t reads the row tiles from the one that holds row
// upper_q0 + t * kBQ on, and its splits divide that range.
hipError_t launch_gemm_range(bool fill, int mode, const void* X, const float* xaux, const void* Q,
                             const float* qaux, int64_t ld, int esize, int ntotal, int nq_pad,
                             int nsplit, const float* thr, int* cnt, const int64_t* off,
                             int* cand, int* err, hipStream_t st, int64_t upper_q0 = -1);
// out[0] = bits of the largest non-NaN norm of rows [0, n), out[1] = out[2] = 0
// (the `stats` of launch_qbound with BoundArgs::rows_exact); part = scratch of
// range_norm_max_parts() entries.
int range_norm_max_parts();
hipError_t launch_range_norm_max(const float* norms, int64_t n, unsigned* part, unsigned* out,
                                 hipStream_t st);
// thr[q] = radkey + bkey[q] rounded up for q < nq (NaN radkey: NaN; a bound
// that is NaN: +inf), NaN for the padding queries [nq, nq_pad).  bstride = 0:
// bkey[0] is every query's bound.
hipError_t launch_range_thr(const double* bkey, int nq, int nq_pad, float radkey, float* thr,
                            hipStream_t st, int bstride = 1);
// off[0 .. n] = the exclusive scan of cnt[0 .. n) (off[n] = the total).
hipError_t launch_range_scan(const int* cnt, int64_t n, int64_t* off, hipStream_t st);
// Candidate c of query q (off[q * nsplit] <= c < off[(q + 1) * nsplit]):
// ekey[c] = its exact key as a score (exact_key<mode>: distance, or inner
// product), flag[c] = the key passes the radius strictly (L2 / L2D: key <
// radius, IP: score > radius) and, with rbits, the row's selector bit is set.
hipError_t launch_range_verify(int mode, const int* cand, int64_t total, const int64_t* off,
                               int nsplit, int nq, const void* X, int xesize, const float* xn,
                               const float* Q, const float* qn, int64_t ld, int ntotal,
                               float radius, const uint32_t* rbits, float* ekey, uint8_t* flag,
                               hipStream_t st);
// The range self-join's verification: query q is row q0 + q of X, candidate c
// as above; ekey[c] = the exact cosine (fp64 sum of the two stored rows'
// products, exact_key<MODE_COS> with rinv = 1/|row| on both sides), flag[c] =
// ekey[c] >= min_sim and the row is not the query's (exclude_self) / comes
// after it (upper).
hipError_t launch_range_join_verify(const int* cand, int64_t total, const int64_t* off, int nsplit,
                                    int nq, const void* X, int xesize, const float* rinv,
                                    int64_t ld, int ntotal, int64_t q0, float min_sim,
                                    int exclude_self, int upper, float* ekey, uint8_t* flag,
                                    hipStream_t st, const int* qrows = nullptr);
// The row-list join's queries: row i < nq of Q (rows of rowbytes, a multiple of
// 16) = row qrows[i] of X and qaux[i] = rinv[qrows[i]]; zero rows / 0 for the
// padding slots [nq, nq_pad).  With `qrows` (device, nq entries),
// launch_range_join_verify's query q is row qrows[q] instead of q0 + q.
hipError_t launch_range_gather_rows(const void* X, int64_t rowbytes, const float* rinv,
                                    const int* qrows, int nq, int nq_pad, void* Q, float* qaux,
                                    hipStream_t st);
// hits[q] = the flags set among query q's candidates.
hipError_t launch_range_hits(const uint8_t* flag, const int64_t* off, int nsplit, int nq,
                             int* hits, hipStream_t st);
// Stable compaction of every query's flagged candidates to D (score) and I
// (row + id_base) at lims[q] (lims = the exclusive scan of hits).
hipError_t launch_range_emit(const int* cand, const float* ekey, const uint8_t* flag,
                             const int64_t* off, int nsplit, int nq, const int64_t* lims,
                             int64_t id_base, float* D, int64_t* I, hipStream_t st);

// Profile searches (vs_profile.hip; vs_api_profile.hip vs_search_excl / vs_mean_rows /
// vs_search_profiles).
// A class batch: dst row s = src row qmap[s] (rows of rowbytes, a multiple of
// 16) and daux[s] = saux[qmap[s]] for s < cnt, zero rows / 0 for the padding
// slots [cnt, nslot).  saux / daux may be null.
hipError_t launch_excl_gather(const void* src, int64_t rowbytes, const float* saux,
                              const int* qmap, int cnt, int nslot, void* dst, float* daux,
                              hipStream_t st);
// launch_sel_drop with one excluded set per query: slot s of Din / Iin
// ([nq][k_in], labels = row + id_base, -1 empty) is query q = qmap[s] (null: s);
// its entries whose row is not in rows[offs[q] .. offs[q + 1]) (ascending), in
// order, are the first k_out entries of row q of Dout / Iout (padded with the
// empty result of `mode`).
hipError_t launch_excl_drop(int mode, const float* Din, const int64_t* Iin, int nq, int k_in,
                            const int64_t* offs, const int64_t* rows, const int* qmap,
                            int64_t id_base, float* Dout, int64_t* Iout, int k_out,
                            hipStream_t st);
// out[q][0 .. d) = the weighted mean of the rows rows[offs[q] .. offs[q + 1])
// (rows in place, fp32 or bf16 of stride ld) with weights wts, divided by W[q]:
// fp32, list order, no FMA, a correctly rounded division (the kernel's header).
// Every segment holds at least one row; out has stride d.
hipError_t launch_mean_rows(const void* X, int esize, int64_t ld, int d, const int64_t* offs,
                            const int64_t* rows, const float* wts, const float* W, int64_t nq,
                            float* out, hipStream_t st);

// MMR searches (vs_mmr.hip; vs_api_mmr.hip vs_mmr_select / vs_search_mmr).
// The longest candidate list of a query: the staged engine's candidate limit.
constexpr int kMmrMaxFetch = 1024;
// rows[i] = the row in place of candidate label labels[i] (id_base applied; the
// sorted dead list skipped), -1 for the empty slot -1.  Any other label that is
// not one of the `live` labels also gives -1 and sets *bad to 1 (bad may be null).
hipError_t launch_mmr_rows(const int64_t* labels, int64_t n, const int64_t* dead, int64_t ndead,
                           int64_t id_base, int64_t live, int64_t* rows, int* bad, hipStream_t st);
// S[q][i] = cos(Q[q], row rows[q][i]) and NN[q][i] = |row|^2 in fp64 (fixed
// summation order, the unit's header) for nq <= 65535 queries (Q: fp32, stride
// d) of F <= kMmrMaxFetch candidates each; an empty slot: S = 0, NN = -1.
hipError_t launch_mmr_sims(const void* X, int esize, int64_t ld, int d, const float* Q,
                           const int64_t* rows, int nq, int F, double* S, double* NN,
                           hipStream_t st);
// The greedy MMR selection over S / NN: pos[q][0 .. k) = the picks' positions
// in pick order, -1 past min(k, candidates).  Dout != null: also the picks'
// entries of Dc / Ic ([q][F]) into Dout / Iout ([q][k]), padded with (pad, -1).
hipError_t launch_mmr_pick(const void* X, int esize, int64_t ld, const int64_t* rows, int nq,
                           int F, int k, double lambda, const double* S, const double* NN,
                           int* pos, const float* Dc, const int64_t* Ic, float pad, float* Dout,
                           int64_t* Iout, hipStream_t st);

// Distinct searches (vs_distinct.hip; vs_api_distinct.hip vs_search_distinct).
// The most groups one collapse keeps: its LDS table holds 2 * 2047 groups
// (inner product under faiss's rule at k = 1024 reads 2k - 1 = 2047).
constexpr int kDistinctMaxK = 1024;
// Slot s of Din / Iin ([ns][w] raw entries: ascending (key, label), labels =
// row + id_base, -1 after the end) -> row s of Dout / Iout ([ns][kout]): the
// first entry of every group in window order (group[row], ngroup rows; -1: the
// row is its own group), at most `need` of them, padded with the empty result
// of `mode`; kept[s] (may be null) = how many; unsettled[qmap ? qmap[s] : s] =
// 1 when the window was too short (fewer than `need` kept, no -1 entry seen,
// and not w_is_all), else 0.  need <= 2047.
hipError_t launch_distinct_collapse(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                                    const int32_t* group, int64_t ngroup, int64_t id_base,
                                    int need, bool w_is_all, const int* qmap, float* Dout,
                                    int64_t* Iout, int kout, int* kept, int* unsettled,
                                    hipStream_t st);
// Row qmap[s] of Dout / Iout = row s of Din / Iin ([ns][k]).
hipError_t launch_distinct_scatter(const float* Din, const int64_t* Iin, int ns, int k,
                                   const int* qmap, float* Dout, int64_t* Iout, hipStream_t st);

// Example searches (vs_examples.hip; vs_api_examples.hip vs_search_examples).
constexpr int kExamplesMaxK = 1024;   // the emit sorts 2 x 1024 packed keys in LDS
constexpr int kExamplesMaxList = 64;  // positives, and negatives, of one user
// out[i][0 .. d) = row rows[i] (in place) as fp32, bf16 widened exactly.
hipError_t launch_examples_gather(const void* X, int esize, int64_t ld, int d, const int64_t* rows,
                                  int64_t n, float* out, hipStream_t st);
// One user of a round's batch.
struct ExamplesUser {
  int pos0 = 0;      // the first of its positives' slots in the round's windows
  int a = 0;         // positives (1 .. kExamplesMaxList)
  int neg0 = 0;      // the first of its negatives' rows in the staged negatives
  int b = 0;         // negatives (0 .. kExamplesMaxList)
  int out = 0;       // its row of D / I / E and of the unsettled flags
  int tbits = 0;     // its table holds 1 << tbits slots, at least 2 a w
  int64_t toff = 0;  // the table's first slot in trow / tval
  int64_t coff = 0;  // its first candidate slot in ckey / cpos (a w of them)
};
// A round's windows -> the users' answers (the unit's header): Din / Iin
// [slots][w] raw entries (labels = row + id_base, -1 after the end); trow (all
// bytes 0xFF) / tval (all bytes 0xFF) the tables, ccount (zeroed) [nu], F [nu],
// ckey / cpos the candidates; X / xn the index's rows and norms, Qp / qp the
// round's positives (fp32 rows of stride ld, by slot) and their |e|^2 (L2),
// Qn / qn the staged negatives likewise.  Writes rows `out` of D / I / E
// ([..][k]) and unsettled[out]; *err = 1 if a table or a candidate list
// overflowed (the sizes above make that impossible; the call must fail).
struct ExamplesCollapse {
  int mode = MODE_IP;
  const ExamplesUser* users = nullptr;  // device, nu entries
  int nu = 0, amax = 0, tbits_max = 0;  // the batch's longest list and largest table
  bool any_neg = false;                 // some user of the batch has negatives
  const float* Din = nullptr;
  const int64_t* Iin = nullptr;
  int w = 0;
  bool w_is_all = false;
  int64_t id_base = 0;
  int* trow = nullptr;
  unsigned long long* tval = nullptr;
  unsigned long long* F = nullptr;
  int* ccount = nullptr;
  unsigned long long* ckey = nullptr;
  int* cpos = nullptr;
  int* err = nullptr;
  const void* X = nullptr;
  int xesize = 4;
  const float* xn = nullptr;
  const float* Qp = nullptr;  // the round's positives, by slot
  const float* qp = nullptr;
  const float* Qn = nullptr;
  const float* qn = nullptr;
  int64_t ld = 0;
  int k = 0;
  float* D = nullptr;
  int64_t* I = nullptr;
  int* E = nullptr;
  int* unsettled = nullptr;
};
hipError_t launch_examples_collapse(const ExamplesCollapse& c, hipStream_t st);

// Where searches (vs_where.hip; vs_api_where.hip vs_attrs_* / vs_search_where).
constexpr int kWhereMaxCols = 4;
// One query's predicate: column c < ncol is tested iff bit c of cmask is set
// and passes iff lo[c] <= v && v <= hi[c] (a NaN value fails); the tag tests
// are any_of == 0 || (tags & any_of), (tags & all_of) == all_of and
// (tags & none_of) == 0.  on == 0: a padding slot, nothing passes.
struct WherePred {
  float lo[kWhereMaxCols];
  float hi[kWhereMaxCols];
  unsigned long long any_of, all_of, none_of;
  unsigned cmask;
  unsigned on;
};
static_assert(sizeof(WherePred) == 64, "sixteen dwords");
// The attributes of the rows in place (device): column c of row r at
// cols[c * stride + r]; tags null: every row's tags are 0; live null: every
// row is live, else live[r] == 0 marks a tombstoned row (it passes nothing).
struct WhereAttrs {
  const float* cols = nullptr;
  const unsigned long long* tags = nullptr;
  const uint8_t* live = nullptr;
  int ncol = 0;
  int64_t stride = 0;
};
// The by-row arrays of a tombstoned index from the by-label ones (nlab labels,
// column stride nlab; by row: stride ntotal): row r holds the attributes of
// label r - (dead rows below r); a dead row NaN columns, tags 0, live 0.
hipError_t launch_attrs_spread(const float* lcols, const unsigned long long* ltags, int64_t nlab,
                               int ncol, const int64_t* dead, int64_t ndead, int64_t ntotal,
                               float* rcols, unsigned long long* rtags, uint8_t* live,
                               hipStream_t st);
// out[q] = the live rows of [0, nrows) that pass preds[q] (out is zeroed first).
hipError_t launch_attrs_count(const WhereAttrs& at, int64_t nrows, const WherePred* preds, int nq,
                              unsigned long long* out, hipStream_t st);
// Slot s of Din / Iin ([ns][w] raw entries: ascending (key, label), labels =
// row + id_base, -1 after the end) is query q = qmap ? qmap[s] : s; its entries
// whose row passes preds[q], in order, at most `need` of them, are the first
// entries of row s of Dout / Iout ([ns][kout], padded with the empty result of
// `mode`); unsettled[q] = 1 when the window was too short (fewer than `need`
// kept, no -1 entry seen, and not w_is_all), else 0.
hipError_t launch_where_drop(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                             const WhereAttrs& at, const WherePred* preds, const int* qmap,
                             int64_t id_base, int need, bool w_is_all, float* Dout, int64_t* Iout,
                             int kout, int* unsettled, hipStream_t st);
// The predicated scan's kernels: launch_gemm_topk / launch_gemv_topk at KP = 64
// with floors, where a row enters query q's list only if it passes preds[q]
// and is not in xrows[xoffs[q] .. xoffs[q + 1]) (ascending rows in place; both
// null: no exclusions).  preds / xoffs / the floors are indexed like qaux (by
// the query's row in Q: qlist[slot] for the GEMM, 0 .. nq - 1 for the GEMV,
// whose preds hold kGemvMaxQ entries, `on` clear past nq).  The boosted scan's
// launchers take the same arguments with specs given (indexed like preds);
// the where scan's take them with specs null.
struct BoostSpec;
struct GemmWhereArgs {
  const void* X = nullptr;
  const float* xaux = nullptr;
  const void* Q = nullptr;
  const float* qaux = nullptr;
  int64_t ld = 0;
  int esize = 4, ntotal = 0, nq_pad = 0, nsplit = 0;
  const int* qlist = nullptr;   // slot s is query row qlist[s], s < *qcount
  const int* qcount = nullptr;
  const float* fkey = nullptr;
  const int* fid = nullptr;
  WhereAttrs at;
  const WherePred* preds = nullptr;
  const int64_t* xoffs = nullptr;
  const int64_t* xrows = nullptr;
  const BoostSpec* specs = nullptr;
};
hipError_t launch_gemm_topk_where(int mode, const GemmWhereArgs& a, Partials part,
                                  hipStream_t st);
struct GemvWhereArgs {
  const void* X = nullptr;
  const float* Q = nullptr;
  int64_t ld = 0;
  int esize = 4, ntotal = 0, nblocks = 0;
  const float* fkey = nullptr;
  const int* fid = nullptr;
  const int* run = nullptr;  // optional: every block exits when *run == 0
  WhereAttrs at;
  const WherePred* preds = nullptr;
  const int64_t* xoffs = nullptr;
  const int64_t* xrows = nullptr;
  // optional: += the rows the launch loaded (the where scan only)
  unsigned long long* streamed = nullptr;
  const BoostSpec* specs = nullptr;
};
// Modes IP and L2D, nq <= kGemvMaxQ, one list per query per block (part.P ==
// nblocks).  A 4-row step none of whose rows passes any query's predicate is
// not loaded.
hipError_t launch_gemv_topk_where(int mode, int nq, const GemvWhereArgs& a, Partials part,
                                  hipStream_t st);

// Boosted searches (vs_boost.hip; vs_api_boost.hip vs_search_boost): exact
// top-k by final_key = fl32(key - b), b a per-query function of the row's
// attributes (boost_value, vs_boost_value.h).
constexpr int kBoostMaxTags = 4;
constexpr int kBoostMaxWindow = 1023;  // boost_rerank sorts a window in LDS
// One query's boost: column c contributes by kind[c] (0 none, 1 near, 2 ramp)
// with (t, s, w, miss)[c]; tag term j adds bonus[j] when (tags & mask[j]) != 0;
// U >= b >= L for every row (boost_bounds).
struct BoostSpec {
  float t[kWhereMaxCols], s[kWhereMaxCols], w[kWhereMaxCols], miss[kWhereMaxCols];
  unsigned long long mask[kBoostMaxTags];
  float bonus[kBoostMaxTags];
  float U, L;
  unsigned char kind[kWhereMaxCols];
  unsigned pad;
};
static_assert(sizeof(BoostSpec) == 128, "thirty-two dwords");
// Route A: slot s of Din / Iin ([ns][w], w <= kBoostMaxWindow, raw entries as
// launch_where_drop reads them) is query q = qmap ? qmap[s] : s.  The entries
// whose row passes preds[q] are ranked by (final_key, label); the first k go to
// row s of Dout / Iout ([ns][k], padded).  state[q] = 0 when the slot is
// settled (the window reached the end of the rows, or k entries were kept and
// final_key[k-1] < fl32(K_w - U) with K_w the window's last raw key), else 1,
// or 2 when its deficit final_key[k-1] - fl32(K_w - U) exceeds giveup times the
// window's raw key spread K_w - K_0 (giveup < 0: never).  deficit / spread
// (optional, by query): those two values.
hipError_t launch_boost_rerank(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                               const WhereAttrs& at, const WherePred* preds,
                               const BoostSpec* specs, const int* qmap, int64_t id_base, int k,
                               bool w_is_all, float giveup, float* Dout, int64_t* Iout,
                               int* state, float* deficit, float* spread, hipStream_t st);
// Route B: launch_gemm_topk_where / launch_gemv_topk_where with the lists, the
// floors and the partials in final keys; a.specs must be given.
hipError_t launch_gemm_topk_boost(int mode, const GemmWhereArgs& a, Partials part,
                                  hipStream_t st);
hipError_t launch_gemv_topk_boost(int mode, int nq, const GemvWhereArgs& a, Partials part,
                                  hipStream_t st);

// Bonus searches (vs_bonus.hip; vs_api_bonus.hip vs_search_bonus): exact top-k
// by final_key = fl32(fl32(key - b) - s), s a per-(query, row) number the
// caller lists for at most kBonusMaxList rows per query.
constexpr int kBonusMaxList = 1024;  // bonus_merge sorts a query's list in LDS
// A chunk's lists: query q (0 .. nq - 1, the chunk's own numbering) lists the
// rows in place rows[offs[q] .. offs[q + 1]) (ascending and distinct within a
// query, every one a live row) with the bonuses vals[...]; e0 = offs[0] and
// total = offs[nq] - offs[0] as the host knows them.
struct BonusLists {
  const int64_t* offs = nullptr;
  const int64_t* rows = nullptr;
  const float* vals = nullptr;
  int64_t e0 = 0, total = 0;
  int nq = 0;
};
// Entry e of the lists gets skey[e - e0] = the final key of its row for its query:
// the rescoring's key (wave_dot's fp64 sum rounded once, exact_key<mode>; mode
// IP, L2 or L2D; qn / xn the squared norms of MODE_L2), minus the query's boost
// of the row (specs null: +0), minus the bonus; srow[e - e0] = the row, or -1 (and
// key FLT_MAX) when the row fails the query's predicate (preds null: no
// predicate; `at` is read only with preds or specs) or is in its exclusion
// segment xrows[xoffs[q] .. xoffs[q + 1]) (both null: none).  preds, specs and
// xoffs are indexed by the chunk's query.
struct BonusScoreArgs {
  int mode = MODE_IP;
  const void* X = nullptr;
  int esize = 4;
  const float* xn = nullptr;
  const float* Q = nullptr;
  const float* qn = nullptr;
  int64_t ld = 0;
  BonusLists lists;
  WhereAttrs at;
  const WherePred* preds = nullptr;
  const BoostSpec* specs = nullptr;
  const int64_t* xoffs = nullptr;
  const int64_t* xrows = nullptr;
  float* skey = nullptr;
  int64_t* srow = nullptr;
};
hipError_t launch_bonus_score(const BonusScoreArgs& a, hipStream_t st);
// Query q's result: the first k of the two-way merge, by (final key, label), of
// its base result Din / Iin ([nq][k], ascending (key, label) with D the key
// (L2) or its negative (inner product), labels = row + id_base, -1 after the
// end) without the entries whose row the query lists, and its scored list
// entries (skey / srow as launch_bonus_score leaves them), into
// row q of Dout / Iout ([nq][k], padded with the empty result of `mode`; not
// Din / Iin).  *entered (optional) += the list entries written.
hipError_t launch_bonus_merge(int mode, const float* Din, const int64_t* Iin, int k,
                              const BonusLists& lists, const float* skey, const int64_t* srow,
                              int64_t id_base, float* Dout, int64_t* Iout,
                              unsigned long long* entered, hipStream_t st);

}  // namespace vs
