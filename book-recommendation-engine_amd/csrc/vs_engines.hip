// vs_engines.hip — the engine dispatch behind every search: run_topk chooses
// among the fused exact GEMM (run_gemm), the filter-and-verify stages over the
// index's planes (run_filter_verify, run_gemm_rescored) and the paged exact
// engine (run_paged), with the environment switches that A/B them.
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// The environment switches of this unit (all for A/B runs and the equality
// tests; the defaults are the product).  "Read": `process` = once, at the
// first search of the process, and kept; `search` = at every search, never per
// launch, so a test may flip it between two searches of one process.
//
//  name              values (default)           read     what                            flipped by
//  VS_ENGINE         fp32|bf16v|i8v (auto)      search   the engine of indexes left on   -
//                                                        VS_ENGINE_AUTO
//  VS_X1_WIDE        0|1 (1)                    process  wide verification of flagged    -
//                                                        queries
//  VS_X1_DUMP        0|1 (1)                    process  dump launches in the filter     tools/ab_dump.sh
//                                                        pass (0: list launches only)
//  VS_X1_DUMP_MFMA   32 (16)                    search   MFMA shape of the int8 IP dump  test_gpu_dump_shape,
//                                                        launches                        test_x1_plan_host
//  VS_X1_RECUT       0|1|2 (1)                  search   query cuts after every replay   test_gpu_cut_refresh,
//                                                        (0 once, 2 separate kernels)    test_gpu_exact_cut
//  VS_X1_ECUT        0|1 (1)                    search   exact-key cuts of the int8 IP   test_gpu_exact_cut
//                                                        pass over fp32 rows
//  VS_X1_WGS         n > 0 (256 / 512)          search   workgroups per filter-pass      -
//                                                        launch (plan_stage)
//  VS_X1_SPLIT_MULT  n > 1 (1)                  process  times as many database splits   -
//  VS_SMALL_BATCH    gemv|skinny (by shape)     process  kernel of small exact batches   -
//  VS_SMALL_FILTER   0|1 (1)                    search   small batches through the       test_gpu_parity
//                                                        staged engine
//  VS_SMALL_L2D      0|1 (1)                    search   ... L2 calls under 20 queries   -
//                                                        too
//  VS_SKINNY_DEEP    0|1 (1)                    search   the deep stage's small-count    test_gpu_parity
//                                                        kernel
//  VS_TAIL_WAIT      0|1 (1)                    search   read the flagged count, skip    test_gpu_cut_refresh,
//                                                        empty later stages              test_gpu_exact_cut,
//                                                                                        test_gpu_streams
//  VS_EXACT_STREAM   0|1 (1)                    search   exact-key stream behind the     -
//                                                        last stage's fp32 bound
// On/off switches parse as env_on: unset or a nonzero number is on
// (VS_X1_WIDE went by its first character once; no tool or test sets it).
bool env_on(const char* name) {
  const char* e = getenv(name);
  return !e || atoi(e) != 0;
}
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

int engine_from_env() {
  const char* e = getenv("VS_ENGINE");
  if (!e) return VS_ENGINE_AUTO;
  if (strcmp(e, "fp32") == 0) return VS_ENGINE_FP32_MFMA;
  if (strcmp(e, "bf16v") == 0) return VS_ENGINE_BF16_VERIFY;
  if (strcmp(e, "i8v") == 0) return VS_ENGINE_I8_VERIFY;
  return VS_ENGINE_AUTO;
}
// The wide verification of flagged queries.
bool wide_enabled() {
  static const bool on = env_on("VS_X1_WIDE");
  return on;
}
// Dump launches in the filter pass (0: every launch a list launch).
bool dump_enabled() {
  static const bool on = env_on("VS_X1_DUMP");
  return on;
}
// The MFMA shape of the int8 inner-product dump launches (vs_gemm_x1.hip,
// x1_has_s16): 16x16x64 by default, 32 runs them on the 32x32x32 form.  Both
// forms leave the same lists.
bool dump_mfma32() { return env_int("VS_X1_DUMP_MFMA", 0) == 32; }
// Query cuts taken again after every replay of a cutting pass (0 sets them
// once, after the list launch; 2 refreshes them with the separate replay and
// cut kernels instead of the fused one).
int recut_mode() {
  const int v = env_int("VS_X1_RECUT", 1);
  return v == 0 ? 0 : v == 2 ? 2 : 1;
}
// Exact-key cuts of the int8 inner-product pass over fp32 rows (0 keeps
// a_M + 2B alone).
bool ecut_enabled() { return env_on("VS_X1_ECUT"); }
// The filter pass's workgroup target (plan_stage; 0: its default).
int x1_wgs_env() { return env_int("VS_X1_WGS", 0); }
// More (shorter) database splits = more lane lists per query.
int x1_split_mult() {
  static const int mult = std::max(env_int("VS_X1_SPLIT_MULT", 1), 1);
  return mult;
}
// The kernel of small exact batches: "gemv" / "skinny" (null: by shape).
const char* small_batch_pref() {
  static const char* pref = getenv("VS_SMALL_BATCH");
  return pref;
}
// Small batches through the staged engine's skinny passes (0 keeps the exact
// streaming kernels), over indexes of at least kSmallFilterMinRows rows.
constexpr int64_t kSmallFilterMinRows = 1 << 18;
bool small_filter_on() { return env_on("VS_SMALL_FILTER"); }
// L2 calls of fewer than 20 queries (faiss's sequential formula: the
// verification rescored with MODE_L2D) through the planes too (0 keeps them on
// the exact GEMV).
bool small_l2d_ok(int mode, const SearchArgs& a) {
  return !(mode == MODE_L2 && a.l2_direct) || env_on("VS_SMALL_L2D");
}
// The deep stage's small-count kernel.
bool skinny_deep_on() { return env_on("VS_SKINNY_DEEP"); }
// The exact-key stream behind the last stage's fp32 bound (run_gemm_rescored,
// run_paged; 0 keeps the fp32 GEMM's candidates / pages).
bool exact_stream_on() { return env_on("VS_EXACT_STREAM"); }

// The exact engine on fp32 / bf16 rows: the fused MFMA GEMM + merge.  With
// qlist/qcount, the batch is the gathered queries qlist[0 .. *qcount)
// (device-side count) and the results go to their rows of D / I.
int run_gemm(vs_index* idx, const SearchArgs& a, int need, hipStream_t st,
              const int* qlist = nullptr, const int* qcount = nullptr) {
  const int KP = kp_for(need);
  const int ntotal = (int)idx->ntotal;
  Scratch scr(st);
  Partials part;
  part.KP = KP;
  const int nqt = a.nq_pad / kBQ;
  const int ntiles = (ntotal + kBN - 1) / kBN;
  const int nsplit = qlist ? gathered_nsplit(ntiles) : gemm_nsplit(ntiles, nqt);
  part.P = 2 * nsplit;
  const size_t n = (size_t)a.nq_pad * part.P * KP;
  VS_HIP(scr.alloc((void**)&part.key, n * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&part.id, n * sizeof(int)), "vs: scratch");
  const void* qmat = a.qb16 ? a.qb16 : (const void*)a.qbuf;
  {
    KernelTimer tm(st, qlist ? nullptr : "gemm_topk");
    VS_HIP(launch_gemm_topk(KP, a.mode, idx->codes, a.xaux, qmat, a.qaux, idx->ld, idx->esize,
                            ntotal, a.nq_pad, nsplit, a.self0, part, st, qlist, qcount),
           "vs: gemm_topk launch");
    tm.stop();
  }
  VS_HIP(launch_merge_partials(a.mode, part, qlist ? a.nq_pad : a.nq, a.k, idx->id_base,
                               a.min_score, a.D, a.I, a.k, st, a.raw, qlist, qcount),
         "vs: merge launch");
  return VS_OK;
}

int adaptive_record(vs_index* idx, const int* handed, int n, hipStream_t st);
int run_paged(vs_index* idx, const SearchArgs& a, hipStream_t st, const int* gl = nullptr,
              const int* gc = nullptr);
int run_gemm_rescored(vs_index* idx, const SearchArgs& a, int need, int KF, int plane,
                      hipStream_t st, const int* gl, const int* gc);

int run_filter_verify(vs_index* idx, const SearchArgs& a, int need, int KF, hipStream_t st,
                      int plane, bool last_plane, bool deep = false, const int* gl = nullptr,
                      const int* gc = nullptr);

// Whether a search reads the count of queries a stage leaves flagged (a 4-byte
// copy to pinned memory and a wait on the stream) and enqueues the later stages
// only when some remain.  Host-output calls wait for their results anyway;
// device-output calls wait too: the later stages over an empty count are ~45
// launches of ~5 us each (0.25 ms of a 2.39-ms C2 search, 0.58 ms of the
// 1.25M-row rank's 10.5 ms, profiles/r06tl), far more than the wait.  Not on a
// capturing stream (a graph keeps every launch).  VS_TAIL_WAIT=0 keeps every
// launch.
bool tail_wait_on(const SearchArgs& a, hipStream_t st) {
  if (!env_on("VS_TAIL_WAIT")) return false;
  if (a.host_wait) return true;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs == hipStreamCaptureStatusNone;
}

// The device-side count *dcount once the stream has reached this point (one
// pinned int per host thread).
int read_count(const int* dcount, hipStream_t st, int* out) {
  static thread_local int* pin = nullptr;
  if (!pin) VS_HIP(hipHostMalloc((void**)&pin, sizeof(int), hipHostMallocPortable), "vs: count");
  VS_HIP(hipMemcpyAsync(pin, dcount, sizeof(int), hipMemcpyDeviceToHost, st), "vs: count");
  VS_HIP(hipStreamSynchronize(st), "vs: count");
  *out = *pin;
  return VS_OK;
}

// One stage of the filter-and-verify engine: what its steps (below, in the
// order run_filter_verify calls them) share.  Scratch is a bump allocator and
// everything is stream-ordered, so the steps' order of allocations and
// launches is part of the result.
struct Stage {
  vs_index* idx;
  const SearchArgs& a;
  hipStream_t st;
  const int need, KF, plane;
  const bool last_plane, deep;
  const int *gl, *gc;   // stages after the first: the batch is queries gl[0 .. *gc) of `a`
  const bool gathered;  // gl != nullptr
  const bool i8;        // plane == FILTER_I8
  // L2: the pass is the inner product of the augmented rows and queries
  // (vs_index::aug_m, either plane); its lists are mapped to L2 keys after it
  const bool aug;
  const int kmode;  // the pass's own metric
  // the verification's exact keys: an L2 call of fewer than 20 queries takes
  // faiss's sequential formula (the rounded exact sum of (x - q)^2), larger
  // ones its BLAS formula
  const int vmode;
  const int ntotal;
  const int L;  // x1_lane_len()
  Scratch scr;
  bool small = false;  // StagePlan::small
  int nq = 0;          // slots of this stage
  int qa_rows = 0;     // rows of Q / qaux
  X1Args x;
  Partials part;  // lane lists: L entries each
  // this stage's fp32 query rows and aux values: the staged batch, the stored
  // rows (self-joins), or a gathered copy of the flagged ones
  const float* Q = nullptr;
  const float* qaux = nullptr;
  const float* qs = nullptr;   // int8: query scales
  const float* qr2 = nullptr;  // int8: query residual norms (for the bound)
  int* qrow = nullptr;
  const unsigned* stats = nullptr;  // the index's maxima (kept by add / remove)
  BoundArgs ba;
  int* qlist = nullptr;   // merge_and_verify: the queries still flagged, as slots of this stage
  int* qcount = nullptr;  // [0] after the first check, [1] after the wide one

  Stage(vs_index* idx_, const SearchArgs& a_, int need_, int KF_, hipStream_t st_, int plane_,
        bool last_plane_, bool deep_, const int* gl_, const int* gc_)
      : idx(idx_), a(a_), st(st_), need(need_), KF(KF_), plane(plane_), last_plane(last_plane_),
        deep(deep_), gl(gl_), gc(gc_), gathered(gl_ != nullptr), i8(plane_ == FILTER_I8),
        aug(a_.mode == MODE_L2 && idx_->l2aug()), kmode(aug ? MODE_IP : a_.mode),
        vmode(a_.mode == MODE_L2 && a_.l2_direct ? MODE_L2D : a_.mode), ntotal((int)idx_->ntotal),
        L(x1_lane_len()), scr(st_) {}
};

// Step 0: the stage's sizes (plan_stage, vs_host.h) and its lane lists.
int size_lists(Stage& s) {
  StageShape sh;
  sh.mode = s.a.mode;
  sh.plane = s.plane;
  sh.KF = s.KF;
  sh.nq = s.a.nq;
  sh.nq_pad = s.a.nq_pad;
  sh.ntotal = s.ntotal;
  sh.gathered = s.gathered;
  sh.deep = s.deep;
  sh.self_join = s.a.self0 >= 0;
  sh.l2aug = s.idx->l2aug();
  sh.L = s.L;
  sh.skinny_max_q = skinny_plane_max_queries();
  sh.wgs_env = x1_wgs_env();
  sh.split_mult = x1_split_mult();
  const StagePlan p = plan_stage(sh);
  s.small = p.small;
  s.x.nq_pad = p.nq_pad;
  s.x.nsplit = p.nsplit;
  s.nq = s.gathered ? p.nq_pad : s.a.nq;
  s.part.KP = s.L;
  s.part.P = 4 * p.nsplit;
  const size_t np_ = (size_t)p.nq_pad * s.part.P * s.part.KP;
  VS_HIP(s.scr.alloc((void**)&s.part.key, np_ * sizeof(float)), "vs: scratch");
  VS_HIP(s.scr.alloc((void**)&s.part.id, np_ * sizeof(int)), "vs: scratch");
  return VS_OK;
}

// Step 1: the stage's queries — the gathered copy, their plane (a conversion,
// or the stored rows' own), the int8 factors — and the pass's arguments.
int stage_queries(Stage& s) {
  vs_index* idx = s.idx;
  const SearchArgs& a = s.a;
  Scratch& scr = s.scr;
  X1Args& x = s.x;
  hipStream_t st = s.st;
  const int mode = a.mode, plane = s.plane;
  const bool gathered = s.gathered, i8 = s.i8, aug = s.aug;
  s.Q = a.self0 >= 0 ? (const float*)idx->row(a.self0) : a.qbuf;
  s.qaux = a.qaux;
  if (gathered) {
    float *qc = nullptr, *ac = nullptr;
    VS_HIP(scr.alloc((void**)&qc, (size_t)x.nq_pad * idx->ld * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&ac, (size_t)x.nq_pad * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&s.qrow, (size_t)x.nq_pad * sizeof(int)), "vs: scratch");
    VS_HIP(launch_gather_queries(s.Q, idx->ld, a.qaux, s.gl, s.gc, x.nq_pad, a.self0, qc, ac,
                                 s.qrow, st),
           "vs: gathered queries");
    s.Q = qc;
    s.qaux = ac;
  }
  const float* Q = s.Q;
  const bool self_rows = a.self0 >= 0 && !gathered;  // queries are stored rows in place
  const int qa_rows = s.qa_rows = gathered ? x.nq_pad : a.nq_pad;
  // query plane: a conversion of the stage's queries, or the stored rows' plane
  if (aug && (idx->aug_m <= 0 || self_rows)) return fail(VS_E_INVALID, "vs: int8 L2 plane");
  const int64_t pb = idx->planebytes(plane);
  const char* QH = nullptr;
  // stored rows starting on a tile boundary are read from the index's own
  // (tile-major) plane; any other batch is converted (the same codes)
  const bool plane_rows = self_rows && a.self0 % kX1Q == 0;
  x.qtile0 = plane_rows ? (int)(a.self0 / kX1Q) : 0;
  if (plane_rows) {
    QH = idx->fplane[plane];
    if (i8) {
      s.qs = idx->fscale + a.self0;
      s.qr2 = idx->rn2[FILTER_I8] + a.self0;
    }
  } else {
    char* qh = nullptr;
    VS_HIP(scr.alloc((void**)&qh, (size_t)x.nq_pad * pb), "vs: scratch");
    if (i8) {
      float *sc = nullptr, *r = nullptr;
      VS_HIP(scr.alloc((void**)&sc, (size_t)qa_rows * sizeof(float)), "vs: scratch");
      VS_HIP(scr.alloc((void**)&r, (size_t)qa_rows * sizeof(float)), "vs: scratch");
      if (aug)
        VS_HIP(launch_quantize_i8_l2aug(Q, idx->ld, 0, qa_rows, idx->aug, nullptr, (int8_t*)qh, sc,
                                        r, nullptr, st),
               "vs: query plane");
      else
        VS_HIP(launch_quantize_i8(Q, idx->ld, 0, qa_rows, (int8_t*)qh, sc, r, st),
               "vs: query plane");
      s.qs = sc;
      s.qr2 = r;
    } else if (aug) {
      VS_HIP(launch_bf16_plane_l2aug(Q, idx->ld, 0, qa_rows, idx->aug, nullptr, (uint16_t*)qh,
                                     nullptr, nullptr, st),
             "vs: query plane");
    } else {
      VS_HIP(launch_bf16_plane(Q, idx->ld, 0, qa_rows, (uint16_t*)qh, st), "vs: query plane");
    }
    VS_HIP(launch_plane_zero_rows(qh, pb, qa_rows, x.nq_pad - qa_rows, st), "vs: query plane");
    QH = qh;
  }
  s.stats = idx->bstats[plane];
  x.filter = plane;
  x.XH = idx->fplane[plane];
  x.xs = idx->fscale;
  if (i8 && mode == MODE_COS) {
    // the cosine folds the inverse norms into the int8 factors: s_x / |x| per
    // row (capacity rows: tiles read past ntotal), s_q / |q| per query
    float* cx = nullptr;
    VS_HIP(scr.alloc((void**)&cx, (size_t)idx->capacity * sizeof(float)), "vs: scratch");
    VS_HIP(launch_mul_arrays(idx->fscale, a.xaux, idx->capacity, cx, st), "vs: cosine factors");
    x.xs = cx;
    if (plane_rows) {
      s.qs = cx + a.self0;
    } else {
      float* cq = nullptr;
      VS_HIP(scr.alloc((void**)&cq, (size_t)qa_rows * sizeof(float)), "vs: scratch");
      VS_HIP(launch_mul_arrays(s.qs, s.qaux, qa_rows, cq, st), "vs: cosine factors");
      s.qs = cq;
    }
  }
  if (i8) {  // the per-lane factor bounds of the fast reject (scalar loads in the kernel)
    float* gm = nullptr;
    const size_t ng = (size_t)(idx->capacity / 16);
    VS_HIP(scr.alloc((void**)&gm, 2 * ng * sizeof(float)), "vs: scratch");
    VS_HIP(launch_group_max(x.xs, idx->capacity, gm, st, s.ntotal, gm + ng), "vs: factor bounds");
    x.xgmax = gm;
    x.xgmin = gm + ng;
  }
  x.xaux = a.xaux;
  x.QH = QH;
  x.qs = s.qs;
  x.qaux = s.qaux;
  x.nqa = qa_rows;
  x.ld = !aug ? idx->ld : i8 ? idx->ld + idx->aug_m : idx->ld + kAugBf16;  // the plane's K
  x.ntotal = s.ntotal;
  x.self0 = self_rows ? a.self0 : -1;
  x.qrow = s.qrow;
  x.qcount = s.gc;
  s.ba = aug ? make_bound_args_l2aug(idx->ld, idx->aug, plane) : make_bound_args(idx->ld, plane);
  return VS_OK;
}

// Step 1b (a first-stage x1 pass long enough to dump): query cuts + dump
// launches (vs_gemm_x1.hip header, vs_x1_cuts.hip "Query cuts").  The cuts are
// set after the pass's first launch and are the verification's floor for the
// rows the dump launches drop.  The dump slots: up to x1_dump_slots() candidate
// rows per lane list and segment within ~4 GB; fewer than 16 (or no memory):
// every launch is a list launch.
int arm_dumps(Stage& s) {
  vs_index* idx = s.idx;
  Scratch& scr = s.scr;
  X1Args& x = s.x;
  hipStream_t st = s.st;
  const int qa_rows = s.qa_rows, need = s.need, mode = s.a.mode;
  if (s.gathered || s.small || !x1_dump_applies(s.kmode, s.plane) || !dump_enabled() ||
      !x1_pass_dumps(s.ntotal, x.nsplit))
    return VS_OK;
  const int64_t lists = (int64_t)x.nq_pad * s.part.P;
  const int dR = (int)std::min<int64_t>(x1_dump_slots(), (int64_t(4) << 30) / (lists * 8));
  if (dR < 16) return VS_OK;
  int *dc = nullptr, *ds = nullptr;
  hipError_t e = scr.alloc((void**)&dc, (size_t)lists * sizeof(int));
  if (e == hipSuccess) e = scr.alloc((void**)&ds, (size_t)lists * dR * 2 * sizeof(int));
  if (e != hipSuccess) {
    (void)hipGetLastError();  // out of memory for the dumps: list launches
    return VS_OK;
  }
  VS_HIP(scr.alloc((void**)&x.qcut, (size_t)qa_rows * sizeof(float)), "vs: scratch");
  double* bk = nullptr;
  VS_HIP(scr.alloc((void**)&bk, (size_t)qa_rows * sizeof(double)), "vs: scratch");
  VS_HIP(hipMemsetD32Async((hipDeviceptr_t)x.qcut, 0x7f7fffff, (size_t)qa_rows, st), "vs: cuts");
  VS_HIP(hipMemsetAsync(dc, 0, (size_t)lists * sizeof(int), st), "vs: dumps");
  VS_HIP(launch_qbound(mode, s.Q, idx->ld, s.qaux, s.plane, s.stats, s.qr2, qa_rows, bk, st, &s.ba),
         "vs: cuts");
  x.qbkey = bk;
  x.qcut_m = need;
  x.dump = true;
  x.dump32 = dump_mfma32();
  x.recut = recut_mode();
  // exact-key cuts: the int8 inner-product pass of an fp32 index (the
  // augmented L2 and bf16-plane passes keep a_M + 2B)
  if (s.i8 && mode == MODE_IP && idx->esize == 4 && need <= kEcutMaxM && ecut_enabled()) {
    int* ci = nullptr;
    VS_HIP(scr.alloc((void**)&x.qam, (size_t)qa_rows * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&x.ecut_key, (size_t)qa_rows * kEcutMaxM * sizeof(float)),
           "vs: scratch");
    VS_HIP(scr.alloc((void**)&ci, (size_t)qa_rows * kEcutMaxM * sizeof(int)), "vs: scratch");
    VS_HIP(hipMemsetD32Async((hipDeviceptr_t)x.qam, 0x7f7fffff, (size_t)qa_rows, st), "vs: cuts");
    VS_HIP(hipMemsetAsync(ci, 0xFF, (size_t)qa_rows * kEcutMaxM * sizeof(int), st), "vs: cuts");
    x.ecut_id = ci;
    x.ecut_x = (const float*)idx->codes;
    x.ecut_q = s.Q;
    x.ecut_ld = idx->ld;
  }
  x.dcount = dc;
  x.dslot = ds;
  x.dR = dR;
  x.dstats = device_stats(idx->device) ? device_stats(idx->device) + 6 : nullptr;
  return VS_OK;
}

// Step 1c: the pass — 8-entry lane lists per query from the x1 kernels or a
// skinny kernel — and, for an augmented pass, its keys mapped to L2.
int run_pass(Stage& s) {
  const SearchArgs& a = s.a;
  X1Args& x = s.x;
  hipStream_t st = s.st;
  const bool gathered = s.gathered, i8 = s.i8;
  {
    // the pass as a whole (list + dump launches and the cut / replay kernels
    // between them) under "<name>_pass", beside the per-launch spans
    KernelTimer whole(st, gathered ? nullptr : i8 ? "gemm_topk_x1_i8_pass" : "gemm_topk_x1_pass",
                      false);
    X1SpanTimer tm(i8 ? "gemm_topk_x1_i8" : "gemm_topk_x1",
                   i8 ? "gemm_topk_x1_i8_list" : "gemm_topk_x1_list");
    if (!gathered) x.timing = &tm;
    // the deep bf16 stage of a few queries (inner product / augmented L2, not
    // a self-join): skinny_plane_topk streams the plane once for them and
    // the x1 pass exits, or the reverse, by the device-side count
    if (gathered && s.deep && !i8 && s.kmode == MODE_IP && a.self0 < 0 && skinny_deep_on()) {
      VS_HIP(launch_skinny_plane(FILTER_BF16, x.XH, x.QH, x.ld, s.ntotal, s.gc, nullptr, nullptr,
                                 s.part, st),
             "vs: skinny deep stage");
      x.qskip = skinny_plane_max_queries();
    }
    if (s.small) {
      int* cnt = nullptr;
      VS_HIP(s.scr.alloc((void**)&cnt, sizeof(int)), "vs: scratch");
      VS_HIP(hipMemsetD32Async((hipDeviceptr_t)cnt, a.nq, 1, st), "vs: count");
      KernelTimer ks(st, i8 ? "skinny_plane_topk_i8" : "skinny_plane_topk");
      VS_HIP(launch_skinny_plane(s.plane, x.XH, x.QH, x.ld, s.ntotal, cnt, s.qs, x.xs, s.part, st,
                                 a.nq),
             "vs: skinny first stage");
      ks.stop();
    } else {
      int nd = 0;
      VS_HIP(launch_gemm_topk_x1(s.kmode, x, s.part, st, &nd), "vs: gemm_topk_x1 launch");
    }
    x.timing = nullptr;
    whole.stop();
  }
  if (s.aug)  // augmented inner-product keys A -> L2 keys |q|^2 + 2A (lists and cuts)
    VS_HIP(launch_l2aug_map(s.part.key, s.part.id, (int64_t)s.part.P * s.part.KP, s.qa_rows,
                            s.qaux, s.idx->aug.nref, x.qcut, st),
           "vs: L2 keys");
  return VS_OK;
}

// Steps 2-5: the approximate merge, the two verifications with the flagged
// queries compacted after each, and the merge that emits the stage's (D, I).
int merge_and_verify(Stage& s) {
  vs_index* idx = s.idx;
  const SearchArgs& a = s.a;
  Scratch& scr = s.scr;
  hipStream_t st = s.st;
  const Partials& part = s.part;
  const int nq = s.nq, KF = s.KF, L = s.L;
  // approximate top-KF per query (plain lexicographic order: the L2 merge)
  float* Dk = nullptr;
  int64_t* Ik = nullptr;
  VS_HIP(scr.alloc((void**)&Dk, (size_t)nq * KF * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&Ik, (size_t)nq * KF * sizeof(int64_t)), "vs: scratch");
  if (KF > 64) {  // 2k - 1 > 64 (inner product, k > 32): the select kernel
    VS_HIP(launch_select_lists(part, L, nq, KF, Dk, Ik, st, s.gc), "vs: merge");
  } else if (select_heads_applies(part, L, KF)) {
    VS_HIP(launch_select_heads(part, nq, KF, Dk, Ik, st, s.gc), "vs: merge");
  } else {
    Partials mp = part;
    mp.KP = kp_for(KF);
    mp.KL = L;
    VS_HIP(launch_merge_partials(MODE_L2, mp, nq, KF, 0, 0.0f, Dk, Ik, KF, st, 0, nullptr, s.gc),
           "vs: merge");
  }
  Partials vp;
  vp.KP = kp_for(KF);
  vp.P = 1;
  int* flags = nullptr;
  VS_HIP(scr.alloc((void**)&vp.key, (size_t)nq * vp.KP * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&vp.id, (size_t)nq * vp.KP * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&flags, (size_t)nq * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&s.qlist, (size_t)s.x.nq_pad * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&s.qcount, 2 * sizeof(int)), "vs: scratch");
  VerifyArgs v;  // one fill for both verifications
  v.mode = s.vmode;
  v.KF = KF;
  v.M = s.need;
  v.X = idx->codes;
  v.xesize = idx->esize;
  v.xn = idx->norms;
  v.Q = s.Q;
  v.qn = s.qaux;
  v.ld = idx->ld;
  v.ba = s.ba;
  v.stats = s.stats;
  v.lists = part;
  v.L = L;
  v.okey = vp.key;
  v.oid = vp.id;
  v.KP = vp.KP;
  v.fail = flags;
  v.qinv = a.mode == MODE_COS ? s.qaux : nullptr;
  v.xinv = a.mode == MODE_COS ? a.xaux : nullptr;
  v.qr2i8 = s.qr2;
  v.qcut = s.x.qcut;
  VS_HIP(launch_verify_rescore(v, nq, Dk, Ik, s.gc, st), "vs: verify");
  unsigned long long* dst = device_stats(idx->device);
  if (!dst) return fail(VS_E_HIP, "vs: statistics buffer");
  // statistics: [0] queries (first stage), [1] flagged by a first check, [2]
  // redone by the exact engine, [3] handed to a second filter stage
  VS_HIP(launch_compact_flags(flags, nq, s.qlist, s.qcount, dst + 1,
                              s.gathered ? nullptr : dst + 0, st),
         "vs: flags");
  if (wide_enabled())
    VS_HIP(launch_verify_wide(v, nq, s.qlist, s.qcount, Dk, Ik, dst + 4, st), "vs: verify wide");
  VS_HIP(launch_compact_flags(flags, nq, s.qlist, s.qcount + 1,
                              s.last_plane ? dst + 2 : dst + 3, nullptr, st),
         "vs: flags");
  VS_HIP(launch_merge_partials(s.vmode, vp, nq, a.k, idx->id_base, a.min_score, a.D, a.I, a.k, st,
                               a.raw, s.gl, s.gc),
         "vs: merge");
  return VS_OK;
}

// Step 6: the queries still flagged go to the next stage — the deep bf16
// stage, or after the last plane the exact redo — as query ids of `a`.
int hand_off(Stage& s) {
  vs_index* idx = s.idx;
  const SearchArgs& a = s.a;
  hipStream_t st = s.st;
  const int* left_count = s.qcount + 1;
  // The first stage's and the deep stage's leftovers, read when the call may
  // wait (tail_wait_on): nothing left, no later stage is enqueued (the live
  // search_catalog path, mcp_book_server.py:142, at batch 1: ~30 launches,
  // 0.13 ms of a 2.6-ms search; C2 ~45, 0.25 ms)
  int left = -1;
  if ((!s.gathered || s.deep) && tail_wait_on(a, st)) {
    int rc = read_count(left_count, st, &left);
    if (rc) return rc;
  }
  // the adaptive order's counters of an int8-first search, whether or not
  // anything is left (a first stage composes no list, so nothing is enqueued
  // between the count's read and this)
  if (!s.last_plane && !s.gathered && s.plane == FILTER_I8) {
    int rc = adaptive_record(idx, left_count, s.nq, st);
    if (rc) return rc;
  }
  if (left == 0) return VS_OK;
  // what is still flagged (usually nothing: every tile exits), as query ids of `a`
  const int* next = s.qlist;
  if (s.gathered) {
    int* composed = nullptr;
    VS_HIP(s.scr.alloc((void**)&composed, (size_t)s.x.nq_pad * sizeof(int)), "vs: scratch");
    VS_HIP(launch_compose_list(s.gl, s.qlist, left_count, s.x.nq_pad, composed, st), "vs: flags");
    next = composed;
  }
  if (!s.last_plane)
    return run_filter_verify(idx, a, s.need, s.KF, st, FILTER_BF16, true, true, next, left_count);
  // the exact redo (untimed: the kernel timer holds the first filter pass)
  return run_gemm_rescored(idx, a, s.need, s.KF, s.plane, st, next, left_count);
}

// The filter-and-verify engine (vs_gemm_x1.hip), entirely stream-ordered, as a
// chain of stages over the planes the index holds (int8, then bf16):
//  0. size the stage's lane lists (plan_stage);
//  1. convert the stage's queries to its plane (int8 codes + scales, or bf16);
//     the x1 pass keeps 8-entry lane lists per query;
//  2. merge them to the KF best approximate candidates;
//  3. verify_rescore: exact keys of the candidates + the bound check (fail[]);
//  4. the flagged queries are compacted on the device and re-checked by the
//     wide verification (every lane-list entry below the list floors);
//  5. the merges emit (D, I) of the stage's queries;
//  6. the queries still flagged go to the next stage as a gathered batch
//     (device-side list and count: the int8 plane's wider bound leaves
//     clustered data to the bf16 plane), and after the last plane to the exact
//     fp32 engine (a launch whose tiles past the device-side count exit at
//     once), whose rows overwrite theirs.
// Counts live in device memory; the host reads one only to skip the later
// stages when none is left (tail_wait_on).  `gl` / `gc` (stages after the
// first): the batch is queries gl[0 .. *gc) of `a`.
int run_filter_verify(vs_index* idx, const SearchArgs& a, int need, int KF, hipStream_t st,
                      int plane, bool last_plane, bool deep, const int* gl, const int* gc) {
  Stage s(idx, a, need, KF, st, plane, last_plane, deep, gl, gc);
  int rc = size_lists(s);                // 0
  if (!rc) rc = stage_queries(s);        // 1: the queries' plane
  if (!rc) rc = arm_dumps(s);            //    the cuts and dump slots
  if (!rc) rc = run_pass(s);             //    the pass
  if (!rc) rc = merge_and_verify(s);     // 2-5
  if (!rc) rc = hand_off(s);             // 6
  return rc;
}

// The staged engine's last stage: the exact fp32 MFMA GEMM (bf16 rows: the
// bf16 one) over the queries no filter stage settled (gathered: gl[0 .. *gc) of
// `a`) keeps KF candidates per query, which are rescored like every other
// stage's (verify_rescore: fp64 sums, one rounding), so every key the staged
// engine returns is the fp32 rounding of the exact score (oracle/flat.py
// key_window); the candidates are proven with the GEMM's own bound and what it
// cannot prove goes to the exact-key stream (below).
// Slots of the exact-key stream per launch (its lists: kExactSlots x up to
// 256 row blocks x KP entries); launches past the device-side count exit.
constexpr int kExactSlots = 256;
constexpr int kXPageSlots = 1024;  // run_paged's exact-key pages

int run_gemm_rescored(vs_index* idx, const SearchArgs& a, int need, int KF, int plane,
                      hipStream_t st, const int* gl, const int* gc) {
  // more than the 64 entries one exact page holds (inner product, k > 32): the
  // paged exact engine over the gathered queries (its keys are the fp32
  // engine's own, as in a search that never went through the filter)
  if (KF > 64) return run_paged(idx, a, st, gl, gc);
  const int ntotal = (int)idx->ntotal;
  const int KP = kp_for(KF);
  const int nslot = (int)round_up(a.nq, kBQ);
  Partials part;
  part.KP = KP;
  const int ntiles = (ntotal + kBN - 1) / kBN;
  const int nsplit = gathered_nsplit(ntiles);
  part.P = 2 * nsplit;
  const int cap = slot_window_cap(nslot, part.P, KP);  // slots per window
  Scratch scr(st);
  const size_t n = (size_t)cap * part.P * KP;
  VS_HIP(scr.alloc((void**)&part.key, n * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&part.id, n * sizeof(int)), "vs: scratch");
  float *qc = nullptr, *ac = nullptr;
  int* qrow = nullptr;
  VS_HIP(scr.alloc((void**)&qc, (size_t)cap * idx->ld * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&ac, (size_t)cap * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&qrow, (size_t)cap * sizeof(int)), "vs: scratch");
  float* Dk = nullptr;
  int64_t* Ik = nullptr;
  VS_HIP(scr.alloc((void**)&Dk, (size_t)cap * KF * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&Ik, (size_t)cap * KF * sizeof(int64_t)), "vs: scratch");
  Partials vp;
  vp.KP = KP;
  vp.P = 1;
  int* flags = nullptr;
  int* wc = nullptr;
  VS_HIP(scr.alloc((void**)&vp.key, (size_t)cap * KP * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&vp.id, (size_t)cap * KP * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&flags, (size_t)cap * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&wc, sizeof(int)), "vs: scratch");
  const float* Qa = a.self0 >= 0 ? (const float*)idx->row(a.self0) : a.qbuf;
  uint16_t* qc16 = nullptr;
  if (idx->esize == 2) {
    if (a.self0 >= 0 || !a.qb16) return fail(VS_E_INVALID, "vs: bf16 last stage");
    VS_HIP(scr.alloc((void**)&qc16, (size_t)cap * idx->ld * sizeof(uint16_t)), "vs: scratch");
  }
  const int emode = a.mode == MODE_L2 && a.l2_direct ? MODE_L2D : a.mode;
  // The candidates are proven with the fp32 GEMM's own error bound (no plane
  // residuals: BoundArgs::rows_exact); a query it cannot settle (more than
  // KF - k rows inside the bound of its k-th: dense near-ties) is ranked over
  // every row by its exact key instead (vs_exact.hip; env VS_EXACT_STREAM=0
  // keeps the fp32 candidates, for A/B), so every answer of the staged engine
  // is the exact top-k of the rescored keys.
  BoundArgs ba = make_bound_args(idx->ld, FILTER_BF16);
  ba.rows_exact = 1;
  const bool stream_ok =
      exact_stream_on() && idx->esize == 4 && exact_stream_nq(idx->ld) > 0 && KP <= 64;
  unsigned long long* dstats = device_stats(idx->device);
  int *fl = nullptr, *fc = nullptr, *ol = nullptr, *ewc = nullptr;
  int xslots = kExactSlots;
  Partials ep;
  if (stream_ok) {
    VS_HIP(scr.alloc((void**)&fl, (size_t)cap * sizeof(int)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&fc, sizeof(int)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&ol, (size_t)cap * sizeof(int)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&ewc, sizeof(int)), "vs: scratch");
    ep.KP = kp_for(need);
    ep.P = exact_stream_lists(ntotal);
    // slots per launch: the whole window when its lists fit in ~256 MB (C3:
    // one launch triple over an empty count instead of 16), else kExactSlots
    xslots = (int)std::min<int64_t>(
        cap, std::max<int64_t>(kExactSlots, ((int64_t)256 << 20) / ((int64_t)ep.P * ep.KP * 8)));
    VS_HIP(scr.alloc((void**)&ep.key, (size_t)xslots * ep.P * ep.KP * sizeof(float)),
           "vs: scratch");
    VS_HIP(scr.alloc((void**)&ep.id, (size_t)xslots * ep.P * ep.KP * sizeof(int)),
           "vs: scratch");
  }
  // A small batch (its flagged queries are at most its a.nq <= kSkinnyMaxQ):
  // the skinny fp32 kernel streams the rows once over the gathered queries
  // (slots past the device-side count score garbage that no merge reads)
  // instead of a GEMM over a whole query tile
  const bool skinny = a.nq <= kSkinnyMaxQ && KP <= 32 && (a.nq <= 16 || KP <= 16) && a.self0 < 0 &&
                      (a.mode == MODE_IP || a.mode == MODE_L2) && (idx->ld * idx->esize) % 128 == 0;
  Partials sp;
  if (skinny) {
    sp.KP = KP;
    sp.P = stream_blocks(ntotal);
    VS_HIP(scr.alloc((void**)&sp.key, (size_t)kSkinnyMaxQ * sp.P * KP * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&sp.id, (size_t)kSkinnyMaxQ * sp.P * KP * sizeof(int)), "vs: scratch");
  }
  VerifyArgs v;  // every window's rescoring: no plane residuals, no cuts
  v.mode = emode;
  v.KF = KF;
  v.M = need;
  v.X = idx->codes;
  v.xesize = idx->esize;
  v.xn = idx->norms;
  v.Q = qc;
  v.qn = ac;
  v.ld = idx->ld;
  v.ba = ba;
  v.stats = idx->bstats[plane];
  v.lists = skinny ? sp : part;
  v.L = KP;
  v.okey = vp.key;
  v.oid = vp.id;
  v.KP = vp.KP;
  v.fail = flags;
  v.qinv = a.mode == MODE_COS ? ac : nullptr;
  v.xinv = a.mode == MODE_COS ? a.xaux : nullptr;
  for (int w0 = 0; w0 < nslot; w0 += cap) {
    const int* wl = gl + w0;  // this window's query ids, wc[0] of them
    VS_HIP(launch_window_count(gc, w0, cap, wc, st), "vs: window");
    // the window's query rows and aux values, slot by slot, for the rescoring
    VS_HIP(launch_gather_queries(Qa, idx->ld, a.qaux, wl, wc, cap, a.self0, qc, ac, qrow, st),
           "vs: gathered queries");
    // bf16 rows: the bf16 kernels take bf16 query rows (the staged values are
    // already bf16-rounded, so the conversion is exact)
    if (qc16) VS_HIP(launch_f32_to_bf16(qc, idx->ld, qc16, idx->ld, cap, idx->ld, st), "vs: bf16 queries");
    if (skinny) {
      VS_HIP(launch_skinny_topk(KP, a.mode, a.nq, idx->codes, idx->esize, a.xaux,
                                qc16 ? (const void*)qc16 : (const void*)qc, ac, idx->ld, ntotal,
                                sp.P, sp, st, wc),
             "vs: skinny_topk launch");
    } else {
      VS_HIP(launch_gemm_topk(KP, a.mode, idx->codes, a.xaux,
                              idx->esize == 2 ? a.qb16 : (const void*)Qa, a.qaux, idx->ld,
                              idx->esize, ntotal, cap, nsplit, a.self0, part, st, wl, wc),
             "vs: gemm_topk launch");
    }
    VS_HIP(launch_merge_partials(MODE_L2, skinny ? sp : part, skinny ? a.nq : cap, KF, 0, 0.0f, Dk,
                                 Ik, KF, st, 0, nullptr, wc),
           "vs: merge");
    VS_HIP(launch_verify_rescore(v, cap, Dk, Ik, wc, st), "vs: rescore");
    VS_HIP(launch_merge_partials(emode, vp, cap, a.k, idx->id_base, a.min_score, a.D, a.I, a.k,
                                 st, a.raw, wl, wc),
           "vs: merge");
    if (!stream_ok) continue;
    // the queries the fp32 bound leaves open: every row ranked by its exact key
    VS_HIP(launch_compact_flags(flags, cap, fl, fc, dstats ? dstats + 8 : nullptr, nullptr, st),
           "vs: exact stream");
    VS_HIP(launch_compose_list(wl, fl, fc, cap, ol, st), "vs: exact stream");
    ExactStreamArgs ea = make_exact_stream_args(idx, a, qc, ac, fl, fc, xslots);
    ea.qrow = a.self0 >= 0 ? qrow : nullptr;
    for (int s0 = 0; s0 < cap; s0 += xslots) {
      ea.s0 = s0;
      VS_HIP(launch_window_count(fc, s0, xslots, ewc, st), "vs: exact stream");
      VS_HIP(launch_exact_stream(ep.KP, emode, ea, ep, st), "vs: exact stream");
      VS_HIP(launch_merge_partials(emode, ep, xslots, a.k, idx->id_base, a.min_score, a.D,
                                   a.I, a.k, st, a.raw, ol + s0, ewc),
             "vs: merge");
    }
  }
  return VS_OK;
}

// Fraction of int8-stage queries handed on to bf16 above which the int8 stage
// costs more than it saves (stage costs ~0.58 and 1 of a bf16-only search:
// break-even ~0.42).
constexpr double kI8HandOffMax = 0.3;

// Whether this search starts on the int8 plane (see vs_index::Adaptive).  While
// the int8 stage hands on too much, searches start on bf16, with an int8 probe
// after 8, 16, 32, 64 of them (each probe's counters arrive with a later
// search; a probe on clustered data costs ~1.4x a bf16-first search).
bool adaptive_use_i8(vs_index* idx) {
  auto& A = idx->ad;
  std::lock_guard<std::mutex> g(A.mu);
  bool fresh = false;
  if (A.pending && hipEventQuery(A.ev) == hipSuccess) {
    const unsigned long long q = A.hmirror[0], h = A.hmirror[1];
    if (q > A.seen_q) {
      const double f = (double)(h - A.seen_h) / (double)(q - A.seen_q);
      A.ema = A.have ? 0.5 * A.ema + 0.5 * f : f;
      A.have = true;
      fresh = true;
    }
    A.seen_q = q;
    A.seen_h = h;
    A.pending = false;
  }
  if (!A.have || A.ema <= kI8HandOffMax) {
    A.backoff = kI8FirstBackoff;
    A.skip_left = 0;
    return true;
  }
  if (fresh) {
    A.skip_left = A.backoff;
    A.backoff = std::min(2 * A.backoff, kI8MaxBackoff);
  }
  if (A.skip_left > 0) {
    --A.skip_left;
    return false;
  }
  A.skip_left = A.backoff;  // a probe; bf16 until its counters arrive
  return true;
}

// The per-index counters of an int8-first search: what the int8 stage saw
// and handed on, then an async copy to the pinned mirror (one in flight).
int adaptive_record(vs_index* idx, const int* handed, int n, hipStream_t st) {
  auto& A = idx->ad;
  std::lock_guard<std::mutex> g(A.mu);
  if (!A.dcount) {
    VS_HIP(hipMalloc(&A.dcount, 2 * sizeof(unsigned long long)), "vs: adaptive counters");
    VS_HIP(hipMemset(A.dcount, 0, 2 * sizeof(unsigned long long)), "vs: adaptive counters");
    VS_HIP(hipHostMalloc(&A.hmirror, 2 * sizeof(unsigned long long)), "vs: adaptive counters");
    A.hmirror[0] = A.hmirror[1] = 0;
    VS_HIP(hipEventCreateWithFlags(&A.ev, hipEventDisableTiming), "vs: adaptive counters");
  }
  VS_HIP(launch_add_counts(handed, n, A.dcount, st), "vs: adaptive counters");
  if (!A.pending) {
    VS_HIP(hipMemcpyAsync(A.hmirror, A.dcount, 2 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st),
           "vs: adaptive counters");
    VS_HIP(hipEventRecord(A.ev, st), "vs: adaptive counters");
    A.pending = true;
  }
  return VS_OK;
}

// The paged exact engine: any k, every metric, for what one 64-entry list
// cannot answer — k > 64, raw (shard) lists past 64, and faiss's inner-product
// tie rule past k = 32 (it reads the k-th key's run of equal keys up to 2k - 1
// entries; service.py:529-531 oversamples to k = 60, and the live tool's k is
// the agent's, mcp_book_server.py:115,142).  faiss's IndexFlat::search has no k
// limit; neither has this.  A query's answer is read off its lexicographic
// (key, row) order in pages of 64 entries:
//  1. page 1: the exact kernel's top-64 (FLOOR form with the floor (-inf, -1));
//  2. page_step: a query takes page p + 1 only while its answer needs it (fewer
//     than k entries so far, or the rule's run of k-th key ties reaching the
//     page's end below 2k - 1) and its page came back full; page p + 1 = the
//     same kernel with the admission floored at page p's last entry, over the
//     queries that need it (gathered on the device; launches past the count
//     exit at once), so every row's key is the same instructions' result in
//     every page;
//  3. page_finish: the pages side by side, faiss's rule (unless raw or not
//     inner product), the k outputs (empty past the rows there are).
// Kernels: the fp32 GEMV for one or two fp32 inner-product queries and for
// faiss's sequential L2 branch (calls under 20 queries, groups of up to 8);
// everything else the fp32 / bf16 MFMA GEMM (self-joins included).  Query
// windows keep the pages within ~2 GB whatever k and the batch.
// gl / gc: a gathered batch, queries gl[0 .. *gc) of `a` (the staged engine's
// last stage for inner product k > 32; device-side count), whose rows alone
// are written.
int run_paged(vs_index* idx, const SearchArgs& a, hipStream_t st, const int* gl, const int* gc) {
  const bool gathered = gl != nullptr;
  const int ntotal = (int)idx->ntotal;
  const bool rule = a.mode == MODE_IP && !a.raw;
  const int64_t need = rule ? 2 * (int64_t)a.k - 1 : (int64_t)a.k;
  // entries past the rows in place never exist: the last page is never needed
  const int64_t npages = std::max<int64_t>(1, (std::min<int64_t>(need, ntotal) + 63) / 64);
  const int64_t KA = npages * 64;
  const bool fits = gemv_fits(idx->ld);
  const bool l2d = a.mode == MODE_L2 && a.l2_direct && idx->esize == 4 && fits && a.self0 < 0;
  const bool gemv = !gathered && a.self0 < 0 && idx->esize == 4 && fits &&
                    (l2d || (a.mode == MODE_IP && a.nq <= 2));
  // The staged engine's last stage (gathered, fp32 rows): the pages are the
  // exact-key stream's (vs_exact.hip, floored), every key the rescoring's own
  // (fp64 sums of the exact products, one rounding), so what no filter stage
  // settled is answered strictly like the rest (inner product k > 32, L2 k >
  // 56), not with the fp32 GEMM's keys.  Env VS_EXACT_STREAM=0 keeps the GEMM
  // pages (A/B).
  const bool xpages =
      gathered && idx->esize == 4 && a.self0 < 0 && exact_stream_on() && exact_stream_nq(idx->ld) > 0;
  const int pmode = l2d || (xpages && a.mode == MODE_L2 && a.l2_direct) ? MODE_L2D : a.mode;
  // query windows: GEMV groups of up to 8, else pages of at most ~2 GB
  int64_t W = a.nq;
  if (gemv) {
    W = kGemvMaxQ;
  } else if (!gathered) {
    W = std::max<int64_t>(kBQ, ((int64_t)2 << 30) / (KA * 12) / kBQ * kBQ);
  }
  const int64_t nw_max = std::min<int64_t>(W, a.nq);
  const int64_t nrow = gathered ? a.nq_pad : round_up(std::max<int64_t>(nw_max, kGemvMaxQ), kBQ);
  Scratch scr(st);
  float* Dacc = nullptr;
  int64_t* Iacc = nullptr;
  float* fkey = nullptr;
  int *fid = nullptr, *member = nullptr, *active = nullptr, *qlist = nullptr, *qcount = nullptr;
  VS_HIP(scr.alloc((void**)&Dacc, (size_t)nrow * KA * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&Iacc, (size_t)nrow * KA * sizeof(int64_t)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&fkey, (size_t)nrow * sizeof(float)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&fid, (size_t)nrow * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&member, (size_t)nrow * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&active, (size_t)nrow * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&qlist, (size_t)nrow * sizeof(int)), "vs: scratch");
  VS_HIP(scr.alloc((void**)&qcount, sizeof(int)), "vs: scratch");
  // the page kernels' partial lists
  Partials part;
  part.KP = 64;
  int nsplit = 1, cap = 0, xslots = 0;
  int* wc = nullptr;
  if (gemv) {
    part.P = stream_blocks(ntotal);
    VS_HIP(scr.alloc((void**)&part.key, (size_t)kGemvMaxQ * part.P * 64 * sizeof(float)),
           "vs: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)kGemvMaxQ * part.P * 64 * sizeof(int)),
           "vs: scratch");
    VS_HIP(scr.alloc((void**)&wc, sizeof(int)), "vs: scratch");
  } else if (xpages) {
    // slots per exact-page launch: the whole gathered batch up to 1,024 (its
    // lists: 1,024 x 256 row blocks x 64 entries = 134 MB), so a page of a
    // 4,096-query search is 4 launch triples, not 16 (they run every search,
    // usually over an empty count)
    part.P = exact_stream_lists(ntotal);
    xslots = (int)std::min<int64_t>(kXPageSlots, round_up(std::max(a.nq, 1), kBQ));
    VS_HIP(scr.alloc((void**)&part.key, (size_t)xslots * part.P * 64 * sizeof(float)),
           "vs: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)xslots * part.P * 64 * sizeof(int)),
           "vs: scratch");
    VS_HIP(scr.alloc((void**)&wc, sizeof(int)), "vs: scratch");
  } else {
    const int ntiles = (ntotal + kBN - 1) / kBN;
    nsplit = gathered_nsplit(ntiles);
    part.P = 2 * nsplit;
    cap = slot_window_cap(nrow, part.P, 64);  // slots per window
    VS_HIP(scr.alloc((void**)&part.key, (size_t)cap * part.P * 64 * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)cap * part.P * 64 * sizeof(int)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&wc, sizeof(int)), "vs: scratch");
  }
  for (int64_t q0 = 0; q0 < a.nq; q0 += W) {
    const int nw = (int)std::min<int64_t>(W, a.nq - q0);
    const int nslot = (int)round_up(nw, kBQ);
    // this window's queries (offsets into the staged rows / aux / outputs)
    const int64_t eoff = q0 * idx->ld;
    const float* qf = a.qbuf ? a.qbuf + eoff : nullptr;
    const void* qmat = a.qb16 ? (const void*)((const uint16_t*)a.qb16 + eoff) : (const void*)qf;
    const float* qaux = a.qaux ? a.qaux + q0 : nullptr;
    const int64_t self0 = a.self0 >= 0 ? a.self0 + q0 : -1;
    VS_HIP(hipMemsetAsync(Iacc, 0xFF, (size_t)nw * KA * sizeof(int64_t), st), "vs: pages");
    if (gathered) {
      VS_HIP(hipMemsetAsync(member, 0, (size_t)nw * sizeof(int), st), "vs: pages");
      VS_HIP(hipMemsetAsync(active, 0, (size_t)nw * sizeof(int), st), "vs: pages");
    }
    VS_HIP(launch_page_init(nw, gemv ? kGemvMaxQ : nw, gl, gc, member, active, fkey, fid, st),
           "vs: pages");
    // (exact-key pages: their queries count as the exact stream's, vs_filter_exact_stats)
    unsigned long long* xst = xpages ? device_stats(idx->device) : nullptr;
    VS_HIP(launch_compact_flags(active, nw, qlist, qcount, xst ? xst + 8 : nullptr, nullptr, st),
           "vs: pages");
    for (int64_t p = 0; p < npages; ++p) {
      if (p > 0) {
        VS_HIP(launch_page_step(Dacc, Iacc, KA, (int)p - 1, nw, a.k, rule ? 1 : 0, pmode, active,
                                fkey, fid, st),
               "vs: pages");
        VS_HIP(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st), "vs: pages");
      }
      if (gemv) {  // every query's lists (finished ones empty); none: the launch exits
        KernelTimer tm(st, p == 0 && !gathered ? "gemv_topk" : nullptr);
        VS_HIP(launch_gemv_topk(64, pmode, nw, idx->codes, idx->esize, qf, idx->ld, ntotal, part.P,
                                part, st, fkey, fid, qcount),
               "vs: gemv_topk launch");
        tm.stop();
        VS_HIP(launch_page_gate(qcount, nw, wc, st), "vs: pages");
        VS_HIP(launch_merge_partials(pmode, part, nw, 64, 0, -INFINITY, Dacc + p * 64,
                                     Iacc + p * 64, KA, st, 1, nullptr, wc),
               "vs: merge launch");
        continue;
      }
      if (xpages) {  // the active queries in launches of xslots (past the count: exit)
        ExactStreamArgs ea = make_exact_stream_args(idx, a, qf, qaux, qlist, qcount, xslots);
        ea.fkey = fkey;
        ea.fid = fid;
        for (int s0 = 0; s0 < nslot; s0 += xslots) {
          ea.s0 = s0;
          VS_HIP(launch_window_count(qcount, s0, xslots, wc, st), "vs: window");
          VS_HIP(launch_exact_stream(64, pmode, ea, part, st), "vs: exact stream");
          VS_HIP(launch_merge_partials(pmode, part, xslots, 64, 0, -INFINITY, Dacc + p * 64,
                                       Iacc + p * 64, KA, st, 1, qlist + s0, wc),
                 "vs: merge launch");
        }
        continue;
      }
      for (int w0 = 0; w0 < nslot; w0 += cap) {
        VS_HIP(launch_window_count(qcount, w0, cap, wc, st), "vs: window");
        KernelTimer tm(st, p == 0 && w0 == 0 && !gathered ? "gemm_topk" : nullptr);
        VS_HIP(launch_gemm_topk(64, a.mode, idx->codes, a.xaux, qmat, qaux, idx->ld, idx->esize,
                                ntotal, cap, nsplit, self0, part, st, qlist + w0, wc, fkey, fid),
               "vs: gemm_topk launch");
        tm.stop();
        VS_HIP(launch_merge_partials(a.mode, part, cap, 64, 0, -INFINITY, Dacc + p * 64,
                                     Iacc + p * 64, KA, st, 1, qlist + w0, wc),
               "vs: merge launch");
      }
    }
    VS_HIP(launch_page_finish(pmode, Dacc, Iacc, KA, nw, a.k, rule ? 1 : 0, member, idx->id_base,
                              a.min_score, a.D + q0 * a.k, a.I + q0 * a.k, st),
           "vs: pages");
  }
  return VS_OK;
}


}  // namespace

namespace vs {
namespace host {

// Shared search driver: queries already staged in `qbuf` ([nq_pad][ld] device,
// zero-padded) with query aux values (`qaux`, L2 norms or 1/|q|).
int run_topk(vs_index* idx, const SearchArgs& a, hipStream_t st, int force_engine) {
  // faiss's inner-product tie rule (vs_support.hip, faiss_ip_tie_order) needs the
  // lowest 2k-1 (key, label) entries of every partial list to be exact; `raw`
  // output (plain lexicographic order) needs k.
  const int mode = a.mode;
  const bool tie_rule = mode == MODE_IP && !a.raw;
  const int need = tie_rule ? 2 * a.k - 1 : a.k;
  const int ntotal = (int)idx->ntotal;
  const int nq = a.nq;
  int engine = force_engine != VS_ENGINE_AUTO ? force_engine
               : idx->engine != VS_ENGINE_AUTO ? idx->engine
                                               : engine_from_env();
  // Large batches of fp32 indexes: the filter-and-verify engine where it applies
  // (candidates for `need` exact entries: x1_list_len, up to 127 — inner
  // product to k = 64), else (or VS_ENGINE=fp32) the fp32 MFMA GEMM.  bf16
  // indexes: the bf16 MFMA GEMM.
  // (past 64 candidates, inner product only: the last stage for what the
  // filter cannot settle is then the two-page exact engine, inner product's;
  // L2 / cosine with k > 56 keep the exact engine)
  const int KF = x1_list_len(need);
  // the planes this search may run through: int8 first, then bf16; a forced
  // *_VERIFY engine runs its plane alone (an L2 index's int8 plane is the
  // augmented one: L2 searches only)
  bool i8_ok = idx->plane_on[FILTER_I8] && idx->ld + idx->aug_m <= kI8MaxLd &&
               (idx->l2aug() ? mode == MODE_L2 && idx->aug_m > 0 : mode != MODE_L2) &&
               engine != VS_ENGINE_BF16_VERIFY;
  const bool b16_ok = idx->plane_on[FILTER_BF16] && engine != VS_ENGINE_I8_VERIFY &&
                      (idx->l2aug() ? mode == MODE_L2 && idx->aug_m > 0 : true);
  // what every route through the staged engine needs: fp32 rows, a candidate
  // count for `need`, and no forced fp32 engine
  const bool staged_ok =
      idx->esize == 4 && engine != VS_ENGINE_FP32_MFMA && KF > 0 && ntotal > 0;
  const bool staged = staged_ok && nq > kSkinnyMaxQ && (i8_ok || b16_ok);
  // Small batches over a large index with a filter plane for the metric (inner
  // product; L2 when faiss would take its BLAS branch): the staged engine with
  // skinny passes (below)
  const bool small_staged = small_filter_on() && (idx->esize == 4 || mode == MODE_IP) &&
                            engine == VS_ENGINE_AUTO && KF > 0 && nq <= kSkinnyMaxQ &&
                            a.self0 < 0 && ntotal >= kSmallFilterMinRows &&
                            (mode == MODE_IP || mode == MODE_L2) && (i8_ok || b16_ok) &&
                            small_l2d_ok(mode, a);
  // more entries than one exact page holds (inner product k > 32, raw k > 64)
  // and no filter pass for them: the paged exact engine
  if (need > VS_MAX_K && !staged && !small_staged) return run_paged(idx, a, st);
  const int KP = kp_for(need);

  // Small batches stream the corpus once.  fp32 L2 searches whose CALL has
  // fewer than 20 queries take faiss's sequential branch (direct sum (x-q)^2,
  // faiss's distance_compute_blas_threshold): the GEMV kernel, 8 queries per
  // pass.  Otherwise the skinny MFMA kernel (any metric / dtype, L2 by the norm
  // expansion like faiss's BLAS branch), or the GEMV for one or two inner-product
  // queries on fp32 rows (measured faster there, profiles/r01_small_batch_ab.txt).
  const char* pref = small_batch_pref();
  const bool small_ok = (mode == MODE_IP || mode == MODE_L2) && a.self0 < 0;
  const bool fits = gemv_fits(idx->ld);
  const bool direct = small_ok && mode == MODE_L2 && a.l2_direct && idx->esize == 4 && fits;
  const bool skinny_ok = small_ok && !direct && nq <= kSkinnyMaxQ && KP <= 32 &&
                         (nq <= 16 || KP <= 16) && (idx->ld * idx->esize) % 64 == 0;
  bool gemv = small_ok && fits && idx->esize == 4 &&
              (direct || (mode == MODE_IP && nq <= 2 && !(pref && strcmp(pref, "skinny") == 0)));
  if (pref && strcmp(pref, "gemv") == 0 && small_ok && fits && nq <= kGemvMaxQ &&
      (mode == MODE_IP || direct))
    gemv = true;
  // Small batches over a large fp32 index with a filter plane for the metric
  // (inner product; L2 when faiss would take its BLAS branch): the staged
  // engine with skinny passes — the int8 plane streamed once (a quarter of the
  // fp32 bytes), candidates rescored and proven exactly as for large batches,
  // the few queries it cannot settle through the bf16 plane and the fp32
  // rows (skinny kernels too) — instead of streaming the fp32 rows.
  if (small_staged) {
    if (i8_ok && b16_ok) i8_ok = adaptive_use_i8(idx);
    if (i8_ok) return run_filter_verify(idx, a, need, KF, st, FILTER_I8, !b16_ok);
    return run_filter_verify(idx, a, need, KF, st, FILTER_BF16, false);
  }
  Scratch scr(st);
  Partials part;
  part.KP = KP;
  if (gemv) {
    const int gmode = direct ? MODE_L2D : MODE_IP;
    const int nblocks = stream_blocks(idx->ntotal);
    part.P = nblocks;
    const int step = kGemvMaxQ;  // queries per corpus pass
    // the kernel writes lists for its padded query count (1, 2, 4 or 8)
    const int nql = nq <= 2 ? nq : (nq <= 4 ? 4 : kGemvMaxQ);
    const size_t n = (size_t)nql * part.P * KP;
    VS_HIP(scr.alloc((void**)&part.key, n * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&part.id, n * sizeof(int)), "vs: scratch");
    for (int q0 = 0; q0 < nq; q0 += step) {
      const int nc = std::min(step, nq - q0);
      KernelTimer tm(st, "gemv_topk");
      VS_HIP(launch_gemv_topk(KP, gmode, nc, idx->codes, idx->esize, a.qbuf + (int64_t)q0 * idx->ld,
                              idx->ld, ntotal, nblocks, part, st),
             "vs: gemv_topk launch");
      tm.stop();
      VS_HIP(launch_merge_partials(gmode, part, nc, a.k, idx->id_base, a.min_score,
                                   a.D + (int64_t)q0 * a.k, a.I + (int64_t)q0 * a.k, a.k, st,
                                   a.raw),
             "vs: merge launch");
    }
    return VS_OK;
  }
  if (skinny_ok) {
    const int nblocks = stream_blocks(idx->ntotal);
    part.P = nblocks;
    const size_t n = (size_t)nq * part.P * KP;
    VS_HIP(scr.alloc((void**)&part.key, n * sizeof(float)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&part.id, n * sizeof(int)), "vs: scratch");
    const void* qsk = a.qb16 ? a.qb16 : (const void*)a.qbuf;
    KernelTimer tm(st, "skinny_topk");
    VS_HIP(launch_skinny_topk(KP, mode, nq, idx->codes, idx->esize, a.xaux, qsk, a.qaux, idx->ld,
                              ntotal, nblocks, part, st),
           "vs: skinny_topk launch");
    tm.stop();
    VS_HIP(launch_merge_partials(mode, part, nq, a.k, idx->id_base, a.min_score, a.D, a.I, a.k,
                                 st, a.raw),
           "vs: merge launch");
    return VS_OK;
  }
  if (staged_ok) {
    // the automatic order adapts to how much the int8 stage settles
    if (i8_ok && b16_ok && engine == VS_ENGINE_AUTO) i8_ok = adaptive_use_i8(idx);
    // stages: [int8] -> bf16 with deep lists over what is left -> exact fp32
    if (i8_ok) return run_filter_verify(idx, a, need, KF, st, FILTER_I8, !b16_ok);
    if (b16_ok) return run_filter_verify(idx, a, need, KF, st, FILTER_BF16, false);
  }
  if (need > VS_MAX_K) return run_paged(idx, a, st);
  // No plane serves this metric (the cosine self-join of an L2 index, whose
  // planes hold the rows augmented for L2): the staged engine's last stage over
  // every query — the exact fp32 GEMM, its candidates rescored in fp64 — so the
  // keys are the same exact roundings the planes' searches return.
  const int bp = idx->bstats[FILTER_BF16] ? FILTER_BF16 : idx->bstats[FILTER_I8] ? FILTER_I8 : -1;
  if (staged_ok && nq > kSkinnyMaxQ && bp >= 0) {
    int* gl = nullptr;
    int* gc = nullptr;
    VS_HIP(scr.alloc((void**)&gl, (size_t)a.nq_pad * sizeof(int)), "vs: scratch");
    VS_HIP(scr.alloc((void**)&gc, sizeof(int)), "vs: scratch");
    VS_HIP(launch_iota(gl, nq, gc, st), "vs: every query");
    return run_gemm_rescored(idx, a, need, KF, bp, st, gl, gc);
  }
  return run_gemm(idx, a, need, st);
}

}  // namespace host
}  // namespace vs

extern "C" {

int vs_x1_plan(int mode, int filter, int64_t ntotal, int nsplit, int can_dump, int ecut,
               int gathered, int recut, int32_t* out, int cap, int* nlaunch) {
  if (!out || !nlaunch || cap < 0) return fail(VS_E_INVALID, "vs_x1_plan: null output");
  if (!x1_plan_describe(mode, filter, ntotal, nsplit, can_dump != 0, ecut != 0, gathered != 0,
                        recut, dump_mfma32(), out, cap, nlaunch))
    return fail(VS_E_INVALID, "vs_x1_plan: no such pass");
  return VS_OK;
}

}  // extern "C"
