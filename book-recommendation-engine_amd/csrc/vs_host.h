// vs_host.h — what the host-only units of the C-ABI share (vs_api*.hip,
// vs_engines.hip, vs_storage.hip, vs_runtime.hip): the handle types, the
// per-call helpers and the declarations of what crosses those units.  The
// kernel units include vs_internal.h alone.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/vsearch.h"
#include "vs_internal.h"

// bf16-first searches between int8 probes: the first gap, doubling to the last.
constexpr int kI8FirstBackoff = 8;
constexpr int kI8MaxBackoff = 64;

struct vs_index {
  int d = 0;
  int metric = VS_METRIC_L2;
  int dtype = VS_DTYPE_F32;
  int device = 0;
  int esize = 4;         // bytes per stored element (4 fp32, 2 bf16)
  int64_t ld = 0;        // row stride in elements, a multiple of 64 (zero padding)
  int64_t ntotal = 0;
  int64_t capacity = 0;  // rows allocated (multiple of kRowPad, >= ntotal + 256)
  int64_t id_base = 0;
  // bumped by whatever moves rows or changes labels (add, remove_ids, reset, a
  // tombstone pack, set_id_base): a selector built before is stale.  An
  // in-place update (vs_update_rows) does neither and leaves it.
  uint64_t gen = 0;
  char* codes = nullptr;   // [capacity][ld] elements
  int64_t rowbytes() const { return ld * esize; }
  char* row(int64_t r) const { return codes + r * rowbytes(); }
  float* norms = nullptr;  // [capacity] squared L2 norms
  // fp32 indexes: the filter planes the filter passes multiply ([capacity][ld]
  // each, kept in step with the rows by add / remove_ids / growth) and
  // |x - plane(x)|^2 per row for the bound: [FILTER_I8] int8 codes + a per-row
  // scale (inner-product indexes), [FILTER_BF16] bf16 (round-to-nearest-even)
  // copies.  bf16 indexes use the exact bf16 engine, no plane.
  bool plane_on[2] = {false, false};
  char* fplane[2] = {nullptr, nullptr};
  float* rn2[2] = {nullptr, nullptr};
  float* fscale = nullptr;  // int8 plane: s = max|x| / 127 per row
  // per plane: max |x|^2, max |x - plane(x)|^2, max of their ratio over the
  // rows (the bound's index maxima; grown by add, recomputed by remove_ids)
  unsigned* bstats[2] = {nullptr, nullptr};
  // L2 indexes: both planes hold augmented rows x' = [x, e_1 .. e_m] whose
  // inner product with q' = [q, C .. C] ranks rows as the L2 key does
  // (launch_quantize_i8_l2aug, launch_bf16_plane_l2aug); the parameters are
  // set by the first add (aug_m = 0 before), anorm / anorm_b = |x'|^2 per row
  // (the planes' bound maxima use them)
  int aug_m = 0;
  vs::L2Aug aug;
  float* anorm = nullptr;
  float* anorm_b = nullptr;
  // Tombstones (indexes without filter planes, e.g. bf16 storage): removed
  // rows stay in place, NaN-filled (no kernel admits them), until a pack; faiss
  // labels are positions among the live rows (searches map their rows through
  // the sorted dead list, launch_label_map).  ntotal counts the rows in place.
  std::string notice;  // the last plane loss (vs_notice), empty if none
  std::vector<int64_t> dead;
  int64_t* ddead = nullptr;  // device copy of `dead`
  int64_t ddead_cap = 0;
  int64_t live() const { return ntotal - (int64_t)dead.size(); }
  // removals fill rows with NaN in place (labels mapped at search time) instead
  // of compacting at once: bf16 indexes (C5: 154 GB of rows cannot move at every
  // removal; an int8 plane of theirs has its factors set to NaN with them) and
  // indexes without planes
  bool tombstones() const { return esize == 2 || (!plane_on[0] && !plane_on[1]); }
  bool l2aug() const { return metric == VS_METRIC_L2 && esize == 4; }
  int64_t planebytes(int p) const {
    if (!l2aug()) return ld * vs::filter_bytes(p);
    return (p == vs::FILTER_I8 ? ld + aug_m : ld + vs::kAugBf16) * vs::filter_bytes(p);
  }
  // Adaptive plane order: the int8 stage pays off while it settles most
  // queries; on data where it hands most of them to bf16 (clustered
  // embeddings) the searches go to bf16 directly, re-probing int8 with an
  // exponential backoff.  Device counters [i8 queries, handed to bf16], read
  // through a pinned mirror when the copy's event has completed (no host wait).
  struct Adaptive {
    std::mutex mu;
    unsigned long long* dcount = nullptr;
    unsigned long long* hmirror = nullptr;
    hipEvent_t ev = nullptr;
    bool pending = false;
    unsigned long long seen_q = 0, seen_h = 0;
    double ema = 0.0;
    bool have = false;
    int skip_left = 0, backoff = kI8FirstBackoff;
  } ad;
  int engine = VS_ENGINE_AUTO;
  std::shared_mutex mu;
  // Completion marks of the calls that read this index's storage on the
  // device: one event per stream a search / self-join / device reconstruct ran
  // on, recorded after its last launch.  Writers that move or free the storage
  // (growth, remove_ids, reset, destroy) wait for these marks only — not for
  // the whole device, where other indexes' searches may be running (faiss's
  // contract: a writer excludes the readers of its own index).
  std::mutex rd_mu;
  std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
  hipStream_t wst = nullptr;  // the index's own (non-blocking) writer stream
};

// A selector of one index (vs_selector_create): the selected rows in place as
// a bitmap and as an ascending list (vs_select.hip), valid while the index's
// generation is the one it was built at.
struct vs_selector {
  vs_index* idx = nullptr;
  int device = 0;
  uint64_t gen = 0;
  int64_t count = 0;         // selected live rows
  uint32_t* rbits = nullptr;  // [whole compaction blocks over ntotal] row bitmap
  int* list = nullptr;        // [count rounded up to kBN] ascending rows, padded
};

// A grouping of one index (vs_grouping_create): the group of every row in
// place (tombstoned rows hold -1; no search returns them), valid while the
// index's generation is the one it was built at.
struct vs_grouping {
  vs_index* idx = nullptr;
  int device = 0;
  uint64_t gen = 0;
  int64_t n = 0;       // labels given = the live rows at creation
  int64_t nrows = 0;   // rows in place the device copy covers
  int64_t groups = 0;  // distinct groups, every -1 row counted as one
  int32_t* dgroup = nullptr;  // [nrows]
};

// The attributes of one index (vs_attrs_create): up to four float columns and
// one 64-bit tag word per label, on the device by label and by row in place
// (one array without tombstones), valid while the index's generation is the
// one they were built at.
struct vs_attrs {
  vs_index* idx = nullptr;
  int device = 0;
  uint64_t gen = 0;
  int64_t n = 0;      // labels given = the live rows at creation
  int64_t nrows = 0;  // rows in place the by-row arrays cover
  int ncol = 0;
  float* lcols = nullptr;               // [ncol][n]
  unsigned long long* ltags = nullptr;  // [n], null: all 0
  float* rcols = nullptr;               // [ncol][nrows]
  unsigned long long* rtags = nullptr;  // [nrows], null: all 0
  uint8_t* rlive = nullptr;             // [nrows], null: no tombstones
  vs::WhereAttrs by_row() const {
    vs::WhereAttrs a;
    a.cols = rcols;
    a.tags = rtags;
    a.live = rlive;
    a.ncol = ncol;
    a.stride = nrows;
    return a;
  }
};

// Route (b) of vs_search_sel serves selections that leave at most this many
// live rows out (a fixed condition of the route, not a tuned threshold).
constexpr int64_t kSelMaxExcluded = 256;

// A range search's result (vs_range_search): device buffers of its own, so it
// outlives the index.
struct vs_range {
  int device = 0;
  int64_t nq = 0;
  int64_t total = 0;
  int64_t ncand = 0;        // rows the candidate passes handed to the verification
  int64_t* lims = nullptr;  // [nq + 1]
  float* D = nullptr;       // [total]
  int64_t* I = nullptr;     // [total]
};

namespace vs {
namespace host {

// The calling thread's last error (vs_last_error); returns `code`.
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define VS_HIP(expr, what)                    \
  do {                                        \
    hipError_t e_ = (expr);                   \
    if (e_ != hipSuccess) return hip_fail(e_, what); \
  } while (0)

// VS_HIP with the message "<what><tail>" (what: the entry point's name, a
// run-time value in the helpers several entry points share; composed only on
// failure).
#define VS_HIPW(expr, what, tail)                                                   \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) return hip_fail(e_, (std::string(what) + (tail)).c_str()); \
  } while (0)

// Selects the index's device for the duration of a call, restoring the caller's.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Records a reader mark of `idx` on `st` when it leaves scope (after the
// caller's last launch on st; also on an error return).
struct ReaderMark {
  vs_index* idx;
  hipStream_t st;
  ReaderMark(vs_index* i, hipStream_t s) : idx(i), st(s) {}
  ~ReaderMark();
};

// Waits (host) until every reader mark of `idx` has completed.  Called with
// the index's writer lock held, so no new reader can start meanwhile.
hipError_t wait_readers(vs_index* idx);

// The index's writer stream (created on first use): non-blocking, so it never
// serialises with the legacy null stream's users, and of the greatest
// priority, which gives it a hardware queue of its own — streams of one
// priority share the process's few hardware queues (GPU_MAX_HW_QUEUES), and a
// shared queue would run the writer behind another stream's search queue.
hipError_t writer_stream(vs_index* idx, hipStream_t* out);

// Per-call scratch: bump allocation from cached chunks, returned at scope end.
struct Scratch {
  static constexpr size_t kAlign = 256;
  hipStream_t st;
  std::vector<ScratchChunk> chunks;
  char* cur = nullptr;
  size_t left = 0;
  explicit Scratch(hipStream_t s) : st(s) {}
  hipError_t alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) return hipSuccess;
    bytes = (bytes + kAlign - 1) & ~(kAlign - 1);
    if (bytes > left) {
      ScratchChunk c;
      hipError_t e = scratch_chunk_get(bytes, st, &c);
      if (e != hipSuccess) return e;
      chunks.push_back(c);
      cur = (char*)c.p;
      left = c.size;
    }
    *p = cur;
    cur += bytes;
    left -= bytes;
    return hipSuccess;
  }
  ~Scratch() {
    for (auto& c : chunks) scratch_chunk_put(c, st);
  }
};

// Filter-and-verify statistics, counted on the device (no host sync in a
// search): [0] queries, [1] flagged by the first check (given to the wide
// check), [2] flagged by both (redone by the exact engine), [3] handed to a
// second filter stage, [4] wide-set entries, [5] of them rescored (the rest
// reuse the first check's keys), [6] rows stored by dump launches (one
// (row, raw sum) slot each), [7] lane lists out of dump slots.  One buffer per device.
constexpr int kStatSlots = 9;  // [8]: queries ranked by the exact-key stream
unsigned long long* device_stats(int dev);

// Kernel timer (measurement hook for bench.py; see vs_timer_* in vsearch.h).
struct KernelTimer {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t st;
  const char* name = nullptr;
  int dispatches = 1;  // kernel launches between the two events
  bool aux = false;
  double share = 1.0;  // of a filter pass's tiles (X1SpanTimer)
  // name == nullptr: untimed (the filter engine's exact redo, which is not the
  // kernel the roofline is quoted on)
  // names_kernel: this span names the search's dominant kernel (vs_timer_kernel);
  // false for an extra span over several kernels (the whole filter pass)
  KernelTimer(hipStream_t s, const char* nm, bool names_kernel = true);
  void stop();
};

// The filter pass's per-launch spans: dump launches (and every launch of a
// pass without dumps) under the pass's timer name, the list launch of a pass
// with dumps under "<name>_list" (bench.py: the roofline is the dominant
// kernel's own time; the cut and replay kernels between launches are in no
// span).
struct X1SpanTimer : X1Timing {
  const char* name;
  const char* list_name;
  KernelTimer* cur = nullptr;
  X1SpanTimer(const char* n, const char* ln) : name(n), list_name(ln) {}
  void begin(hipStream_t st, bool dominant, double share) override {
    cur = new KernelTimer(st, dominant ? name : list_name);
    cur->share = share;
  }
  void end(hipStream_t) override {
    if (!cur) return;
    cur->stop();
    delete cur;
    cur = nullptr;
  }
  ~X1SpanTimer() override { end(nullptr); }
};

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline int kp_for(int64_t k) {
  return k <= 8      ? 8
         : k <= 16   ? 16
         : k <= 32   ? 32
         : k <= 64   ? 64
         : k <= 128  ? 128
         : k <= 256  ? 256
         : k <= 512  ? 512
                     : 1024;
}

// What a search computes, shared by every engine.
struct SearchArgs {
  int mode = MODE_IP;
  const float* qbuf = nullptr;   // [nq_pad][ld] fp32 query rows (zero padded)
  const void* qb16 = nullptr;    // bf16 copy of the queries (bf16 indexes)
  const float* qaux = nullptr;   // |q|^2 (L2) or 1/|q| (COS), nq_pad entries
  const float* xaux = nullptr;   // per-row norms (L2) or 1/|x| (COS)
  int nq = 0, nq_pad = 0, k = 0;
  int64_t self0 = -1;            // self-join: query q is row self0 + q
  float min_score = 0.0f;
  int raw = 0;                   // VS_RAW_ORDER
  bool l2_direct = false;        // faiss's sequential branch (the call's nq < 20)
  // the call waits for its results anyway (host outputs): a small batch may
  // read its device-side count after the first stage and skip the empty rest
  bool host_wait = false;
  float* D = nullptr;
  int64_t* I = nullptr;
};

// ---- vs_storage.hip ---------------------------------------------------------
void planes_for(vs_index* idx);
void reset_l2aug(vs_index* idx);
int derive_plane(vs_index* idx, int64_t r0, int64_t n, hipStream_t st, bool appended = false);
int ensure_capacity(vs_index* idx, int64_t rows, hipStream_t st);
void free_storage(vs_index* idx);
int make_room(vs_index* idx, int64_t n, hipStream_t st);
int compact_rows(vs_index* idx, const std::vector<int64_t>& rm, hipStream_t st);
int pack_dead(vs_index* idx);
int pack_den();
int64_t row_of_label(const vs_index* idx, int64_t l);

// ---- vs_engines.hip ---------------------------------------------------------
int run_topk(vs_index* idx, const SearchArgs& a, hipStream_t st, int force_engine);

// Database splits of an exact GEMM launch over `ntiles` row tiles and `nqt`
// query tiles (at most 512: one chunk of queries): ~2 workgroups per CU on 256
// CUs, never more splits than tiles.
inline int gemm_nsplit(int ntiles, int nqt) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (512 + nqt - 1) / nqt));
}
// Database splits of an exact GEMM launch over a gathered batch of unknown
// size: each query tile spread over the chip.
inline int gathered_nsplit(int ntiles) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, 256));
}
// Row blocks (lists per query) of the streaming kernels (GEMV, skinny): 256
// rows each, at most 2,048.
inline int stream_blocks(int64_t ntotal) {
  return (int)std::min<int64_t>(2048, std::max<int64_t>(1, (ntotal + 255) / 256));
}
// Row blocks (lists per slot) of the exact-key stream: 1,024 rows each, at
// most 256.
inline int exact_stream_lists(int64_t ntotal) {
  return (int)std::min<int64_t>(256, std::max<int64_t>(1, (ntotal + 1023) / 1024));
}
// The gathered queries run in slot windows of at most this many slots (whole
// query tiles, at least one), so their `lists` lists of KP entries stay within
// ~1 GB whatever the batch (a 65,536-student self-join chunk at KP = 64 would
// need 16 GB for every slot at once); windows past the device-side count exit
// at once (usually all but the first).
inline int slot_window_cap(int64_t nslot, int lists, int KP) {
  return (int)std::min<int64_t>(
      nslot, std::max<int64_t>(kBQ, ((int64_t)1 << 30) / ((int64_t)lists * KP * 8) / kBQ * kBQ));
}
// The GEMV kernel stages kGemvMaxQ query rows and its lists in 64 KB of LDS.
inline bool gemv_fits(int64_t ld) {
  return (size_t)kGemvMaxQ * ld * sizeof(float) + 4 * kGemvMaxQ * 64 * 8 <= 64 * 1024;
}
// The exact-key stream's arguments over the fp32 rows of `idx` for the queries
// at Q / qaux of a search `a`: slots[0 .. *count) in launches of nslot (the
// caller sets s0 per launch, and qrow / the floors where it has them).
inline ExactStreamArgs make_exact_stream_args(const vs_index* idx, const SearchArgs& a,
                                              const float* Q, const float* qaux, const int* slots,
                                              const int* count, int nslot) {
  ExactStreamArgs ea;
  ea.X = (const float*)idx->codes;
  ea.xn = idx->norms;
  ea.xinv = a.mode == MODE_COS ? a.xaux : nullptr;
  ea.ld = idx->ld;
  ea.ntotal = (int)idx->ntotal;
  ea.Q = Q;
  ea.qaux = qaux;
  ea.slots = slots;
  ea.count = count;
  ea.nslot = nslot;
  return ea;
}

// The sizes of one filter-and-verify stage (vs_engines.hip, run_filter_verify):
// a pure function of the stage's shape, checked without a GPU
// (tools/host_checks.hip).
struct StageShape {
  int mode = MODE_IP, plane = FILTER_I8, KF = 0;
  int nq = 0, nq_pad = 0;  // the search's queries (SearchArgs)
  int64_t ntotal = 0;
  bool gathered = false, deep = false;
  bool self_join = false;  // SearchArgs::self0 >= 0
  bool l2aug = false;      // vs_index::l2aug()
  int L = 8;               // x1_lane_len()
  int skinny_max_q = 0;    // skinny_plane_max_queries()
  int wgs_env = 0;         // VS_X1_WGS (0 = default)
  int split_mult = 1;      // VS_X1_SPLIT_MULT (>= 1)
};
struct StagePlan {
  int nq_pad = 0;  // the stage's query slots, a multiple of kX1Q
  int nsplit = 0;  // database splits: 4 * nsplit lane lists of L per query
  bool small = false;  // the pass is skinny_plane_topk, not an x1 pass
};
inline StagePlan plan_stage(const StageShape& s) {
  StagePlan p;
  p.nq_pad = (int)round_up(s.nq_pad, kX1Q);
  const int nqt = p.nq_pad / kX1Q;
  const int64_t ntiles = (s.ntotal + kX1Q - 1) / kX1Q;
  // enough lists that their 4*nsplit*L entries cover 16*KF candidates (C4's
  // self-join, KF = 64: 128 lists, which lets the int8 stage settle it: 283k ->
  // 372k students/s, profiles/r02zc), and the workgroup target (below: two per
  // CU on 256 CUs at C3, 128 lists per query; one per CU up to 8 query tiles).
  // More lists put the wide check's floor T (the best last entry of a full
  // list) deeper behind the top-M, which the bound needs on clustered data and
  // on the int8 plane (profiles/r02l_ab_split.txt; one workgroup per CU left
  // 0.7 % of the C3 queries to the exact engine on int8)
  // Inner product past k = 32 (M = 2k - 1 of 59 .. 127, KF = 64 / 128) takes
  // twice as many lists again: at C3 (B = 4096) k = 30 left 13 queries per
  // search and k = 60 815 to the deep bf16 stage (a 10M-row pass of ~20-30 ms
  // however few they are); with 8 KF / L lists 0 and 26 (60.5 vs 78.9 and 85.9
  // vs 94.2 ms per search, profiles/r05q, VS_X1_SPLIT_MULT=2)
  const int lists_per_cand = s.mode == MODE_IP && s.KF >= 64 ? 8 : 4;
  // Workgroups per filter-pass launch the database splits aim at: one round
  // (256, one per CU) for batches of at most 8 query tiles, whose lane lists
  // stay at 128+ per query (C2, 4 query tiles: 256 lists, 405-407k -> 436-441k
  // queries/s, profiles/r06wgs); two rounds (512) above, where one round would
  // cut the lists to 64 per query and saturate some (the 1.25M-row rank of an
  // 8-GPU C3: 11 queries per search to the deep stage, 441k -> 423k).
  const int wg_target = s.wgs_env > 0 ? s.wgs_env : nqt <= 8 ? 256 : 512;
  int64_t n = std::max<int64_t>(
      std::min<int64_t>(ntiles, lists_per_cand * ((s.KF + s.L - 1) / s.L)),
      std::min<int64_t>(ntiles, (wg_target + nqt - 1) / nqt));
  // the deep stage (a gathered batch of the few queries an earlier stage could
  // not settle): as many lists as two workgroups per CU give ONE query tile, so
  // the floors sit far behind the top (the a_M + 2B threshold keeps the wide
  // set small)
  // (lane lists of at most ~1 GB: nq_pad slots x 4 nsplit lists x 8 entries x 8 B)
  if (s.deep)
    n = std::max<int64_t>(
        n, std::min<int64_t>({ntiles, 512, (1ll << 30) / ((int64_t)p.nq_pad * 4 * 8 * 8)}));
  // A first pass on the bf16 plane (the adaptive order's choice when int8
  // hands on too many: embedding-like clustered rows) takes twice the lists:
  // its checks then settle more queries and fewer go to the deep stage
  // (clustered C3 37.1k -> 43.0k queries/s; on uniform rows the int8 pass
  // loses 3 % with them; profiles/r05s)
  if (!s.gathered && !s.deep && s.plane == FILTER_BF16) n = std::min<int64_t>(ntiles, 2 * n);
  // A small batch (at most skinny_max_q queries, the first stage of a search
  // routed here by run_topk) streams its plane once through skinny_plane_topk
  // instead of an x1 pass over a whole query tile: 2,048 lists of 8 per query,
  // the deep stage's count
  p.small = !s.gathered && !s.deep && s.nq <= s.skinny_max_q && !s.self_join &&
            (s.mode == MODE_IP || (s.mode == MODE_L2 && s.l2aug));  // the pass's IP
  if (p.small) n = std::min<int64_t>(512, std::max<int64_t>(1, (ntiles + 3) / 4));
  n = std::max<int64_t>(n, 1);
  // A/B: more (shorter) database splits = more lane lists per query
  p.nsplit = (int)std::min<int64_t>(ntiles, n * s.split_mult);
  return p;
}

// ---- vs_api.hip: what the search entry points share -------------------------
// The argument checks of a search, in the order every entry point makes them:
// the index, the selector (sel_ok: false where a required one is null), n
// (null: the caller checks its own count), k, then the buffers (bufs_ok; a
// call of no queries needs none).  An entry point with checks of its own
// before its buffers' (vs_search_excl's offsets) passes true and checks them
// after those.  Messages are "<what>: ...".
int check_search_args(const char* what, const vs_index* idx, const int64_t* n, int64_t k,
                      bool bufs_ok = true, bool sel_ok = true);

// A call's results on the device: the caller's buffers under VS_OUT_DEVICE,
// else scratch that finish() copies to them before it waits for the stream.
// I == nullptr: a call with one output (vs_mean_rows).
struct HostOut {
  float* D = nullptr;  // where the kernels write
  int64_t* I = nullptr;
  float* hD = nullptr;  // the caller's buffers
  int64_t* hI = nullptr;
  size_t count = 0;  // entries of each
  bool out_dev = false;
  int begin(const char* what, Scratch& scr, float* D_, int64_t* I_, size_t count_, int flags);
  // last_error: a call with device outputs reports the thread's pending HIP
  // error (vs_selfjoin never has: false)
  int finish(const char* what, hipStream_t st, bool last_error = true);
};

// The staged queries of a call: fp32 rows of stride ld, zero padded to whole
// query tiles, |q|^2 of every row (L2) and, for bf16 indexes, the rounded copy.
struct QueryStage {
  float* qbuf = nullptr;
  float* qaux = nullptr;
  uint16_t* qb16 = nullptr;
};
// Buffers for chunks of at most `cmax` queries.
int stage_alloc(const char* what, const vs_index* idx, int64_t cmax, Scratch& scr, QueryStage* qs);
// Stages the nc queries at x (host, or device under VS_IN_DEVICE) and fills
// the SearchArgs fields that describe them: mode, qbuf, qb16, qaux, xaux, nq,
// nq_pad.
int stage_chunk(const char* what, const vs_index* idx, const QueryStage& qs, const float* x,
                int64_t nc, int flags, hipStream_t st, SearchArgs* sa);

// A search over n staged queries: the outputs (HostOut), the answer of an
// index without rows to search (`empty`), else the queries in chunks of 65536
// so that scratch stays bounded for any n — run(sa, c0) ranks the chunk that
// starts at query c0 into sa.D / sa.I — and the rows found mapped to faiss
// labels.  The caller holds the reader lock, the device and a reader mark on
// `st`; `scr` is the call's scratch.
template <class Run>
int search_staged(const char* what, vs_index* idx, const float* x, int64_t n, int64_t k, float* D,
                  int64_t* I, int flags, Scratch& scr, hipStream_t st, bool empty, Run run) {
  HostOut out;
  int rc = out.begin(what, scr, D, I, (size_t)n * k, flags);
  if (rc) return rc;
  if (empty) {
    const int mode = idx->metric == VS_METRIC_L2 ? MODE_L2 : MODE_IP;
    VS_HIPW(launch_fill_empty(mode, out.D, out.I, n * k, st), what, ": fill");
    return out.finish(what, st);
  }
  const int64_t chunk = 65536;
  QueryStage qs;
  rc = stage_alloc(what, idx, std::min(n, chunk), scr, &qs);
  if (rc) return rc;
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    SearchArgs sa;
    rc = stage_chunk(what, idx, qs, x + c0 * idx->d, std::min(chunk, n - c0), flags, st, &sa);
    if (rc) return rc;
    sa.k = (int)k;
    sa.raw = (flags & VS_RAW_ORDER) ? 1 : 0;
    sa.l2_direct = n < kBlasThreshold;  // faiss decides on the whole call's nq
    sa.host_wait = !out.out_dev;
    sa.D = out.D + c0 * k;
    sa.I = out.I + c0 * k;
    rc = run(sa, c0);
    if (rc) return rc;
  }
  // tombstoned rows never enter a list; the rows found become faiss labels
  if (!idx->dead.empty())
    VS_HIPW(launch_label_map(out.I, n * k, idx->ddead, (int64_t)idx->dead.size(), idx->id_base, st),
            what, ": labels");
  return out.finish(what, st);
}

// ---- vs_api_profile.hip: for the entry points built on vs_search_excl --------
// vs_search_excl's checks of its lists ("<what>: ..."; null offsets: no lists).
int check_excl_lists(const char* what, const int64_t* excl_offs, const int64_t* excl_labels,
                     int64_t n);
// vs_search / vs_search_excl (lists null or all empty: the plain search) for a
// caller that holds the reader lock, the device and a reader mark on `st`, its
// arguments checked.
int search_excl_held(vs_index* idx, const float* x, int64_t n, int64_t k, const int64_t* excl_offs,
                     const int64_t* excl_labels, float* D, int64_t* I, int flags, hipStream_t st);

// One chunk of a search with exclusion sets (run_excluded) for
// vs_search_distinct: hoffs / doffs = the chunk's nq + 1 CSR offsets (host /
// device) into drows, the excluded rows in place, every segment ascending and
// distinct.
int run_excluded_chunk(vs_index* idx, const SearchArgs& a, const int64_t* hoffs,
                       const int64_t* doffs, const int64_t* drows, hipStream_t st);
// The exclusion sets of n queries as rows in place (labels that are not live
// labels, -1 and duplicates dropped): offs (n + 1, from 0) and rows.  The
// caller holds the reader lock.
void excl_rows_build(const vs_index* idx, int64_t n, const int64_t* excl_offs,
                     const int64_t* excl_labels, std::vector<int64_t>* offs,
                     std::vector<int64_t>* rows);

// ---- distinct searches (vs_api_distinct.hip) ---------------------------------
// The entries a distinct search's answer is a function of: faiss's
// inner-product rule reads 2k - 1, every other order k.
inline int64_t distinct_need(int64_t k, int metric, int raw) {
  return metric == VS_METRIC_INNER_PRODUCT && !raw ? 2 * k - 1 : k;
}
// The window (raw entries per query) of round `round` of a distinct search
// over `live` rows: need + max(16, need / 2), four times longer every round,
// clipped to the live rows.  A cost knob only: any non-decreasing schedule
// that ends at the live rows is exact (DESIGN.md "Distinct searches").
inline int64_t distinct_window(int64_t need, int round, int64_t live) {
  int64_t w = need + std::max<int64_t>(16, need / 2);
  for (int r = 0; r < round && w < live; ++r) w *= 4;
  return std::min(w, live);
}

// ---- where searches (vs_api_where.hip) -----------------------------------------
// The longest window of route A: the staged engine's candidate limit.  Past
// it the paged engine would answer in w / 64 passes; the predicated scan
// answers in one.
constexpr int64_t kWhereMaxWindow = 1023;
// Calls of at most kWhereCountMaxQ queries count their predicates' rows first
// and scan at once the queries whose passing fraction is below the crossover.
// Measured (DESIGN.md section 7 "Where searches", 10M x 1536 fp32, k = 10): the
// scan wins at p = 0.03 and below at batch 1 (7.1-7.2 ms against 11.9-21.8)
// and from p = 0.01 at batch 8 (13.5 against 26-29; p = 0.03 is a tie), the
// windows win at p = 0.1 at batch 8 (12.3-15.8 against 34.6-38.3) and for L2
// at batch 1.  The byte ratio of the int8 plane to the fp32 row (1/4), the
// value this started from, sent p = 0.1 at batch 8 to a scan 2.2-3.1x slower.
constexpr int kWhereCountMaxQ = 32;
constexpr double kWhereCrossover = 0.05;
// The windows of a where search (distinct_window's, while at most
// kWhereMaxWindow or every live row) into out[0 .. nmax); returns how many the
// whole schedule has, *scan = what they leave unsettled goes to the scan
// (false: the last window is every live row).
inline int where_windows(int64_t need, int64_t live, int64_t* out, int nmax, bool* scan) {
  int n = 0;
  *scan = false;
  if (live <= 0) return 0;
  for (int r = 0;; ++r) {
    const int64_t w = distinct_window(need, r, live);
    if (w < live && w > kWhereMaxWindow) {
      *scan = true;
      break;
    }
    if (n < nmax) out[n] = w;
    ++n;
    if (w >= live) break;
  }
  return n;
}
// What vs_api_where.hip defines for the boosted and the bonus searches too
// (`what`: the entry point's name, the prefix of every message).
// A NaN in lo / hi ([n][ncol], either may be null) is VS_E_INVALID.
int check_bounds(const char* what, const float* lo, const float* hi, int64_t n, int ncol);
// The n predicates of a call's where arrays (all null: every live row passes).
void build_preds(const float* lo, const float* hi, const uint64_t* masks, int64_t n, int ncol,
                 std::vector<vs::WherePred>* out);
// The staged queries list[0 .. cnt) (device) of chunk `a` as a batch of their own.
int gather_batch(const vs_index* idx, const SearchArgs& a, const int* list, int cnt, Scratch& scr,
                 SearchArgs* b, hipStream_t st, const char* what);
// The exclusion sets (CSR xoffs / xrows by the call's query) of the chunk's
// queries `list` (c0: the chunk's first query) as a CSR by slot.
void slot_excl(const std::vector<int64_t>& xoffs, const std::vector<int64_t>& xrows, int64_t c0,
               const std::vector<int>& list, std::vector<int64_t>* offs,
               std::vector<int64_t>* rows);
// *dst = scratch holding the `bytes` at src (copied on `st`; src must live
// until the stream has passed the copy).
int upload(Scratch& scr, const void* src, size_t bytes, void** dst, hipStream_t st,
           const char* what);
// The checks of an attribute handle against its index (foreign, stale); the
// caller holds the reader lock.
int check_attrs(const char* what, const vs_index* idx, const vs_attrs* at);

// The counters of one kind of search on the route driver (vs_where_stats,
// vs_boost_stats): queries searched, window rounds run (summed over chunks),
// queries searched again after their first window, queries answered by the
// scan, rows the where scan's streaming kernel loaded (the boosted scan counts
// none).
struct RouteStats {
  std::atomic<int64_t> searches{0}, rounds{0}, requeried{0}, scanned{0}, streamed{0};
  void reset() { searches = 0, rounds = 0, requeried = 0, scanned = 0, streamed = 0; }
};
// What the chunks of one where or boosted call share.  Specs given (hs / ds):
// a boosted call, whose chunks arrive in raw order.
struct WhereCall {
  const vs_attrs* attrs = nullptr;
  std::vector<vs::WherePred> hp;  // the call's predicates, by query
  std::vector<vs::BoostSpec> hs;  // the call's boosts, by query (empty: a where call)
  vs::WherePred* dp = nullptr;
  vs::BoostSpec* ds = nullptr;
  std::vector<int64_t> xoffs, xrows;  // the exclusion sets as rows in place (empty: none)
  int64_t* dxoffs = nullptr;
  int64_t* dxrows = nullptr;
  bool scan_only = false;    // VS_WHERE_SCAN / VS_BOOST_SCAN
  bool count_first = false;  // a small where call: count, then choose the route per query
  RouteStats* stats = nullptr;  // the kind's counters
  bool excl() const { return !xrows.empty(); }
  bool boosted() const { return !hs.empty(); }
};
// The device copies of the call's predicates (where it has any), boosts and
// exclusion sets into `scr`; the vectors must live until `st` has passed them.
int upload_call(const char* what, Scratch& scr, WhereCall* c, hipStream_t st);
// One chunk of a where or boosted search into a.D / a.I (labels = row +
// id_base; c0 = the chunk's first query in the call's arrays): the window
// rounds of route A, then the predicated scan (route B) for what they leave.
// Its messages name vs_search_where or vs_search_boost by the call's kind.
int run_where(vs_index* idx, const WhereCall& c, const SearchArgs& a, int64_t c0, hipStream_t st);
// vs_search_where / vs_search_boost after the checks of their own arguments
// (idx, attrs, n > 0, k, the boosts): the checks of the where arrays, the
// exclusion lists and the buffers, the lock, the device, the uploads and the
// chunks.  c: attrs, hs, scan_only, count_first and stats set.
int search_where_call(const char* what, vs_index* idx, WhereCall* c, const float* x, int64_t n,
                      int64_t k, const float* lo, const float* hi, const uint64_t* masks,
                      const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                      int flags, hipStream_t st);

// ---- boosted searches (vs_api_boost.hip) ---------------------------------------
// The give-up rule of route A: after a round, a query whose deficit
// final_key[k-1] - fl32(K_w - U) exceeds kBoostGiveUp times the window's own
// raw key spread K_w - K_0 goes to the scan at once instead of to a window four
// times longer.  A cost rule only (the scan is exact).  Env VS_BOOST_GIVEUP
// (read at every search, for tools/bench_boost.py's A/B runs; a negative value
// runs every window before the scan).  1.0 is the starting value: the A/B on a
// 10M-row corpus that DESIGN.md section 7 "Boosted searches" describes has not
// been run yet, so it is neither confirmed nor replaced.
constexpr double kBoostGiveUp = 1.0;
float boost_giveup();
// The windows of a boosted search: where_windows', while boost_rerank can sort
// them (kBoostMaxWindow entries); *scan = what they leave goes to the scan.
int boost_windows(int64_t k, int64_t live, int64_t* out, int nmax, bool* scan);
// The n specs of a call from vs_search_boost's boost arrays, checked
// ("<what>: ...").
int build_specs(const char* what, int ncol, const int32_t* kinds, const float* params,
                const uint64_t* tag_masks, const float* tag_bonus, int64_t n,
                std::vector<vs::BoostSpec>* out);
// vs_boost_stats' counters (a bonus search's base search counts there too).
extern RouteStats g_boost_stats;

}  // namespace host
}  // namespace vs
