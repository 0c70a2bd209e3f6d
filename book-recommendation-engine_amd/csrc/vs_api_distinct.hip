// vs_api_distinct.hip — distinct searches (DESIGN.md "Distinct searches"):
// vs_grouping_*, vs_search_distinct, vs_distinct_plan, vs_distinct_stats and
// the per-chunk rounds behind the search.
#include <atomic>
#include <memory>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// Process-wide counters (vs_distinct_stats): queries searched, rounds run
// (summed over chunks), queries searched again after their first window.
std::atomic<int64_t> g_searches{0}, g_rounds{0}, g_requeried{0};

// The exclusion sets of a call as rows in place (empty: none).
struct DistinctExcl {
  std::vector<int64_t> offs, rows;
  int64_t* doffs = nullptr;
  int64_t* drows = nullptr;
  bool any() const { return !rows.empty(); }
};

// The staged queries list[0 .. cnt) of chunk `a` as a batch of their own.
int gather_queries(const vs_index* idx, const SearchArgs& a, const int* list, int cnt,
                   Scratch& scr, SearchArgs* b, hipStream_t st) {
  const size_t rowb = (size_t)idx->ld * sizeof(float);
  const int nq_pad = (int)round_up(std::max<int64_t>(cnt, kGemvMaxQ), kBQ);
  float* gq = nullptr;
  float* gaux = nullptr;
  uint16_t* gq16 = nullptr;
  VS_HIP(scr.alloc((void**)&gq, (size_t)nq_pad * rowb), "vs_search_distinct: scratch");
  if (a.mode == MODE_L2)
    VS_HIP(scr.alloc((void**)&gaux, (size_t)nq_pad * sizeof(float)), "vs_search_distinct: scratch");
  VS_HIP(launch_excl_gather(a.qbuf, (int64_t)rowb, a.mode == MODE_L2 ? a.qaux : nullptr, list, cnt,
                            nq_pad, gq, gaux, st),
         "vs_search_distinct: gather launch");
  *b = a;
  if (a.qb16) {
    VS_HIP(scr.alloc((void**)&gq16, (size_t)nq_pad * rowb / 2), "vs_search_distinct: scratch");
    VS_HIP(launch_excl_gather(a.qb16, (int64_t)rowb / 2, nullptr, list, cnt, nq_pad, gq16, nullptr,
                              st),
           "vs_search_distinct: gather launch");
    b->qb16 = gq16;
  }
  b->qbuf = gq;
  if (gaux) b->qaux = gaux;
  b->nq = cnt;
  b->nq_pad = nq_pad;
  return VS_OK;
}

// One chunk of a distinct search, in rounds: round r searches the queries
// still unsettled (every query in round 0) in raw order for a window of
// distinct_window(need, r, live) entries, collapses each window to the first
// entry of every group, applies faiss's inner-product rule where the call
// asks for it, and writes the rows of those queries.  After a round the host
// reads how many queries found their window too short; the last window is
// every live row, which settles every query.  ex: the call's exclusion sets,
// c0: the chunk's first query.
int run_distinct(vs_index* idx, const vs_grouping* grp, const SearchArgs& a, const DistinctExcl& ex,
                 int64_t c0, hipStream_t st) {
  const bool tie_rule = a.mode == MODE_IP && !a.raw;
  const int64_t need = tie_rule ? 2 * (int64_t)a.k - 1 : a.k;
  const int64_t live = idx->live();
  const int kin = (int)std::min<int64_t>(need, live);
  const int kout = tie_rule ? kin : a.k;
  Scratch scr(st);
  int* unsettled = nullptr;
  int* lists = nullptr;  // two lists of nq: a round reads one and writes the other
  int* dcount = nullptr;
  VS_HIP(scr.alloc((void**)&unsettled, (size_t)a.nq * sizeof(int)), "vs_search_distinct: scratch");
  VS_HIP(scr.alloc((void**)&lists, 2 * (size_t)a.nq * sizeof(int)), "vs_search_distinct: scratch");
  VS_HIP(scr.alloc((void**)&dcount, sizeof(int)), "vs_search_distinct: scratch");
  g_searches += a.nq;

  SearchArgs cur = a;
  const int* qmap = nullptr;  // the round's slots -> the chunk's queries (null: every query)
  int cnt = a.nq;
  // the round's exclusion CSR (round 0: the chunk's part of the call's)
  const int64_t* hoffs = ex.any() ? ex.offs.data() + c0 : nullptr;
  const int64_t* doffs = ex.any() ? ex.doffs + c0 : nullptr;
  const int64_t* drows = ex.drows;
  std::vector<int64_t> soffs, srows;
  std::vector<int> hlist;
  std::unique_ptr<Scratch> batch;  // the gathered queries of the current round
  for (int round = 0;; ++round) {
    ++g_rounds;
    const int64_t w = distinct_window(need, round, live);
    const bool all = w >= live;
    Scratch rs(st);  // the round's windows and lists
    SearchArgs b = cur;
    b.raw = 1;
    b.k = (int)w;
    VS_HIP(rs.alloc((void**)&b.D, (size_t)cnt * w * sizeof(float)), "vs_search_distinct: scratch");
    VS_HIP(rs.alloc((void**)&b.I, (size_t)cnt * w * sizeof(int64_t)),
           "vs_search_distinct: scratch");
    {
      // extra spans for tools/bench_distinct.py (they name no search kernel):
      // "distinct_topk" the engine's part of a round, "distinct_collapse" the rest
      KernelTimer tt(st, "distinct_topk", false);
      const int rc = hoffs ? run_excluded_chunk(idx, b, hoffs, doffs, drows, st)
                           : run_topk(idx, b, st, VS_ENGINE_AUTO);
      tt.stop();
      if (rc) return rc;
    }
    KernelTimer tc(st, "distinct_collapse", false);
    // round 0 writes the chunk's rows in place; a later round writes its slots
    // and scatters them, so the rows of settled queries are not written again
    float* Dk = a.D;  // the collapse's output
    int64_t* Ik = a.I;
    float* Dr = a.D;  // the round's results, by slot
    int64_t* Ir = a.I;
    if (round > 0) {
      VS_HIP(rs.alloc((void**)&Dr, (size_t)cnt * a.k * sizeof(float)),
             "vs_search_distinct: scratch");
      VS_HIP(rs.alloc((void**)&Ir, (size_t)cnt * a.k * sizeof(int64_t)),
             "vs_search_distinct: scratch");
      Dk = Dr;
      Ik = Ir;
    }
    if (tie_rule) {
      VS_HIP(rs.alloc((void**)&Dk, (size_t)cnt * kin * sizeof(float)),
             "vs_search_distinct: scratch");
      VS_HIP(rs.alloc((void**)&Ik, (size_t)cnt * kin * sizeof(int64_t)),
             "vs_search_distinct: scratch");
    }
    VS_HIP(launch_distinct_collapse(a.mode, b.D, b.I, cnt, (int)w, grp->dgroup, grp->nrows,
                                    idx->id_base, (int)need, all, qmap, Dk, Ik, kout, nullptr,
                                    unsettled, st),
           "vs_search_distinct: collapse launch");
    if (tie_rule)
      VS_HIP(launch_merge_parts(a.mode, Dk, Ik, 1, cnt, kin, a.k, Dr, Ir, st),
             "vs_search_distinct: merge launch");
    if (round > 0)
      VS_HIP(launch_distinct_scatter(Dr, Ir, cnt, a.k, qmap, a.D, a.I, st),
             "vs_search_distinct: scatter launch");
    if (all) {  // every allowed row was in the window
      tc.stop();
      break;
    }
    int* list = lists + (size_t)(round & 1) * a.nq;
    VS_HIP(launch_compact_flags(unsettled, a.nq, list, dcount, nullptr, nullptr, st),
           "vs_search_distinct: flags");
    tc.stop();
    int left = 0;
    VS_HIP(hipMemcpyAsync(&left, dcount, sizeof(int), hipMemcpyDeviceToHost, st),
           "vs_search_distinct: count");
    VS_HIP(hipStreamSynchronize(st), "vs_search_distinct: synchronise");
    if (left <= 0) break;
    if (round == 0) g_requeried += left;
    // the next round's batch (the previous one is released behind it)
    std::unique_ptr<Scratch> next(new Scratch(st));
    const int rc = gather_queries(idx, a, list, left, *next, &cur, st);
    if (rc) return rc;
    if (ex.any()) {
      // the exclusion sets of the queries left, as a CSR of their own
      hlist.resize((size_t)left);
      VS_HIP(hipMemcpyAsync(hlist.data(), list, (size_t)left * sizeof(int), hipMemcpyDeviceToHost,
                            st),
             "vs_search_distinct: list");
      VS_HIP(hipStreamSynchronize(st), "vs_search_distinct: synchronise");
      soffs.assign((size_t)left + 1, 0);
      srows.clear();
      for (int s = 0; s < left; ++s) {
        const int64_t q = c0 + hlist[(size_t)s];
        srows.insert(srows.end(), ex.rows.begin() + ex.offs[(size_t)q],
                     ex.rows.begin() + ex.offs[(size_t)q + 1]);
        soffs[(size_t)s + 1] = (int64_t)srows.size();
      }
      int64_t* d1 = nullptr;
      int64_t* d2 = nullptr;
      VS_HIP(next->alloc((void**)&d1, soffs.size() * sizeof(int64_t)),
             "vs_search_distinct: scratch");
      VS_HIP(next->alloc((void**)&d2, std::max<size_t>(srows.size(), 1) * sizeof(int64_t)),
             "vs_search_distinct: scratch");
      VS_HIP(hipMemcpyAsync(d1, soffs.data(), soffs.size() * sizeof(int64_t),
                            hipMemcpyHostToDevice, st),
             "vs_search_distinct: offsets");
      if (!srows.empty())
        VS_HIP(hipMemcpyAsync(d2, srows.data(), srows.size() * sizeof(int64_t),
                              hipMemcpyHostToDevice, st),
               "vs_search_distinct: rows");
      // (the host vectors outlive the copies: the next round's count read waits)
      hoffs = soffs.data();
      doffs = d1;
      drows = d2;
    }
    batch = std::move(next);
    qmap = list;
    cnt = left;
  }
  return VS_OK;
}

void free_grouping(vs_grouping* g) {
  if (g->dgroup) (void)hipFree(g->dgroup);
  delete g;
}

}  // namespace

extern "C" {

int vs_grouping_create(vs_index* idx, const int32_t* group_of_label, int64_t n, void* stream,
                       vs_grouping** out) {
  if (!out) return fail(VS_E_INVALID, "vs_grouping_create: null output");
  *out = nullptr;
  if (!idx) return fail(VS_E_INVALID, "vs_grouping_create: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_grouping_create: n < 0");
  if (n > 0 && !group_of_label) return fail(VS_E_INVALID, "vs_grouping_create: null groups");
  for (int64_t i = 0; i < n; ++i)
    if (group_of_label[i] < -1)
      return fail(VS_E_INVALID, "vs_grouping_create: a group must be >= 0, or -1 for a row of its own");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (n != idx->live())
    return fail(VS_E_INVALID, "vs_grouping_create: n must equal the live row count");
  vs_grouping* g = new vs_grouping();
  g->idx = idx;
  g->device = idx->device;
  g->gen = idx->gen;
  g->n = n;
  {
    std::vector<int32_t> s(group_of_label, group_of_label + n);
    std::sort(s.begin(), s.end());
    const int64_t own = std::upper_bound(s.begin(), s.end(), -1) - s.begin();
    g->groups = own + (std::unique(s.begin() + own, s.end()) - (s.begin() + own));
  }
  if (n == 0) {
    *out = g;
    return VS_OK;
  }
  DeviceGuard dg(idx->device);
  if (!dg.ok) {
    free_grouping(g);
    return fail(VS_E_HIP, "vs_grouping_create: hipSetDevice failed");
  }
  // labels are positions among the live rows; the searches' raw entries name
  // rows in place: spread the groups over the tombstones
  g->nrows = idx->ntotal;
  std::vector<int32_t> spread;
  const int32_t* src = group_of_label;
  if (!idx->dead.empty()) {
    spread.assign((size_t)idx->ntotal, -1);
    size_t j = 0;
    int64_t l = 0;
    for (int64_t r = 0; r < idx->ntotal; ++r) {
      if (j < idx->dead.size() && idx->dead[j] == r) {
        ++j;
        continue;
      }
      spread[(size_t)r] = group_of_label[l++];
    }
    src = spread.data();
  }
  hipError_t e = hipMalloc(&g->dgroup, (size_t)g->nrows * sizeof(int32_t));
  if (e == hipSuccess)
    e = hipMemcpyAsync(g->dgroup, src, (size_t)g->nrows * sizeof(int32_t), hipMemcpyHostToDevice,
                       st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    free_grouping(g);
    return hip_fail(e, "vs_grouping_create: upload");
  }
  *out = g;
  return VS_OK;
}

int vs_grouping_groups(const vs_grouping* grp, int64_t* out) {
  if (!grp || !out) return fail(VS_E_INVALID, "vs_grouping_groups: null argument");
  *out = grp->groups;
  return VS_OK;
}

int vs_grouping_destroy(vs_grouping* grp) {
  if (!grp) return VS_OK;
  DeviceGuard g(grp->device);
  // the searches that read it were enqueued before this call: let them finish
  if (grp->dgroup) (void)hipDeviceSynchronize();
  free_grouping(grp);
  return VS_OK;
}

int vs_search_distinct(vs_index* idx, const vs_grouping* grp, const float* x, int64_t n, int64_t k,
                       const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                       int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_search_distinct: null index");
  if (!grp) return fail(VS_E_INVALID, "vs_search_distinct: null grouping");
  const int rc = check_search_args("vs_search_distinct", idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  if (k > kDistinctMaxK)
    return fail(VS_E_UNSUPPORTED,
                "vs_search_distinct: k > 1024 (the collapse's table holds 2 x 2047 groups, what "
                "inner product's tie rule reads at k = 1024)");
  if (n == 0) return VS_OK;
  const int rcl = check_excl_lists("vs_search_distinct", excl_offs, excl_labels, n);
  if (rcl) return rcl;
  if (!x || !D || !I) return fail(VS_E_INVALID, "vs_search_distinct: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (grp->idx != idx)
    return fail(VS_E_INVALID, "vs_search_distinct: the grouping belongs to another index");
  if (grp->gen != idx->gen)
    return fail(VS_E_INVALID,
                "vs_search_distinct: stale grouping (the index changed since it was built)");
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_distinct: hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIP(hipStreamIsCapturing(st, &cs), "vs_search_distinct: stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                "vs_search_distinct: a capturing stream (the call reads a count on the host after "
                "every round)");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  DistinctExcl ex;
  const bool empty = idx->ntotal == 0 || idx->live() == 0;
  if (!empty && excl_offs && excl_offs[n] > 0)
    excl_rows_build(idx, n, excl_offs, excl_labels, &ex.offs, &ex.rows);
  if (ex.any()) {
    VS_HIP(scr.alloc((void**)&ex.doffs, ex.offs.size() * sizeof(int64_t)),
           "vs_search_distinct: scratch");
    VS_HIP(scr.alloc((void**)&ex.drows, ex.rows.size() * sizeof(int64_t)),
           "vs_search_distinct: scratch");
    VS_HIP(hipMemcpyAsync(ex.doffs, ex.offs.data(), ex.offs.size() * sizeof(int64_t),
                          hipMemcpyHostToDevice, st),
           "vs_search_distinct: offsets");
    VS_HIP(hipMemcpyAsync(ex.drows, ex.rows.data(), ex.rows.size() * sizeof(int64_t),
                          hipMemcpyHostToDevice, st),
           "vs_search_distinct: rows");
  }
  return search_staged("vs_search_distinct", idx, x, n, k, D, I, flags, scr, st, empty,
                       [&](const SearchArgs& sa, int64_t c0) {
                         return run_distinct(idx, grp, sa, ex, c0, st);
                       });
}

int vs_distinct_plan(int64_t k, int metric, int raw, int64_t live, int64_t* out, int nmax) {
  if (k <= 0 || k > kDistinctMaxK) return fail(VS_E_INVALID, "vs_distinct_plan: k out of range");
  if (metric != VS_METRIC_L2 && metric != VS_METRIC_INNER_PRODUCT)
    return fail(VS_E_INVALID, "vs_distinct_plan: bad metric");
  if (live < 0 || nmax < 0 || (nmax > 0 && !out))
    return fail(VS_E_INVALID, "vs_distinct_plan: bad sizes");
  const int64_t need = distinct_need(k, metric, raw);
  int rounds = 0;
  if (live == 0) return 0;
  for (;; ++rounds) {
    const int64_t w = distinct_window(need, rounds, live);
    if (rounds < nmax) out[rounds] = w;
    if (w >= live) break;
  }
  return rounds + 1;
}

int vs_distinct_stats(int64_t* searches, int64_t* rounds, int64_t* requeried, int reset) {
  if (!searches || !rounds || !requeried)
    return fail(VS_E_INVALID, "vs_distinct_stats: null output");
  *searches = g_searches.load();
  *rounds = g_rounds.load();
  *requeried = g_requeried.load();
  if (reset) g_searches = 0, g_rounds = 0, g_requeried = 0;
  return VS_OK;
}

}  // extern "C"
