// vs_api_bonus.hip — bonus searches (DESIGN.md "Bonus searches"):
// vs_search_bonus, vs_bonus_stats.  The base search is the boosted search's
// chunk (run_where on a boosted call) with an attribute handle and the plain
// raw-order search without one; the listed rows are scored and merged by
// vs_bonus.hip.
#include <atomic>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

const char* const kWhat = "vs_search_bonus";

// Process-wide counters (vs_bonus_stats): queries searched, listed live rows
// scored, queries whose base search carried an extra exclusion, result entries
// that are listed rows.
std::atomic<int64_t> g_searches{0}, g_listed{0}, g_demoted{0}, g_entered{0};

// What the chunks of one call share.
struct BonusCall {
  // the lists as rows in place: a CSR over the call's queries, every segment
  // ascending and distinct, live rows only
  std::vector<int64_t> offs, rows;
  std::vector<float> vals;
  int64_t* doffs = nullptr;
  int64_t* drows = nullptr;
  float* dvals = nullptr;
  // the caller's exclusion sets as rows in place (empty: none): what a listed
  // row is tested against.  base.xoffs / base.xrows hold them joined with the
  // listed rows of negative bonus: what the base search excludes.
  std::vector<int64_t> xoffs, xrows;
  int64_t* dxoffs = nullptr;
  int64_t* dxrows = nullptr;
  WhereCall base;  // a boosted call; without attributes only its exclusion sets are used
  unsigned long long* dentered = nullptr;
  bool any() const { return !rows.empty(); }
  bool excl() const { return !xrows.empty(); }
};

// The checks of the lists that need no index.
int check_bonus_lists(const int64_t* offs, const int64_t* labels, const float* vals, int64_t n) {
  if (!offs) return VS_OK;
  bool mono = offs[0] == 0;
  for (int64_t q = 0; q < n && mono; ++q) mono = offs[q + 1] >= offs[q];
  if (!mono)
    return fail(VS_E_INVALID, "vs_search_bonus: bonus offsets must start at 0 and not decrease");
  if (offs[n] > 0 && (!labels || !vals))
    return fail(VS_E_INVALID, "vs_search_bonus: null bonus labels or values");
  for (int64_t e = 0; e < offs[n]; ++e)
    if (!std::isfinite(vals[e]))
      return fail(VS_E_INVALID, "vs_search_bonus: a bonus that is not finite");
  std::vector<int64_t> seg;
  for (int64_t q = 0; q < n; ++q) {
    seg.assign(labels + offs[q], labels + offs[q + 1]);
    std::sort(seg.begin(), seg.end());
    if (std::adjacent_find(seg.begin(), seg.end()) != seg.end())
      return fail(VS_E_INVALID, "vs_search_bonus: a label twice in one bonus list");
  }
  for (int64_t q = 0; q < n; ++q)
    if (offs[q + 1] - offs[q] > kBonusMaxList)
      return fail(VS_E_UNSUPPORTED, "vs_search_bonus: a bonus list longer than " +
                                        std::to_string(kBonusMaxList) + " entries");
  return VS_OK;
}

// The lists of n queries as rows in place, and the base search's exclusion
// sets.  The caller holds the reader lock; c->xoffs / c->xrows are built.
void build_lists(const vs_index* idx, int64_t n, const int64_t* offs, const int64_t* labels,
                 const float* vals, BonusCall* c, int64_t* demoted) {
  const int64_t live = idx->live();
  c->offs.assign((size_t)n + 1, 0);
  std::vector<std::pair<int64_t, float>> seg;
  std::vector<int64_t> neg, joined;
  std::vector<int64_t>& boffs = c->base.xoffs;
  std::vector<int64_t>& brows = c->base.xrows;
  boffs.assign((size_t)n + 1, 0);
  brows.clear();
  *demoted = 0;
  for (int64_t q = 0; q < n; ++q) {
    seg.clear();
    for (int64_t e = offs[q]; e < offs[q + 1]; ++e) {
      const int64_t r = labels[e] - idx->id_base;
      if (r >= 0 && r < live) seg.emplace_back(r, vals[e]);
    }
    std::sort(seg.begin(), seg.end(),
              [](const std::pair<int64_t, float>& a, const std::pair<int64_t, float>& b) {
                return a.first < b.first;
              });
    // positions among the live rows -> rows in place (excl_rows_build's walk)
    if (!idx->dead.empty()) {
      size_t j = 0;
      int64_t shift = 0;
      for (auto& pr : seg) {
        while (j < idx->dead.size() && idx->dead[j] <= pr.first + shift) ++j, ++shift;
        pr.first += shift;
      }
    }
    neg.clear();
    for (const auto& pr : seg) {
      c->rows.push_back(pr.first);
      c->vals.push_back(pr.second);
      if (pr.second < 0.0f) neg.push_back(pr.first);  // (-0 is not negative)
    }
    c->offs[(size_t)q + 1] = (int64_t)c->rows.size();
    const int64_t* ub = c->excl() ? c->xrows.data() + c->xoffs[(size_t)q] : nullptr;
    const int64_t un = c->excl() ? c->xoffs[(size_t)q + 1] - c->xoffs[(size_t)q] : 0;
    joined.resize((size_t)un + neg.size());
    joined.resize((size_t)(std::set_union(ub, ub + un, neg.begin(), neg.end(), joined.begin()) -
                           joined.begin()));
    if ((int64_t)joined.size() > un) ++*demoted;
    brows.insert(brows.end(), joined.begin(), joined.end());
    boffs[(size_t)q + 1] = (int64_t)brows.size();
  }
}

// The base search of one chunk into b.D / b.I: raw order, labels = row + id_base.
int run_base(vs_index* idx, const BonusCall& c, const SearchArgs& b, int64_t c0, hipStream_t st) {
  if (c.base.attrs) return run_where(idx, c.base, b, c0, st);
  if (c.base.excl())
    return run_excluded_chunk(idx, b, c.base.xoffs.data() + c0, c.base.dxoffs + c0, c.base.dxrows,
                              st);
  return run_topk(idx, b, st, VS_ENGINE_AUTO);
}

// One chunk: the base search, the listed rows' final keys, the merge.
int run_bonus(vs_index* idx, const BonusCall& c, const SearchArgs& a, int64_t c0, hipStream_t st) {
  BonusLists bl;
  bl.offs = c.doffs + c0;
  bl.rows = c.drows;
  bl.vals = c.dvals;
  bl.e0 = c.offs[(size_t)c0];
  bl.total = c.offs[(size_t)(c0 + a.nq)] - bl.e0;
  bl.nq = a.nq;
  if (bl.total == 0) return run_base(idx, c, a, c0, st);  // no list in this chunk
  Scratch scr(st);
  SearchArgs b = a;
  float* skey = nullptr;
  int64_t* srow = nullptr;
  VS_HIP(scr.alloc((void**)&b.D, (size_t)a.nq * a.k * sizeof(float)), "vs_search_bonus: scratch");
  VS_HIP(scr.alloc((void**)&b.I, (size_t)a.nq * a.k * sizeof(int64_t)), "vs_search_bonus: scratch");
  VS_HIP(scr.alloc((void**)&skey, (size_t)bl.total * sizeof(float)), "vs_search_bonus: scratch");
  VS_HIP(scr.alloc((void**)&srow, (size_t)bl.total * sizeof(int64_t)), "vs_search_bonus: scratch");
  {
    // extra spans for tools/bench_bonus.py (they name no search kernel):
    // "bonus_base" the base search, "bonus_score" and "bonus_merge" the rest
    KernelTimer tt(st, "bonus_base", false);
    const int rc = run_base(idx, c, b, c0, st);
    tt.stop();
    if (rc) return rc;
  }
  BonusScoreArgs s;
  s.mode = a.mode == MODE_L2 && a.l2_direct ? MODE_L2D : a.mode;
  s.X = idx->codes;
  s.esize = idx->esize;
  s.xn = idx->norms;
  s.Q = a.qbuf;
  s.qn = a.qaux;
  s.ld = idx->ld;
  s.lists = bl;
  if (c.base.attrs) {
    s.at = c.base.attrs->by_row();
    s.preds = c.base.dp + c0;
    s.specs = c.base.ds + c0;
  }
  if (c.excl()) {
    s.xoffs = c.dxoffs + c0;
    s.xrows = c.dxrows;
  }
  s.skey = skey;
  s.srow = srow;
  KernelTimer ts(st, "bonus_score", false);
  VS_HIP(launch_bonus_score(s, st), "vs_search_bonus: score launch");
  ts.stop();
  VS_HIP(hipMemsetAsync(c.dentered, 0, sizeof(unsigned long long), st), "vs_search_bonus: count");
  KernelTimer tm(st, "bonus_merge", false);
  VS_HIP(launch_bonus_merge(a.mode, b.D, b.I, a.k, bl, skey, srow, idx->id_base, a.D, a.I,
                            c.dentered, st),
         "vs_search_bonus: merge launch");
  tm.stop();
  unsigned long long entered = 0;
  VS_HIP(hipMemcpyAsync(&entered, c.dentered, sizeof(entered), hipMemcpyDeviceToHost, st),
         "vs_search_bonus: count");
  VS_HIP(hipStreamSynchronize(st), "vs_search_bonus: synchronise");
  g_entered += (int64_t)entered;
  g_listed += bl.total;
  return VS_OK;
}

}  // namespace

extern "C" {

int vs_search_bonus(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const int64_t* bonus_offs, const int64_t* bonus_labels,
                    const float* bonus_vals, const int32_t* kinds, const float* params,
                    const uint64_t* tag_masks, const float* tag_bonus, const float* lo,
                    const float* hi, const uint64_t* masks, const int64_t* excl_offs,
                    const int64_t* excl_labels, float* D, int64_t* I, int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_search_bonus: null index");
  int rc = check_search_args(kWhat, idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  if (n == 0) return VS_OK;
  BonusCall c;
  if (attrs) {
    rc = build_specs(kWhat, attrs->ncol, kinds, params, tag_masks, tag_bonus, n, &c.base.hs);
    if (rc) return rc;
  } else if (kinds || params || tag_masks || tag_bonus || lo || hi || masks) {
    return fail(VS_E_INVALID, "vs_search_bonus: boost or predicate arrays without attributes");
  }
  rc = check_bonus_lists(bonus_offs, bonus_labels, bonus_vals, n);
  if (rc) return rc;
  if (attrs) {
    rc = check_bounds(kWhat, lo, hi, n, attrs->ncol);
    if (rc) return rc;
  }
  rc = check_excl_lists(kWhat, excl_offs, excl_labels, n);
  if (rc) return rc;
  if (!x || !D || !I) return fail(VS_E_INVALID, "vs_search_bonus: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (attrs) {
    rc = check_attrs(kWhat, idx, attrs);
    if (rc) return rc;
  }
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_bonus: hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIP(hipStreamIsCapturing(st, &cs), "vs_search_bonus: stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                "vs_search_bonus: a capturing stream (the call reads a count on the host after "
                "every chunk)");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  c.base.attrs = attrs;
  c.base.scan_only = (flags & VS_BOOST_SCAN) != 0;
  c.base.stats = &g_boost_stats;
  const bool empty = idx->ntotal == 0 || idx->live() == 0;
  int64_t demoted = 0;
  if (!empty) {
    if (excl_offs && excl_offs[n] > 0)
      excl_rows_build(idx, n, excl_offs, excl_labels, &c.xoffs, &c.xrows);
    if (bonus_offs && bonus_offs[n] > 0)
      build_lists(idx, n, bonus_offs, bonus_labels, bonus_vals, &c, &demoted);
    if (!c.any()) {  // no listed live row: the base search's own exclusion sets
      c.base.xoffs = c.xoffs;
      c.base.xrows = c.xrows;
    }
    if (attrs) build_preds(lo, hi, masks, n, attrs->ncol, &c.base.hp);
    rc = upload_call(kWhat, scr, &c.base, st);
    if (rc) return rc;
    if (c.any()) {
      rc = upload(scr, c.offs.data(), c.offs.size() * sizeof(int64_t), (void**)&c.doffs, st, kWhat);
      if (!rc)
        rc = upload(scr, c.rows.data(), c.rows.size() * sizeof(int64_t), (void**)&c.drows, st,
                    kWhat);
      if (!rc)
        rc = upload(scr, c.vals.data(), c.vals.size() * sizeof(float), (void**)&c.dvals, st, kWhat);
      if (!rc && c.excl()) {
        rc = upload(scr, c.xoffs.data(), c.xoffs.size() * sizeof(int64_t), (void**)&c.dxoffs, st,
                    kWhat);
        if (!rc)
          rc = upload(scr, c.xrows.data(), c.xrows.size() * sizeof(int64_t), (void**)&c.dxrows, st,
                      kWhat);
      }
      if (rc) return rc;
      VS_HIP(scr.alloc((void**)&c.dentered, sizeof(unsigned long long)),
             "vs_search_bonus: scratch");
    }
  }
  g_searches += n;
  g_demoted += demoted;
  // the order is the raw one for both metrics, as for the boosted search
  rc = search_staged(kWhat, idx, x, n, k, D, I, (flags & ~VS_BOOST_SCAN) | VS_RAW_ORDER, scr, st,
                     empty, [&](const SearchArgs& sa, int64_t c0) {
                       if (!c.any()) return run_base(idx, c, sa, c0, st);
                       return run_bonus(idx, c, sa, c0, st);
                     });
  if (rc) return rc;
  // the uploads' sources are this call's vectors
  VS_HIP(hipStreamSynchronize(st), "vs_search_bonus: synchronise");
  return VS_OK;
}

int vs_bonus_stats(int64_t* searches, int64_t* listed, int64_t* demoted, int64_t* entered,
                   int reset) {
  if (!searches || !listed || !demoted || !entered)
    return fail(VS_E_INVALID, "vs_bonus_stats: null output");
  *searches = g_searches.load();
  *listed = g_listed.load();
  *demoted = g_demoted.load();
  *entered = g_entered.load();
  if (reset) g_searches = 0, g_listed = 0, g_demoted = 0, g_entered = 0;
  return VS_OK;
}

}  // extern "C"
