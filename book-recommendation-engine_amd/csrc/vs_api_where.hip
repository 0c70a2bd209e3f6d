// vs_api_where.hip — where searches (DESIGN.md "Where searches"): vs_attrs_*,
// vs_search_where, vs_where_plan, vs_where_stats, the window rounds of route A
// and the page loop of route B (the predicated scan).
#include <atomic>
#include <memory>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

// What vs_api_boost.hip shares with this unit (declared in vs_host.h).
namespace vs {
namespace host {

int check_bounds(const char* what, const float* lo, const float* hi, int64_t n, int ncol) {
  for (int64_t i = 0; i < n * ncol; ++i)
    if ((lo && std::isnan(lo[i])) || (hi && std::isnan(hi[i])))
      return fail(VS_E_INVALID, std::string(what) + ": a NaN bound");
  return VS_OK;
}

void build_preds(const float* lo, const float* hi, const uint64_t* masks, int64_t n, int ncol,
                 std::vector<WherePred>* out) {
  out->resize((size_t)n);
  for (int64_t q = 0; q < n; ++q) {
    WherePred& p = (*out)[(size_t)q];
    p.cmask = 0;
    p.on = 1;
    for (int c = 0; c < kWhereMaxCols; ++c) {
      p.lo[c] = c < ncol && lo ? lo[q * ncol + c] : -INFINITY;
      p.hi[c] = c < ncol && hi ? hi[q * ncol + c] : INFINITY;
      if (!(p.lo[c] == -INFINITY && p.hi[c] == INFINITY)) p.cmask |= 1u << c;
    }
    p.any_of = masks ? masks[q * 3 + 0] : 0;
    p.all_of = masks ? masks[q * 3 + 1] : 0;
    p.none_of = masks ? masks[q * 3 + 2] : 0;
  }
}

// The staged queries list[0 .. cnt) (device) of chunk `a` as a batch of their own.
int gather_batch(const vs_index* idx, const SearchArgs& a, const int* list, int cnt, Scratch& scr,
                 SearchArgs* b, hipStream_t st, const char* what) {
  const size_t rowb = (size_t)idx->ld * sizeof(float);
  const int nq_pad = (int)round_up(std::max<int64_t>(cnt, kGemvMaxQ), kBQ);
  float* gq = nullptr;
  float* gaux = nullptr;
  uint16_t* gq16 = nullptr;
  VS_HIPW(scr.alloc((void**)&gq, (size_t)nq_pad * rowb), what, ": scratch");
  if (a.mode == MODE_L2)
    VS_HIPW(scr.alloc((void**)&gaux, (size_t)nq_pad * sizeof(float)), what, ": scratch");
  VS_HIPW(launch_excl_gather(a.qbuf, (int64_t)rowb, a.mode == MODE_L2 ? a.qaux : nullptr, list, cnt,
                            nq_pad, gq, gaux, st), what, ": gather launch");
  *b = a;
  if (a.qb16) {
    VS_HIPW(scr.alloc((void**)&gq16, (size_t)nq_pad * rowb / 2), what, ": scratch");
    VS_HIPW(launch_excl_gather(a.qb16, (int64_t)rowb / 2, nullptr, list, cnt, nq_pad, gq16, nullptr,
                              st), what, ": gather launch");
    b->qb16 = gq16;
  }
  b->qbuf = gq;
  if (gaux) b->qaux = gaux;
  b->nq = cnt;
  b->nq_pad = nq_pad;
  return VS_OK;
}

// The exclusion sets of the chunk's queries `list` (c0: the chunk's first
// query) as a CSR by slot.
void slot_excl(const std::vector<int64_t>& xoffs, const std::vector<int64_t>& xrows, int64_t c0,
               const std::vector<int>& list, std::vector<int64_t>* offs,
               std::vector<int64_t>* rows) {
  offs->assign(list.size() + 1, 0);
  rows->clear();
  for (size_t s = 0; s < list.size(); ++s) {
    const size_t q = (size_t)(c0 + list[s]);
    rows->insert(rows->end(), xrows.begin() + xoffs[q], xrows.begin() + xoffs[q + 1]);
    (*offs)[s + 1] = (int64_t)rows->size();
  }
}

int upload(Scratch& scr, const void* src, size_t bytes, void** dst, hipStream_t st,
           const char* what) {
  VS_HIPW(scr.alloc(dst, std::max<size_t>(bytes, 8)), what, ": scratch");
  if (bytes)
    VS_HIPW(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st), what, ": upload");
  return VS_OK;
}

// The checks of a handle against its index; the caller holds the reader lock.
int check_attrs(const char* what, const vs_index* idx, const vs_attrs* at) {
  if (at->idx != idx)
    return fail(VS_E_INVALID, std::string(what) + ": the attributes belong to another index");
  if (at->gen != idx->gen)
    return fail(VS_E_INVALID,
                std::string(what) + ": stale attributes (the index changed since they were built)");
  return VS_OK;
}

}  // namespace host
}  // namespace vs

namespace {

// Process-wide counters (vs_where_stats): queries searched, window rounds run
// (summed over chunks), queries searched again after their first window,
// queries answered by the scan, rows gemv_topk_where loaded.
std::atomic<int64_t> g_searches{0}, g_rounds{0}, g_requeried{0}, g_scanned{0}, g_streamed{0};

// What the chunks of one call share.
struct WhereCall {
  const vs_attrs* attrs = nullptr;
  std::vector<WherePred> hp;  // the call's predicates, by query
  WherePred* dp = nullptr;
  std::vector<int64_t> xoffs, xrows;  // the exclusion sets as rows in place (empty: none)
  int64_t* dxoffs = nullptr;
  int64_t* dxrows = nullptr;
  bool scan_only = false;    // VS_WHERE_SCAN
  bool count_first = false;  // a small call: count, then choose the route per query
  bool excl() const { return !xrows.empty(); }
};

// The passing fraction below which a counted query goes to the scan at once.
// Env VS_WHERE_CROSSOVER (read at every search, for tools/bench_where.py's A/B
// runs: 0 keeps every counted query on the windows, 2 scans them all).
double where_crossover() {
  const char* e = getenv("VS_WHERE_CROSSOVER");
  return e ? atof(e) : kWhereCrossover;
}

// Route B over batch `b` (its nq queries staged and padded; results by slot in
// b.D / b.I): run_paged's page loop (vs_engines.hip) with the predicated
// kernels.  preds: the slots' predicates, padded with kGemvMaxQ cleared ones;
// xoffs / xrows: the slots' exclusion CSR or null.  Batches of at most 32
// queries whose metric the streaming kernel computes (inner product, or the
// direct L2 sum of fp32 rows a small call takes) run gemv_topk_where, 8
// queries per pass; everything else gemm_topk_where.
int scan_pages(vs_index* idx, const WhereAttrs& at, const SearchArgs& b, const WherePred* preds,
               const int64_t* xoffs, const int64_t* xrows, unsigned long long* streamed,
               hipStream_t st) {
  const int ntotal = (int)idx->ntotal;
  const bool rule = b.mode == MODE_IP && !b.raw;
  const int64_t need = rule ? 2 * (int64_t)b.k - 1 : (int64_t)b.k;
  const int64_t npages = std::max<int64_t>(1, (std::min<int64_t>(need, ntotal) + 63) / 64);
  const int64_t KA = npages * 64;
  const bool gemv = b.nq <= kSkinnyMaxQ && gemv_fits(idx->ld) &&
                    (b.mode == MODE_IP || (b.mode == MODE_L2 && b.l2_direct && idx->esize == 4));
  const int pmode = gemv && b.mode == MODE_L2 ? MODE_L2D : b.mode;
  const int64_t W =
      gemv ? kGemvMaxQ : std::max<int64_t>(kBQ, ((int64_t)2 << 30) / (KA * 12) / kBQ * kBQ);
  const int64_t nw_max = std::min<int64_t>(W, b.nq);
  const int64_t nrow = round_up(std::max<int64_t>(nw_max, kGemvMaxQ), kBQ);
  Scratch scr(st);
  float* Dacc = nullptr;
  int64_t* Iacc = nullptr;
  float* fkey = nullptr;
  int *fid = nullptr, *member = nullptr, *active = nullptr, *qlist = nullptr, *qcount = nullptr;
  int* wc = nullptr;
  VS_HIP(scr.alloc((void**)&Dacc, (size_t)nrow * KA * sizeof(float)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&Iacc, (size_t)nrow * KA * sizeof(int64_t)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&fkey, (size_t)nrow * sizeof(float)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&fid, (size_t)nrow * sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&member, (size_t)nrow * sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&active, (size_t)nrow * sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&qlist, (size_t)nrow * sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&qcount, sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&wc, sizeof(int)), "vs_search_where: scratch");
  Partials part;
  part.KP = 64;
  int nsplit = 1, cap = 0;
  if (gemv) {
    part.P = stream_blocks(ntotal);
    VS_HIP(scr.alloc((void**)&part.key, (size_t)kGemvMaxQ * part.P * 64 * sizeof(float)),
           "vs_search_where: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)kGemvMaxQ * part.P * 64 * sizeof(int)),
           "vs_search_where: scratch");
  } else {
    const int ntiles = (ntotal + kBN - 1) / kBN;
    nsplit = gathered_nsplit(ntiles);
    part.P = 2 * nsplit;
    cap = slot_window_cap(nrow, part.P, 64);
    VS_HIP(scr.alloc((void**)&part.key, (size_t)cap * part.P * 64 * sizeof(float)),
           "vs_search_where: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)cap * part.P * 64 * sizeof(int)),
           "vs_search_where: scratch");
  }
  for (int64_t q0 = 0; q0 < b.nq; q0 += W) {
    const int nw = (int)std::min<int64_t>(W, b.nq - q0);
    const int nslot = (int)round_up(nw, kBQ);
    const int64_t eoff = q0 * idx->ld;
    const float* qf = b.qbuf + eoff;
    const void* qmat = b.qb16 ? (const void*)((const uint16_t*)b.qb16 + eoff) : (const void*)qf;
    const float* qaux = b.qaux ? b.qaux + q0 : nullptr;
    VS_HIP(hipMemsetAsync(Iacc, 0xFF, (size_t)nw * KA * sizeof(int64_t), st),
           "vs_search_where: pages");
    VS_HIP(launch_page_init(nw, gemv ? kGemvMaxQ : nw, nullptr, nullptr, member, active, fkey, fid,
                            st),
           "vs_search_where: pages");
    VS_HIP(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st),
           "vs_search_where: pages");
    for (int64_t p = 0; p < npages; ++p) {
      if (p > 0) {
        VS_HIP(launch_page_step(Dacc, Iacc, KA, (int)p - 1, nw, b.k, rule ? 1 : 0, pmode, active,
                                fkey, fid, st),
               "vs_search_where: pages");
        VS_HIP(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st),
               "vs_search_where: pages");
      }
      if (gemv) {  // every query's lists (finished ones empty); none: the launch exits
        GemvWhereArgs g;
        g.X = idx->codes;
        g.Q = qf;
        g.ld = idx->ld;
        g.esize = idx->esize;
        g.ntotal = ntotal;
        g.nblocks = part.P;
        g.fkey = fkey;
        g.fid = fid;
        g.run = qcount;
        g.at = at;
        g.preds = preds + q0;
        g.xoffs = xoffs ? xoffs + q0 : nullptr;
        g.xrows = xrows;
        g.streamed = streamed;
        KernelTimer tm(st, p == 0 ? "gemv_topk_where" : nullptr);
        VS_HIP(launch_gemv_topk_where(pmode, nw, g, part, st),
               "vs_search_where: gemv_topk_where launch");
        tm.stop();
        VS_HIP(launch_page_gate(qcount, nw, wc, st), "vs_search_where: pages");
        VS_HIP(launch_merge_partials(pmode, part, nw, 64, 0, -INFINITY, Dacc + p * 64,
                                     Iacc + p * 64, KA, st, 1, nullptr, wc),
               "vs_search_where: merge launch");
        continue;
      }
      for (int w0 = 0; w0 < nslot; w0 += cap) {
        VS_HIP(launch_window_count(qcount, w0, cap, wc, st), "vs_search_where: window");
        GemmWhereArgs g;
        g.X = idx->codes;
        g.xaux = b.xaux;
        g.Q = qmat;
        g.qaux = qaux;
        g.ld = idx->ld;
        g.esize = idx->esize;
        g.ntotal = ntotal;
        g.nq_pad = cap;
        g.nsplit = nsplit;
        g.qlist = qlist + w0;
        g.qcount = wc;
        g.fkey = fkey;
        g.fid = fid;
        g.at = at;
        g.preds = preds + q0;
        g.xoffs = xoffs ? xoffs + q0 : nullptr;
        g.xrows = xrows;
        KernelTimer tm(st, p == 0 && w0 == 0 ? "gemm_topk_where" : nullptr);
        VS_HIP(launch_gemm_topk_where(b.mode, g, part, st),
               "vs_search_where: gemm_topk_where launch");
        tm.stop();
        VS_HIP(launch_merge_partials(b.mode, part, cap, 64, 0, -INFINITY, Dacc + p * 64,
                                     Iacc + p * 64, KA, st, 1, qlist + w0, wc),
               "vs_search_where: merge launch");
      }
    }
    VS_HIP(launch_page_finish(pmode, Dacc, Iacc, KA, nw, b.k, rule ? 1 : 0, member, idx->id_base,
                              b.min_score, b.D + q0 * b.k, b.I + q0 * b.k, st),
           "vs_search_where: pages");
  }
  return VS_OK;
}

// Route B for the chunk's queries `sl` (ascending).
int run_scan(vs_index* idx, const WhereCall& c, const SearchArgs& a, int64_t c0,
             const std::vector<int>& sl, hipStream_t st) {
  const int cnt = (int)sl.size();
  const bool whole = cnt == a.nq;
  Scratch scr(st);
  SearchArgs b = a;
  int* dl = nullptr;
  if (!whole) {
    int rc = upload(scr, sl.data(), sl.size() * sizeof(int), (void**)&dl, st);
    if (!rc) rc = gather_batch(idx, a, dl, cnt, scr, &b, st);
    if (rc) return rc;
  }
  std::vector<WherePred> sp((size_t)round_up(cnt, kGemvMaxQ) + kGemvMaxQ);
  memset(sp.data(), 0, sp.size() * sizeof(WherePred));
  for (int s = 0; s < cnt; ++s) sp[(size_t)s] = c.hp[(size_t)(c0 + sl[(size_t)s])];
  WherePred* dsp = nullptr;
  int rc = upload(scr, sp.data(), sp.size() * sizeof(WherePred), (void**)&dsp, st);
  if (rc) return rc;
  std::vector<int64_t> soffs, srows;
  int64_t* dxo = nullptr;
  int64_t* dxr = nullptr;
  if (c.excl()) {
    slot_excl(c.xoffs, c.xrows, c0, sl, &soffs, &srows);
    rc = upload(scr, soffs.data(), soffs.size() * sizeof(int64_t), (void**)&dxo, st);
    if (!rc) rc = upload(scr, srows.data(), srows.size() * sizeof(int64_t), (void**)&dxr, st);
    if (rc) return rc;
  }
  if (!whole) {
    VS_HIP(scr.alloc((void**)&b.D, (size_t)cnt * a.k * sizeof(float)), "vs_search_where: scratch");
    VS_HIP(scr.alloc((void**)&b.I, (size_t)cnt * a.k * sizeof(int64_t)),
           "vs_search_where: scratch");
  }
  unsigned long long* dstream = nullptr;
  VS_HIP(scr.alloc((void**)&dstream, sizeof(unsigned long long)), "vs_search_where: scratch");
  VS_HIP(hipMemsetAsync(dstream, 0, sizeof(unsigned long long), st), "vs_search_where: counter");
  rc = scan_pages(idx, c.attrs->by_row(), b, dsp, dxo, dxr, dstream, st);
  if (rc) return rc;
  if (!whole)
    VS_HIP(launch_distinct_scatter(b.D, b.I, cnt, a.k, dl, a.D, a.I, st),
           "vs_search_where: scatter launch");
  unsigned long long streamed = 0;
  VS_HIP(hipMemcpyAsync(&streamed, dstream, sizeof(streamed), hipMemcpyDeviceToHost, st),
         "vs_search_where: counter");
  VS_HIP(hipStreamSynchronize(st), "vs_search_where: synchronise");  // (the uploads' sources too)
  g_streamed += (int64_t)streamed;
  g_scanned += cnt;
  return VS_OK;
}

// One chunk of a where search.  Route A, in rounds as run_distinct
// (vs_api_distinct.hip): round r searches the queries still unsettled in raw
// order for a window of where_windows' r-th length, where_drop keeps the
// entries whose row passes the slot's predicate, one merge applies faiss's
// inner-product rule where the call asks for it, and the rows of those queries
// are written.  What the last window leaves unsettled, and what the call sent
// there at once, is answered by route B.
int run_where(vs_index* idx, const WhereCall& c, const SearchArgs& a, int64_t c0, hipStream_t st) {
  const bool tie_rule = a.mode == MODE_IP && !a.raw;
  const int64_t need = tie_rule ? 2 * (int64_t)a.k - 1 : a.k;
  const int64_t live = idx->live();
  const int kin = (int)std::min<int64_t>(need, live);
  const int kout = tie_rule ? kin : a.k;
  const WhereAttrs at = c.attrs->by_row();
  const WherePred* dp = c.dp + c0;
  g_searches += a.nq;
  int64_t wins[64];
  bool scan_tail = false;
  int nwin = where_windows(need, live, wins, 64, &scan_tail);
  if (c.scan_only) nwin = 0;
  Scratch scr(st);
  std::vector<int> cur, sl;  // the queries of the next window round / of the scan
  if (nwin == 0) {
    for (int q = 0; q < a.nq; ++q) sl.push_back(q);
  } else if (c.count_first && scan_tail) {
    unsigned long long* dcnt = nullptr;
    VS_HIP(scr.alloc((void**)&dcnt, (size_t)a.nq * sizeof(unsigned long long)),
           "vs_search_where: scratch");
    VS_HIP(launch_attrs_count(at, c.attrs->nrows, dp, a.nq, dcnt, st),
           "vs_search_where: count launch");
    std::vector<unsigned long long> hc((size_t)a.nq);
    VS_HIP(hipMemcpyAsync(hc.data(), dcnt, hc.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st),
           "vs_search_where: count");
    VS_HIP(hipStreamSynchronize(st), "vs_search_where: synchronise");
    const double cross = where_crossover();
    for (int q = 0; q < a.nq; ++q)
      ((double)hc[(size_t)q] < cross * (double)live ? sl : cur).push_back(q);
  } else {
    for (int q = 0; q < a.nq; ++q) cur.push_back(q);
  }

  int* unsettled = nullptr;
  int* list = nullptr;
  int* dcount = nullptr;
  VS_HIP(scr.alloc((void**)&unsettled, (size_t)a.nq * sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&list, (size_t)a.nq * sizeof(int)), "vs_search_where: scratch");
  VS_HIP(scr.alloc((void**)&dcount, sizeof(int)), "vs_search_where: scratch");
  std::vector<int64_t> soffs, srows;
  bool uploads = false;  // host vectors read by copies not yet waited for
  for (int round = 0; round < nwin && !cur.empty(); ++round) {
    ++g_rounds;
    const int64_t w = wins[round];
    const bool all = w >= live;
    const int cnt = (int)cur.size();
    const bool whole = cnt == a.nq;
    Scratch rs(st);  // the round's batch, windows and lists
    SearchArgs b = a;
    int* qmap = nullptr;
    const int64_t* hoffs = c.excl() ? c.xoffs.data() + c0 : nullptr;
    const int64_t* doffs = c.excl() ? c.dxoffs + c0 : nullptr;
    const int64_t* drows = c.dxrows;
    if (!whole) {
      int rc = upload(rs, cur.data(), cur.size() * sizeof(int), (void**)&qmap, st);
      if (!rc) rc = gather_batch(idx, a, qmap, cnt, rs, &b, st);
      if (rc) return rc;
      uploads = true;
      if (c.excl()) {
        slot_excl(c.xoffs, c.xrows, c0, cur, &soffs, &srows);
        int64_t* d1 = nullptr;
        int64_t* d2 = nullptr;
        rc = upload(rs, soffs.data(), soffs.size() * sizeof(int64_t), (void**)&d1, st);
        if (!rc) rc = upload(rs, srows.data(), srows.size() * sizeof(int64_t), (void**)&d2, st);
        if (rc) return rc;
        hoffs = soffs.data();
        doffs = d1;
        drows = d2;
      }
    }
    b.raw = 1;
    b.k = (int)w;
    VS_HIP(rs.alloc((void**)&b.D, (size_t)cnt * w * sizeof(float)), "vs_search_where: scratch");
    VS_HIP(rs.alloc((void**)&b.I, (size_t)cnt * w * sizeof(int64_t)), "vs_search_where: scratch");
    {
      // extra spans for tools/bench_where.py (they name no search kernel):
      // "where_topk" the engine's part of a round, "where_drop" the rest
      KernelTimer tt(st, "where_topk", false);
      const int rc = hoffs ? run_excluded_chunk(idx, b, hoffs, doffs, drows, st)
                           : run_topk(idx, b, st, VS_ENGINE_AUTO);
      tt.stop();
      if (rc) return rc;
    }
    KernelTimer td(st, "where_drop", false);
    float* Dr = a.D;  // the round's results, by slot
    int64_t* Ir = a.I;
    if (!whole) {
      VS_HIP(rs.alloc((void**)&Dr, (size_t)cnt * a.k * sizeof(float)), "vs_search_where: scratch");
      VS_HIP(rs.alloc((void**)&Ir, (size_t)cnt * a.k * sizeof(int64_t)),
             "vs_search_where: scratch");
    }
    float* Dk = Dr;  // the drop's output
    int64_t* Ik = Ir;
    if (tie_rule) {
      VS_HIP(rs.alloc((void**)&Dk, (size_t)cnt * kin * sizeof(float)), "vs_search_where: scratch");
      VS_HIP(rs.alloc((void**)&Ik, (size_t)cnt * kin * sizeof(int64_t)),
             "vs_search_where: scratch");
    }
    VS_HIP(hipMemsetAsync(unsettled, 0, (size_t)a.nq * sizeof(int), st), "vs_search_where: flags");
    VS_HIP(launch_where_drop(a.mode, b.D, b.I, cnt, (int)w, at, dp, qmap, idx->id_base, (int)need,
                             all, Dk, Ik, kout, unsettled, st),
           "vs_search_where: drop launch");
    if (tie_rule)
      VS_HIP(launch_merge_parts(a.mode, Dk, Ik, 1, cnt, kin, a.k, Dr, Ir, st),
             "vs_search_where: merge launch");
    if (!whole)
      VS_HIP(launch_distinct_scatter(Dr, Ir, cnt, a.k, qmap, a.D, a.I, st),
             "vs_search_where: scatter launch");
    if (all) {  // every allowed row was in the window
      td.stop();
      cur.clear();
      break;
    }
    VS_HIP(launch_compact_flags(unsettled, a.nq, list, dcount, nullptr, nullptr, st),
           "vs_search_where: flags");
    td.stop();
    int left = 0;
    VS_HIP(hipMemcpyAsync(&left, dcount, sizeof(int), hipMemcpyDeviceToHost, st),
           "vs_search_where: count");
    VS_HIP(hipStreamSynchronize(st), "vs_search_where: synchronise");
    uploads = false;
    if (round == 0) g_requeried += left;
    cur.resize((size_t)std::max(left, 0));
    if (left > 0) {
      VS_HIP(hipMemcpyAsync(cur.data(), list, (size_t)left * sizeof(int), hipMemcpyDeviceToHost,
                            st),
             "vs_search_where: list");
      VS_HIP(hipStreamSynchronize(st), "vs_search_where: synchronise");
    }
  }
  if (uploads) VS_HIP(hipStreamSynchronize(st), "vs_search_where: synchronise");
  if (!cur.empty()) {  // past the last window: the scan
    sl.insert(sl.end(), cur.begin(), cur.end());
    std::sort(sl.begin(), sl.end());
  }
  if (sl.empty()) return VS_OK;
  return run_scan(idx, c, a, c0, sl, st);
}

void free_attrs(vs_attrs* a) {
  if (a->rcols && a->rcols != a->lcols) (void)hipFree(a->rcols);
  if (a->rtags && a->rtags != a->ltags) (void)hipFree(a->rtags);
  if (a->rlive) (void)hipFree(a->rlive);
  if (a->lcols) (void)hipFree(a->lcols);
  if (a->ltags) (void)hipFree(a->ltags);
  delete a;
}

}  // namespace

extern "C" {

int vs_attrs_create(vs_index* idx, int ncol, const float* cols, const uint64_t* tags, int64_t n,
                    void* stream, vs_attrs** out) {
  if (!out) return fail(VS_E_INVALID, "vs_attrs_create: null output");
  *out = nullptr;
  if (!idx) return fail(VS_E_INVALID, "vs_attrs_create: null index");
  if (ncol < 0 || ncol > kWhereMaxCols)
    return fail(VS_E_INVALID, "vs_attrs_create: ncol must be in 0 .. 4");
  if (n < 0) return fail(VS_E_INVALID, "vs_attrs_create: n < 0");
  if (n > 0 && ncol > 0 && !cols) return fail(VS_E_INVALID, "vs_attrs_create: null columns");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (n != idx->live())
    return fail(VS_E_INVALID, "vs_attrs_create: n must equal the live row count");
  vs_attrs* a = new vs_attrs();
  a->idx = idx;
  a->device = idx->device;
  a->gen = idx->gen;
  a->n = n;
  a->ncol = ncol;
  a->nrows = idx->ntotal;
  if (n == 0) {
    *out = a;
    return VS_OK;
  }
  DeviceGuard dg(idx->device);
  if (!dg.ok) {
    free_attrs(a);
    return fail(VS_E_HIP, "vs_attrs_create: hipSetDevice failed");
  }
  hipError_t e = hipSuccess;
  const size_t cb = (size_t)ncol * n * sizeof(float);
  if (ncol > 0) {
    e = hipMalloc(&a->lcols, cb);
    if (e == hipSuccess) e = hipMemcpyAsync(a->lcols, cols, cb, hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess && tags) {
    e = hipMalloc(&a->ltags, (size_t)n * sizeof(uint64_t));
    if (e == hipSuccess)
      e = hipMemcpyAsync(a->ltags, tags, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess && idx->dead.empty()) {  // labels are rows: one array serves both
    a->rcols = a->lcols;
    a->rtags = a->ltags;
  } else if (e == hipSuccess) {
    const int64_t nr = a->nrows;
    if (ncol > 0) e = hipMalloc(&a->rcols, (size_t)ncol * nr * sizeof(float));
    if (e == hipSuccess && tags) e = hipMalloc(&a->rtags, (size_t)nr * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&a->rlive, (size_t)nr);
    if (e == hipSuccess)
      e = launch_attrs_spread(a->lcols, a->ltags, n, ncol, idx->ddead, (int64_t)idx->dead.size(),
                              nr, a->rcols, a->rtags, a->rlive, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    free_attrs(a);
    return hip_fail(e, "vs_attrs_create: upload");
  }
  *out = a;
  return VS_OK;
}

int vs_attrs_destroy(vs_attrs* attrs) {
  if (!attrs) return VS_OK;
  DeviceGuard g(attrs->device);
  // the searches that read it were enqueued before this call: let them finish
  if (attrs->lcols || attrs->ltags || attrs->rlive) (void)hipDeviceSynchronize();
  free_attrs(attrs);
  return VS_OK;
}

int vs_attrs_count(const vs_attrs* attrs, const float* lo, const float* hi, const uint64_t* masks,
                   int64_t nq, int64_t* out, void* stream) {
  if (!attrs) return fail(VS_E_INVALID, "vs_attrs_count: null attributes");
  if (nq < 0) return fail(VS_E_INVALID, "vs_attrs_count: nq < 0");
  if (nq > INT_MAX / 2) return fail(VS_E_INVALID, "vs_attrs_count: nq too large");
  if (nq == 0) return VS_OK;
  if (!out) return fail(VS_E_INVALID, "vs_attrs_count: null output");
  int rc = check_bounds("vs_attrs_count", lo, hi, nq, attrs->ncol);
  if (rc) return rc;
  vs_index* idx = attrs->idx;
  if (!idx) return fail(VS_E_INVALID, "vs_attrs_count: the attributes have no index");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  rc = check_attrs("vs_attrs_count", idx, attrs);
  if (rc) return rc;
  if (attrs->n == 0) {
    for (int64_t q = 0; q < nq; ++q) out[q] = 0;
    return VS_OK;
  }
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_attrs_count: hipSetDevice failed");
  std::vector<WherePred> hp;
  build_preds(lo, hi, masks, nq, attrs->ncol, &hp);
  Scratch scr(st);
  WherePred* dp = nullptr;
  unsigned long long* dc = nullptr;
  VS_HIP(scr.alloc((void**)&dp, hp.size() * sizeof(WherePred)), "vs_attrs_count: scratch");
  VS_HIP(scr.alloc((void**)&dc, (size_t)nq * sizeof(unsigned long long)), "vs_attrs_count: scratch");
  VS_HIP(hipMemcpyAsync(dp, hp.data(), hp.size() * sizeof(WherePred), hipMemcpyHostToDevice, st),
         "vs_attrs_count: predicates");
  VS_HIP(launch_attrs_count(attrs->by_row(), attrs->nrows, dp, (int)nq, dc, st),
         "vs_attrs_count: launch");
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts copy in place");
  VS_HIP(hipMemcpyAsync(out, dc, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToHost, st),
         "vs_attrs_count: counts");
  VS_HIP(hipStreamSynchronize(st), "vs_attrs_count: synchronise");
  return VS_OK;
}

int vs_search_where(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const float* lo, const float* hi, const uint64_t* masks,
                    const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                    int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_search_where: null index");
  if (!attrs) return fail(VS_E_INVALID, "vs_search_where: null attributes");
  int rc = check_search_args("vs_search_where", idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  if (n == 0) return VS_OK;
  rc = check_bounds("vs_search_where", lo, hi, n, attrs->ncol);
  if (rc) return rc;
  rc = check_excl_lists("vs_search_where", excl_offs, excl_labels, n);
  if (rc) return rc;
  if (!x || !D || !I) return fail(VS_E_INVALID, "vs_search_where: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  rc = check_attrs("vs_search_where", idx, attrs);
  if (rc) return rc;
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_where: hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIP(hipStreamIsCapturing(st, &cs), "vs_search_where: stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                "vs_search_where: a capturing stream (the call reads a count on the host after "
                "every round)");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  WhereCall c;
  c.attrs = attrs;
  c.scan_only = (flags & VS_WHERE_SCAN) != 0;
  c.count_first = !c.scan_only && n <= kWhereCountMaxQ;
  const bool empty = idx->ntotal == 0 || idx->live() == 0;
  if (!empty) {
    build_preds(lo, hi, masks, n, attrs->ncol, &c.hp);
    rc = upload(scr, c.hp.data(), c.hp.size() * sizeof(WherePred), (void**)&c.dp, st);
    if (rc) return rc;
    if (excl_offs && excl_offs[n] > 0)
      excl_rows_build(idx, n, excl_offs, excl_labels, &c.xoffs, &c.xrows);
    if (c.excl()) {
      rc = upload(scr, c.xoffs.data(), c.xoffs.size() * sizeof(int64_t), (void**)&c.dxoffs, st);
      if (!rc)
        rc = upload(scr, c.xrows.data(), c.xrows.size() * sizeof(int64_t), (void**)&c.dxrows, st);
      if (rc) return rc;
    }
  }
  return search_staged("vs_search_where", idx, x, n, k, D, I, flags & ~VS_WHERE_SCAN, scr, st,
                       empty, [&](const SearchArgs& sa, int64_t c0) {
                         return run_where(idx, c, sa, c0, st);
                       });
}

int vs_where_plan(int64_t k, int metric, int raw, int64_t live, int64_t* out, int nmax) {
  if (k <= 0 || k > INT_MAX / 2) return fail(VS_E_INVALID, "vs_where_plan: k out of range");
  if (metric != VS_METRIC_L2 && metric != VS_METRIC_INNER_PRODUCT)
    return fail(VS_E_INVALID, "vs_where_plan: bad metric");
  if (live < 0 || nmax < 0 || (nmax > 0 && !out))
    return fail(VS_E_INVALID, "vs_where_plan: bad sizes");
  bool scan = false;
  int n = where_windows(distinct_need(k, metric, raw), live, out, nmax, &scan);
  if (scan) {
    if (n < nmax) out[n] = 0;
    ++n;
  }
  return n;
}

int vs_where_stats(int64_t* searches, int64_t* rounds, int64_t* requeried, int64_t* scanned,
                   int64_t* rows_streamed, int reset) {
  if (!searches || !rounds || !requeried || !scanned || !rows_streamed)
    return fail(VS_E_INVALID, "vs_where_stats: null output");
  *searches = g_searches.load();
  *rounds = g_rounds.load();
  *requeried = g_requeried.load();
  *scanned = g_scanned.load();
  *rows_streamed = g_streamed.load();
  if (reset) g_searches = 0, g_rounds = 0, g_requeried = 0, g_scanned = 0, g_streamed = 0;
  return VS_OK;
}

}  // extern "C"
