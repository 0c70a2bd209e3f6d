// vs_api_where.hip — where searches (DESIGN.md "Where searches"): vs_attrs_*,
// vs_search_where, vs_where_plan, vs_where_stats, and the route driver that the
// where and the boosted searches share (run_where): the window rounds of route
// A and the page loop of route B (the predicated scan).
#include <atomic>
#include <memory>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

// What vs_api_boost.hip and vs_api_bonus.hip share with this unit (declared in
// vs_host.h).
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

// vs_where_stats' counters.
RouteStats g_stats;

const char* what_of(const WhereCall& c) { return c.boosted() ? "vs_search_boost" : "vs_search_where"; }

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
// specs: the slots' boosts, padded alike, or null (a where call); xoffs /
// xrows: the slots' exclusion CSR or null.  Batches of at most 32 queries whose
// metric the streaming kernel computes (inner product, or the direct L2 sum of
// fp32 rows a small call takes) run gemv_topk_where / _boost, 8 queries per
// pass; everything else gemm_topk_where / _boost.  With specs the lists,
// floors and pages hold final keys in raw (key, label) order: b.raw is set,
// so the page loop is the raw one.
int scan_pages(const char* what, vs_index* idx, const WhereAttrs& at, const SearchArgs& b,
               const WherePred* preds, const BoostSpec* specs, const int64_t* xoffs,
               const int64_t* xrows, unsigned long long* streamed, hipStream_t st) {
  const char* const kgemm = specs ? "gemm_topk_boost" : "gemm_topk_where";  // the timer spans
  const char* const kgemv = specs ? "gemv_topk_boost" : "gemv_topk_where";
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
  VS_HIPW(scr.alloc((void**)&Dacc, (size_t)nrow * KA * sizeof(float)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&Iacc, (size_t)nrow * KA * sizeof(int64_t)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&fkey, (size_t)nrow * sizeof(float)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&fid, (size_t)nrow * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&member, (size_t)nrow * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&active, (size_t)nrow * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&qlist, (size_t)nrow * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&qcount, sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&wc, sizeof(int)), what, ": scratch");
  Partials part;
  part.KP = 64;
  int nsplit = 1, cap = 0;
  if (gemv) {
    part.P = stream_blocks(ntotal);
    VS_HIPW(scr.alloc((void**)&part.key, (size_t)kGemvMaxQ * part.P * 64 * sizeof(float)), what,
            ": scratch");
    VS_HIPW(scr.alloc((void**)&part.id, (size_t)kGemvMaxQ * part.P * 64 * sizeof(int)), what,
            ": scratch");
  } else {
    const int ntiles = (ntotal + kBN - 1) / kBN;
    nsplit = gathered_nsplit(ntiles);
    part.P = 2 * nsplit;
    cap = slot_window_cap(nrow, part.P, 64);
    VS_HIPW(scr.alloc((void**)&part.key, (size_t)cap * part.P * 64 * sizeof(float)), what,
            ": scratch");
    VS_HIPW(scr.alloc((void**)&part.id, (size_t)cap * part.P * 64 * sizeof(int)), what,
            ": scratch");
  }
  for (int64_t q0 = 0; q0 < b.nq; q0 += W) {
    const int nw = (int)std::min<int64_t>(W, b.nq - q0);
    const int nslot = (int)round_up(nw, kBQ);
    const int64_t eoff = q0 * idx->ld;
    const float* qf = b.qbuf + eoff;
    const void* qmat = b.qb16 ? (const void*)((const uint16_t*)b.qb16 + eoff) : (const void*)qf;
    const float* qaux = b.qaux ? b.qaux + q0 : nullptr;
    VS_HIPW(hipMemsetAsync(Iacc, 0xFF, (size_t)nw * KA * sizeof(int64_t), st), what, ": pages");
    VS_HIPW(launch_page_init(nw, gemv ? kGemvMaxQ : nw, nullptr, nullptr, member, active, fkey,
                             fid, st),
            what, ": pages");
    VS_HIPW(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st), what,
            ": pages");
    for (int64_t p = 0; p < npages; ++p) {
      if (p > 0) {
        VS_HIPW(launch_page_step(Dacc, Iacc, KA, (int)p - 1, nw, b.k, rule ? 1 : 0, pmode, active,
                                 fkey, fid, st),
                what, ": pages");
        VS_HIPW(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st), what,
                ": pages");
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
        g.specs = specs ? specs + q0 : nullptr;
        g.xoffs = xoffs ? xoffs + q0 : nullptr;
        g.xrows = xrows;
        g.streamed = streamed;
        KernelTimer tm(st, p == 0 ? kgemv : nullptr);
        VS_HIPW((specs ? launch_gemv_topk_boost : launch_gemv_topk_where)(pmode, nw, g, part, st),
                what, std::string(": ") + kgemv + " launch");
        tm.stop();
        VS_HIPW(launch_page_gate(qcount, nw, wc, st), what, ": pages");
        VS_HIPW(launch_merge_partials(pmode, part, nw, 64, 0, -INFINITY, Dacc + p * 64,
                                      Iacc + p * 64, KA, st, 1, nullptr, wc),
                what, ": merge launch");
        continue;
      }
      for (int w0 = 0; w0 < nslot; w0 += cap) {
        VS_HIPW(launch_window_count(qcount, w0, cap, wc, st), what, ": window");
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
        g.specs = specs ? specs + q0 : nullptr;
        g.xoffs = xoffs ? xoffs + q0 : nullptr;
        g.xrows = xrows;
        KernelTimer tm(st, p == 0 && w0 == 0 ? kgemm : nullptr);
        VS_HIPW((specs ? launch_gemm_topk_boost : launch_gemm_topk_where)(b.mode, g, part, st),
                what, std::string(": ") + kgemm + " launch");
        tm.stop();
        VS_HIPW(launch_merge_partials(b.mode, part, cap, 64, 0, -INFINITY, Dacc + p * 64,
                                      Iacc + p * 64, KA, st, 1, qlist + w0, wc),
                what, ": merge launch");
      }
    }
    VS_HIPW(launch_page_finish(pmode, Dacc, Iacc, KA, nw, b.k, rule ? 1 : 0, member, idx->id_base,
                               b.min_score, b.D + q0 * b.k, b.I + q0 * b.k, st),
            what, ": pages");
  }
  return VS_OK;
}

// Route B for the chunk's queries `sl` (ascending).
int run_scan(vs_index* idx, const WhereCall& c, const SearchArgs& a, int64_t c0,
             const std::vector<int>& sl, hipStream_t st) {
  const char* const what = what_of(c);
  const int cnt = (int)sl.size();
  const bool whole = cnt == a.nq;
  Scratch scr(st);
  SearchArgs b = a;
  int* dl = nullptr;
  if (!whole) {
    int rc = upload(scr, sl.data(), sl.size() * sizeof(int), (void**)&dl, st, what);
    if (!rc) rc = gather_batch(idx, a, dl, cnt, scr, &b, st, what);
    if (rc) return rc;
  }
  // the slots' predicates and boosts, padded with cleared ones
  const size_t npad = (size_t)round_up(cnt, kGemvMaxQ) + kGemvMaxQ;
  std::vector<WherePred> sp(npad);
  std::vector<BoostSpec> ss(c.boosted() ? npad : 0);
  memset(sp.data(), 0, sp.size() * sizeof(WherePred));
  if (c.boosted()) memset(ss.data(), 0, ss.size() * sizeof(BoostSpec));
  for (int s = 0; s < cnt; ++s) {
    sp[(size_t)s] = c.hp[(size_t)(c0 + sl[(size_t)s])];
    if (c.boosted()) ss[(size_t)s] = c.hs[(size_t)(c0 + sl[(size_t)s])];
  }
  WherePred* dsp = nullptr;
  BoostSpec* dss = nullptr;
  int rc = upload(scr, sp.data(), sp.size() * sizeof(WherePred), (void**)&dsp, st, what);
  if (!rc && c.boosted())
    rc = upload(scr, ss.data(), ss.size() * sizeof(BoostSpec), (void**)&dss, st, what);
  if (rc) return rc;
  std::vector<int64_t> soffs, srows;
  int64_t* dxo = nullptr;
  int64_t* dxr = nullptr;
  if (c.excl()) {
    slot_excl(c.xoffs, c.xrows, c0, sl, &soffs, &srows);
    rc = upload(scr, soffs.data(), soffs.size() * sizeof(int64_t), (void**)&dxo, st, what);
    if (!rc) rc = upload(scr, srows.data(), srows.size() * sizeof(int64_t), (void**)&dxr, st, what);
    if (rc) return rc;
  }
  if (!whole) {
    VS_HIPW(scr.alloc((void**)&b.D, (size_t)cnt * a.k * sizeof(float)), what, ": scratch");
    VS_HIPW(scr.alloc((void**)&b.I, (size_t)cnt * a.k * sizeof(int64_t)), what, ": scratch");
  }
  unsigned long long* dstream = nullptr;  // the rows the where scan's streaming kernel loads
  if (!c.boosted()) {
    VS_HIPW(scr.alloc((void**)&dstream, sizeof(unsigned long long)), what, ": scratch");
    VS_HIPW(hipMemsetAsync(dstream, 0, sizeof(unsigned long long), st), what, ": counter");
  }
  rc = scan_pages(what, idx, c.attrs->by_row(), b, dsp, dss, dxo, dxr, dstream, st);
  if (rc) return rc;
  if (!whole)
    VS_HIPW(launch_distinct_scatter(b.D, b.I, cnt, a.k, dl, a.D, a.I, st), what,
            ": scatter launch");
  unsigned long long streamed = 0;
  if (dstream)
    VS_HIPW(hipMemcpyAsync(&streamed, dstream, sizeof(streamed), hipMemcpyDeviceToHost, st), what,
            ": counter");
  VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");  // (the uploads' sources too)
  c.stats->streamed += (int64_t)streamed;
  c.stats->scanned += cnt;
  return VS_OK;
}

}  // namespace

namespace vs {
namespace host {

int upload_call(const char* what, Scratch& scr, WhereCall* c, hipStream_t st) {
  int rc = VS_OK;
  if (!c->hp.empty())
    rc = upload(scr, c->hp.data(), c->hp.size() * sizeof(WherePred), (void**)&c->dp, st, what);
  if (!rc && c->boosted())
    rc = upload(scr, c->hs.data(), c->hs.size() * sizeof(BoostSpec), (void**)&c->ds, st, what);
  if (!rc && c->excl()) {
    rc = upload(scr, c->xoffs.data(), c->xoffs.size() * sizeof(int64_t), (void**)&c->dxoffs, st,
                what);
    if (!rc)
      rc = upload(scr, c->xrows.data(), c->xrows.size() * sizeof(int64_t), (void**)&c->dxrows, st,
                  what);
  }
  return rc;
}

// Route A, in rounds as run_distinct (vs_api_distinct.hip): round r searches
// the queries still unsettled in raw order for a window of the schedule's r-th
// length, reduces each raw window to the query's k results and flags the
// queries it does not settle, and the rows of those queries are written.
//  - A where call: where_windows; where_drop keeps the entries whose row
//    passes the slot's predicate, and one merge applies faiss's inner-product
//    rule where the call asks for it.  A small call counts first and sends the
//    queries whose predicate passes few rows to the scan at once.
//  - A boosted call: boost_windows; boost_rerank drops the entries that fail
//    the predicate, ranks the rest by final key and decides whether the window
//    was sufficient (state 1), or not worth a longer one (state 2: the scan).
// What the last window leaves unsettled, and what was sent there at once, is
// answered by route B.
int run_where(vs_index* idx, const WhereCall& c, const SearchArgs& a, int64_t c0, hipStream_t st) {
  const char* const what = what_of(c);
  const bool boost = c.boosted();
  if (boost && !a.raw)  // final keys have no faiss tie rule: the scan's page loop is the raw one
    return fail(VS_E_INVALID, std::string(what) + ": a boosted chunk not in raw order");
  const bool tie_rule = a.mode == MODE_IP && !a.raw;
  const int64_t need = tie_rule ? 2 * (int64_t)a.k - 1 : a.k;
  const int64_t live = idx->live();
  const int kin = (int)std::min<int64_t>(need, live);
  const int kout = tie_rule ? kin : a.k;
  const WhereAttrs at = c.attrs->by_row();
  const WherePred* dp = c.dp + c0;
  RouteStats& stats = *c.stats;
  stats.searches += a.nq;
  int64_t wins[64];
  bool scan_tail = false;
  int nwin = boost ? boost_windows(need, live, wins, 64, &scan_tail)
                   : where_windows(need, live, wins, 64, &scan_tail);
  if (c.scan_only) nwin = 0;
  const float giveup = boost && scan_tail ? boost_giveup() : -1.0f;
  Scratch scr(st);
  std::vector<int> cur, sl;  // the queries of the next window round / of the scan
  if (nwin == 0) {
    for (int q = 0; q < a.nq; ++q) sl.push_back(q);
  } else if (c.count_first && scan_tail) {
    unsigned long long* dcnt = nullptr;
    VS_HIPW(scr.alloc((void**)&dcnt, (size_t)a.nq * sizeof(unsigned long long)), what, ": scratch");
    VS_HIPW(launch_attrs_count(at, c.attrs->nrows, dp, a.nq, dcnt, st), what, ": count launch");
    std::vector<unsigned long long> hc((size_t)a.nq);
    VS_HIPW(hipMemcpyAsync(hc.data(), dcnt, hc.size() * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st),
            what, ": count");
    VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
    const double cross = where_crossover();
    for (int q = 0; q < a.nq; ++q)
      ((double)hc[(size_t)q] < cross * (double)live ? sl : cur).push_back(q);
  } else {
    for (int q = 0; q < a.nq; ++q) cur.push_back(q);
  }

  int* flags = nullptr;  // by query: unsettled (where), boost_rerank's state (boosted)
  int* list = nullptr;
  int* dcount = nullptr;
  VS_HIPW(scr.alloc((void**)&flags, (size_t)a.nq * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&list, (size_t)a.nq * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&dcount, sizeof(int)), what, ": scratch");
  std::vector<int64_t> soffs, srows;
  std::vector<int> hstate(boost ? (size_t)a.nq : 0);
  bool uploads = false;  // host vectors read by copies not yet waited for
  for (int round = 0; round < nwin && !cur.empty(); ++round) {
    ++stats.rounds;
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
      int rc = upload(rs, cur.data(), cur.size() * sizeof(int), (void**)&qmap, st, what);
      if (!rc) rc = gather_batch(idx, a, qmap, cnt, rs, &b, st, what);
      if (rc) return rc;
      uploads = true;
      if (c.excl()) {
        slot_excl(c.xoffs, c.xrows, c0, cur, &soffs, &srows);
        int64_t* d1 = nullptr;
        int64_t* d2 = nullptr;
        rc = upload(rs, soffs.data(), soffs.size() * sizeof(int64_t), (void**)&d1, st, what);
        if (!rc) rc = upload(rs, srows.data(), srows.size() * sizeof(int64_t), (void**)&d2, st, what);
        if (rc) return rc;
        hoffs = soffs.data();
        doffs = d1;
        drows = d2;
      }
    }
    b.raw = 1;
    b.k = (int)w;
    VS_HIPW(rs.alloc((void**)&b.D, (size_t)cnt * w * sizeof(float)), what, ": scratch");
    VS_HIPW(rs.alloc((void**)&b.I, (size_t)cnt * w * sizeof(int64_t)), what, ": scratch");
    {
      // extra spans for tools/bench_where.py / bench_boost.py (they name no
      // search kernel): "where_topk" / "boost_topk" the engine's part of a
      // round, "where_drop" / "boost_rerank" the rest
      KernelTimer tt(st, boost ? "boost_topk" : "where_topk", false);
      const int rc = hoffs ? run_excluded_chunk(idx, b, hoffs, doffs, drows, st)
                           : run_topk(idx, b, st, VS_ENGINE_AUTO);
      tt.stop();
      if (rc) return rc;
    }
    KernelTimer td(st, boost ? "boost_rerank" : "where_drop", false);
    float* Dr = a.D;  // the round's results, by slot
    int64_t* Ir = a.I;
    if (!whole) {
      VS_HIPW(rs.alloc((void**)&Dr, (size_t)cnt * a.k * sizeof(float)), what, ": scratch");
      VS_HIPW(rs.alloc((void**)&Ir, (size_t)cnt * a.k * sizeof(int64_t)), what, ": scratch");
    }
    float* Dk = Dr;  // where_drop's output
    int64_t* Ik = Ir;
    if (tie_rule) {
      VS_HIPW(rs.alloc((void**)&Dk, (size_t)cnt * kin * sizeof(float)), what, ": scratch");
      VS_HIPW(rs.alloc((void**)&Ik, (size_t)cnt * kin * sizeof(int64_t)), what, ": scratch");
    }
    VS_HIPW(hipMemsetAsync(flags, 0, (size_t)a.nq * sizeof(int), st), what, ": flags");
    if (boost) {
      VS_HIPW(launch_boost_rerank(a.mode, b.D, b.I, cnt, (int)w, at, dp, c.ds + c0, qmap,
                                  idx->id_base, a.k, all, giveup, Dr, Ir, flags, nullptr, nullptr,
                                  st),
              what, ": rerank launch");
    } else {
      VS_HIPW(launch_where_drop(a.mode, b.D, b.I, cnt, (int)w, at, dp, qmap, idx->id_base,
                                (int)need, all, Dk, Ik, kout, flags, st),
              what, ": drop launch");
      if (tie_rule)
        VS_HIPW(launch_merge_parts(a.mode, Dk, Ik, 1, cnt, kin, a.k, Dr, Ir, st), what,
                ": merge launch");
    }
    if (!whole)
      VS_HIPW(launch_distinct_scatter(Dr, Ir, cnt, a.k, qmap, a.D, a.I, st), what,
              ": scatter launch");
    if (all) {  // every allowed row was in the window
      td.stop();
      cur.clear();
      break;
    }
    VS_HIPW(launch_compact_flags(flags, a.nq, list, dcount, nullptr, nullptr, st), what, ": flags");
    td.stop();
    int left = 0;
    VS_HIPW(hipMemcpyAsync(&left, dcount, sizeof(int), hipMemcpyDeviceToHost, st), what, ": count");
    VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
    uploads = false;
    if (round == 0) stats.requeried += left;
    cur.clear();
    if (left <= 0) break;
    if (boost) {  // who is left, and who of them gave up
      VS_HIPW(hipMemcpyAsync(hstate.data(), flags, (size_t)a.nq * sizeof(int),
                             hipMemcpyDeviceToHost, st),
              what, ": list");
      VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
      for (int q = 0; q < a.nq; ++q) {
        if (hstate[(size_t)q] == 1) cur.push_back(q);
        else if (hstate[(size_t)q] == 2) sl.push_back(q);
      }
    } else {
      cur.resize((size_t)left);
      VS_HIPW(hipMemcpyAsync(cur.data(), list, (size_t)left * sizeof(int), hipMemcpyDeviceToHost,
                             st),
              what, ": list");
      VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
    }
  }
  if (uploads) VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
  sl.insert(sl.end(), cur.begin(), cur.end());  // past the last window: the scan
  if (sl.empty()) return VS_OK;
  std::sort(sl.begin(), sl.end());
  return run_scan(idx, c, a, c0, sl, st);
}

int search_where_call(const char* what, vs_index* idx, WhereCall* c, const float* x, int64_t n,
                      int64_t k, const float* lo, const float* hi, const uint64_t* masks,
                      const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                      int flags, hipStream_t st) {
  int rc = check_bounds(what, lo, hi, n, c->attrs->ncol);
  if (rc) return rc;
  rc = check_excl_lists(what, excl_offs, excl_labels, n);
  if (rc) return rc;
  if (!x || !D || !I) return fail(VS_E_INVALID, std::string(what) + ": null buffer");
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  rc = check_attrs(what, idx, c->attrs);
  if (rc) return rc;
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, std::string(what) + ": hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIPW(hipStreamIsCapturing(st, &cs), what, ": stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                std::string(what) + ": a capturing stream (the call reads a count on the host "
                                    "after every round)");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  const bool empty = idx->ntotal == 0 || idx->live() == 0;
  if (!empty) {
    build_preds(lo, hi, masks, n, c->attrs->ncol, &c->hp);
    if (excl_offs && excl_offs[n] > 0)
      excl_rows_build(idx, n, excl_offs, excl_labels, &c->xoffs, &c->xrows);
    rc = upload_call(what, scr, c, st);
    if (rc) return rc;
  }
  return search_staged(what, idx, x, n, k, D, I, flags, scr, st, empty,
                       [&](const SearchArgs& sa, int64_t c0) {
                         return run_where(idx, *c, sa, c0, st);
                       });
}

}  // namespace host
}  // namespace vs

namespace {

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
  const int rc = check_search_args("vs_search_where", idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  if (n == 0) return VS_OK;
  WhereCall c;
  c.attrs = attrs;
  c.scan_only = (flags & VS_WHERE_SCAN) != 0;
  c.count_first = !c.scan_only && n <= kWhereCountMaxQ;
  c.stats = &g_stats;
  return search_where_call("vs_search_where", idx, &c, x, n, k, lo, hi, masks, excl_offs,
                           excl_labels, D, I, flags & ~VS_WHERE_SCAN, (hipStream_t)stream);
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
  *searches = g_stats.searches.load();
  *rounds = g_stats.rounds.load();
  *requeried = g_stats.requeried.load();
  *scanned = g_stats.scanned.load();
  *rows_streamed = g_stats.streamed.load();
  if (reset) g_stats.reset();
  return VS_OK;
}

}  // extern "C"
