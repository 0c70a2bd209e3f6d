// vs_api_boost.hip — boosted searches (DESIGN.md "Boosted searches"):
// vs_search_boost, vs_boost_eval, vs_boost_stats; the window rounds of route A
// and the page loop of route B, restated from vs_api_where.hip for final keys.
#include <atomic>
#include <memory>

#include "vs_boost_value.h"
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

const char* const kWhat = "vs_search_boost";

// Process-wide counters (vs_boost_stats): queries searched, window rounds run
// (summed over chunks), queries searched again after their first window,
// queries answered by the scan.
std::atomic<int64_t> g_searches{0}, g_rounds{0}, g_requeried{0}, g_scanned{0};

float boost_giveup() {
  const char* e = getenv("VS_BOOST_GIVEUP");
  return (float)(e ? atof(e) : kBoostGiveUp);
}

}  // namespace

// The n specs of a call from its arrays; every parameter must be finite and
// s > 0 (a column of kind 0 too), every bonus finite.
int vs::host::build_specs(const char* what, int ncol, const int32_t* kinds, const float* params,
                const uint64_t* tag_masks, const float* tag_bonus, int64_t n,
                std::vector<BoostSpec>* out) {
  if (ncol < 0 || ncol > kWhereMaxCols)
    return fail(VS_E_INVALID, std::string(what) + ": ncol must be in 0 .. 4");
  if (ncol > 0 && n > 0 && (!kinds || !params))
    return fail(VS_E_INVALID, std::string(what) + ": null kinds or parameters");
  if ((tag_masks == nullptr) != (tag_bonus == nullptr))
    return fail(VS_E_INVALID, std::string(what) + ": tag masks and bonuses go together");
  out->resize((size_t)n);
  for (int64_t q = 0; q < n; ++q) {
    BoostSpec& sp = (*out)[(size_t)q];
    memset(&sp, 0, sizeof(sp));
    for (int c = 0; c < kWhereMaxCols; ++c) {
      sp.s[c] = 1.0f;
      if (c >= ncol) continue;
      const int32_t kd = kinds[q * ncol + c];
      if (kd < 0 || kd > 2) return fail(VS_E_INVALID, std::string(what) + ": kind must be 0, 1 or 2");
      const float* p = params + (q * ncol + c) * 4;
      for (int i = 0; i < 4; ++i)
        if (!std::isfinite(p[i]))
          return fail(VS_E_INVALID, std::string(what) + ": a parameter that is not finite");
      if (!(p[1] > 0.0f)) return fail(VS_E_INVALID, std::string(what) + ": s must be > 0");
      if (kd == 0) continue;
      sp.kind[c] = (unsigned char)kd;
      sp.t[c] = p[0];
      sp.s[c] = p[1];
      sp.w[c] = p[2];
      sp.miss[c] = p[3];
    }
    for (int j = 0; j < kBoostMaxTags; ++j) {
      if (!tag_masks) continue;
      if (!std::isfinite(tag_bonus[q * kBoostMaxTags + j]))
        return fail(VS_E_INVALID, std::string(what) + ": a bonus that is not finite");
      sp.mask[j] = tag_masks[q * kBoostMaxTags + j];
      sp.bonus[j] = tag_bonus[q * kBoostMaxTags + j];
    }
    boost_bounds(&sp);
  }
  return VS_OK;
}

namespace {

// The windows of a boosted search: where_windows', while boost_rerank can sort
// them (kBoostMaxWindow entries); *scan = what they leave goes to the scan.
int boost_windows(int64_t k, int64_t live, int64_t* out, int nmax, bool* scan) {
  int n = where_windows(k, live, out, nmax, scan);
  n = std::min(n, nmax);
  int m = 0;
  while (m < n && out[m] <= kBoostMaxWindow) ++m;
  if (m < n) *scan = true;
  return m;
}

// Route B over batch `b`: scan_pages of vs_api_where.hip with the boost
// kernels.  Lists, floors and pages hold final keys in raw (key, label) order
// (a boosted search has no faiss tie rule), so the page loop is the raw one.
int scan_pages(vs_index* idx, const WhereAttrs& at, const SearchArgs& b, const WherePred* preds,
               const BoostSpec* specs, const int64_t* xoffs, const int64_t* xrows,
               hipStream_t st) {
  const int ntotal = (int)idx->ntotal;
  const int64_t npages = std::max<int64_t>(1, (std::min<int64_t>(b.k, ntotal) + 63) / 64);
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
  VS_HIP(scr.alloc((void**)&Dacc, (size_t)nrow * KA * sizeof(float)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&Iacc, (size_t)nrow * KA * sizeof(int64_t)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&fkey, (size_t)nrow * sizeof(float)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&fid, (size_t)nrow * sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&member, (size_t)nrow * sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&active, (size_t)nrow * sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&qlist, (size_t)nrow * sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&qcount, sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&wc, sizeof(int)), "vs_search_boost: scratch");
  Partials part;
  part.KP = 64;
  int nsplit = 1, cap = 0;
  if (gemv) {
    part.P = stream_blocks(ntotal);
    VS_HIP(scr.alloc((void**)&part.key, (size_t)kGemvMaxQ * part.P * 64 * sizeof(float)),
           "vs_search_boost: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)kGemvMaxQ * part.P * 64 * sizeof(int)),
           "vs_search_boost: scratch");
  } else {
    const int ntiles = (ntotal + kBN - 1) / kBN;
    nsplit = gathered_nsplit(ntiles);
    part.P = 2 * nsplit;
    cap = slot_window_cap(nrow, part.P, 64);
    VS_HIP(scr.alloc((void**)&part.key, (size_t)cap * part.P * 64 * sizeof(float)),
           "vs_search_boost: scratch");
    VS_HIP(scr.alloc((void**)&part.id, (size_t)cap * part.P * 64 * sizeof(int)),
           "vs_search_boost: scratch");
  }
  for (int64_t q0 = 0; q0 < b.nq; q0 += W) {
    const int nw = (int)std::min<int64_t>(W, b.nq - q0);
    const int nslot = (int)round_up(nw, kBQ);
    const int64_t eoff = q0 * idx->ld;
    const float* qf = b.qbuf + eoff;
    const void* qmat = b.qb16 ? (const void*)((const uint16_t*)b.qb16 + eoff) : (const void*)qf;
    const float* qaux = b.qaux ? b.qaux + q0 : nullptr;
    VS_HIP(hipMemsetAsync(Iacc, 0xFF, (size_t)nw * KA * sizeof(int64_t), st),
           "vs_search_boost: pages");
    VS_HIP(launch_page_init(nw, gemv ? kGemvMaxQ : nw, nullptr, nullptr, member, active, fkey, fid,
                            st),
           "vs_search_boost: pages");
    VS_HIP(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st),
           "vs_search_boost: pages");
    for (int64_t p = 0; p < npages; ++p) {
      if (p > 0) {
        VS_HIP(launch_page_step(Dacc, Iacc, KA, (int)p - 1, nw, b.k, 0, pmode, active, fkey, fid,
                                st),
               "vs_search_boost: pages");
        VS_HIP(launch_compact_flags(active, nw, qlist, qcount, nullptr, nullptr, st),
               "vs_search_boost: pages");
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
        KernelTimer tm(st, p == 0 ? "gemv_topk_boost" : nullptr);
        VS_HIP(launch_gemv_topk_boost(pmode, nw, g, specs + q0, part, st),
               "vs_search_boost: gemv_topk_boost launch");
        tm.stop();
        VS_HIP(launch_page_gate(qcount, nw, wc, st), "vs_search_boost: pages");
        VS_HIP(launch_merge_partials(pmode, part, nw, 64, 0, -INFINITY, Dacc + p * 64,
                                     Iacc + p * 64, KA, st, 1, nullptr, wc),
               "vs_search_boost: merge launch");
        continue;
      }
      for (int w0 = 0; w0 < nslot; w0 += cap) {
        VS_HIP(launch_window_count(qcount, w0, cap, wc, st), "vs_search_boost: window");
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
        KernelTimer tm(st, p == 0 && w0 == 0 ? "gemm_topk_boost" : nullptr);
        VS_HIP(launch_gemm_topk_boost(b.mode, g, specs + q0, part, st),
               "vs_search_boost: gemm_topk_boost launch");
        tm.stop();
        VS_HIP(launch_merge_partials(b.mode, part, cap, 64, 0, -INFINITY, Dacc + p * 64,
                                     Iacc + p * 64, KA, st, 1, qlist + w0, wc),
               "vs_search_boost: merge launch");
      }
    }
    VS_HIP(launch_page_finish(pmode, Dacc, Iacc, KA, nw, b.k, 0, member, idx->id_base,
                              b.min_score, b.D + q0 * b.k, b.I + q0 * b.k, st),
           "vs_search_boost: pages");
  }
  return VS_OK;
}

// Route B for the chunk's queries `sl` (ascending).
int run_scan(vs_index* idx, const BoostCall& c, const SearchArgs& a, int64_t c0,
             const std::vector<int>& sl, hipStream_t st) {
  const int cnt = (int)sl.size();
  const bool whole = cnt == a.nq;
  Scratch scr(st);
  SearchArgs b = a;
  int* dl = nullptr;
  if (!whole) {
    int rc = upload(scr, sl.data(), sl.size() * sizeof(int), (void**)&dl, st, kWhat);
    if (!rc) rc = gather_batch(idx, a, dl, cnt, scr, &b, st, kWhat);
    if (rc) return rc;
  }
  const size_t npad = (size_t)round_up(cnt, kGemvMaxQ) + kGemvMaxQ;
  std::vector<WherePred> sp(npad);
  std::vector<BoostSpec> ss(npad);
  memset(sp.data(), 0, sp.size() * sizeof(WherePred));
  memset(ss.data(), 0, ss.size() * sizeof(BoostSpec));
  for (int s = 0; s < cnt; ++s) {
    sp[(size_t)s] = c.hp[(size_t)(c0 + sl[(size_t)s])];
    ss[(size_t)s] = c.hs[(size_t)(c0 + sl[(size_t)s])];
  }
  WherePred* dsp = nullptr;
  BoostSpec* dss = nullptr;
  int rc = upload(scr, sp.data(), sp.size() * sizeof(WherePred), (void**)&dsp, st, kWhat);
  if (!rc) rc = upload(scr, ss.data(), ss.size() * sizeof(BoostSpec), (void**)&dss, st, kWhat);
  if (rc) return rc;
  std::vector<int64_t> soffs, srows;
  int64_t* dxo = nullptr;
  int64_t* dxr = nullptr;
  if (c.excl()) {
    slot_excl(c.xoffs, c.xrows, c0, sl, &soffs, &srows);
    rc = upload(scr, soffs.data(), soffs.size() * sizeof(int64_t), (void**)&dxo, st, kWhat);
    if (!rc) rc = upload(scr, srows.data(), srows.size() * sizeof(int64_t), (void**)&dxr, st, kWhat);
    if (rc) return rc;
  }
  if (!whole) {
    VS_HIP(scr.alloc((void**)&b.D, (size_t)cnt * a.k * sizeof(float)), "vs_search_boost: scratch");
    VS_HIP(scr.alloc((void**)&b.I, (size_t)cnt * a.k * sizeof(int64_t)),
           "vs_search_boost: scratch");
  }
  rc = scan_pages(idx, c.attrs->by_row(), b, dsp, dss, dxo, dxr, st);
  if (rc) return rc;
  if (!whole)
    VS_HIP(launch_distinct_scatter(b.D, b.I, cnt, a.k, dl, a.D, a.I, st),
           "vs_search_boost: scatter launch");
  VS_HIP(hipStreamSynchronize(st), "vs_search_boost: synchronise");  // (the uploads' sources)
  g_scanned += cnt;
  return VS_OK;
}

// One chunk of a boosted search.  Route A, in rounds as run_where
// (vs_api_where.hip): round r searches the queries still unsettled in raw
// order for a window of boost_windows' r-th length, boost_rerank drops the
// entries that fail the slot's predicate, ranks the rest by final key and
// decides whether the window was sufficient, and the rows of those queries are
// written.  What the last window leaves unsettled, what the give-up rule sent
// away, and what the call sent there at once is answered by route B.
int run_boost_chunk(vs_index* idx, const BoostCall& c, const SearchArgs& a, int64_t c0,
                    hipStream_t st) {
  const int64_t live = idx->live();
  const WhereAttrs at = c.attrs->by_row();
  const WherePred* dp = c.dp + c0;
  const BoostSpec* ds = c.ds + c0;
  g_searches += a.nq;
  int64_t wins[64];
  bool scan_tail = false;
  int nwin = boost_windows(a.k, live, wins, 64, &scan_tail);
  if (c.scan_only) nwin = 0;
  const float giveup = scan_tail ? boost_giveup() : -1.0f;
  Scratch scr(st);
  std::vector<int> cur, sl;  // the queries of the next window round / of the scan
  for (int q = 0; q < a.nq; ++q) (nwin == 0 ? sl : cur).push_back(q);

  int* state = nullptr;
  int* list = nullptr;
  int* dcount = nullptr;
  VS_HIP(scr.alloc((void**)&state, (size_t)a.nq * sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&list, (size_t)a.nq * sizeof(int)), "vs_search_boost: scratch");
  VS_HIP(scr.alloc((void**)&dcount, sizeof(int)), "vs_search_boost: scratch");
  std::vector<int64_t> soffs, srows;
  std::vector<int> hstate((size_t)a.nq);
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
      int rc = upload(rs, cur.data(), cur.size() * sizeof(int), (void**)&qmap, st, kWhat);
      if (!rc) rc = gather_batch(idx, a, qmap, cnt, rs, &b, st, kWhat);
      if (rc) return rc;
      uploads = true;
      if (c.excl()) {
        slot_excl(c.xoffs, c.xrows, c0, cur, &soffs, &srows);
        int64_t* d1 = nullptr;
        int64_t* d2 = nullptr;
        rc = upload(rs, soffs.data(), soffs.size() * sizeof(int64_t), (void**)&d1, st, kWhat);
        if (!rc)
          rc = upload(rs, srows.data(), srows.size() * sizeof(int64_t), (void**)&d2, st, kWhat);
        if (rc) return rc;
        hoffs = soffs.data();
        doffs = d1;
        drows = d2;
      }
    }
    b.raw = 1;
    b.k = (int)w;
    VS_HIP(rs.alloc((void**)&b.D, (size_t)cnt * w * sizeof(float)), "vs_search_boost: scratch");
    VS_HIP(rs.alloc((void**)&b.I, (size_t)cnt * w * sizeof(int64_t)), "vs_search_boost: scratch");
    {
      // extra spans for tools/bench_boost.py (they name no search kernel):
      // "boost_topk" the engine's part of a round, "boost_rerank" the rest
      KernelTimer tt(st, "boost_topk", false);
      const int rc = hoffs ? run_excluded_chunk(idx, b, hoffs, doffs, drows, st)
                           : run_topk(idx, b, st, VS_ENGINE_AUTO);
      tt.stop();
      if (rc) return rc;
    }
    KernelTimer td(st, "boost_rerank", false);
    float* Dr = a.D;  // the round's results, by slot
    int64_t* Ir = a.I;
    if (!whole) {
      VS_HIP(rs.alloc((void**)&Dr, (size_t)cnt * a.k * sizeof(float)), "vs_search_boost: scratch");
      VS_HIP(rs.alloc((void**)&Ir, (size_t)cnt * a.k * sizeof(int64_t)),
             "vs_search_boost: scratch");
    }
    VS_HIP(hipMemsetAsync(state, 0, (size_t)a.nq * sizeof(int), st), "vs_search_boost: flags");
    VS_HIP(launch_boost_rerank(a.mode, b.D, b.I, cnt, (int)w, at, dp, ds, qmap, idx->id_base, a.k,
                               all, giveup, Dr, Ir, state, nullptr, nullptr, st),
           "vs_search_boost: rerank launch");
    if (!whole)
      VS_HIP(launch_distinct_scatter(Dr, Ir, cnt, a.k, qmap, a.D, a.I, st),
             "vs_search_boost: scatter launch");
    if (all) {  // every allowed row was in the window
      td.stop();
      cur.clear();
      break;
    }
    VS_HIP(launch_compact_flags(state, a.nq, list, dcount, nullptr, nullptr, st),
           "vs_search_boost: flags");
    td.stop();
    int left = 0;
    VS_HIP(hipMemcpyAsync(&left, dcount, sizeof(int), hipMemcpyDeviceToHost, st),
           "vs_search_boost: count");
    VS_HIP(hipStreamSynchronize(st), "vs_search_boost: synchronise");
    uploads = false;
    if (round == 0) g_requeried += left;
    cur.clear();
    if (left > 0) {  // who is left, and who of them gave up
      VS_HIP(hipMemcpyAsync(hstate.data(), state, (size_t)a.nq * sizeof(int),
                            hipMemcpyDeviceToHost, st),
             "vs_search_boost: list");
      VS_HIP(hipStreamSynchronize(st), "vs_search_boost: synchronise");
      for (int q = 0; q < a.nq; ++q) {
        if (hstate[(size_t)q] == 1) cur.push_back(q);
        else if (hstate[(size_t)q] == 2) sl.push_back(q);
      }
    }
  }
  if (uploads) VS_HIP(hipStreamSynchronize(st), "vs_search_boost: synchronise");
  if (!cur.empty()) sl.insert(sl.end(), cur.begin(), cur.end());  // past the last window
  if (sl.empty()) return VS_OK;
  std::sort(sl.begin(), sl.end());
  return run_scan(idx, c, a, c0, sl, st);
}

}  // namespace

int vs::host::run_boost(vs_index* idx, const BoostCall& c, const SearchArgs& a, int64_t c0,
                        hipStream_t st) {
  return run_boost_chunk(idx, c, a, c0, st);
}

extern "C" {

int vs_search_boost(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const int32_t* kinds, const float* params, const uint64_t* tag_masks,
                    const float* tag_bonus, const float* lo, const float* hi,
                    const uint64_t* masks, const int64_t* excl_offs, const int64_t* excl_labels,
                    float* D, int64_t* I, int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_search_boost: null index");
  if (!attrs) return fail(VS_E_INVALID, "vs_search_boost: null attributes");
  int rc = check_search_args(kWhat, idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  if (n == 0) return VS_OK;
  BoostCall c;
  rc = build_specs(kWhat, attrs->ncol, kinds, params, tag_masks, tag_bonus, n, &c.hs);
  if (rc) return rc;
  rc = check_bounds(kWhat, lo, hi, n, attrs->ncol);
  if (rc) return rc;
  rc = check_excl_lists(kWhat, excl_offs, excl_labels, n);
  if (rc) return rc;
  if (!x || !D || !I) return fail(VS_E_INVALID, "vs_search_boost: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  rc = check_attrs(kWhat, idx, attrs);
  if (rc) return rc;
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_boost: hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIP(hipStreamIsCapturing(st, &cs), "vs_search_boost: stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                "vs_search_boost: a capturing stream (the call reads a count on the host after "
                "every round)");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  c.attrs = attrs;
  c.scan_only = (flags & VS_BOOST_SCAN) != 0;
  const bool empty = idx->ntotal == 0 || idx->live() == 0;
  if (!empty) {
    build_preds(lo, hi, masks, n, attrs->ncol, &c.hp);
    rc = upload(scr, c.hp.data(), c.hp.size() * sizeof(WherePred), (void**)&c.dp, st, kWhat);
    if (!rc) rc = upload(scr, c.hs.data(), c.hs.size() * sizeof(BoostSpec), (void**)&c.ds, st, kWhat);
    if (rc) return rc;
    if (excl_offs && excl_offs[n] > 0)
      excl_rows_build(idx, n, excl_offs, excl_labels, &c.xoffs, &c.xrows);
    if (c.excl()) {
      rc = upload(scr, c.xoffs.data(), c.xoffs.size() * sizeof(int64_t), (void**)&c.dxoffs, st,
                  kWhat);
      if (!rc)
        rc = upload(scr, c.xrows.data(), c.xrows.size() * sizeof(int64_t), (void**)&c.dxrows, st,
                    kWhat);
      if (rc) return rc;
    }
  }
  // the order is the raw one for both metrics: no faiss tie rule to mirror
  return search_staged(kWhat, idx, x, n, k, D, I, (flags & ~VS_BOOST_SCAN) | VS_RAW_ORDER, scr, st,
                       empty, [&](const SearchArgs& sa, int64_t c0) {
                         return run_boost(idx, c, sa, c0, st);
                       });
}

int vs_boost_eval(int ncol, const float* cols, const uint64_t* tags, int64_t nrows,
                  const int32_t* kinds, const float* params, const uint64_t* tag_masks,
                  const float* tag_bonus, int64_t nq, float* b, float* bounds) {
  if (nrows < 0 || nq < 0) return fail(VS_E_INVALID, "vs_boost_eval: a negative count");
  if (nrows > 0 && ncol > 0 && !cols) return fail(VS_E_INVALID, "vs_boost_eval: null columns");
  std::vector<BoostSpec> hs;
  const int rc = build_specs("vs_boost_eval", ncol, kinds, params, tag_masks, tag_bonus, nq, &hs);
  if (rc) return rc;
  if (nq > 0 && ((nrows > 0 && !b) || !bounds))
    return fail(VS_E_INVALID, "vs_boost_eval: null output");
  for (int64_t q = 0; q < nq; ++q) {
    const BoostSpec& sp = hs[(size_t)q];
    bounds[2 * q] = sp.L;
    bounds[2 * q + 1] = sp.U;
    for (int64_t r = 0; r < nrows; ++r) {
      float v[kWhereMaxCols];
      for (int c = 0; c < kWhereMaxCols; ++c) v[c] = c < ncol ? cols[(int64_t)c * nrows + r] : 0.0f;
      b[q * nrows + r] = boost_value(sp, v, tags ? tags[r] : 0ull);
    }
  }
  return VS_OK;
}

int vs_boost_stats(int64_t* searches, int64_t* rounds, int64_t* requeried, int64_t* scanned,
                   int reset) {
  if (!searches || !rounds || !requeried || !scanned)
    return fail(VS_E_INVALID, "vs_boost_stats: null output");
  *searches = g_searches.load();
  *rounds = g_rounds.load();
  *requeried = g_requeried.load();
  *scanned = g_scanned.load();
  if (reset) g_searches = 0, g_rounds = 0, g_requeried = 0, g_scanned = 0;
  return VS_OK;
}

}  // extern "C"
