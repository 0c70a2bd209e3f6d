// vs_api_boost.hip — boosted searches (DESIGN.md "Boosted searches"):
// vs_search_boost, vs_boost_eval, vs_boost_stats, and what a boosted call adds
// to the route driver of vs_api_where.hip (run_where): its specs, its window
// schedule and its give-up value.
#include <atomic>
#include <memory>

#include "vs_boost_value.h"
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

RouteStats vs::host::g_boost_stats;

float vs::host::boost_giveup() {
  const char* e = getenv("VS_BOOST_GIVEUP");
  return (float)(e ? atof(e) : kBoostGiveUp);
}

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

int vs::host::boost_windows(int64_t k, int64_t live, int64_t* out, int nmax, bool* scan) {
  int n = where_windows(k, live, out, nmax, scan);
  n = std::min(n, nmax);
  int m = 0;
  while (m < n && out[m] <= kBoostMaxWindow) ++m;
  if (m < n) *scan = true;
  return m;
}

extern "C" {

int vs_search_boost(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const int32_t* kinds, const float* params, const uint64_t* tag_masks,
                    const float* tag_bonus, const float* lo, const float* hi,
                    const uint64_t* masks, const int64_t* excl_offs, const int64_t* excl_labels,
                    float* D, int64_t* I, int flags, void* stream) {
  const char* const what = "vs_search_boost";
  if (!idx) return fail(VS_E_INVALID, "vs_search_boost: null index");
  if (!attrs) return fail(VS_E_INVALID, "vs_search_boost: null attributes");
  int rc = check_search_args(what, idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  if (n == 0) return VS_OK;
  WhereCall c;
  rc = build_specs(what, attrs->ncol, kinds, params, tag_masks, tag_bonus, n, &c.hs);
  if (rc) return rc;
  c.attrs = attrs;
  c.scan_only = (flags & VS_BOOST_SCAN) != 0;
  c.stats = &g_boost_stats;
  // the order is the raw one for both metrics: no faiss tie rule to mirror
  return search_where_call(what, idx, &c, x, n, k, lo, hi, masks, excl_offs, excl_labels, D, I,
                           (flags & ~VS_BOOST_SCAN) | VS_RAW_ORDER, (hipStream_t)stream);
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
  *searches = g_boost_stats.searches.load();
  *rounds = g_boost_stats.rounds.load();
  *requeried = g_boost_stats.requeried.load();
  *scanned = g_boost_stats.scanned.load();
  if (reset) g_boost_stats.reset();
  return VS_OK;
}

}  // extern "C"
