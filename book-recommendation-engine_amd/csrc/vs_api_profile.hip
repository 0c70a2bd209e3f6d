// vs_api_profile.hip — profile searches (DESIGN.md "Profile searches"):
// vs_search_excl, vs_mean_rows, vs_search_profiles.
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// Queries are sorted into classes by the size m of their exclusion set: class 0
// holds m == 0 (no drop), class i the sets of at most kExclCaps[i - 1] rows,
// the last class everything larger.  A class runs the engine for need + c
// entries, c its own longest set (at most its cap), so a few long lists do not
// charge every query the longest one.  Neighbouring classes whose entry counts
// the staged engine serves with the same list length (x1_list_len) run as one
// class: one pass over the rows fewer, no longer lists.  The table and the
// merging are cost knobs only: any c >= m is exact (route (b) of the selector
// search).
constexpr int64_t kExclCaps[] = {16, 64, 256, 1024};
constexpr int kExclClasses = (int)(sizeof(kExclCaps) / sizeof(kExclCaps[0])) + 2;

// The exclusion sets of one call as rows in place: a CSR over the queries,
// every segment ascending and distinct.
struct ExclSets {
  std::vector<int64_t> offs;  // n + 1
  std::vector<int64_t> rows;
  int64_t* doffs = nullptr;  // device copies (the call's scratch)
  int64_t* drows = nullptr;
  bool any() const { return !rows.empty(); }
};

// offs[0] == 0 and offs non-decreasing over n + 1 entries.
bool csr_offsets_ok(const int64_t* offs, int64_t n) {
  if (offs[0] != 0) return false;
  for (int64_t q = 0; q < n; ++q)
    if (offs[q + 1] < offs[q]) return false;
  return true;
}

// Builds the sets from up to two label CSRs per query (either may be null).
// Labels that are not live labels of the index, -1 and duplicates drop out, as
// in vs_remove_ids.  The caller holds the reader lock.
void build_excl_sets(const vs_index* idx, int64_t n, const int64_t* offs_a, const int64_t* lab_a,
                     const int64_t* offs_b, const int64_t* lab_b, ExclSets* es) {
  const int64_t live = idx->live();
  es->offs.assign((size_t)n + 1, 0);
  es->rows.clear();
  std::vector<int64_t> seg;
  for (int64_t q = 0; q < n; ++q) {
    seg.clear();
    const int64_t* offs[2] = {offs_a, offs_b};
    const int64_t* lab[2] = {lab_a, lab_b};
    for (int s = 0; s < 2; ++s) {
      if (!offs[s]) continue;
      for (int64_t e = offs[s][q]; e < offs[s][q + 1]; ++e) {
        const int64_t r = lab[s][e] - idx->id_base;
        if (r >= 0 && r < live) seg.push_back(r);
      }
    }
    std::sort(seg.begin(), seg.end());
    seg.erase(std::unique(seg.begin(), seg.end()), seg.end());
    // positions among the live rows -> rows in place (both ascending: one
    // merge walk over the dead list, as vs_remove_ids)
    if (!idx->dead.empty()) {
      size_t j = 0;
      int64_t shift = 0;
      for (auto& r : seg) {
        while (j < idx->dead.size() && idx->dead[j] <= r + shift) ++j, ++shift;
        r += shift;
      }
    }
    es->rows.insert(es->rows.end(), seg.begin(), seg.end());
    es->offs[(size_t)q + 1] = (int64_t)es->rows.size();
  }
}

// One chunk of a search with exclusion sets: hoffs / doffs = the chunk's n + 1
// CSR offsets (host / device), drows = the call's rows.
int run_excluded(vs_index* idx, const SearchArgs& a, const int64_t* hoffs, const int64_t* doffs,
                 const int64_t* drows, hipStream_t st) {
  const bool tie_rule = a.mode == MODE_IP && !a.raw;
  const int64_t need = tie_rule ? 2 * (int64_t)a.k - 1 : a.k;
  const int64_t live = idx->live();
  int64_t caps[kExclClasses] = {0};
  for (int i = 1; i + 1 < kExclClasses; ++i) caps[i] = kExclCaps[i - 1];
  std::vector<int> members[kExclClasses];
  int64_t cmax[kExclClasses] = {0};  // the longest set of each class
  int64_t mmax = 0;
  for (int q = 0; q < a.nq; ++q) {
    const int64_t m = hoffs[q + 1] - hoffs[q];
    mmax = std::max(mmax, m);
    int c = 0;
    while (c + 1 < kExclClasses && m > caps[c]) ++c;
    members[c].push_back(q);
    cmax[c] = std::max(cmax[c], m);
  }
  // a chunk without exclusions is a plain search
  if (mmax == 0) return run_topk(idx, a, st, VS_ENGINE_AUTO);
  if (std::min(need + mmax, live) > INT_MAX / 2)
    return fail(VS_E_INVALID, "vs_search_excl: k plus the longest exclusion list is too large");
  // merge downwards: class c takes in the next class below it (not class 0,
  // which needs no drop) while both ask for the same staged list length
  for (int c = kExclClasses - 1; c > 1; --c) {
    if (members[c].empty()) continue;
    const int kf = x1_list_len((int)std::min<int64_t>(need + cmax[c], INT_MAX));
    for (int p = c - 1; p >= 1 && kf > 0; --p) {
      if (members[p].empty()) continue;
      if (x1_list_len((int)std::min<int64_t>(need + cmax[p], INT_MAX)) != kf) break;
      members[c].insert(members[c].end(), members[p].begin(), members[p].end());
      members[p].clear();
      std::sort(members[c].begin(), members[c].end());
    }
  }

  Scratch scr(st);
  // every class's slots -> queries, one upload
  std::vector<int> hmap;
  hmap.reserve((size_t)a.nq);
  for (auto& v : members) hmap.insert(hmap.end(), v.begin(), v.end());
  int* dmap = nullptr;
  VS_HIP(scr.alloc((void**)&dmap, hmap.size() * sizeof(int)), "vs_search_excl: scratch");
  VS_HIP(hipMemcpyAsync(dmap, hmap.data(), hmap.size() * sizeof(int), hipMemcpyHostToDevice, st),
         "vs_search_excl: query map");

  // inner product under faiss's rule: every class leaves its `kin` best allowed
  // entries (raw order) in the query's row of D3 / I3 and one merge applies the
  // rule, as run_selected does; otherwise the drop writes the results themselves
  const int kin = (int)std::min<int64_t>(need, live);
  float* D3 = a.D;
  int64_t* I3 = a.I;
  const int kout = tie_rule ? kin : a.k;
  if (tie_rule) {
    VS_HIP(scr.alloc((void**)&D3, (size_t)a.nq * kin * sizeof(float)), "vs_search_excl: scratch");
    VS_HIP(scr.alloc((void**)&I3, (size_t)a.nq * kin * sizeof(int64_t)),
           "vs_search_excl: scratch");
  }
  const size_t rowb = (size_t)idx->ld * sizeof(float);
  int slot0 = 0;
  for (int c = 0; c < kExclClasses; ++c) {
    const int cnt = (int)members[c].size();
    if (cnt == 0) continue;
    const int* qmap = dmap + slot0;
    slot0 += cnt;
    SearchArgs b = a;
    if (cnt < a.nq) {  // (a class that holds the whole chunk is the chunk itself, in order)
      const int nq_pad = (int)round_up(std::max<int64_t>(cnt, kGemvMaxQ), kBQ);
      float* gq = nullptr;
      float* gaux = nullptr;
      uint16_t* gq16 = nullptr;
      VS_HIP(scr.alloc((void**)&gq, (size_t)nq_pad * rowb), "vs_search_excl: scratch");
      if (a.mode == MODE_L2)
        VS_HIP(scr.alloc((void**)&gaux, (size_t)nq_pad * sizeof(float)), "vs_search_excl: scratch");
      VS_HIP(launch_excl_gather(a.qbuf, (int64_t)rowb, a.mode == MODE_L2 ? a.qaux : nullptr, qmap,
                                cnt, nq_pad, gq, gaux, st),
             "vs_search_excl: gather launch");
      if (a.qb16) {
        VS_HIP(scr.alloc((void**)&gq16, (size_t)nq_pad * rowb / 2), "vs_search_excl: scratch");
        VS_HIP(launch_excl_gather(a.qb16, (int64_t)rowb / 2, nullptr, qmap, cnt, nq_pad, gq16,
                                  nullptr, st),
               "vs_search_excl: gather launch");
        b.qb16 = gq16;
      }
      b.qbuf = gq;
      if (gaux) b.qaux = gaux;
      b.nq = cnt;
      b.nq_pad = nq_pad;
    } else {
      qmap = nullptr;
    }
    const int64_t k2 = c == 0 ? kout : std::min<int64_t>(need + cmax[c], live);
    if (tie_rule || c > 0) b.raw = 1;
    b.k = (int)k2;
    VS_HIP(scr.alloc((void**)&b.D, (size_t)cnt * k2 * sizeof(float)), "vs_search_excl: scratch");
    VS_HIP(scr.alloc((void**)&b.I, (size_t)cnt * k2 * sizeof(int64_t)), "vs_search_excl: scratch");
    // extra spans for tools/bench_profiles.py (they name no search kernel):
    // "excl_topk" the engine's part of the step, "excl_drop" the drop's
    KernelTimer tt(st, "excl_topk", false);
    const int rc = run_topk(idx, b, st, VS_ENGINE_AUTO);
    tt.stop();
    if (rc) return rc;
    KernelTimer td(st, "excl_drop", false);
    VS_HIP(launch_excl_drop(a.mode, b.D, b.I, cnt, (int)k2, doffs, drows, qmap, idx->id_base, D3,
                            I3, kout, st),
           "vs_search_excl: drop launch");
    td.stop();
  }
  if (tie_rule) {
    KernelTimer td(st, "excl_drop", false);
    VS_HIP(launch_merge_parts(a.mode, D3, I3, 1, a.nq, kin, a.k, a.D, a.I, st),
           "vs_search_excl: merge launch");
    td.stop();
  }
  return VS_OK;
}

// vs_search over queries with exclusion sets (es may be null or empty: the
// plain search).  The caller holds the reader lock, the device and a reader
// mark on `st`.
int search_excl_locked(vs_index* idx, const float* x, int64_t n, int64_t k, ExclSets* es,
                       float* D, int64_t* I, int flags, hipStream_t st) {
  const bool excl = es && es->any();  // (rows in place: the index has live rows)
  Scratch scr(st);
  if (excl) {
    VS_HIP(scr.alloc((void**)&es->doffs, es->offs.size() * sizeof(int64_t)),
           "vs_search_excl: scratch");
    VS_HIP(scr.alloc((void**)&es->drows, es->rows.size() * sizeof(int64_t)),
           "vs_search_excl: scratch");
    VS_HIP(hipMemcpyAsync(es->doffs, es->offs.data(), es->offs.size() * sizeof(int64_t),
                          hipMemcpyHostToDevice, st),
           "vs_search_excl: offsets");
    VS_HIP(hipMemcpyAsync(es->drows, es->rows.data(), es->rows.size() * sizeof(int64_t),
                          hipMemcpyHostToDevice, st),
           "vs_search_excl: rows");
  }
  return search_staged("vs_search_excl", idx, x, n, k, D, I, flags, scr, st,
                       idx->ntotal == 0 || idx->live() == 0,
                       [&](const SearchArgs& sa, int64_t c0) {
                         return excl ? run_excluded(idx, sa, es->offs.data() + c0, es->doffs + c0,
                                                    es->drows, st)
                                     : run_topk(idx, sa, st, VS_ENGINE_AUTO);
                       });
}

// The means of n profiles (host CSR of labels and weights) into the device
// buffer dout ([n][d]), enqueued on st.  The caller holds the reader lock, the
// device and a reader mark; scr outlives the launch.
int mean_rows_locked(vs_index* idx, const int64_t* offs, const int64_t* labels,
                     const float* weights, int64_t n, float* dout, Scratch& scr, hipStream_t st) {
  const int64_t total = offs[n];
  const int64_t live = idx->live();
  std::vector<int64_t> rows((size_t)total);
  std::vector<float> W((size_t)n);
  for (int64_t q = 0; q < n; ++q) {
    if (offs[q + 1] == offs[q]) return fail(VS_E_INVALID, "vs_mean_rows: empty profile");
    double w = 0.0;
    for (int64_t e = offs[q]; e < offs[q + 1]; ++e) {
      const int64_t l = labels[e] - idx->id_base;
      if (l < 0 || l >= live)
        return fail(VS_E_INVALID, "vs_mean_rows: key out of range");  // faiss reconstruct throws
      rows[(size_t)e] = row_of_label(idx, l);
      w += (double)weights[e];
    }
    const float wf = (float)w;
    if (!(wf != 0.0f) || !std::isfinite(wf))
      return fail(VS_E_INVALID, "vs_mean_rows: the weights of a profile sum to zero or are not finite");
    W[(size_t)q] = wf;
  }
  int64_t* doffs = nullptr;
  int64_t* drows = nullptr;
  float* dw = nullptr;
  float* dW = nullptr;
  VS_HIP(scr.alloc((void**)&doffs, (size_t)(n + 1) * sizeof(int64_t)), "vs_mean_rows: scratch");
  VS_HIP(scr.alloc((void**)&drows, (size_t)total * sizeof(int64_t)), "vs_mean_rows: scratch");
  VS_HIP(scr.alloc((void**)&dw, (size_t)total * sizeof(float)), "vs_mean_rows: scratch");
  VS_HIP(scr.alloc((void**)&dW, (size_t)n * sizeof(float)), "vs_mean_rows: scratch");
  VS_HIP(hipMemcpyAsync(doffs, offs, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st),
         "vs_mean_rows: offsets");
  VS_HIP(hipMemcpyAsync(drows, rows.data(), (size_t)total * sizeof(int64_t), hipMemcpyHostToDevice,
                        st),
         "vs_mean_rows: rows");
  VS_HIP(hipMemcpyAsync(dw, weights, (size_t)total * sizeof(float), hipMemcpyHostToDevice, st),
         "vs_mean_rows: weights");
  VS_HIP(hipMemcpyAsync(dW, W.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, st),
         "vs_mean_rows: weight sums");
  KernelTimer tm(st, "mean_rows", false);  // an extra span, for tools/bench_profiles.py
  VS_HIP(launch_mean_rows(idx->codes, idx->esize, idx->ld, idx->d, doffs, drows, dw, dW, n, dout,
                          st),
         "vs_mean_rows: launch");
  tm.stop();
  return VS_OK;
}

// The argument checks of a profile CSR that need no device.
int check_profiles(const char* what, const int64_t* offs, const int64_t* labels,
                   const float* weights, int64_t n) {
  if (n < 0) return fail(VS_E_INVALID, std::string(what) + ": n < 0");
  if (n == 0) return VS_OK;
  if (!offs) return fail(VS_E_INVALID, std::string(what) + ": null offsets");
  if (!csr_offsets_ok(offs, n))
    return fail(VS_E_INVALID, std::string(what) + ": offsets must start at 0 and not decrease");
  for (int64_t q = 0; q < n; ++q)
    if (offs[q + 1] == offs[q]) return fail(VS_E_INVALID, std::string(what) + ": empty profile");
  if (!labels || !weights) return fail(VS_E_INVALID, std::string(what) + ": null buffer");
  return VS_OK;
}

}  // namespace

namespace vs {
namespace host {

int check_excl_lists(const char* what, const int64_t* excl_offs, const int64_t* excl_labels,
                     int64_t n) {
  if (!excl_offs) return VS_OK;
  if (!csr_offsets_ok(excl_offs, n))
    return fail(VS_E_INVALID, std::string(what) + ": offsets must start at 0 and not decrease");
  if (excl_offs[n] > 0 && !excl_labels)
    return fail(VS_E_INVALID, std::string(what) + ": null exclusion labels");
  return VS_OK;
}

int run_excluded_chunk(vs_index* idx, const SearchArgs& a, const int64_t* hoffs,
                       const int64_t* doffs, const int64_t* drows, hipStream_t st) {
  return run_excluded(idx, a, hoffs, doffs, drows, st);
}

void excl_rows_build(const vs_index* idx, int64_t n, const int64_t* excl_offs,
                     const int64_t* excl_labels, std::vector<int64_t>* offs,
                     std::vector<int64_t>* rows) {
  ExclSets es;
  build_excl_sets(idx, n, excl_offs, excl_labels, nullptr, nullptr, &es);
  offs->swap(es.offs);
  rows->swap(es.rows);
}

int search_excl_held(vs_index* idx, const float* x, int64_t n, int64_t k, const int64_t* excl_offs,
                     const int64_t* excl_labels, float* D, int64_t* I, int flags, hipStream_t st) {
  ExclSets es;
  if (excl_offs && excl_offs[n] > 0)
    build_excl_sets(idx, n, excl_offs, excl_labels, nullptr, nullptr, &es);
  return search_excl_locked(idx, x, n, k, &es, D, I, flags, st);
}

}  // namespace host
}  // namespace vs

extern "C" {

int vs_search_excl(vs_index* idx, const float* x, int64_t n, int64_t k, const int64_t* excl_offs,
                   const int64_t* excl_labels, float* D, int64_t* I, int flags, void* stream) {
  const int rc = check_search_args("vs_search_excl", idx, &n, k);  // buffers: after the offsets
  if (rc) return rc;
  const int rcl = check_excl_lists("vs_search_excl", excl_offs, excl_labels, n);
  if (rcl) return rcl;
  // no list holds a label: vs_search itself
  if (!excl_offs || excl_offs[n] == 0) return vs_search(idx, x, n, k, D, I, flags, stream);
  if (!x || !D || !I) return fail(VS_E_INVALID, "vs_search_excl: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_excl: hipSetDevice failed");
  ReaderMark mark(idx, st);
  ExclSets es;
  build_excl_sets(idx, n, excl_offs, excl_labels, nullptr, nullptr, &es);
  return search_excl_locked(idx, x, n, k, &es, D, I, flags, st);
}

int vs_mean_rows(vs_index* idx, const int64_t* offs, const int64_t* labels, const float* weights,
                 int64_t n, float* out, int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_mean_rows: null index");
  const int rc0 = check_profiles("vs_mean_rows", offs, labels, weights, n);
  if (rc0) return rc0;
  if (n == 0) return VS_OK;
  if (!out) return fail(VS_E_INVALID, "vs_mean_rows: null output");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_mean_rows: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  HostOut res;
  int rc = res.begin("vs_mean_rows", scr, out, nullptr, (size_t)n * idx->d, flags);
  if (rc) return rc;
  rc = mean_rows_locked(idx, offs, labels, weights, n, res.D, scr, st);
  if (rc) return rc;
  return res.finish("vs_mean_rows", st);
}

int vs_search_profiles(vs_index* idx, const int64_t* offs, const int64_t* labels,
                       const float* weights, int64_t n, int64_t k, const int64_t* excl_offs,
                       const int64_t* excl_labels, int exclude_profile, float* D, int64_t* I,
                       int flags, void* stream) {
  const int rck = check_search_args("vs_search_profiles", idx, nullptr, k);
  if (rck) return rck;
  const int rc0 = check_profiles("vs_search_profiles", offs, labels, weights, n);
  if (rc0) return rc0;
  if (n == 0) return VS_OK;
  const int rcl = check_excl_lists("vs_search_profiles", excl_offs, excl_labels, n);
  if (rcl) return rcl;
  if (!D || !I) return fail(VS_E_INVALID, "vs_search_profiles: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_profiles: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  float* qmean = nullptr;
  VS_HIP(scr.alloc((void**)&qmean, (size_t)n * idx->d * sizeof(float)),
         "vs_search_profiles: scratch");
  const int rc = mean_rows_locked(idx, offs, labels, weights, n, qmean, scr, st);
  if (rc) return rc;
  ExclSets es;
  build_excl_sets(idx, n, excl_offs, excl_labels, exclude_profile ? offs : nullptr, labels, &es);
  return search_excl_locked(idx, qmean, n, k, &es, D, I, flags | VS_IN_DEVICE, st);
}

}  // extern "C"
