// vs_api_examples.hip — example searches (DESIGN.md "Example searches"):
// vs_search_examples, vs_search_examples_x, vs_examples_stats and the
// per-chunk rounds behind them.
#include <atomic>
#include <memory>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// Process-wide counters (vs_examples_stats): users searched, rounds run (summed
// over chunks), users searched again after their first window.
std::atomic<int64_t> g_users{0}, g_rounds{0}, g_requeried{0};

// Device scratch of one batch of users: per window entry 12 B of windows, at
// most 4 table slots of 12 B and 12 B of candidates.  A round's users run in
// sub-batches under this budget; a single user over it cannot be answered.
constexpr size_t kExamplesScratchBudget = (size_t)1 << 30;
constexpr size_t kExamplesEntryBytes = 12 + 4 * 12 + 12;

// One call's users: CSRs over the users (host), the example matrix E on the
// device (fp32, stride d: every positive in CSR order, then every negative).
struct ExamplesCall {
  const char* what = nullptr;
  int64_t n = 0;
  int k = 0;
  const int64_t* pos_offs = nullptr;
  const int64_t* neg_offs = nullptr;  // null: no negatives
  std::vector<int64_t> xoffs, xrows;  // exclusion sets, rows in place (empty: none)
  bool excl() const { return !xrows.empty(); }
  float* D = nullptr;  // device outputs of the whole call
  int64_t* I = nullptr;
  int* E = nullptr;
  bool host_wait = false;
  int64_t npos(int64_t u) const { return pos_offs[u + 1] - pos_offs[u]; }
  int64_t nneg(int64_t u) const { return neg_offs ? neg_offs[u + 1] - neg_offs[u] : 0; }
};

// Host arrays of a round kept until the round's copies have been waited for.
struct Keep {
  std::vector<std::unique_ptr<std::vector<char>>> v;
  template <class T>
  const T* hold(const std::vector<T>& src) {
    v.emplace_back(new std::vector<char>((const char*)src.data(),
                                         (const char*)src.data() + src.size() * sizeof(T)));
    return (const T*)v.back()->data();
  }
};

template <class T>
int upload(const char* what, Scratch& scr, Keep& keep, const std::vector<T>& h, T** d,
           hipStream_t st) {
  VS_HIPW(scr.alloc((void**)d, std::max<size_t>(h.size(), 1) * sizeof(T)), what, ": scratch");
  if (!h.empty())
    VS_HIPW(hipMemcpyAsync(*d, keep.hold(h), h.size() * sizeof(T), hipMemcpyHostToDevice, st), what,
            ": upload");
  return VS_OK;
}

// One batch of a round: the users us[0 .. cnt) (indices into the chunk, whose
// first user is u0 and whose staged positives / negatives are sp / sn) searched
// with a window of w entries per positive and collapsed into their output rows.
int run_batch(vs_index* idx, const ExamplesCall& c, const SearchArgs& sp, const SearchArgs& sn,
              int64_t u0, const int* us, int cnt, bool whole_chunk, int64_t w, bool all,
              int* unsettled, int* err, Keep& keep, hipStream_t st) {
  const char* what = c.what;
  const int64_t p0 = c.pos_offs[u0];
  const int64_t n0 = c.neg_offs ? c.neg_offs[u0] : 0;
  Scratch scr(st);
  // the batch's positives as slots, its users' descriptors and tables
  std::vector<int> slots;
  std::vector<ExamplesUser> users((size_t)cnt);
  std::vector<int64_t> soffs, srows;
  if (c.excl()) soffs.push_back(0);
  int64_t tslots = 0, cands = 0;
  int amax = 0, tbits_max = 0;
  bool any_neg = false;
  for (int i = 0; i < cnt; ++i) {
    const int64_t u = u0 + us[i];
    ExamplesUser& U = users[(size_t)i];
    U.pos0 = (int)slots.size();
    U.a = (int)c.npos(u);
    U.neg0 = (int)((c.neg_offs ? c.neg_offs[u] : 0) - n0);
    U.b = (int)c.nneg(u);
    U.out = us[i];
    int bits = 1;
    while (((int64_t)1 << bits) < 2 * (int64_t)U.a * w) ++bits;
    if (bits > 31)
      return fail(VS_E_UNSUPPORTED, std::string(what) + ": a user's window entries exceed 2^30");
    U.tbits = bits;
    U.toff = tslots;
    U.coff = cands;
    tslots += (int64_t)1 << bits;
    cands += (int64_t)U.a * w;
    amax = std::max(amax, U.a);
    tbits_max = std::max(tbits_max, bits);
    any_neg = any_neg || U.b > 0;
    for (int j = 0; j < U.a; ++j) {
      slots.push_back((int)(c.pos_offs[u] - p0) + j);
      if (c.excl()) {  // each positive carries its user's exclusion set
        srows.insert(srows.end(), c.xrows.begin() + c.xoffs[(size_t)u],
                     c.xrows.begin() + c.xoffs[(size_t)u + 1]);
        soffs.push_back((int64_t)srows.size());
      }
    }
  }
  const int ns = (int)slots.size();
  ExamplesUser* dusers = nullptr;
  int rc = upload(what, scr, keep, users, &dusers, st);
  if (rc) return rc;

  // the positives as a batch of their own (the whole chunk: as staged)
  SearchArgs b = sp;
  if (!whole_chunk) {
    int* dslots = nullptr;
    rc = upload(what, scr, keep, slots, &dslots, st);
    if (rc) return rc;
    const size_t rowb = (size_t)idx->ld * sizeof(float);
    const int nq_pad = (int)round_up(std::max<int64_t>(ns, kGemvMaxQ), kBQ);
    float* gq = nullptr;
    float* gaux = nullptr;
    uint16_t* gq16 = nullptr;
    VS_HIPW(scr.alloc((void**)&gq, (size_t)nq_pad * rowb), what, ": scratch");
    if (sp.mode == MODE_L2)
      VS_HIPW(scr.alloc((void**)&gaux, (size_t)nq_pad * sizeof(float)), what, ": scratch");
    VS_HIPW(launch_excl_gather(sp.qbuf, (int64_t)rowb, sp.mode == MODE_L2 ? sp.qaux : nullptr,
                               dslots, ns, nq_pad, gq, gaux, st),
            what, ": gather launch");
    if (sp.qb16) {
      VS_HIPW(scr.alloc((void**)&gq16, (size_t)nq_pad * rowb / 2), what, ": scratch");
      VS_HIPW(launch_excl_gather(sp.qb16, (int64_t)rowb / 2, nullptr, dslots, ns, nq_pad, gq16,
                                 nullptr, st),
              what, ": gather launch");
      b.qb16 = gq16;
    }
    b.qbuf = gq;
    if (gaux) b.qaux = gaux;
    b.nq = ns;
    b.nq_pad = nq_pad;
  }
  b.raw = 1;
  b.k = (int)w;
  b.l2_direct = false;  // one L2 form whatever the call holds
  b.host_wait = c.host_wait;
  VS_HIPW(scr.alloc((void**)&b.D, (size_t)ns * w * sizeof(float)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&b.I, (size_t)ns * w * sizeof(int64_t)), what, ": scratch");
  {
    // extra spans for tools/bench_examples.py (they name no search kernel):
    // "examples_topk" the engine's part of a round, "examples_collapse" the rest
    KernelTimer tt(st, "examples_topk", false);
    if (c.excl()) {
      int64_t* doffs = nullptr;
      int64_t* drows = nullptr;
      rc = upload(what, scr, keep, soffs, &doffs, st);
      if (!rc) rc = upload(what, scr, keep, srows, &drows, st);
      if (!rc) rc = run_excluded_chunk(idx, b, keep.hold(soffs), doffs, drows, st);
    } else {
      rc = run_topk(idx, b, st, VS_ENGINE_AUTO);
    }
    tt.stop();
    if (rc) return rc;
  }
  KernelTimer tc(st, "examples_collapse", false);
  ExamplesCollapse cc;
  cc.mode = sp.mode;
  cc.users = dusers;
  cc.nu = cnt;
  cc.amax = amax;
  cc.tbits_max = tbits_max;
  cc.any_neg = any_neg;
  cc.Din = b.D;
  cc.Iin = b.I;
  cc.w = (int)w;
  cc.w_is_all = all;
  cc.id_base = idx->id_base;
  VS_HIPW(scr.alloc((void**)&cc.trow, (size_t)tslots * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&cc.tval, (size_t)tslots * sizeof(unsigned long long)), what,
          ": scratch");
  VS_HIPW(scr.alloc((void**)&cc.F, (size_t)cnt * sizeof(unsigned long long)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&cc.ccount, (size_t)cnt * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&cc.ckey, (size_t)cands * sizeof(unsigned long long)), what,
          ": scratch");
  VS_HIPW(scr.alloc((void**)&cc.cpos, (size_t)cands * sizeof(int)), what, ": scratch");
  VS_HIPW(hipMemsetAsync(cc.trow, 0xFF, (size_t)tslots * sizeof(int), st), what, ": table");
  VS_HIPW(hipMemsetAsync(cc.tval, 0xFF, (size_t)tslots * sizeof(unsigned long long), st), what,
          ": table");
  VS_HIPW(hipMemsetAsync(cc.ccount, 0, (size_t)cnt * sizeof(int), st), what, ": counts");
  cc.err = err;
  cc.X = idx->codes;
  cc.xesize = idx->esize;
  cc.xn = idx->norms;
  cc.Qp = b.qbuf;
  cc.qp = b.qaux;
  cc.Qn = sn.qbuf;
  cc.qn = sn.qaux;
  cc.ld = idx->ld;
  cc.k = c.k;
  cc.D = c.D + u0 * c.k;
  cc.I = c.I + u0 * c.k;
  cc.E = c.E + u0 * c.k;
  cc.unsettled = unsettled;
  VS_HIPW(launch_examples_collapse(cc, st), what, ": collapse launch");
  tc.stop();
  return VS_OK;
}

// One chunk of users [u0, u0 + nu) in rounds: round r searches the positives
// of the users still unsettled (every user in round 0) for a window of
// distinct_window(k, r, live) entries each; after a round the host reads how
// many users found their windows too short.  The last window is every live
// row, which settles every user.
int run_examples(vs_index* idx, const ExamplesCall& c, const SearchArgs& sp, const SearchArgs& sn,
                 int64_t u0, int nu, hipStream_t st) {
  const char* what = c.what;
  const int64_t live = idx->live();
  Scratch scr(st);
  int* unsettled = nullptr;
  int* list = nullptr;
  int* dstate = nullptr;  // [0] the users left, [1] the collapse's error flag
  VS_HIPW(scr.alloc((void**)&unsettled, (size_t)nu * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&list, (size_t)nu * sizeof(int)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&dstate, 2 * sizeof(int)), what, ": scratch");
  VS_HIPW(hipMemsetAsync(dstate, 0, 2 * sizeof(int), st), what, ": state");
  g_users += nu;
  std::vector<int> us((size_t)nu);
  for (int i = 0; i < nu; ++i) us[(size_t)i] = i;
  for (int round = 0;; ++round) {
    ++g_rounds;
    const int64_t w = distinct_window(c.k, round, live);
    const bool all = w >= live;
    Keep keep;
    VS_HIPW(hipMemsetAsync(unsettled, 0, (size_t)nu * sizeof(int), st), what, ": flags");
    // sub-batches of whole users under the scratch budget
    const int cnt = (int)us.size();
    for (int i0 = 0; i0 < cnt;) {
      size_t bytes = 0;
      int i1 = i0;
      while (i1 < cnt) {
        const size_t ub = (size_t)c.npos(u0 + us[(size_t)i1]) * (size_t)w * kExamplesEntryBytes;
        if (ub > kExamplesScratchBudget)
          return fail(VS_E_UNSUPPORTED,
                      std::string(what) + ": a user needs a window of " + std::to_string(w) +
                          " entries for each of its " +
                          std::to_string(c.npos(u0 + us[(size_t)i1])) +
                          " positives, more than the 1 GiB scratch budget of a batch holds");
        if (i1 > i0 && bytes + ub > kExamplesScratchBudget) break;
        bytes += ub;
        ++i1;
      }
      const int rc = run_batch(idx, c, sp, sn, u0, us.data() + i0, i1 - i0,
                               round == 0 && i0 == 0 && i1 == nu, w, all, unsettled, dstate + 1,
                               keep, st);
      if (rc) return rc;
      i0 = i1;
    }
    if (!all)
      VS_HIPW(launch_compact_flags(unsettled, nu, list, dstate, nullptr, nullptr, st), what,
              ": flags");
    int state[2] = {0, 0};
    VS_HIPW(hipMemcpyAsync(state, dstate, 2 * sizeof(int), hipMemcpyDeviceToHost, st), what,
            ": count");
    VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
    if (state[1])
      return fail(VS_E_HIP, std::string(what) + ": the merge's table overflowed (internal error)");
    const int left = all ? 0 : state[0];
    if (left <= 0) break;
    if (round == 0) g_requeried += left;
    us.resize((size_t)left);
    VS_HIPW(hipMemcpyAsync(us.data(), list, (size_t)left * sizeof(int), hipMemcpyDeviceToHost, st),
            what, ": list");
    VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
  }
  return VS_OK;
}

bool csr_ok(const int64_t* offs, int64_t n) {
  if (offs[0] != 0) return false;
  for (int64_t q = 0; q < n; ++q)
    if (offs[q + 1] < offs[q]) return false;
  return true;
}

// The checks both entry points make before the index is read, in the header's
// order; *done: a call of no users.
int check_examples(const char* what, const vs_index* idx, const int64_t* pos_offs,
                   const int64_t* neg_offs, int64_t n, int64_t k, const int64_t* excl_offs,
                   const int64_t* excl_labels, bool* done) {
  *done = false;
  const int rc = check_search_args(what, idx, &n, k);
  if (rc) return rc;
  if (k > kExamplesMaxK)
    return fail(VS_E_UNSUPPORTED,
                std::string(what) + ": k > 1024 (the emit sorts 2 x 1024 candidates at a time)");
  if (n == 0) {
    *done = true;
    return VS_OK;
  }
  if (!pos_offs) return fail(VS_E_INVALID, std::string(what) + ": null offsets");
  if (!csr_ok(pos_offs, n) || (neg_offs && !csr_ok(neg_offs, n)))
    return fail(VS_E_INVALID, std::string(what) + ": offsets must start at 0 and not decrease");
  for (int64_t u = 0; u < n; ++u)
    if (pos_offs[u + 1] == pos_offs[u])
      return fail(VS_E_INVALID, std::string(what) + ": a user without a positive example");
  for (int64_t u = 0; u < n; ++u)
    if (pos_offs[u + 1] - pos_offs[u] > kExamplesMaxList ||
        (neg_offs && neg_offs[u + 1] - neg_offs[u] > kExamplesMaxList))
      return fail(VS_E_UNSUPPORTED,
                  std::string(what) + ": more than 64 positive or 64 negative examples of one user");
  return check_excl_lists(what, excl_offs, excl_labels, n);
}

// The search over the example matrix ex (device, fp32, stride d: the call's
// positives, then its negatives).  The caller holds the reader lock, the device
// and a reader mark on st; c.xoffs / c.xrows are set.
int search_examples_held(vs_index* idx, ExamplesCall& c, const float* ex, float* D, int64_t* I,
                         int32_t* E, int flags, Scratch& scr, hipStream_t st) {
  const char* what = c.what;
  const int64_t n = c.n, k = c.k;
  HostOut out;
  int rc = out.begin(what, scr, D, I, (size_t)n * k, flags);
  if (rc) return rc;
  int* dE = E;
  if (!E || !out.out_dev)
    VS_HIPW(scr.alloc((void**)&dE, (size_t)n * k * sizeof(int)), what, ": scratch");
  auto finish = [&]() -> int {
    if (E && !out.out_dev)
      VS_HIPW(hipMemcpyAsync(E, dE, (size_t)n * k * sizeof(int), hipMemcpyDeviceToHost, st), what,
              ": copy E");
    return out.finish(what, st);
  };
  const int mode = idx->metric == VS_METRIC_L2 ? MODE_L2 : MODE_IP;
  if (idx->ntotal == 0 || idx->live() == 0) {
    VS_HIPW(launch_fill_empty(mode, out.D, out.I, n * k, st), what, ": fill");
    VS_HIPW(hipMemsetAsync(dE, 0xFF, (size_t)n * k * sizeof(int), st), what, ": fill");
    return finish();
  }
  c.D = out.D;
  c.I = out.I;
  c.E = dE;
  c.host_wait = !out.out_dev;
  // chunks of whole users: every user's examples lie in one engine chunk
  const int64_t chunk = 65536;
  const int64_t P = c.pos_offs[n];
  std::vector<int64_t> cuts{0};
  int64_t pmax = 0, nmax = 0;
  for (int64_t u = 0, cp = 0, cn = 0; u < n; ++u) {
    if (cp + c.npos(u) > chunk || cn + c.nneg(u) > chunk) {
      cuts.push_back(u);
      cp = cn = 0;
    }
    cp += c.npos(u);
    cn += c.nneg(u);
    pmax = std::max(pmax, cp);
    nmax = std::max(nmax, cn);
  }
  cuts.push_back(n);
  QueryStage qp, qn;
  rc = stage_alloc(what, idx, pmax, scr, &qp);
  if (rc) return rc;
  if (nmax > 0) {
    rc = stage_alloc(what, idx, nmax, scr, &qn);
    if (rc) return rc;
  }
  for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
    const int64_t u0 = cuts[ci], u1 = cuts[ci + 1];
    const int64_t p0 = c.pos_offs[u0], p1 = c.pos_offs[u1];
    const int64_t n0 = c.neg_offs ? c.neg_offs[u0] : 0, n1 = c.neg_offs ? c.neg_offs[u1] : 0;
    SearchArgs sp, sn;
    rc = stage_chunk(what, idx, qp, ex + p0 * idx->d, p1 - p0, VS_IN_DEVICE, st, &sp);
    if (rc) return rc;
    if (n1 > n0) {
      rc = stage_chunk(what, idx, qn, ex + (P + n0) * idx->d, n1 - n0, VS_IN_DEVICE, st, &sn);
      if (rc) return rc;
    }
    rc = run_examples(idx, c, sp, sn, u0, (int)(u1 - u0), st);
    if (rc) return rc;
  }
  // tombstoned rows never enter a list; the rows found become faiss labels
  if (!idx->dead.empty())
    VS_HIPW(launch_label_map(out.I, n * k, idx->ddead, (int64_t)idx->dead.size(), idx->id_base, st),
            what, ": labels");
  return finish();
}

int not_capturing(const char* what, hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIPW(hipStreamIsCapturing(st, &cs), what, ": stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED, std::string(what) + ": a capturing stream (the call reads a "
                                                      "count on the host after every round)");
  return VS_OK;
}

}  // namespace

extern "C" {

int vs_search_examples(vs_index* idx, const int64_t* pos_offs, const int64_t* pos_labels,
                       const int64_t* neg_offs, const int64_t* neg_labels, int64_t n, int64_t k,
                       const int64_t* excl_offs, const int64_t* excl_labels, int exclude_examples,
                       float* D, int64_t* I, int32_t* E, int flags, void* stream) {
  const char* what = "vs_search_examples";
  bool done = false;
  int rc = check_examples(what, idx, pos_offs, neg_offs, n, k, excl_offs, excl_labels, &done);
  if (rc || done) return rc;
  if (!pos_labels || (neg_offs && neg_offs[n] > 0 && !neg_labels) || !D || !I)
    return fail(VS_E_INVALID, "vs_search_examples: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_examples: hipSetDevice failed");
  rc = not_capturing(what, st);
  if (rc) return rc;
  // the examples' rows in place: every positive, then every negative
  const int64_t live = idx->live();
  const int64_t P = pos_offs[n], N = neg_offs ? neg_offs[n] : 0;
  std::vector<int64_t> rows((size_t)(P + N));
  for (int64_t e = 0; e < P + N; ++e) {
    const int64_t l = (e < P ? pos_labels[e] : neg_labels[e - P]) - idx->id_base;
    if (l < 0 || l >= live)
      return fail(VS_E_INVALID, "vs_search_examples: an example is not a live label");
    rows[(size_t)e] = row_of_label(idx, l);
  }
  ExamplesCall c;
  c.what = what;
  c.n = n;
  c.k = (int)k;
  c.pos_offs = pos_offs;
  c.neg_offs = N > 0 ? neg_offs : nullptr;
  {
    // the exclusion lists, with the users' own examples where asked for
    std::vector<int64_t> lo((size_t)n + 1, 0), ll;
    for (int64_t u = 0; u < n; ++u) {
      if (excl_offs)
        ll.insert(ll.end(), excl_labels + excl_offs[u], excl_labels + excl_offs[u + 1]);
      if (exclude_examples) {
        ll.insert(ll.end(), pos_labels + pos_offs[u], pos_labels + pos_offs[u + 1]);
        if (N > 0) ll.insert(ll.end(), neg_labels + neg_offs[u], neg_labels + neg_offs[u + 1]);
      }
      lo[(size_t)u + 1] = (int64_t)ll.size();
    }
    if (!ll.empty()) excl_rows_build(idx, n, lo.data(), ll.data(), &c.xoffs, &c.xrows);
  }
  ReaderMark mark(idx, st);
  Scratch scr(st);
  int64_t* drows = nullptr;
  float* ex = nullptr;
  VS_HIP(scr.alloc((void**)&drows, rows.size() * sizeof(int64_t)), "vs_search_examples: scratch");
  VS_HIP(scr.alloc((void**)&ex, rows.size() * (size_t)idx->d * sizeof(float)),
         "vs_search_examples: scratch");
  VS_HIP(hipMemcpyAsync(drows, rows.data(), rows.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                        st),
         "vs_search_examples: rows");
  VS_HIP(launch_examples_gather(idx->codes, idx->esize, idx->ld, idx->d, drows, P + N, ex, st),
         "vs_search_examples: gather launch");
  // (`rows` outlives its copy: the first round's count read waits for the stream)
  return search_examples_held(idx, c, ex, D, I, E, flags, scr, st);
}

int vs_search_examples_x(vs_index* idx, const int64_t* pos_offs, const float* pos_x,
                         const int64_t* neg_offs, const float* neg_x, int64_t n, int64_t k,
                         const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                         int32_t* E, int flags, void* stream) {
  const char* what = "vs_search_examples_x";
  bool done = false;
  int rc = check_examples(what, idx, pos_offs, neg_offs, n, k, excl_offs, excl_labels, &done);
  if (rc || done) return rc;
  if (!pos_x || (neg_offs && neg_offs[n] > 0 && !neg_x) || !D || !I)
    return fail(VS_E_INVALID, "vs_search_examples_x: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_examples_x: hipSetDevice failed");
  rc = not_capturing(what, st);
  if (rc) return rc;
  const int64_t P = pos_offs[n], N = neg_offs ? neg_offs[n] : 0;
  ExamplesCall c;
  c.what = what;
  c.n = n;
  c.k = (int)k;
  c.pos_offs = pos_offs;
  c.neg_offs = N > 0 ? neg_offs : nullptr;
  const bool empty = idx->ntotal == 0 || idx->live() == 0;
  if (!empty && excl_offs && excl_offs[n] > 0)
    excl_rows_build(idx, n, excl_offs, excl_labels, &c.xoffs, &c.xrows);
  ReaderMark mark(idx, st);
  Scratch scr(st);
  float* ex = nullptr;
  const size_t rowb = (size_t)idx->d * sizeof(float);
  VS_HIP(scr.alloc((void**)&ex, (size_t)(P + N) * rowb), "vs_search_examples_x: scratch");
  const hipMemcpyKind kind =
      (flags & VS_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  VS_HIP(hipMemcpyAsync(ex, pos_x, (size_t)P * rowb, kind, st), "vs_search_examples_x: examples");
  if (N > 0)
    VS_HIP(hipMemcpyAsync(ex + P * idx->d, neg_x, (size_t)N * rowb, kind, st),
           "vs_search_examples_x: examples");
  return search_examples_held(idx, c, ex, D, I, E, flags, scr, st);
}

int vs_examples_stats(int64_t* users, int64_t* rounds, int64_t* requeried, int reset) {
  if (!users || !rounds || !requeried)
    return fail(VS_E_INVALID, "vs_examples_stats: null output");
  *users = g_users.load();
  *rounds = g_rounds.load();
  *requeried = g_requeried.load();
  if (reset) g_users = 0, g_rounds = 0, g_requeried = 0;
  return VS_OK;
}

}  // extern "C"
