// vs_api_range.hip — range searches ("Range search" and "Range
// self-join"): vs_range_search, vs_range_selfjoin, its row-list form
// vs_range_selfjoin_rows ("In-place updates") and the vs_range result's exports.
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

void free_range(vs_range* r) {
  if (r->lims) (void)hipFree(r->lims);
  if (r->D) (void)hipFree(r->D);
  if (r->I) (void)hipFree(r->I);
  delete r;
}

// What a range call hands to the passes it shares with the others: the
// candidate passes' operands (the rows are the index's), the thresholds, and
// the messages' prefix.
struct RangeJob {
  const char* who = nullptr;
  int mode = MODE_IP;           // the candidate passes' key (launch_gemm_range)
  const void* qmat = nullptr;   // [nq_pad][ld] query rows in the index's element type
  const float* qaux = nullptr;  // the queries' aux values (nq_pad entries)
  const float* xaux = nullptr;  // the rows' aux values
  int64_t n = 0, nq_pad = 0;
  const float* thr = nullptr;   // [nq_pad], launch_range_thr
  int64_t upper_q0 = -1;        // the self-join's triangle: the first query's row
};

// count / scan / fill, the verification (verify(cand, ncand, off, nsplit, ekey,
// flag) enqueues it), the hit counts, their scan into r->lims and the emission
// into r->D / r->I (labels row + id_base).  r->total stays 0 where nothing is
// found.  The caller synchronises after whatever it adds.
template <class Verify>
int range_passes(vs_index* idx, const RangeJob& j, Scratch& scr, hipStream_t st, vs_range* r,
                 Verify verify) {
  const char* who = j.who;
  const int ntotal = (int)idx->ntotal;
  const int64_t n = j.n, nq_pad = j.nq_pad;
  const int nsplit = gemm_nsplit((ntotal + kBN - 1) / kBN, (int)(nq_pad / kBQ));
  const int64_t nseg = nq_pad * nsplit;
  int* cnt = nullptr;
  int64_t* off = nullptr;
  int* err = nullptr;
  VS_HIPW(scr.alloc((void**)&cnt, (size_t)nseg * sizeof(int)), who, ": scratch");
  VS_HIPW(scr.alloc((void**)&off, (size_t)(nseg + 1) * sizeof(int64_t)), who, ": scratch");
  VS_HIPW(scr.alloc((void**)&err, sizeof(int)), who, ": scratch");
  VS_HIPW(hipMemsetAsync(err, 0, sizeof(int), st), who, ": flag");
  {
    KernelTimer tm(st, "gemm_range");
    VS_HIPW(launch_gemm_range(false, j.mode, idx->codes, j.xaux, j.qmat, j.qaux, idx->ld,
                              idx->esize, ntotal, (int)nq_pad, nsplit, j.thr, cnt, nullptr, nullptr,
                              nullptr, st, j.upper_q0),
            who, ": gemm_range count launch");
    tm.stop();
  }
  VS_HIPW(launch_range_scan(cnt, nseg, off, st), who, ": scan");
  int64_t ncand = 0;
  VS_HIPW(hipMemcpyAsync(&ncand, off + nseg, sizeof(int64_t), hipMemcpyDeviceToHost, st), who,
          ": candidate total");
  VS_HIPW(hipStreamSynchronize(st), who, ": synchronise");
  if (ncand >= ((int64_t)1 << 31))
    return fail(VS_E_UNSUPPORTED, std::string(who) + ": " + std::to_string(ncand) +
                                      " candidates (2^31 or more): search fewer queries per call");
  r->ncand = ncand;
  const int64_t lbytes = (n + 1) * (int64_t)sizeof(int64_t);
  if (ncand == 0) {
    VS_HIPW(hipMemsetAsync(r->lims, 0, (size_t)lbytes, st), who, ": lims");
    return VS_OK;
  }
  int* cand = nullptr;
  float* ekey = nullptr;
  uint8_t* flag = nullptr;
  int* hits = nullptr;
  VS_HIPW(scr.alloc((void**)&cand, (size_t)ncand * sizeof(int)), who, ": candidates");
  VS_HIPW(scr.alloc((void**)&ekey, (size_t)ncand * sizeof(float)), who, ": candidates");
  VS_HIPW(scr.alloc((void**)&flag, (size_t)ncand), who, ": candidates");
  VS_HIPW(scr.alloc((void**)&hits, (size_t)n * sizeof(int)), who, ": scratch");
  // a slot the fill pass left (it never does: *err) holds no row
  VS_HIPW(hipMemsetAsync(cand, 0xFF, (size_t)ncand * sizeof(int), st), who, ": candidates");
  {
    KernelTimer tm(st, "gemm_range");
    VS_HIPW(launch_gemm_range(true, j.mode, idx->codes, j.xaux, j.qmat, j.qaux, idx->ld, idx->esize,
                              ntotal, (int)nq_pad, nsplit, j.thr, nullptr, off, cand, err, st,
                              j.upper_q0),
            who, ": gemm_range fill launch");
    tm.stop();
  }
  VS_HIPW(verify(cand, ncand, off, nsplit, ekey, flag), who, ": verification");
  VS_HIPW(launch_range_hits(flag, off, nsplit, (int)n, hits, st), who, ": hit counts");
  VS_HIPW(launch_range_scan(hits, n, r->lims, st), who, ": lims");
  int64_t total = 0;
  int herr = 0;
  VS_HIPW(hipMemcpyAsync(&total, r->lims + n, sizeof(int64_t), hipMemcpyDeviceToHost, st), who,
          ": hit total");
  VS_HIPW(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, st), who, ": flag");
  VS_HIPW(hipStreamSynchronize(st), who, ": synchronise");
  if (herr) return fail(VS_E_HIP, std::string(who) + ": range fill disagrees with its count");
  if (total == 0) return VS_OK;
  hipError_t e = hipMalloc(&r->D, (size_t)total * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&r->I, (size_t)total * sizeof(int64_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? VS_E_OOM : VS_E_HIP,
                std::string(who) + ": no memory for " + std::to_string(total) +
                    " results: " + hipGetErrorString(e));
  }
  r->total = total;
  VS_HIPW(launch_range_emit(cand, ekey, flag, off, nsplit, (int)n, r->lims, idx->id_base, r->D,
                            r->I, st),
          who, ": emission");
  return VS_OK;
}

// The search behind vs_range_search, with the index's lock held and the
// queries not yet staged: fills r->lims / D / I ("Range search").
int run_range(vs_index* idx, const vs_selector* sel, const float* x, int64_t n, float radius,
              int flags, hipStream_t st, vs_range* r) {
  const int mode = idx->metric == VS_METRIC_L2 ? MODE_L2 : MODE_IP;
  // the exact key that decides a row: faiss's branch for a call of this size
  const int emode = mode == MODE_L2 && n < kBlasThreshold ? MODE_L2D : mode;
  const int ntotal = (int)idx->ntotal;
  Scratch scr(st);
  QueryStage qs;
  SearchArgs sa;
  int rc = stage_alloc("vs_range_search", idx, n, scr, &qs);
  if (!rc) rc = stage_chunk("vs_range_search", idx, qs, x, n, flags, st, &sa);
  if (rc) return rc;
  const int64_t nq_pad = sa.nq_pad;
  const float* qbuf = qs.qbuf;
  const float* qaux = qs.qaux;
  const uint16_t* qb16 = qs.qb16;

  // thr[q] = the radius key + the GEMM's bound for query q (the rows and the
  // queries themselves are multiplied: BoundArgs::rows_exact), over the largest
  // norm of the index: a plane's maxima where one keeps them, else one
  // reduction over the stored norms
  const unsigned* stats = nullptr;
  if (idx->esize == 4)
    stats = idx->bstats[FILTER_BF16] ? idx->bstats[FILTER_BF16] : idx->bstats[FILTER_I8];
  if (!stats) {
    unsigned* ns = nullptr;
    VS_HIP(scr.alloc((void**)&ns, (size_t)(range_norm_max_parts() + 4) * sizeof(unsigned)),
           "vs_range_search: scratch");
    VS_HIP(launch_range_norm_max(idx->norms, ntotal, ns + 4, ns, st), "vs_range_search: norm maximum");
    stats = ns;
  }
  BoundArgs ba = make_bound_args(idx->ld, FILTER_BF16);
  ba.rows_exact = 1;
  double* bkey = nullptr;
  float* thr = nullptr;
  VS_HIP(scr.alloc((void**)&bkey, (size_t)n * sizeof(double)), "vs_range_search: scratch");
  VS_HIP(scr.alloc((void**)&thr, (size_t)nq_pad * sizeof(float)), "vs_range_search: scratch");
  VS_HIP(launch_qbound(emode, qbuf, idx->ld, qaux, FILTER_BF16, stats, nullptr, (int)n, bkey, st,
                       &ba),
         "vs_range_search: bound");
  VS_HIP(launch_range_thr(bkey, (int)n, (int)nq_pad, mode == MODE_IP ? -radius : radius, thr, st),
         "vs_range_search: thresholds");

  RangeJob job;
  job.who = "vs_range_search";
  job.mode = mode;
  job.qmat = qb16 ? (const void*)qb16 : (const void*)qbuf;
  job.qaux = qaux;
  job.xaux = idx->norms;
  job.n = n;
  job.nq_pad = nq_pad;
  job.thr = thr;
  rc = range_passes(idx, job, scr, st, r,
                    [&](const int* cand, int64_t ncand, const int64_t* off, int nsplit,
                        float* ekey, uint8_t* flag) {
                      return launch_range_verify(emode, cand, ncand, off, nsplit, (int)n,
                                                 idx->codes, idx->esize, idx->norms, qbuf, qaux,
                                                 idx->ld, ntotal, radius,
                                                 sel ? sel->rbits : nullptr, ekey, flag, st);
                    });
  if (rc) return rc;
  // tombstoned rows never match; the rows found become faiss labels
  if (r->total > 0 && !idx->dead.empty())
    VS_HIP(launch_label_map(r->I, r->total, idx->ddead, (int64_t)idx->dead.size(), idx->id_base,
                            st),
           "vs_range_search: labels");
  VS_HIP(hipStreamSynchronize(st), "vs_range_search: synchronise");
  return VS_OK;
}

// The join behind vs_range_selfjoin / vs_range_selfjoin_rows, with the index's
// lock held and no tombstones in place: queries are rows q0 .. q0 + nq, read
// where they are stored ("Range self-join"), or, with `qrows`
// (host, nq checked positions), the rows qrows[0 .. nq) gathered into a scratch
// block of their own ("In-place updates").
int run_range_join(const char* who, vs_index* idx, int64_t q0, const int64_t* qrows, int64_t nq,
                   float min_sim, int exclude_self, int upper, hipStream_t st, vs_range* r) {
  const int ntotal = (int)idx->ntotal;
  const int64_t nq_pad = round_up(nq, kBQ);
  Scratch scr(st);
  float* rinv = nullptr;
  VS_HIPW(scr.alloc((void**)&rinv, (size_t)idx->capacity * sizeof(float)), who, ": scratch");
  VS_HIPW(launch_rsqrt(idx->norms, idx->capacity, rinv, st), who, ": rsqrt");
  // thr[q] = -min_sim + B: the cosine bound of a pass that multiplies the
  // stored values themselves (BoundArgs::rows_exact; products of two bf16
  // values are exact in the bf16 MFMA too).  It depends on ld alone, not on
  // the query or the index's norms, so it is computed once over a zero row
  // (`zero` is that row, and the all-zero index maxima before it).
  float* zero = nullptr;
  double* bkey = nullptr;
  float* thr = nullptr;
  VS_HIPW(scr.alloc((void**)&zero, (size_t)(idx->ld + 4) * sizeof(float)), who, ": scratch");
  VS_HIPW(scr.alloc((void**)&bkey, sizeof(double)), who, ": scratch");
  VS_HIPW(scr.alloc((void**)&thr, (size_t)nq_pad * sizeof(float)), who, ": scratch");
  VS_HIPW(hipMemsetAsync(zero, 0, (size_t)(idx->ld + 4) * sizeof(float), st), who, ": scratch");
  BoundArgs ba = make_bound_args(idx->ld, FILTER_BF16);
  ba.rows_exact = 1;
  VS_HIPW(launch_qbound(MODE_COS, zero + 4, idx->ld, nullptr, FILTER_BF16, (const unsigned*)zero,
                        nullptr, 1, bkey, st, &ba),
          who, ": bound");
  VS_HIPW(launch_range_thr(bkey, (int)nq, (int)nq_pad, -min_sim, thr, st, 0), who,
          ": thresholds");

  // the row list's queries: the rows and their inverse norms side by side, as
  // the window form finds them in place
  int* dqrows = nullptr;
  char* qmat = nullptr;
  float* qinv = nullptr;
  std::vector<int> hq;
  if (qrows) {
    hq.assign(qrows, qrows + nq);
    VS_HIPW(scr.alloc((void**)&dqrows, (size_t)nq * sizeof(int)), who, ": scratch");
    VS_HIPW(scr.alloc((void**)&qmat, (size_t)nq_pad * idx->rowbytes()), who, ": scratch");
    VS_HIPW(scr.alloc((void**)&qinv, (size_t)nq_pad * sizeof(float)), who, ": scratch");
    VS_HIPW(hipMemcpyAsync(dqrows, hq.data(), (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st),
            who, ": upload");
    VS_HIPW(launch_range_gather_rows(idx->codes, idx->rowbytes(), rinv, dqrows, (int)nq,
                                     (int)nq_pad, qmat, qinv, st),
            who, ": gather");
  }

  RangeJob job;
  job.who = who;
  job.mode = MODE_COS;
  // capacity keeps kBQ rows of slack (as vs_selfjoin)
  job.qmat = qrows ? (const void*)qmat : (const void*)idx->row(q0);
  job.qaux = qrows ? qinv : rinv + q0;
  job.xaux = rinv;
  job.n = nq;
  job.nq_pad = nq_pad;
  job.thr = thr;
  job.upper_q0 = upper ? q0 : -1;
  const int rc = range_passes(idx, job, scr, st, r,
                              [&](const int* cand, int64_t ncand, const int64_t* off, int nsplit,
                                  float* ekey, uint8_t* flag) {
                                return launch_range_join_verify(
                                    cand, ncand, off, nsplit, (int)nq, idx->codes, idx->esize,
                                    rinv, idx->ld, ntotal, q0, min_sim, exclude_self, upper, ekey,
                                    flag, st, dqrows);
                              });
  if (rc) return rc;
  VS_HIPW(hipStreamSynchronize(st), who, ": synchronise");
  return VS_OK;
}

// What vs_range_selfjoin and vs_range_selfjoin_rows share once their own
// arguments are checked: the pack of tombstones (as vs_selfjoin: query rows are
// read in place and labels are row numbers), the check of the query rows
// against the rows then in place, the stream, the result handle and the join.
int range_join_call(const char* who, vs_index* idx, int64_t q0, const int64_t* qrows, int64_t nq,
                    float min_sim, int exclude_self, int upper, hipStream_t st, vs_range** out) {
  const std::string w(who);
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  while (!idx->dead.empty()) {
    lk.unlock();
    {
      std::unique_lock<std::shared_mutex> wl(idx->mu);
      const int rc = pack_dead(idx);
      if (rc) return rc;
    }
    lk.lock();
  }
  if (!qrows && q0 + nq > idx->ntotal) return fail(VS_E_INVALID, w + ": query rows out of range");
  for (int64_t i = 0; qrows && i < nq; ++i)
    if (qrows[i] < 0 || qrows[i] >= idx->ntotal)
      return fail(VS_E_INVALID, w + ": row " + std::to_string(qrows[i]) + " out of range");
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, w + ": hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIPW(hipStreamIsCapturing(st, &cs), who, ": stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                w + ": a capturing stream (the call reads its totals on the host)");
  vs_range* r = new vs_range();
  r->device = idx->device;
  r->nq = nq;
  hipError_t e = hipMalloc(&r->lims, (size_t)(nq + 1) * sizeof(int64_t));
  if (e != hipSuccess) {
    delete r;
    return hip_fail(e, (w + ": lims").c_str());
  }
  int rc = VS_OK;
  if (nq == 0 || idx->ntotal == 0) {
    e = hipMemsetAsync(r->lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = hip_fail(e, (w + ": lims").c_str());
  } else {
    ReaderMark mark(idx, st);
    rc = run_range_join(who, idx, q0, qrows, nq, min_sim, exclude_self ? 1 : 0, upper ? 1 : 0, st,
                        r);
  }
  if (rc) {
    free_range(r);
    return rc;
  }
  *out = r;
  return VS_OK;
}

}  // namespace

extern "C" {

int vs_range_search(vs_index* idx, const vs_selector* sel, const float* x, int64_t n,
                    float radius, int flags, void* stream, vs_range** out) {
  if (!out) return fail(VS_E_INVALID, "vs_range_search: null output");
  *out = nullptr;
  if (!idx) return fail(VS_E_INVALID, "vs_range_search: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_range_search: n < 0");
  if (n > 65536)
    return fail(VS_E_UNSUPPORTED, "vs_range_search: more than 65536 queries in one call");
  if (n > 0 && !x) return fail(VS_E_INVALID, "vs_range_search: null buffer");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (sel && sel->idx != idx)
    return fail(VS_E_INVALID, "vs_range_search: the selector belongs to another index");
  if (sel && sel->gen != idx->gen)
    return fail(VS_E_INVALID,
                "vs_range_search: stale selector (the index changed since it was built)");
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_range_search: hipSetDevice failed");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  VS_HIP(hipStreamIsCapturing(st, &cs), "vs_range_search: stream");
  if (cs != hipStreamCaptureStatusNone)
    return fail(VS_E_UNSUPPORTED,
                "vs_range_search: a capturing stream (the call reads its totals on the host)");
  vs_range* r = new vs_range();
  r->device = idx->device;
  r->nq = n;
  hipError_t e = hipMalloc(&r->lims, (size_t)(n + 1) * sizeof(int64_t));
  if (e != hipSuccess) {
    delete r;
    return hip_fail(e, "vs_range_search: lims");
  }
  int rc = VS_OK;
  if (n == 0 || idx->ntotal == 0 || (sel && sel->count == 0)) {
    e = hipMemsetAsync(r->lims, 0, (size_t)(n + 1) * sizeof(int64_t), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = hip_fail(e, "vs_range_search: lims");
  } else {
    ReaderMark mark(idx, st);
    rc = run_range(idx, sel, x, n, radius, flags, st, r);
  }
  if (rc) {
    free_range(r);
    return rc;
  }
  *out = r;
  return VS_OK;
}

int vs_range_selfjoin(vs_index* idx, int64_t q0, int64_t nq, float min_sim, int exclude_self,
                      int upper, int flags, void* stream, vs_range** out) {
  (void)flags;
  if (!out) return fail(VS_E_INVALID, "vs_range_selfjoin: null output");
  *out = nullptr;
  if (!idx) return fail(VS_E_INVALID, "vs_range_selfjoin: null index");
  if (q0 < 0 || nq < 0) return fail(VS_E_INVALID, "vs_range_selfjoin: query rows out of range");
  if (nq > 65536)
    return fail(VS_E_UNSUPPORTED, "vs_range_selfjoin: more than 65536 query rows in one call");
  return range_join_call("vs_range_selfjoin", idx, q0, nullptr, nq, min_sim, exclude_self, upper,
                         (hipStream_t)stream, out);
}

int vs_range_selfjoin_rows(vs_index* idx, const int64_t* qrows, int64_t nq, float min_sim,
                           int exclude_self, int flags, void* stream, vs_range** out) {
  (void)flags;
  if (!out) return fail(VS_E_INVALID, "vs_range_selfjoin_rows: null output");
  *out = nullptr;
  if (!idx) return fail(VS_E_INVALID, "vs_range_selfjoin_rows: null index");
  if (nq < 0) return fail(VS_E_INVALID, "vs_range_selfjoin_rows: nq < 0");
  if (nq > 65536)
    return fail(VS_E_UNSUPPORTED,
                "vs_range_selfjoin_rows: more than 65536 query rows in one call");
  if (nq > 0 && !qrows) return fail(VS_E_INVALID, "vs_range_selfjoin_rows: null buffer");
  return range_join_call("vs_range_selfjoin_rows", idx, 0, qrows, nq, min_sim, exclude_self, 0,
                         (hipStream_t)stream, out);
}

int vs_range_size(const vs_range* r, int64_t* nq, int64_t* total) {
  if (!r || !nq || !total) return fail(VS_E_INVALID, "vs_range_size: null argument");
  *nq = r->nq;
  *total = r->total;
  return VS_OK;
}

int vs_range_candidates(const vs_range* r, int64_t* out) {
  if (!r || !out) return fail(VS_E_INVALID, "vs_range_candidates: null argument");
  *out = r->ncand;
  return VS_OK;
}

int vs_range_copy(const vs_range* r, int64_t* lims, float* D, int64_t* I, int flags,
                  void* stream) {
  if (!r || !lims) return fail(VS_E_INVALID, "vs_range_copy: null argument");
  if (r->total > 0 && (!D || !I)) return fail(VS_E_INVALID, "vs_range_copy: null buffer");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard g(r->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_range_copy: hipSetDevice failed");
  const bool out_dev = (flags & VS_OUT_DEVICE) != 0;
  const hipMemcpyKind kind = out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  VS_HIP(hipMemcpyAsync(lims, r->lims, (size_t)(r->nq + 1) * sizeof(int64_t), kind, st),
         "vs_range_copy: lims");
  if (r->total > 0) {
    VS_HIP(hipMemcpyAsync(D, r->D, (size_t)r->total * sizeof(float), kind, st), "vs_range_copy: D");
    VS_HIP(hipMemcpyAsync(I, r->I, (size_t)r->total * sizeof(int64_t), kind, st),
           "vs_range_copy: I");
  }
  if (!out_dev) VS_HIP(hipStreamSynchronize(st), "vs_range_copy: synchronise");
  return VS_OK;
}

int vs_range_destroy(vs_range* r) {
  if (!r) return VS_OK;
  DeviceGuard g(r->device);
  // the copies that read it were enqueued before this call: let them finish
  (void)hipDeviceSynchronize();
  free_range(r);
  return VS_OK;
}

}  // extern "C"
