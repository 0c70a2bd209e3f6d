// vs_api_range.hip — range searches ("Range search"):
// vs_range_search and the vs_range result's exports.
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

  // count / scan / fill
  const int nsplit = gemm_nsplit((ntotal + kBN - 1) / kBN, (int)(nq_pad / kBQ));
  const int64_t nseg = nq_pad * nsplit;
  int* cnt = nullptr;
  int64_t* off = nullptr;
  int* err = nullptr;
  VS_HIP(scr.alloc((void**)&cnt, (size_t)nseg * sizeof(int)), "vs_range_search: scratch");
  VS_HIP(scr.alloc((void**)&off, (size_t)(nseg + 1) * sizeof(int64_t)), "vs_range_search: scratch");
  VS_HIP(scr.alloc((void**)&err, sizeof(int)), "vs_range_search: scratch");
  VS_HIP(hipMemsetAsync(err, 0, sizeof(int), st), "vs_range_search: flag");
  const void* qmat = qb16 ? (const void*)qb16 : (const void*)qbuf;
  {
    KernelTimer tm(st, "gemm_range");
    VS_HIP(launch_gemm_range(false, mode, idx->codes, idx->norms, qmat, qaux, idx->ld, idx->esize,
                             ntotal, (int)nq_pad, nsplit, thr, cnt, nullptr, nullptr, nullptr, st),
           "vs_range_search: gemm_range count launch");
    tm.stop();
  }
  VS_HIP(launch_range_scan(cnt, nseg, off, st), "vs_range_search: scan");
  int64_t ncand = 0;
  VS_HIP(hipMemcpyAsync(&ncand, off + nseg, sizeof(int64_t), hipMemcpyDeviceToHost, st),
         "vs_range_search: candidate total");
  VS_HIP(hipStreamSynchronize(st), "vs_range_search: synchronise");
  if (ncand >= ((int64_t)1 << 31))
    return fail(VS_E_UNSUPPORTED, "vs_range_search: " + std::to_string(ncand) +
                                      " candidates (2^31 or more): search fewer queries per call");
  r->ncand = ncand;
  const int64_t lbytes = (n + 1) * (int64_t)sizeof(int64_t);
  if (ncand == 0) {
    VS_HIP(hipMemsetAsync(r->lims, 0, (size_t)lbytes, st), "vs_range_search: lims");
    VS_HIP(hipStreamSynchronize(st), "vs_range_search: synchronise");
    return VS_OK;
  }
  int* cand = nullptr;
  float* ekey = nullptr;
  uint8_t* flag = nullptr;
  int* hits = nullptr;
  VS_HIP(scr.alloc((void**)&cand, (size_t)ncand * sizeof(int)), "vs_range_search: candidates");
  VS_HIP(scr.alloc((void**)&ekey, (size_t)ncand * sizeof(float)), "vs_range_search: candidates");
  VS_HIP(scr.alloc((void**)&flag, (size_t)ncand), "vs_range_search: candidates");
  VS_HIP(scr.alloc((void**)&hits, (size_t)n * sizeof(int)), "vs_range_search: scratch");
  // a slot the fill pass left (it never does: *err) holds no row
  VS_HIP(hipMemsetAsync(cand, 0xFF, (size_t)ncand * sizeof(int), st), "vs_range_search: candidates");
  {
    KernelTimer tm(st, "gemm_range");
    VS_HIP(launch_gemm_range(true, mode, idx->codes, idx->norms, qmat, qaux, idx->ld, idx->esize,
                             ntotal, (int)nq_pad, nsplit, thr, nullptr, off, cand, err, st),
           "vs_range_search: gemm_range fill launch");
    tm.stop();
  }
  VS_HIP(launch_range_verify(emode, cand, ncand, off, nsplit, (int)n, idx->codes, idx->esize,
                             idx->norms, qbuf, qaux, idx->ld, ntotal, radius,
                             sel ? sel->rbits : nullptr, ekey, flag, st),
         "vs_range_search: verification");
  VS_HIP(launch_range_hits(flag, off, nsplit, (int)n, hits, st), "vs_range_search: hit counts");
  VS_HIP(launch_range_scan(hits, n, r->lims, st), "vs_range_search: lims");
  int64_t total = 0;
  int herr = 0;
  VS_HIP(hipMemcpyAsync(&total, r->lims + n, sizeof(int64_t), hipMemcpyDeviceToHost, st),
         "vs_range_search: hit total");
  VS_HIP(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, st),
         "vs_range_search: flag");
  VS_HIP(hipStreamSynchronize(st), "vs_range_search: synchronise");
  if (herr) return fail(VS_E_HIP, "vs_range_search: range fill disagrees with its count");
  if (total == 0) return VS_OK;
  hipError_t e = hipMalloc(&r->D, (size_t)total * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&r->I, (size_t)total * sizeof(int64_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? VS_E_OOM : VS_E_HIP,
                "vs_range_search: no memory for " + std::to_string(total) + " results: " +
                    hipGetErrorString(e));
  }
  r->total = total;
  VS_HIP(launch_range_emit(cand, ekey, flag, off, nsplit, (int)n, r->lims, idx->id_base, r->D,
                           r->I, st),
         "vs_range_search: emission");
  // tombstoned rows never match; the rows found become faiss labels
  if (!idx->dead.empty())
    VS_HIP(launch_label_map(r->I, total, idx->ddead, (int64_t)idx->dead.size(), idx->id_base, st),
           "vs_range_search: labels");
  VS_HIP(hipStreamSynchronize(st), "vs_range_search: synchronise");
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
