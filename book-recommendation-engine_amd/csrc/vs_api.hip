// vs_api.hip — the C-ABI of libvsearch.so (declared in include/vsearch.h).
//
// A vs_index is one device's exact flat index: library-owned row storage in HBM
// (fp32 or bf16 elements, stride `ld` elements = a multiple of 128 B, zero
// padding), the squared norms of every row, and ntotal.  It mirrors faiss::IndexFlat (faiss-cpu 1.11.0, not vendored; see
// the reference's poetry.lock:866-867): add copies the caller's rows, search
// writes caller-allocated D/I, remove_ids compacts stably.
//
// Concurrency follows faiss's contract (concurrent searches allowed, add/remove
// exclusive): a shared_mutex guards the storage; per-call scratch comes from a
// chunk cache whose chunks carry the event of their last use, so a search on
// another stream waits (on the device) before it reuses one.
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace vs {
namespace host {

int check_search_args(const char* what, const vs_index* idx, const int64_t* n, int64_t k,
                      bool bufs_ok, bool sel_ok) {
  auto bad = [what](const char* tail) { return fail(VS_E_INVALID, std::string(what) + tail); };
  if (!idx) return bad(": null index");
  if (!sel_ok) return bad(": null selector");
  if (n && *n < 0) return bad(": n < 0");
  if (k <= 0) return bad(": k must be > 0");  // faiss: FAISS_THROW_IF_NOT(k > 0)
  // any k, as faiss-cpu's IndexFlat::search (k > 64: the paged exact engine,
  // run_paged); the bound only keeps 2k - 1 inside the engines' int arithmetic
  if (k > INT_MAX / 2) return bad(": k too large");
  if (!bufs_ok && !(n && *n == 0)) return bad(": null buffer");
  return VS_OK;
}

int HostOut::begin(const char* what, Scratch& scr, float* D_, int64_t* I_, size_t count_,
                   int flags) {
  D = hD = D_;
  I = hI = I_;
  count = count_;
  out_dev = (flags & VS_OUT_DEVICE) != 0;
  if (out_dev) return VS_OK;
  VS_HIPW(scr.alloc((void**)&D, count * sizeof(float)), what, ": scratch");
  if (hI) VS_HIPW(scr.alloc((void**)&I, count * sizeof(int64_t)), what, ": scratch");
  return VS_OK;
}

int HostOut::finish(const char* what, hipStream_t st, bool last_error) {
  if (out_dev) {
    if (last_error) VS_HIP(hipGetLastError(), what);
    return VS_OK;
  }
  VS_HIPW(hipMemcpyAsync(hD, D, count * sizeof(float), hipMemcpyDeviceToHost, st), what,
          hI ? ": copy D" : ": copy");
  if (hI)
    VS_HIPW(hipMemcpyAsync(hI, I, count * sizeof(int64_t), hipMemcpyDeviceToHost, st), what,
            ": copy I");
  VS_HIPW(hipStreamSynchronize(st), what, ": synchronise");
  return VS_OK;
}

int stage_alloc(const char* what, const vs_index* idx, int64_t cmax, Scratch& scr,
                QueryStage* qs) {
  const int64_t qrows = round_up(std::max<int64_t>(cmax, kGemvMaxQ), kBQ);
  VS_HIPW(scr.alloc((void**)&qs->qbuf, (size_t)qrows * idx->ld * sizeof(float)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&qs->qaux, (size_t)qrows * sizeof(float)), what, ": scratch");
  if (idx->esize == 2)
    VS_HIPW(scr.alloc((void**)&qs->qb16, (size_t)qrows * idx->ld * sizeof(uint16_t)), what,
            ": scratch");
  return VS_OK;
}

int stage_chunk(const char* what, const vs_index* idx, const QueryStage& qs, const float* x,
                int64_t nc, int flags, hipStream_t st, SearchArgs* sa) {
  const int mode = idx->metric == VS_METRIC_L2 ? MODE_L2 : MODE_IP;
  const hipMemcpyKind kind =
      (flags & VS_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  float* qbuf = qs.qbuf;
  const int64_t nq_pad = round_up(std::max<int64_t>(nc, kGemvMaxQ), kBQ);
  // zero what the copy leaves: padding rows, and the column tail when d < ld
  if (idx->d == idx->ld) {
    if (nq_pad > nc)
      VS_HIPW(hipMemsetAsync(qbuf + nc * idx->ld, 0,
                             (size_t)(nq_pad - nc) * idx->ld * sizeof(float), st),
              what, ": zero queries");
  } else {
    VS_HIPW(hipMemsetAsync(qbuf, 0, (size_t)nq_pad * idx->ld * sizeof(float), st), what,
            ": zero queries");
  }
  VS_HIPW(hipMemcpy2DAsync(qbuf, idx->ld * sizeof(float), x, (size_t)idx->d * sizeof(float),
                           (size_t)idx->d * sizeof(float), (size_t)nc, kind, st),
          what, ": staging queries");
  if (idx->esize == 2) {
    // bf16 index: queries are rounded to bf16 too, so every path (GEMV in fp32
    // on the rounded values, GEMM on bf16 operands) scores the same numbers
    VS_HIPW(launch_round_bf16(qbuf, nq_pad * idx->ld, st), what, ": rounding queries");
    VS_HIPW(launch_f32_to_bf16(qbuf, idx->ld, qs.qb16, idx->ld, nq_pad, idx->ld, st), what,
            ": bf16 queries");
  }
  if (mode == MODE_L2)
    VS_HIPW(launch_row_norms(qbuf, 4, idx->ld, 0, nq_pad, qs.qaux, st), what, ": query norms");
  sa->mode = mode;
  sa->qbuf = qbuf;
  sa->qb16 = qs.qb16;
  sa->qaux = qs.qaux;
  sa->xaux = idx->norms;
  sa->nq = (int)nc;
  sa->nq_pad = (int)nq_pad;
  return VS_OK;
}

}  // namespace host
}  // namespace vs

namespace {

// Rows in place [i0, i0 + n) -> fp32 out (the caller holds the reader lock).
int reconstruct_rows(vs_index* idx, int64_t i0, int64_t n, float* out, int flags, hipStream_t st) {
  const hipMemcpyKind kind =
      (flags & VS_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (idx->esize == 4) {
    VS_HIP(hipMemcpy2DAsync(out, (size_t)idx->d * sizeof(float), idx->row(i0), idx->rowbytes(),
                            (size_t)idx->d * sizeof(float), (size_t)n, kind, st),
           "vs_reconstruct_n: copy");
  } else {
    // widen bf16 rows in bounded chunks, then copy out
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(64ull << 20) / (idx->d * 4));
    Scratch scr(st);
    float* tmp = nullptr;
    VS_HIP(scr.alloc((void**)&tmp, (size_t)std::min(chunk, n) * idx->d * sizeof(float)),
           "vs_reconstruct_n: scratch");
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
      const int64_t m = std::min(chunk, n - r0);
      VS_HIP(launch_bf16_to_f32((const uint16_t*)idx->row(i0 + r0), idx->ld, tmp, idx->d, m,
                                idx->d, st),
             "vs_reconstruct_n: widen");
      VS_HIP(hipMemcpyAsync(out + r0 * idx->d, tmp, (size_t)m * idx->d * sizeof(float), kind, st),
             "vs_reconstruct_n: copy");
    }
    VS_HIP(hipStreamSynchronize(st), "vs_reconstruct_n: synchronise");
  }
  return VS_OK;
}

}  // namespace

extern "C" {

int vs_version(void) { return 100; }

int vs_device_count(int* n) {
  if (!n) return fail(VS_E_INVALID, "vs_device_count: null output");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return hip_fail(e, "vs_device_count");
  }
  *n = c;
  return VS_OK;
}

int vs_create(int d, int metric, int dtype, int device, vs_index** out) {
  if (!out) return fail(VS_E_INVALID, "vs_create: null output");
  *out = nullptr;
  if (d <= 0) return fail(VS_E_INVALID, "vs_create: d must be > 0");
  if (metric != VS_METRIC_L2 && metric != VS_METRIC_INNER_PRODUCT)
    return fail(VS_E_INVALID, "vs_create: metric must be METRIC_L2 or METRIC_INNER_PRODUCT");
  if (dtype != VS_DTYPE_F32 && dtype != VS_DTYPE_BF16)
    return fail(VS_E_INVALID, "vs_create: dtype must be VS_DTYPE_F32 or VS_DTYPE_BF16");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(VS_E_HIP, "vs_create: no HIP device available");
  if (device < 0 || device >= ndev) return fail(VS_E_INVALID, "vs_create: bad device ordinal");
  DeviceGuard g(device);
  if (!g.ok) return fail(VS_E_HIP, "vs_create: hipSetDevice failed");
  // Keep freed stream-ordered scratch cached in the pool instead of returning it
  // to the driver at every synchronisation.
  hipMemPool_t pool;
  if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) {
    uint64_t thr = UINT64_MAX;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
  }
  vs_index* idx = new vs_index();
  idx->d = d;
  idx->metric = metric;
  idx->dtype = dtype;
  idx->device = device;
  idx->esize = dtype == VS_DTYPE_BF16 ? 2 : 4;
  planes_for(idx);
  idx->ld = round_up(d, 64);  // 64-element K-steps of the filter pass (128-B plane rows)
  *out = idx;
  return VS_OK;
}

int vs_destroy(vs_index* idx) {
  if (!idx) return VS_OK;
  {
    DeviceGuard g(idx->device);
    (void)wait_readers(idx);
    if (idx->wst) (void)hipStreamSynchronize(idx->wst);
    free_storage(idx);
    for (auto& r : idx->readers) (void)hipEventDestroy(r.second);
    idx->readers.clear();
    if (idx->wst) (void)hipStreamDestroy(idx->wst);
    for (int p = 0; p < 2; ++p)
      if (idx->bstats[p]) (void)hipFree(idx->bstats[p]);
    if (idx->ad.dcount) (void)hipFree(idx->ad.dcount);
    if (idx->ddead) (void)hipFree(idx->ddead);
    if (idx->ad.hmirror) (void)hipHostFree(idx->ad.hmirror);
    if (idx->ad.ev) (void)hipEventDestroy(idx->ad.ev);
  }
  delete idx;
  return VS_OK;
}

int vs_reserve(vs_index* idx, int64_t n) {
  if (!idx) return fail(VS_E_INVALID, "vs_reserve: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_reserve: n < 0");
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  // an index that tombstones its removals keeps room for the appends that
  // come before the next pack (1 / pack_den of the rows): at C5's size a
  // storage growth (a copy beside the old rows) does not fit in HBM
  const int64_t want = std::max(n, idx->ntotal);
  if (idx->tombstones() && want / pack_den() > 0) {
    // the headroom is a convenience: without room for it, the exact request
    if (ensure_capacity(idx, want + want / pack_den(), nullptr) == VS_OK) return VS_OK;
    (void)hipGetLastError();
  }
  return ensure_capacity(idx, want, nullptr);
}

int vs_add(vs_index* idx, const float* x, int64_t n, int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_add: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_add: n < 0");
  if (n == 0) return VS_OK;
  if (!x) return fail(VS_E_INVALID, "vs_add: null vectors");
  if (idx->ntotal + n >= (int64_t)INT32_MAX - 2 * kRowPad)
    return fail(VS_E_UNSUPPORTED, "vs_add: a shard holds fewer than 2^31 rows");
  hipStream_t st = (hipStream_t)stream;
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  ++idx->gen;
  int rc = make_room(idx, n, st);
  if (rc) return rc;
  const hipMemcpyKind kind = (flags & VS_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (idx->esize == 4) {
    VS_HIP(hipMemcpy2DAsync(idx->row(idx->ntotal), idx->rowbytes(), x,
                            (size_t)idx->d * sizeof(float), (size_t)idx->d * sizeof(float),
                            (size_t)n, kind, st),
           "vs_add: copying rows");
  } else {
    // bf16 storage: stage fp32 rows on the device in bounded chunks, round into place
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(64ull << 20) / (idx->d * 4));
    Scratch scr(st);
    float* tmp = nullptr;
    VS_HIP(scr.alloc((void**)&tmp, (size_t)std::min(chunk, n) * idx->d * sizeof(float)),
           "vs_add: scratch");
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
      const int64_t m = std::min(chunk, n - r0);
      VS_HIP(hipMemcpyAsync(tmp, x + r0 * idx->d, (size_t)m * idx->d * sizeof(float), kind, st),
             "vs_add: staging rows");
      VS_HIP(launch_f32_to_bf16(tmp, idx->d, (uint16_t*)idx->row(idx->ntotal + r0), idx->ld, m,
                                idx->d, st),
             "vs_add: rounding to bf16");
    }
    VS_HIP(hipStreamSynchronize(st), "vs_add: synchronise");
  }
  VS_HIP(launch_row_norms(idx->codes, idx->esize, idx->ld, idx->ntotal, n, idx->norms, st),
         "vs_add: norms");
  rc = derive_plane(idx, idx->ntotal, n, st, true);
  if (rc) return rc;
  // Source host buffers may be released by the caller as soon as we return.
  VS_HIP(hipStreamSynchronize(st), "vs_add: synchronise");
  idx->ntotal += n;
  return VS_OK;
}

int vs_add_synthetic(vs_index* idx, int64_t n, uint64_t seed, int64_t row0, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_add_synthetic: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_add_synthetic: n < 0");
  if (n == 0) return VS_OK;
  if (idx->ntotal + n >= (int64_t)INT32_MAX - 2 * kRowPad)
    return fail(VS_E_UNSUPPORTED, "vs_add_synthetic: a shard holds fewer than 2^31 rows");
  hipStream_t st = (hipStream_t)stream;
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  ++idx->gen;
  int rc = make_room(idx, n, st);
  if (rc) return rc;
  VS_HIP(launch_fill_synthetic(idx->row(idx->ntotal), idx->esize, n, idx->d, idx->ld, seed, row0,
                               st),
         "vs_add_synthetic: fill");
  VS_HIP(launch_row_norms(idx->codes, idx->esize, idx->ld, idx->ntotal, n, idx->norms, st),
         "vs_add_synthetic: norms");
  rc = derive_plane(idx, idx->ntotal, n, st, true);
  if (rc) return rc;
  VS_HIP(hipStreamSynchronize(st), "vs_add_synthetic: synchronise");
  idx->ntotal += n;
  return VS_OK;
}

int vs_add_synthetic_ids(vs_index* idx, const int64_t* ids, int64_t n, uint64_t seed,
                         void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_add_synthetic_ids: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_add_synthetic_ids: n < 0");
  if (n == 0) return VS_OK;
  if (!ids) return fail(VS_E_INVALID, "vs_add_synthetic_ids: null ids");
  if (idx->ntotal + n >= (int64_t)INT32_MAX - 2 * kRowPad)
    return fail(VS_E_UNSUPPORTED, "vs_add_synthetic_ids: a shard holds fewer than 2^31 rows");
  hipStream_t st = (hipStream_t)stream;
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  ++idx->gen;
  int rc = make_room(idx, n, st);
  if (rc) return rc;
  Scratch scr(st);
  int64_t* dids = nullptr;
  VS_HIP(scr.alloc((void**)&dids, (size_t)n * sizeof(int64_t)), "vs_add_synthetic_ids: scratch");
  VS_HIP(hipMemcpyAsync(dids, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st),
         "vs_add_synthetic_ids: upload");
  VS_HIP(launch_fill_synthetic_ids(idx->row(idx->ntotal), idx->esize, dids, n, idx->d, idx->ld,
                                   seed, st),
         "vs_add_synthetic_ids: fill");
  VS_HIP(launch_row_norms(idx->codes, idx->esize, idx->ld, idx->ntotal, n, idx->norms, st),
         "vs_add_synthetic_ids: norms");
  rc = derive_plane(idx, idx->ntotal, n, st, true);
  if (rc) return rc;
  VS_HIP(hipStreamSynchronize(st), "vs_add_synthetic_ids: synchronise");
  idx->ntotal += n;
  return VS_OK;
}

int vs_reset(vs_index* idx) {
  if (!idx) return fail(VS_E_INVALID, "vs_reset: null index");
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  VS_HIP(wait_readers(idx), "vs_reset");
  ++idx->gen;
  free_storage(idx);
  for (int p = 0; p < 2; ++p)
    if (idx->bstats[p]) VS_HIP(hipMemset(idx->bstats[p], 0, 4 * sizeof(unsigned)), "vs_reset");
  idx->ntotal = 0;
  idx->dead.clear();
  // an empty index starts over: the planes a memory shortage dropped come back
  // (the next add allocates them with the rows), and the next add's rows fix a
  // fresh L2 augmentation
  planes_for(idx);
  reset_l2aug(idx);
  return VS_OK;
}

int vs_ntotal(const vs_index* idx, int64_t* out) {
  if (!idx || !out) return fail(VS_E_INVALID, "vs_ntotal: null argument");
  *out = idx->live();  // faiss ntotal: the live rows
  return VS_OK;
}

int vs_dim(const vs_index* idx, int* out) {
  if (!idx || !out) return fail(VS_E_INVALID, "vs_dim: null argument");
  *out = idx->d;
  return VS_OK;
}

int vs_metric(const vs_index* idx, int* out) {
  if (!idx || !out) return fail(VS_E_INVALID, "vs_metric: null argument");
  *out = idx->metric;
  return VS_OK;
}

int vs_dtype(const vs_index* idx, int* out) {
  if (!idx || !out) return fail(VS_E_INVALID, "vs_dtype: null argument");
  *out = idx->dtype;
  return VS_OK;
}

int vs_set_engine(vs_index* idx, int engine) {
  if (!idx) return fail(VS_E_INVALID, "vs_set_engine: null index");
  if (engine != VS_ENGINE_AUTO && engine != VS_ENGINE_FP32_MFMA &&
      engine != VS_ENGINE_BF16_VERIFY && engine != VS_ENGINE_I8_VERIFY)
    return fail(VS_E_INVALID, "vs_set_engine: unknown engine");
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  if (idx->esize == 4 && engine == VS_ENGINE_I8_VERIFY && !idx->plane_on[FILTER_I8])
    return fail(VS_E_UNSUPPORTED,
                "vs_set_engine: no int8 filter plane (it serves inner-product indexes)");
  if (idx->esize == 4 && engine == VS_ENGINE_BF16_VERIFY && !idx->plane_on[FILTER_BF16])
    return fail(VS_E_UNSUPPORTED, "vs_set_engine: no bf16 filter plane (VS_FILTER=i8)");
  idx->engine = engine;
  return VS_OK;
}

const char* vs_notice(const vs_index* idx) { return idx ? idx->notice.c_str() : ""; }

int vs_filter_plane(const vs_index* idx, int* out) {
  if (!idx || !out) return fail(VS_E_INVALID, "vs_filter_plane: null argument");
  *out = (idx->plane_on[FILTER_I8] ? VS_FILTER_I8 : 0) |
         (idx->plane_on[FILTER_BF16] ? VS_FILTER_BF16 : 0);
  return VS_OK;
}

int vs_set_id_base(vs_index* idx, int64_t id_base) {
  if (!idx) return fail(VS_E_INVALID, "vs_set_id_base: null index");
  if (id_base < 0) return fail(VS_E_INVALID, "vs_set_id_base: negative base");
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  if (id_base != idx->id_base) ++idx->gen;
  idx->id_base = id_base;
  return VS_OK;
}

int vs_search(vs_index* idx, const float* x, int64_t n, int64_t k, float* D, int64_t* I,
              int flags, void* stream) {
  const int rc = check_search_args("vs_search", idx, &n, k, x && D && I);
  if (rc) return rc;
  if (n == 0) return VS_OK;
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  return search_staged("vs_search", idx, x, n, k, D, I, flags, scr, st, idx->ntotal == 0,
                       [&](const SearchArgs& sa, int64_t) {
                         return run_topk(idx, sa, st, VS_ENGINE_AUTO);
                       });
}

int vs_reconstruct_n(vs_index* idx, int64_t i0, int64_t n, float* out, int flags, void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_reconstruct_n: null index");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (n < 0 || i0 < 0 || i0 + n > idx->live())
    return fail(VS_E_INVALID, "vs_reconstruct_n: key out of range");  // faiss: FAISS_THROW_IF_NOT
  if (n == 0) return VS_OK;
  if (!out) return fail(VS_E_INVALID, "vs_reconstruct_n: null output");
  DeviceGuard g(idx->device);
  ReaderMark mark(idx, st);
  // labels [i0, i0 + n) are runs of rows in place between tombstones
  int64_t p = row_of_label(idx, i0), done = 0;
  size_t j = std::upper_bound(idx->dead.begin(), idx->dead.end(), p) - idx->dead.begin();
  while (done < n) {
    const int64_t stop = j < idx->dead.size() ? idx->dead[j] : idx->ntotal;
    const int64_t run = std::min(n - done, stop - p);
    const int rc = reconstruct_rows(idx, p, run, out + done * idx->d, flags, st);
    if (rc) return rc;
    done += run;
    p += run;
    while (j < idx->dead.size() && idx->dead[j] == p) ++p, ++j;  // skip the tombstones
  }
  if (!(flags & VS_OUT_DEVICE)) VS_HIP(hipStreamSynchronize(st), "vs_reconstruct_n: synchronise");
  return VS_OK;
}

int vs_remove_ids(vs_index* idx, const int64_t* ids, int64_t n, int64_t* nremoved) {
  if (!idx) return fail(VS_E_INVALID, "vs_remove_ids: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_remove_ids: n < 0");
  if (nremoved) *nremoved = 0;
  if (n == 0) return VS_OK;
  if (!ids) return fail(VS_E_INVALID, "vs_remove_ids: null ids");
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  // IDSelectorBatch semantics: membership test; duplicates and out-of-range ids
  // are ignored.  Labels here are global (id_base applied), as faiss sees them.
  std::vector<int64_t> rm;
  rm.reserve((size_t)n);
  const int64_t live = idx->live();
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = ids[i] - idx->id_base;
    if (r >= 0 && r < live) rm.push_back(r);
  }
  std::sort(rm.begin(), rm.end());
  rm.erase(std::unique(rm.begin(), rm.end()), rm.end());
  const int64_t nrem = (int64_t)rm.size();
  if (nrem == 0) return VS_OK;
  ++idx->gen;
  DeviceGuard g(idx->device);
  // Searches of this index already queued on other streams read the rows we
  // are about to move or overwrite: wait for their marks (not for the device).
  VS_HIP(wait_readers(idx), "vs_remove_ids: drain");
  hipStream_t st = nullptr;
  VS_HIP(writer_stream(idx, &st), "vs_remove_ids: stream");
  // labels -> rows in place (both ascending: one merge walk over the dead list)
  if (!idx->dead.empty()) {
    size_t j = 0;
    int64_t shift = 0;
    for (auto& r : rm) {
      while (j < idx->dead.size() && idx->dead[j] <= r + shift) ++j, ++shift;
      r += shift;
    }
  }
  if (!idx->tombstones()) {  // filter planes to keep in step: compact now
    const int rc = compact_rows(idx, rm, st);
    if (rc) return rc;
  } else {
    Scratch scr(st);
    int64_t* drm = nullptr;
    VS_HIP(scr.alloc((void**)&drm, (size_t)nrem * sizeof(int64_t)), "vs_remove_ids: scratch");
    VS_HIP(hipMemcpyAsync(drm, rm.data(), (size_t)nrem * sizeof(int64_t), hipMemcpyHostToDevice,
                          st),
           "vs_remove_ids: upload");
    VS_HIP(launch_fill_nan_rows(idx->codes, idx->rowbytes(), idx->norms, idx->esize, drm, nrem, st,
                                idx->plane_on[FILTER_I8] ? idx->fscale : nullptr),
           "vs_remove_ids: tombstones");
    std::vector<int64_t> merged;
    merged.reserve(idx->dead.size() + rm.size());
    std::merge(idx->dead.begin(), idx->dead.end(), rm.begin(), rm.end(),
               std::back_inserter(merged));
    idx->dead.swap(merged);
    VS_HIP(hipStreamSynchronize(st), "vs_remove_ids: synchronise");
    if ((int64_t)idx->dead.size() * pack_den() >= idx->ntotal) {
      const int rc = pack_dead(idx);
      if (rc) return rc;
    } else {
      const int64_t nd = (int64_t)idx->dead.size();
      if (nd > idx->ddead_cap) {
        const int64_t cap = std::max<int64_t>(nd, 2 * idx->ddead_cap);
        if (idx->ddead) (void)hipFree(idx->ddead);
        idx->ddead = nullptr;
        idx->ddead_cap = 0;
        VS_HIP(hipMalloc(&idx->ddead, (size_t)cap * sizeof(int64_t)), "vs_remove_ids: dead list");
        idx->ddead_cap = cap;
      }
      VS_HIP(hipMemcpyAsync(idx->ddead, idx->dead.data(), (size_t)nd * sizeof(int64_t),
                            hipMemcpyHostToDevice, st),
             "vs_remove_ids: dead list");
      VS_HIP(hipStreamSynchronize(st), "vs_remove_ids: synchronise");
    }
  }
  // every row removed: the next add's rows fix a fresh L2 augmentation (the
  // old one followed rows that are gone)
  if (idx->ntotal == 0) reset_l2aug(idx);
  if (nremoved) *nremoved = nrem;
  return VS_OK;
}

int vs_selfjoin(vs_index* idx, int64_t q0, int64_t nq, int64_t k, int exclude_self,
                float min_sim, float* D, int64_t* I, int flags, void* stream) {
  const int rc0 = check_search_args("vs_selfjoin", idx, nullptr, k);
  if (rc0) return rc0;
  if (q0 < 0 || nq < 0) return fail(VS_E_INVALID, "vs_selfjoin: query rows out of range");
  if (nq > 0 && (!D || !I)) return fail(VS_E_INVALID, "vs_selfjoin: null buffer");
  hipStream_t st = (hipStream_t)stream;
  // The self-join reads its query rows in place and emits row numbers as labels,
  // so it runs on an index without tombstones: under the shared lock it checks
  // for them, and if a removal left some, packs them under the unique lock and
  // looks again (a removal can land between the two locks).
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
  if (q0 + nq > idx->ntotal) return fail(VS_E_INVALID, "vs_selfjoin: query rows out of range");
  if (nq == 0) return VS_OK;
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_selfjoin: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  HostOut out;
  int rc = out.begin("vs_selfjoin", scr, D, I, (size_t)nq * k, flags);
  if (rc) return rc;
  float* rinv = nullptr;
  VS_HIP(scr.alloc((void**)&rinv, (size_t)idx->capacity * sizeof(float)), "vs_selfjoin: scratch");
  VS_HIP(launch_rsqrt(idx->norms, idx->capacity, rinv, st), "vs_selfjoin: rsqrt");
  // Query tiles read stored rows directly (capacity keeps kBQ rows of slack).
  const int64_t chunk = 65536;
  for (int64_t c0 = 0; c0 < nq; c0 += chunk) {
    const int64_t nc = std::min(chunk, nq - c0);
    const int64_t nq_pad = round_up(nc, kBQ);
    const int64_t qrow = q0 + c0;
    const bool b16 = idx->esize == 2;
    SearchArgs sa;
    sa.mode = MODE_COS;
    sa.qbuf = b16 ? nullptr : (const float*)idx->row(qrow);
    sa.qb16 = b16 ? (const void*)idx->row(qrow) : nullptr;
    sa.qaux = rinv + qrow;
    sa.xaux = rinv;
    sa.nq = (int)nc;
    sa.nq_pad = (int)nq_pad;
    sa.k = (int)k;
    sa.self0 = exclude_self ? qrow : -1;
    sa.min_score = min_sim;
    sa.D = out.D + c0 * k;
    sa.I = out.I + c0 * k;
    rc = run_topk(idx, sa, st, VS_ENGINE_AUTO);
    if (rc) return rc;
  }
  // device outputs: unlike the searches, the self-join does not report the
  // thread's pending HIP error (an earlier call's would fail this one)
  return out.finish("vs_selfjoin", st, false);
}

int vs_merge_topk(const float* D_parts, const int64_t* I_parts, int64_t nparts, int64_t nq,
                  int64_t k_in, int64_t k, int metric, float* D, int64_t* I, void* stream) {
  if (nparts < 1 || nq < 0 || k_in < 1 || k < 1)
    return fail(VS_E_INVALID, "vs_merge_topk: bad sizes");
  if (k > INT_MAX / 2) return fail(VS_E_INVALID, "vs_merge_topk: k too large");
  if (nparts > 64) return fail(VS_E_UNSUPPORTED, "vs_merge_topk: more than 64 parts");
  if (metric != VS_METRIC_L2 && metric != VS_METRIC_INNER_PRODUCT)
    return fail(VS_E_INVALID, "vs_merge_topk: bad metric");
  if (nq == 0) return VS_OK;
  if (!D_parts || !I_parts || !D || !I) return fail(VS_E_INVALID, "vs_merge_topk: null buffer");
  VS_HIP(launch_merge_parts(metric == VS_METRIC_L2 ? MODE_L2 : MODE_IP, D_parts, I_parts,
                            (int)nparts, (int)nq, (int)k_in, (int)k, D, I, (hipStream_t)stream),
         "vs_merge_topk: launch");
  return VS_OK;
}

int vs_fill_synthetic(float* out, int64_t rows, int64_t d, uint64_t seed, int64_t row0,
                      void* stream) {
  if (rows < 0 || d <= 0 || row0 < 0) return fail(VS_E_INVALID, "vs_fill_synthetic: bad sizes");
  if (rows == 0) return VS_OK;
  if (!out) return fail(VS_E_INVALID, "vs_fill_synthetic: null output");
  VS_HIP(launch_fill_synthetic(out, 4, rows, d, d, seed, row0, (hipStream_t)stream),
         "vs_fill_synthetic: launch");
  return VS_OK;
}

}  // extern "C"
