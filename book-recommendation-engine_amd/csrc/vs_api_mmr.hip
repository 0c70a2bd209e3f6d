// vs_api_mmr.hip — MMR searches (DESIGN.md "MMR searches"): vs_mmr_select,
// vs_search_mmr.
#include <cstdlib>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// The re-rank's own scratch per chunk of queries (candidate rows, s and |c|^2
// of every candidate, staged queries, staged labels and positions) stays
// within this budget: F = 1024 at d = 1536 is ~38 KB a query, 1,700 queries a
// chunk.  A chunk holds at most kMmrChunkMax queries (the grid's y dimension);
// env VS_MMR_CHUNK lowers the cap (tests chunk small batches with it).
constexpr size_t kMmrScratchBudget = 64u << 20;
constexpr int64_t kMmrChunkMax = 16384;

int64_t mmr_chunk(int64_t n, size_t per_query) {
  int64_t c = std::min<int64_t>(kMmrChunkMax, (int64_t)(kMmrScratchBudget / per_query));
  const char* e = getenv("VS_MMR_CHUNK");
  const int64_t v = e ? atoll(e) : 0;
  if (v > 0) c = std::min(c, v);
  return std::max<int64_t>(1, std::min(c, n));
}

// What one re-rank works on.  x: the queries, fp32 of stride d (host, or
// device under x_dev).  labels: n * F candidate labels (host, or device under
// lab_dev); host labels were checked by the caller, device ones raise *dbad
// (device, may be null) when they are no candidates.  pos: n * k positions
// (host, or device under pos_dev), null for none.  Dc / Ic (device, n * F) with
// Dout / Iout (device, n * k): the picks' scores and labels gathered as well.
struct MmrArgs {
  const float* x = nullptr;
  bool x_dev = false;
  const int64_t* labels = nullptr;
  bool lab_dev = false;
  int* dbad = nullptr;
  int* pos = nullptr;
  bool pos_dev = false;
  const float* Dc = nullptr;
  const int64_t* Ic = nullptr;
  float* Dout = nullptr;
  int64_t* Iout = nullptr;
};

// The caller holds the reader lock, the device and a reader mark on `st`.
int mmr_run(const char* what, vs_index* idx, const MmrArgs& a, int64_t n, int F, int k,
            double lambda, Scratch& scr, hipStream_t st) {
  const int d = idx->d;
  const bool stage_pos = !(a.pos && a.pos_dev);
  const size_t per_query = (size_t)F * (sizeof(int64_t) + 2 * sizeof(double)) +
                           (a.x_dev ? 0 : (size_t)d * sizeof(float)) +
                           (a.lab_dev ? 0 : (size_t)F * sizeof(int64_t)) +
                           (stage_pos ? (size_t)k * sizeof(int) : 0);
  const int64_t cq = mmr_chunk(n, per_query);
  int64_t* rows = nullptr;
  double* S = nullptr;
  double* NN = nullptr;
  float* xbuf = nullptr;
  int64_t* lbuf = nullptr;
  int* pbuf = nullptr;
  VS_HIPW(scr.alloc((void**)&rows, (size_t)cq * F * sizeof(int64_t)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&S, (size_t)cq * F * sizeof(double)), what, ": scratch");
  VS_HIPW(scr.alloc((void**)&NN, (size_t)cq * F * sizeof(double)), what, ": scratch");
  if (!a.x_dev) VS_HIPW(scr.alloc((void**)&xbuf, (size_t)cq * d * sizeof(float)), what, ": scratch");
  if (!a.lab_dev)
    VS_HIPW(scr.alloc((void**)&lbuf, (size_t)cq * F * sizeof(int64_t)), what, ": scratch");
  if (stage_pos) VS_HIPW(scr.alloc((void**)&pbuf, (size_t)cq * k * sizeof(int)), what, ": scratch");
  const float pad = idx->metric == VS_METRIC_L2 ? FLT_MAX : -FLT_MAX;
  for (int64_t c0 = 0; c0 < n; c0 += cq) {
    const int64_t nc = std::min(cq, n - c0);
    const float* xq = a.x + c0 * d;
    if (!a.x_dev) {
      VS_HIPW(hipMemcpyAsync(xbuf, xq, (size_t)nc * d * sizeof(float), hipMemcpyHostToDevice, st),
              what, ": staging queries");
      xq = xbuf;
    }
    const int64_t* lab = a.labels + c0 * F;
    if (!a.lab_dev) {
      VS_HIPW(hipMemcpyAsync(lbuf, lab, (size_t)nc * F * sizeof(int64_t), hipMemcpyHostToDevice,
                             st),
              what, ": staging candidates");
      lab = lbuf;
    }
    VS_HIPW(launch_mmr_rows(lab, nc * F, idx->ddead, (int64_t)idx->dead.size(), idx->id_base,
                            idx->live(), rows, a.dbad, st),
            what, ": rows launch");
    // extra spans for tools/bench_mmr.py (they name no search kernel)
    KernelTimer ts(st, "mmr_sims", false);
    VS_HIPW(launch_mmr_sims(idx->codes, idx->esize, idx->ld, d, xq, rows, (int)nc, F, S, NN, st),
            what, ": sims launch");
    ts.stop();
    int* dpos = stage_pos ? pbuf : a.pos + c0 * k;
    KernelTimer tp(st, "mmr_pick", false);
    VS_HIPW(launch_mmr_pick(idx->codes, idx->esize, idx->ld, rows, (int)nc, F, k, lambda, S, NN,
                            dpos, a.Dc ? a.Dc + c0 * F : nullptr, a.Ic ? a.Ic + c0 * F : nullptr,
                            pad, a.Dout ? a.Dout + c0 * k : nullptr,
                            a.Iout ? a.Iout + c0 * k : nullptr, st),
            what, ": pick launch");
    tp.stop();
    if (a.pos && !a.pos_dev)
      VS_HIPW(hipMemcpyAsync(a.pos + c0 * k, pbuf, (size_t)nc * k * sizeof(int),
                             hipMemcpyDeviceToHost, st),
              what, ": copy");
  }
  return VS_OK;
}

// The checks both entry points make after check_search_args, in the header's
// order: fetch_k, lambda, (no queries: done), buffers, the fetch_k limit.
int check_mmr_args(const char* what, int64_t n, int64_t fetch_k, double lambda, bool bufs_ok,
                   bool* done) {
  auto bad = [what](const char* tail) { return fail(VS_E_INVALID, std::string(what) + tail); };
  *done = false;
  if (fetch_k <= 0) return bad(": fetch_k must be > 0");
  if (!std::isfinite(lambda)) return bad(": lambda_mult is not finite");
  if (n == 0) {
    *done = true;
    return VS_OK;
  }
  if (!bufs_ok) return bad(": null buffer");
  if (fetch_k > kMmrMaxFetch)
    return fail(VS_E_UNSUPPORTED,
                std::string(what) + ": fetch_k > 1024 (the staged engine's candidate limit; "
                                    "re-rank longer lists in pieces)");
  return VS_OK;
}

}  // namespace

extern "C" {

int vs_mmr_select(vs_index* idx, const float* x, int64_t n, const int64_t* cand, int64_t fetch_k,
                  int64_t k, double lambda_mult, int32_t* pos, int flags, void* stream) {
  int rc = check_search_args("vs_mmr_select", idx, &n, k);
  if (rc) return rc;
  bool done = false;
  rc = check_mmr_args("vs_mmr_select", n, fetch_k, lambda_mult, x && cand && pos, &done);
  if (rc || done) return rc;
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  const bool in_dev = (flags & VS_IN_DEVICE) != 0;
  if (!in_dev) {
    const int64_t live = idx->live();
    for (int64_t i = 0; i < n * fetch_k; ++i) {
      const int64_t l = cand[i] - idx->id_base;
      if (cand[i] != -1 && (l < 0 || l >= live))
        return fail(VS_E_INVALID, "vs_mmr_select: key out of range");  // faiss reconstruct throws
    }
  }
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_mmr_select: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  MmrArgs a;
  a.x = x;
  a.x_dev = in_dev;
  a.labels = cand;
  a.lab_dev = in_dev;
  a.pos = pos;
  a.pos_dev = (flags & VS_OUT_DEVICE) != 0;
  if (in_dev) {
    VS_HIP(scr.alloc((void**)&a.dbad, sizeof(int)), "vs_mmr_select: scratch");
    VS_HIP(hipMemsetAsync(a.dbad, 0, sizeof(int), st), "vs_mmr_select: flag");
  }
  rc = mmr_run("vs_mmr_select", idx, a, n, (int)fetch_k, (int)k, lambda_mult, scr, st);
  if (rc) return rc;
  int hbad = 0;
  if (in_dev)
    VS_HIP(hipMemcpyAsync(&hbad, a.dbad, sizeof(int), hipMemcpyDeviceToHost, st),
           "vs_mmr_select: flag");
  if (in_dev || !a.pos_dev) VS_HIP(hipStreamSynchronize(st), "vs_mmr_select: synchronise");
  if (hbad) return fail(VS_E_INVALID, "vs_mmr_select: key out of range");
  if (a.pos_dev) VS_HIP(hipGetLastError(), "vs_mmr_select");
  return VS_OK;
}

int vs_search_mmr(vs_index* idx, const float* x, int64_t n, int64_t k, int64_t fetch_k,
                  double lambda_mult, const int64_t* excl_offs, const int64_t* excl_labels,
                  float* D, int64_t* I, int flags, void* stream) {
  int rc = check_search_args("vs_search_mmr", idx, &n, k);
  if (rc) return rc;
  bool done = false;
  rc = check_mmr_args("vs_search_mmr", n, fetch_k, lambda_mult, x && D && I, &done);
  if (rc || done) return rc;
  rc = check_excl_lists("vs_search_mmr", excl_offs, excl_labels, n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_mmr: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  // the candidates: the search's own results for fetch_k, kept on the device
  // (n * fetch_k entries, what a search with device outputs would hold)
  float* Dc = nullptr;
  int64_t* Ic = nullptr;
  VS_HIP(scr.alloc((void**)&Dc, (size_t)n * fetch_k * sizeof(float)), "vs_search_mmr: scratch");
  VS_HIP(scr.alloc((void**)&Ic, (size_t)n * fetch_k * sizeof(int64_t)), "vs_search_mmr: scratch");
  rc = search_excl_held(idx, x, n, fetch_k, excl_offs, excl_labels, Dc, Ic,
                        (flags & VS_IN_DEVICE) | VS_OUT_DEVICE, st);
  if (rc) return rc;
  HostOut out;
  rc = out.begin("vs_search_mmr", scr, D, I, (size_t)n * k, flags);
  if (rc) return rc;
  MmrArgs a;
  a.x = x;
  a.x_dev = (flags & VS_IN_DEVICE) != 0;
  a.labels = Ic;
  a.lab_dev = true;
  a.Dc = Dc;
  a.Ic = Ic;
  a.Dout = out.D;
  a.Iout = out.I;
  rc = mmr_run("vs_search_mmr", idx, a, n, (int)fetch_k, (int)k, lambda_mult, scr, st);
  if (rc) return rc;
  return out.finish("vs_search_mmr", st);
}

}  // extern "C"
