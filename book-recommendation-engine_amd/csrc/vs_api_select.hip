// vs_api_select.hip — selector searches (DESIGN.md "Selector searches"):
// vs_selector_*, vs_search_sel and the per-chunk engine behind it.
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// One chunk of a selector search (vs_search_sel; DESIGN.md "Selector searches").
// `streaming`: the call has at most kSkinnyMaxQ queries (the streaming kernel
// where its queries fit the LDS).
int run_selected(vs_index* idx, const vs_selector* sel, const SearchArgs& a, bool streaming,
                 hipStream_t st) {
  const bool tie_rule = a.mode == MODE_IP && !a.raw;
  const int64_t need = tie_rule ? 2 * (int64_t)a.k - 1 : a.k;
  const int64_t excluded = idx->live() - sel->count;
  if (excluded <= kSelMaxExcluded) {
    // Route (b): the unselected engine in raw order for need + excluded
    // entries (never more than the live rows), the unselected entries dropped
    // stably, then faiss's tie rule over what is left.  The need + m
    // lexicographically best rows minus m excluded ones hold the `need` best
    // selected rows, and the rule is a function of those.
    const int64_t k2 = std::min<int64_t>(need + excluded, idx->live());
    if (k2 > INT_MAX / 2) return fail(VS_E_INVALID, "vs_search_sel: k too large");
    Scratch scr(st);
    float* D2 = nullptr;
    int64_t* I2 = nullptr;
    VS_HIP(scr.alloc((void**)&D2, (size_t)a.nq * k2 * sizeof(float)), "vs_search_sel: scratch");
    VS_HIP(scr.alloc((void**)&I2, (size_t)a.nq * k2 * sizeof(int64_t)), "vs_search_sel: scratch");
    SearchArgs b = a;
    b.raw = 1;
    b.k = (int)k2;
    b.D = D2;
    b.I = I2;
    const int rc = run_topk(idx, b, st, VS_ENGINE_AUTO);
    if (rc) return rc;
    if (!tie_rule) {
      VS_HIP(launch_sel_drop(a.mode, D2, I2, a.nq, (int)k2, sel->rbits, idx->id_base, a.D, a.I,
                             a.k, st),
             "vs_search_sel: drop launch");
      return VS_OK;
    }
    const int kin = (int)std::min<int64_t>(need, sel->count);
    float* D3 = nullptr;
    int64_t* I3 = nullptr;
    VS_HIP(scr.alloc((void**)&D3, (size_t)a.nq * kin * sizeof(float)), "vs_search_sel: scratch");
    VS_HIP(scr.alloc((void**)&I3, (size_t)a.nq * kin * sizeof(int64_t)), "vs_search_sel: scratch");
    VS_HIP(launch_sel_drop(a.mode, D2, I2, a.nq, (int)k2, sel->rbits, idx->id_base, D3, I3, kin,
                           st),
           "vs_search_sel: drop launch");
    VS_HIP(launch_merge_parts(a.mode, D3, I3, 1, a.nq, kin, a.k, a.D, a.I, st),
           "vs_search_sel: merge launch");
    return VS_OK;
  }
  // Route (c): the gathered engine, one exact page.
  if (need > VS_MAX_K)
    return fail(VS_E_UNSUPPORTED,
                "vs_search_sel: the gathered engine holds one exact page (inner product k <= 32, "
                "L2 / raw order k <= 64); selections that leave at most 256 rows out take any k");
  const int KP = kp_for(need);
  const int count = (int)sel->count;
  Scratch scr(st);
  Partials part;
  part.KP = KP;
  if (streaming && gemv_fits(idx->ld)) {
    const int gmode = a.mode == MODE_L2 ? MODE_L2D : MODE_IP;
    const int nblocks = stream_blocks(count);
    part.P = nblocks;
    const int nql = a.nq <= 2 ? a.nq : (a.nq <= 4 ? 4 : kGemvMaxQ);
    const size_t n = (size_t)nql * part.P * KP;
    VS_HIP(scr.alloc((void**)&part.key, n * sizeof(float)), "vs_search_sel: scratch");
    VS_HIP(scr.alloc((void**)&part.id, n * sizeof(int)), "vs_search_sel: scratch");
    for (int q0 = 0; q0 < a.nq; q0 += kGemvMaxQ) {
      const int nc = std::min(kGemvMaxQ, a.nq - q0);
      KernelTimer tm(st, "gemv_topk_rows");
      VS_HIP(launch_gemv_topk_rows(KP, gmode, nc, idx->codes, idx->esize,
                                   a.qbuf + (int64_t)q0 * idx->ld, idx->ld, sel->list, count,
                                   nblocks, part, st),
             "vs_search_sel: gemv_topk_rows launch");
      tm.stop();
      VS_HIP(launch_merge_partials(gmode, part, nc, a.k, idx->id_base, a.min_score,
                                   a.D + (int64_t)q0 * a.k, a.I + (int64_t)q0 * a.k, a.k, st,
                                   a.raw),
             "vs_search_sel: merge launch");
    }
    return VS_OK;
  }
  const int nsplit = gemm_nsplit((count + kBN - 1) / kBN, a.nq_pad / kBQ);
  part.P = 2 * nsplit;
  const size_t n = (size_t)a.nq_pad * part.P * KP;
  VS_HIP(scr.alloc((void**)&part.key, n * sizeof(float)), "vs_search_sel: scratch");
  VS_HIP(scr.alloc((void**)&part.id, n * sizeof(int)), "vs_search_sel: scratch");
  const void* qmat = a.qb16 ? a.qb16 : (const void*)a.qbuf;
  {
    KernelTimer tm(st, "gemm_topk_rows");
    VS_HIP(launch_gemm_topk_rows(KP, a.mode, idx->codes, a.xaux, qmat, a.qaux, idx->ld,
                                 idx->esize, sel->list, count, a.nq_pad, nsplit, part, st),
           "vs_search_sel: gemm_topk_rows launch");
    tm.stop();
  }
  VS_HIP(launch_merge_partials(a.mode, part, a.nq, a.k, idx->id_base, a.min_score, a.D, a.I, a.k,
                               st, a.raw),
         "vs_search_sel: merge launch");
  return VS_OK;
}

void free_selector(vs_selector* sel) {
  if (sel->rbits) (void)hipFree(sel->rbits);
  if (sel->list) (void)hipFree(sel->list);
  delete sel;
}

}  // namespace

extern "C" {

int vs_selector_create(vs_index* idx, const uint8_t* bitmap, int64_t nbits, void* stream,
                       vs_selector** out) {
  if (!out) return fail(VS_E_INVALID, "vs_selector_create: null output");
  *out = nullptr;
  if (!idx) return fail(VS_E_INVALID, "vs_selector_create: null index");
  if (nbits < 0) return fail(VS_E_INVALID, "vs_selector_create: nbits < 0");
  if (nbits > 0 && !bitmap) return fail(VS_E_INVALID, "vs_selector_create: null bitmap");
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_selector_create: hipSetDevice failed");
  vs_selector* sel = new vs_selector();
  sel->idx = idx;
  sel->device = idx->device;
  sel->gen = idx->gen;
  const int64_t nb = std::min(nbits, idx->live());  // labels past ntotal are not selected
  if (idx->ntotal == 0 || nb == 0) {
    *out = sel;
    return VS_OK;
  }
  ReaderMark mark(idx, st);
  const int ntotal = (int)idx->ntotal;
  const int nblocks = (ntotal + kSelBlockRows - 1) / kSelBlockRows;
  const int64_t nwords = (int64_t)nblocks * (kSelBlockRows / 32);
  int rc = VS_OK;
  do {
    hipError_t e = hipMalloc(&sel->rbits, (size_t)nwords * sizeof(uint32_t));
    if (e != hipSuccess) { rc = hip_fail(e, "vs_selector_create: bitmap"); break; }
    Scratch scr(st);
    uint8_t* lbits = nullptr;
    int* bsum = nullptr;
    int* dcount = nullptr;
    const size_t lbytes = (size_t)((nb + 7) / 8);
    if ((e = scr.alloc((void**)&lbits, lbytes)) != hipSuccess ||
        (e = scr.alloc((void**)&bsum, (size_t)nblocks * sizeof(int))) != hipSuccess ||
        (e = scr.alloc((void**)&dcount, sizeof(int))) != hipSuccess) {
      rc = hip_fail(e, "vs_selector_create: scratch");
      break;
    }
    int hcount = 0;
    if ((e = hipMemcpyAsync(lbits, bitmap, lbytes, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = launch_sel_row_bits(lbits, nb, idx->ddead, (int64_t)idx->dead.size(), ntotal,
                                 sel->rbits, nwords, st)) != hipSuccess ||
        (e = launch_sel_block_counts(sel->rbits, nblocks, bsum, st)) != hipSuccess ||
        (e = launch_sel_scan(bsum, nblocks, dcount, st)) != hipSuccess ||
        (e = hipMemcpyAsync(&hcount, dcount, sizeof(int), hipMemcpyDeviceToHost, st)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess) {
      rc = hip_fail(e, "vs_selector_create: compaction");
      break;
    }
    sel->count = hcount;
    if (hcount > 0) {
      const int64_t npad = round_up(hcount, kBN);
      if ((e = hipMalloc(&sel->list, (size_t)npad * sizeof(int))) != hipSuccess) {
        rc = hip_fail(e, "vs_selector_create: row list");
        break;
      }
      if ((e = launch_sel_scatter(sel->rbits, nblocks, bsum, dcount, sel->list, st)) !=
              hipSuccess ||
          (e = hipStreamSynchronize(st)) != hipSuccess) {
        rc = hip_fail(e, "vs_selector_create: scatter");
        break;
      }
    }
  } while (0);
  if (rc) {
    free_selector(sel);
    return rc;
  }
  *out = sel;
  return VS_OK;
}

int vs_selector_count(const vs_selector* sel, int64_t* out) {
  if (!sel || !out) return fail(VS_E_INVALID, "vs_selector_count: null argument");
  *out = sel->count;
  return VS_OK;
}

int vs_selector_destroy(vs_selector* sel) {
  if (!sel) return VS_OK;
  DeviceGuard g(sel->device);
  // the searches that read it were enqueued before this call: let them finish
  if (sel->rbits || sel->list) (void)hipDeviceSynchronize();
  free_selector(sel);
  return VS_OK;
}

int vs_search_sel(vs_index* idx, const vs_selector* sel, const float* x, int64_t n, int64_t k,
                  float* D, int64_t* I, int flags, void* stream) {
  const int rc = check_search_args("vs_search_sel", idx, &n, k, x && D && I, sel != nullptr);
  if (rc) return rc;
  if (n == 0) return VS_OK;
  hipStream_t st = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> lk(idx->mu);
  if (sel->idx != idx) return fail(VS_E_INVALID, "vs_search_sel: the selector belongs to another index");
  if (sel->gen != idx->gen)
    return fail(VS_E_INVALID, "vs_search_sel: stale selector (the index changed since it was built)");
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_search_sel: hipSetDevice failed");
  ReaderMark mark(idx, st);
  Scratch scr(st);
  return search_staged("vs_search_sel", idx, x, n, k, D, I, flags, scr, st,
                       idx->ntotal == 0 || sel->count == 0, [&](const SearchArgs& sa, int64_t) {
                         return run_selected(idx, sel, sa, n <= kSkinnyMaxQ, st);
                       });
}

}  // extern "C"
