// vs_api_update.hip — in-place updates ("In-place updates"):
// vs_update_rows gives live rows new values where they are stored.  The new
// rows are staged as a contiguous block in the index's element type, the
// derivation kernels of an add run over that block into staged outputs (so
// every derived byte is the one vs_add would have produced), and one scatter
// launch (vs_update.hip) moves the block's rows to their places.  Nothing the
// call launches, copies or loops over grows with ntotal, but for the walk over
// the dead list that maps labels to rows.
#include <numeric>

#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {

// labels (id_base applied) -> rows in place, in the caller's order; every label
// a live one and given once, else VS_E_INVALID with nothing touched.
int rows_of_labels(const vs_index* idx, const int64_t* labels, int64_t n,
                   std::vector<int64_t>* rows) {
  const int64_t live = idx->live();
  std::vector<int64_t> order((size_t)n);
  std::iota(order.begin(), order.end(), (int64_t)0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t l = labels[i] - idx->id_base;
    if (l < 0 || l >= live)  // faiss reconstruct throws for the same labels
      return fail(VS_E_INVALID, "vs_update_rows: label " + std::to_string(labels[i]) +
                                    " is not a live label");
  }
  std::sort(order.begin(), order.end(),
            [labels](int64_t a, int64_t b) { return labels[a] < labels[b]; });
  for (int64_t i = 1; i < n; ++i)
    if (labels[order[i]] == labels[order[i - 1]])
      return fail(VS_E_INVALID, "vs_update_rows: label " + std::to_string(labels[order[i]]) +
                                    " given more than once");
  // both ascending: one merge walk over the dead list (as vs_remove_ids)
  rows->resize((size_t)n);
  size_t j = 0;
  int64_t shift = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t l = labels[order[i]] - idx->id_base;
    while (j < idx->dead.size() && idx->dead[j] <= l + shift) ++j, ++shift;
    (*rows)[order[i]] = l + shift;
  }
  return VS_OK;
}

// One chunk of an update: the m rows at x (host or device) to the rows hrows.
int update_chunk(vs_index* idx, const int64_t* hrows, const float* x, int64_t m,
                 hipMemcpyKind kind, hipStream_t st) {
  Scratch scr(st);
  const int64_t ld = idx->ld;
  char* sx = nullptr;
  float* snorm = nullptr;
  int64_t* drows = nullptr;
  VS_HIP(scr.alloc((void**)&sx, (size_t)m * idx->rowbytes()), "vs_update_rows: scratch");
  VS_HIP(scr.alloc((void**)&snorm, (size_t)m * sizeof(float)), "vs_update_rows: scratch");
  VS_HIP(scr.alloc((void**)&drows, (size_t)m * sizeof(int64_t)), "vs_update_rows: scratch");
  VS_HIP(hipMemcpyAsync(drows, hrows, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st),
         "vs_update_rows: upload");
  if (idx->esize == 4) {
    if (idx->d != ld)  // the padding columns stay zero
      VS_HIP(hipMemsetAsync(sx, 0, (size_t)m * idx->rowbytes(), st), "vs_update_rows: zero rows");
    VS_HIP(hipMemcpy2DAsync(sx, idx->rowbytes(), x, (size_t)idx->d * sizeof(float),
                            (size_t)idx->d * sizeof(float), (size_t)m, kind, st),
           "vs_update_rows: staging rows");
  } else {
    float* tmp = nullptr;
    VS_HIP(scr.alloc((void**)&tmp, (size_t)m * idx->d * sizeof(float)), "vs_update_rows: scratch");
    VS_HIP(hipMemcpyAsync(tmp, x, (size_t)m * idx->d * sizeof(float), kind, st),
           "vs_update_rows: staging rows");
    VS_HIP(launch_f32_to_bf16(tmp, idx->d, (uint16_t*)sx, ld, m, idx->d, st),
           "vs_update_rows: rounding to bf16");
  }
  VS_HIP(launch_row_norms(sx, idx->esize, ld, 0, m, snorm, st), "vs_update_rows: norms");

  UpdateScatter sc;
  sc.s_codes = sx;
  sc.codes = idx->codes;
  sc.rowbytes = idx->rowbytes();
  sc.s_scal[0] = snorm;
  sc.scal[0] = idx->norms;
  // the planes of the staged block, as derive_plane derives them in place
  const bool aug = idx->l2aug();
  const bool i8 = idx->plane_on[FILTER_I8], b16 = idx->plane_on[FILTER_BF16];
  if (aug && (i8 || b16) && idx->aug_m <= 0)
    return fail(VS_E_HIP, "vs_update_rows: an L2 index with rows and no plane parameters");
  char* splane[2] = {nullptr, nullptr};
  float* srn2[2] = {nullptr, nullptr};
  float* sscale = nullptr;
  float* sanorm[2] = {nullptr, nullptr};  // [FILTER_BF16]: anorm_b, [FILTER_I8]: anorm
  for (int p = 0; p < 2; ++p) {
    if (!idx->plane_on[p]) continue;
    VS_HIP(scr.alloc((void**)&splane[p], (size_t)round_up(m, 256) * idx->planebytes(p)),
           "vs_update_rows: scratch");
    VS_HIP(scr.alloc((void**)&srn2[p], (size_t)m * sizeof(float)), "vs_update_rows: scratch");
    if (aug)
      VS_HIP(scr.alloc((void**)&sanorm[p], (size_t)m * sizeof(float)), "vs_update_rows: scratch");
  }
  if (i8) VS_HIP(scr.alloc((void**)&sscale, (size_t)m * sizeof(float)), "vs_update_rows: scratch");
  if (i8 && aug)
    VS_HIP(launch_quantize_i8_l2aug((const float*)sx, ld, 0, m, idx->aug, snorm,
                                    (int8_t*)splane[FILTER_I8], sscale, srn2[FILTER_I8],
                                    sanorm[FILTER_I8], st),
           "vs_update_rows: int8 L2 filter plane");
  else if (i8)
    VS_HIP(launch_quantize_i8(sx, ld, 0, m, (int8_t*)splane[FILTER_I8], sscale, srn2[FILTER_I8],
                              st, idx->esize),
           "vs_update_rows: int8 filter plane");
  if (b16 && aug) {
    VS_HIP(launch_bf16_plane_l2aug((const float*)sx, ld, 0, m, idx->aug, snorm,
                                   (uint16_t*)splane[FILTER_BF16], srn2[FILTER_BF16],
                                   sanorm[FILTER_BF16], st),
           "vs_update_rows: bf16 L2 filter plane");
  } else if (b16) {
    VS_HIP(launch_bf16_plane((const float*)sx, ld, 0, m, (uint16_t*)splane[FILTER_BF16], st),
           "vs_update_rows: bf16 filter plane");
    VS_HIP(launch_resid_norms((const float*)sx, ld, 0, m, srn2[FILTER_BF16], st),
           "vs_update_rows: residual norms");
  }
  for (int p = 0; p < 2; ++p) {
    if (!idx->plane_on[p]) continue;
    // the new rows' maxima fold into the index's: they only grow, and a maximum
    // left higher than the rows now stored is still a bound
    if (idx->bstats[p])
      VS_HIP(launch_bound_stats(aug ? sanorm[p] : snorm, srn2[p], m, idx->bstats[p], st, true),
             "vs_update_rows: bound maxima");
    sc.s_plane[p] = splane[p];
    sc.plane[p] = idx->fplane[p];
    sc.ldb[p] = idx->planebytes(p);
  }
  if (i8) sc.s_scal[1] = sscale, sc.scal[1] = idx->fscale;
  sc.s_scal[2] = srn2[0], sc.scal[2] = idx->rn2[0];
  sc.s_scal[3] = srn2[1], sc.scal[3] = idx->rn2[1];
  if (aug && i8) sc.s_scal[4] = sanorm[FILTER_I8], sc.scal[4] = idx->anorm;
  if (aug && b16) sc.s_scal[5] = sanorm[FILTER_BF16], sc.scal[5] = idx->anorm_b;
  for (int s = 0; s < UpdateScatter::kScalars; ++s)
    if (!sc.s_scal[s]) sc.scal[s] = nullptr;
  VS_HIP(launch_update_scatter(sc, drows, m, st), "vs_update_rows: scatter");
  return VS_OK;
}

}  // namespace

extern "C" {

int vs_update_rows(vs_index* idx, const int64_t* labels, const float* x, int64_t n, int flags,
                   void* stream) {
  if (!idx) return fail(VS_E_INVALID, "vs_update_rows: null index");
  if (n < 0) return fail(VS_E_INVALID, "vs_update_rows: n < 0");
  if (n == 0) return VS_OK;
  if (!labels) return fail(VS_E_INVALID, "vs_update_rows: null labels");
  if (!x) return fail(VS_E_INVALID, "vs_update_rows: null vectors");
  hipStream_t st = (hipStream_t)stream;
  std::unique_lock<std::shared_mutex> lk(idx->mu);
  std::vector<int64_t> rows;
  int rc = rows_of_labels(idx, labels, n, &rows);
  if (rc) return rc;
  DeviceGuard g(idx->device);
  if (!g.ok) return fail(VS_E_HIP, "vs_update_rows: hipSetDevice failed");
  // searches of this index already queued on other streams read the rows we
  // are about to overwrite.  The generation stays: no row moves, no label changes.
  VS_HIP(wait_readers(idx), "vs_update_rows: drain");
  const hipMemcpyKind kind =
      (flags & VS_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // bounded chunks (64 MiB of fp32 input each, as vs_add stages bf16 rows)
  const int64_t chunk = std::max<int64_t>(1, (int64_t)(64ull << 20) / (idx->d * 4));
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    rc = update_chunk(idx, rows.data() + c0, x + c0 * idx->d, std::min(chunk, n - c0), kind, st);
    if (rc) return rc;
  }
  // the caller may release x as soon as we return
  VS_HIP(hipStreamSynchronize(st), "vs_update_rows: synchronise");
  return VS_OK;
}

}  // extern "C"
