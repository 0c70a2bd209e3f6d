// vs_storage.hip — an index's row storage: which filter planes it keeps and
// how they are derived from the rows, growth, and the compaction of removed
// rows (immediate, or of tombstones at a pack).
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace vs {
namespace host {

// Filter planes of a new fp32 index: int8 + bf16 (the staged engine; an L2
// index's int8 plane holds the augmented rows, vs_index::aug_m).  Env
// VS_FILTER=bf16 | i8 keeps only that plane (A/B).
void planes_for(vs_index* idx) {
  const char* e = getenv("VS_FILTER");
  if (e && strcmp(e, "none") == 0) {  // no planes: the exact fp32 engine alone
    idx->plane_on[FILTER_BF16] = idx->plane_on[FILTER_I8] = false;
    return;
  }
  const bool f32 = idx->esize == 4;
  // bf16 indexes: an int8 plane for inner product (C5: the small-batch filter
  // pass streams 1 B per element instead of the rows' 2; the verification
  // rescores the stored bf16 values)
  const bool i8able = f32 ? (idx->metric == VS_METRIC_INNER_PRODUCT || idx->metric == VS_METRIC_L2)
                          : idx->metric == VS_METRIC_INNER_PRODUCT;
  idx->plane_on[FILTER_BF16] = f32 && !(i8able && e && strcmp(e, "i8") == 0);
  idx->plane_on[FILTER_I8] = i8able && !(e && strcmp(e, "bf16") == 0);
}

// An L2 index without rows forgets its augmentation (vs_reset, or removals
// down to ntotal = 0): the first add after it chooses m, C and nref again.
void reset_l2aug(vs_index* idx) {
  idx->aug_m = 0;
  idx->aug = L2Aug{};
}

// The augmentation of an L2 index's int8 plane, fixed by its first add (rows
// [0, n) in place, their norms too): m extra columns and C (l2aug_params),
// then the plane reallocated at ld + m bytes per row (it holds no row yet).
static int choose_l2aug(vs_index* idx, int64_t n, hipStream_t st) {
  L2Aug g;
  VS_HIP(l2aug_params((const float*)idx->codes, idx->ld, 0, n, idx->norms, &g, st),
         "vs: L2 plane parameters");
  VS_HIP(hipStreamSynchronize(st), "vs: L2 plane");
  if (!idx->plane_on[FILTER_I8]) {  // the bf16 plane's width does not depend on them
    idx->aug_m = g.m;
    idx->aug = g;
    return VS_OK;
  }
  VS_HIP(wait_readers(idx), "vs: L2 plane");
  if (idx->fplane[FILTER_I8]) (void)hipFree(idx->fplane[FILTER_I8]);
  idx->fplane[FILTER_I8] = nullptr;
  idx->aug_m = g.m;
  idx->aug = g;
  hipError_t e = hipMalloc(&idx->fplane[FILTER_I8], (size_t)idx->capacity * idx->planebytes(FILTER_I8));
  if (e != hipSuccess) {  // no room for the wider plane: the index goes on without it
    (void)hipGetLastError();
    idx->fplane[FILTER_I8] = nullptr;
    idx->plane_on[FILTER_I8] = false;
    return VS_OK;
  }
  VS_HIP(launch_plane_zero_rows(idx->fplane[FILTER_I8], idx->planebytes(FILTER_I8), 0,
                                idx->capacity, st),
         "vs: L2 plane");
  return VS_OK;
}

// The norms a plane's bound maxima take: |x'|^2 for an L2 index's augmented
// int8 plane, the stored |x|^2 otherwise.
static const float* plane_norms(const vs_index* idx, int p) {
  if (!idx->l2aug()) return idx->norms;
  return p == FILTER_I8 ? idx->anorm : idx->anorm_b;
}

// The filter plane and residual norms of fp32 rows [r0, r0+n) (after the rows
// and their norms are in place).
int derive_plane(vs_index* idx, int64_t r0, int64_t n, hipStream_t st, bool appended) {
  if (n <= 0 || (idx->esize != 4 && !idx->plane_on[FILTER_I8])) return VS_OK;
  for (int p = 0; p < 2; ++p) {
    if (!idx->plane_on[p] || idx->bstats[p]) continue;
    VS_HIP(hipMalloc(&idx->bstats[p], 4 * sizeof(unsigned)), "vs: bound maxima");
    VS_HIP(hipMemsetAsync(idx->bstats[p], 0, 4 * sizeof(unsigned), st), "vs: bound maxima");
  }
  // An add that at least doubles an L2 index re-derives its augmentation over
  // every row (a few first rows would otherwise fix m, C and nref for good, and
  // rows of other norms get coarse codes and a wide bound); amortised O(1) per
  // row, like the storage's own growth.
  if (appended && idx->l2aug() && idx->aug_m > 0 && r0 > 0 && n >= r0) {
    reset_l2aug(idx);
    for (int p = 0; p < 2; ++p)
      if (idx->bstats[p])
        VS_HIP(hipMemsetAsync(idx->bstats[p], 0, 4 * sizeof(unsigned), st), "vs: bound maxima");
  }
  if (idx->l2aug() && idx->aug_m == 0 && (idx->plane_on[FILTER_I8] || idx->plane_on[FILTER_BF16])) {
    // the first rows fix the augmentation (and the int8 plane's width)
    const int64_t n0 = r0 + n;
    int rc = choose_l2aug(idx, n0, st);
    if (rc) return rc;
    r0 = 0;
    n = n0;
  }
  if (idx->plane_on[FILTER_I8] && idx->l2aug()) {
    if (idx->plane_on[FILTER_I8])
      VS_HIP(launch_quantize_i8_l2aug((const float*)idx->codes, idx->ld, r0, n, idx->aug,
                                      idx->norms, (int8_t*)idx->fplane[FILTER_I8], idx->fscale,
                                      idx->rn2[FILTER_I8], idx->anorm, st),
             "vs: int8 L2 filter plane");
  } else if (idx->plane_on[FILTER_I8]) {
    VS_HIP(launch_quantize_i8(idx->codes, idx->ld, r0, n, (int8_t*)idx->fplane[FILTER_I8],
                              idx->fscale, idx->rn2[FILTER_I8], st, idx->esize),
           "vs: int8 filter plane");
  }
  if (idx->plane_on[FILTER_BF16] && idx->l2aug()) {
    VS_HIP(launch_bf16_plane_l2aug((const float*)idx->codes, idx->ld, r0, n, idx->aug, idx->norms,
                                   (uint16_t*)idx->fplane[FILTER_BF16], idx->rn2[FILTER_BF16],
                                   idx->anorm_b, st),
           "vs: bf16 L2 filter plane");
  } else if (idx->plane_on[FILTER_BF16]) {
    VS_HIP(launch_bf16_plane((const float*)idx->codes, idx->ld, r0, n,
                             (uint16_t*)idx->fplane[FILTER_BF16], st),
           "vs: bf16 filter plane");
    VS_HIP(launch_resid_norms((const float*)idx->codes, idx->ld, r0, n, idx->rn2[FILTER_BF16], st),
           "vs: residual norms");
  }
  // the new rows' maxima fold into the index's (they only grow on add)
  for (int p = 0; p < 2; ++p)
    if (idx->plane_on[p])
      VS_HIP(launch_bound_stats(plane_norms(idx, p) + r0, idx->rn2[p] + r0, n, idx->bstats[p], st,
                                true),
             "vs: bound maxima");
  return VS_OK;
}

// Grows storage to hold `rows` rows (plus the tile slack), preserving content.
int ensure_capacity(vs_index* idx, int64_t rows, hipStream_t st) {
  const int64_t need = round_up(rows + 256, kRowPad);  // 256-row query tiles of self-joins
  if (need <= idx->capacity) return VS_OK;
  int64_t cap = std::max(need, round_up(idx->capacity + idx->capacity / 2, kRowPad));
  char* codes = nullptr;
  float* norms = nullptr;
  char* fplane[2] = {nullptr, nullptr};
  float* rn2[2] = {nullptr, nullptr};
  float* fscale = nullptr;
  float* anorm = nullptr;
  float* anorm_b = nullptr;
  // the planes the new storage keeps: committed to the index only once the
  // allocation succeeded (a failed growth leaves the index as it was)
  bool on[2] = {idx->plane_on[0], idx->plane_on[1]};
  auto release = [&]() {
    if (codes) (void)hipFree(codes);
    if (norms) (void)hipFree(norms);
    for (int p = 0; p < 2; ++p) {
      if (fplane[p]) (void)hipFree(fplane[p]);
      if (rn2[p]) (void)hipFree(rn2[p]);
      fplane[p] = nullptr;
      rn2[p] = nullptr;
    }
    if (fscale) (void)hipFree(fscale);
    if (anorm) (void)hipFree(anorm);
    if (anorm_b) (void)hipFree(anorm_b);
    codes = nullptr;
    norms = nullptr;
    fscale = nullptr;
    anorm = nullptr;
    anorm_b = nullptr;
  };
  // test hook (tests/test_gpu_planes.py): VS_TEST_PLANE_OOM=1 fails the bf16
  // plane's allocation as a full HBM would, 2 every plane's
  static const int plane_oom = [] {
    const char* v = getenv("VS_TEST_PLANE_OOM");
    return v ? atoi(v) : 0;
  }();
  auto allocate = [&](int64_t c) -> hipError_t {
    hipError_t e = hipMalloc(&codes, (size_t)c * idx->rowbytes());
    if (e == hipSuccess) e = hipMalloc(&norms, (size_t)c * sizeof(float));
    for (int p = 0; p < 2; ++p) {
      if (e == hipSuccess && on[p] && (plane_oom >= 2 || (plane_oom == 1 && p == FILTER_BF16)))
        e = hipErrorOutOfMemory;
      if (e == hipSuccess && on[p]) e = hipMalloc(&fplane[p], (size_t)c * idx->planebytes(p));
      if (e == hipSuccess && on[p]) e = hipMalloc(&rn2[p], (size_t)c * sizeof(float));
    }
    if (e == hipSuccess && on[FILTER_I8])
      e = hipMalloc(&fscale, (size_t)c * sizeof(float));
    if (e == hipSuccess && on[FILTER_I8] && idx->l2aug())
      e = hipMalloc(&anorm, (size_t)c * sizeof(float));
    if (e == hipSuccess && on[FILTER_BF16] && idx->l2aug())
      e = hipMalloc(&anorm_b, (size_t)c * sizeof(float));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      release();
    }
    return e;
  };
  hipError_t e = allocate(cap);
  if (e != hipSuccess) scratch_trim(), e = allocate(cap);  // cached scratch chunks first
  if (e != hipSuccess) {  // retry without the growth headroom
    cap = need;
    e = allocate(cap);
  }
  // Still short of HBM: give up filter planes rather than rows (an fp32 inner-
  // product index holds 10 B per element with both planes, 7 with int8 only,
  // 4 without; searches then use the plane that remains, or the exact fp32
  // engine): bf16 first, then every plane.
  if (e != hipSuccess && on[FILTER_BF16] && on[FILTER_I8]) {
    on[FILTER_BF16] = false;
    e = allocate(cap);
  }
  if (e != hipSuccess && (on[FILTER_BF16] || on[FILTER_I8])) {
    on[FILTER_BF16] = on[FILTER_I8] = false;
    e = allocate(cap);
  }
  if (e != hipSuccess) return hip_fail(e, "vs: allocating row storage");
  const bool i8 = on[FILTER_I8];
  // zero every tail (tile reads past ntotal must see zeros, never NaN garbage)
  const int64_t keep = idx->ntotal;
  VS_HIP(hipMemsetAsync(codes + keep * idx->rowbytes(), 0, (size_t)(cap - keep) * idx->rowbytes(),
                        st),
         "vs: zeroing storage");
  VS_HIP(hipMemsetAsync(norms + keep, 0, (size_t)(cap - keep) * sizeof(float), st),
         "vs: zeroing norms");
  for (int p = 0; p < 2; ++p) {
    if (!on[p]) continue;
    VS_HIP(hipMemsetAsync(rn2[p] + keep, 0, (size_t)(cap - keep) * sizeof(float), st),
           "vs: zeroing residual norms");
  }
  if (i8)
    VS_HIP(hipMemsetAsync(fscale + keep, 0, (size_t)(cap - keep) * sizeof(float), st),
           "vs: zeroing scales");
  if (anorm)
    VS_HIP(hipMemsetAsync(anorm + keep, 0, (size_t)(cap - keep) * sizeof(float), st),
           "vs: zeroing augmented norms");
  if (anorm_b)
    VS_HIP(hipMemsetAsync(anorm_b + keep, 0, (size_t)(cap - keep) * sizeof(float), st),
           "vs: zeroing augmented norms");
  if (idx->codes && keep > 0) {
    VS_HIP(hipMemcpyAsync(codes, idx->codes, (size_t)keep * idx->rowbytes(),
                          hipMemcpyDeviceToDevice, st),
           "vs: copying storage");
    VS_HIP(hipMemcpyAsync(norms, idx->norms, (size_t)keep * sizeof(float),
                          hipMemcpyDeviceToDevice, st),
           "vs: copying norms");
    for (int p = 0; p < 2; ++p) {
      if (!on[p]) continue;
      // tile-major planes: rows [0, keep) are the first ceil(keep / 256) tiles
      VS_HIP(hipMemcpyAsync(fplane[p], idx->fplane[p],
                            (size_t)round_up(keep, 256) * idx->planebytes(p),
                            hipMemcpyDeviceToDevice, st),
             "vs: copying plane");
      VS_HIP(hipMemcpyAsync(rn2[p], idx->rn2[p], (size_t)keep * sizeof(float),
                            hipMemcpyDeviceToDevice, st),
             "vs: copying residual norms");
    }
    if (i8)
      VS_HIP(hipMemcpyAsync(fscale, idx->fscale, (size_t)keep * sizeof(float),
                            hipMemcpyDeviceToDevice, st),
             "vs: copying scales");
    if (anorm && idx->anorm)
      VS_HIP(hipMemcpyAsync(anorm, idx->anorm, (size_t)keep * sizeof(float),
                            hipMemcpyDeviceToDevice, st),
             "vs: copying augmented norms");
    if (anorm_b && idx->anorm_b)
      VS_HIP(hipMemcpyAsync(anorm_b, idx->anorm_b, (size_t)keep * sizeof(float),
                            hipMemcpyDeviceToDevice, st),
             "vs: copying augmented norms");
  }
  // the planes' rows past the kept ones read zeros (after the prefix copy,
  // which brings whole tiles)
  for (int p = 0; p < 2; ++p)
    if (on[p])
      VS_HIP(launch_plane_zero_rows(fplane[p], idx->planebytes(p), keep, cap - keep, st),
             "vs: zeroing plane");
  // The copies above, and searches of this index still in flight (any
  // stream), read the old storage; other indexes' work is not waited for.
  VS_HIP(hipStreamSynchronize(st), "vs: storage growth");
  VS_HIP(wait_readers(idx), "vs: storage growth");
  free_storage(idx);
  if (on[0] != idx->plane_on[0] || on[1] != idx->plane_on[1]) {
    // a plane lost to a memory shortage: said once on stderr and kept for
    // vs_notice (searches stay exact; the engines that remain are slower)
    char buf[256];
    snprintf(buf, sizeof(buf),
             "vsearch: HBM short at %lld rows: filter planes dropped (int8 %s, bf16 %s); "
             "searches use %s",
             (long long)cap, on[FILTER_I8] ? "kept" : "dropped",
             on[FILTER_BF16] ? "kept" : "dropped",
             on[FILTER_I8] || on[FILTER_BF16] ? "the remaining plane" : "the exact fp32 engine");
    idx->notice = buf;
    fprintf(stderr, "%s\n", buf);
  }
  idx->plane_on[0] = on[0];
  idx->plane_on[1] = on[1];
  idx->codes = codes;
  idx->norms = norms;
  for (int p = 0; p < 2; ++p) {
    idx->fplane[p] = fplane[p];
    idx->rn2[p] = rn2[p];
  }
  idx->fscale = fscale;
  idx->anorm = anorm;
  idx->anorm_b = anorm_b;
  idx->capacity = cap;
  return VS_OK;
}

void free_storage(vs_index* idx) {
  if (idx->codes) (void)hipFree(idx->codes);
  if (idx->norms) (void)hipFree(idx->norms);
  for (int p = 0; p < 2; ++p) {
    if (idx->fplane[p]) (void)hipFree(idx->fplane[p]);
    if (idx->rn2[p]) (void)hipFree(idx->rn2[p]);
    idx->fplane[p] = nullptr;
    idx->rn2[p] = nullptr;
  }
  if (idx->fscale) (void)hipFree(idx->fscale);
  if (idx->anorm) (void)hipFree(idx->anorm);
  if (idx->anorm_b) (void)hipFree(idx->anorm_b);
  idx->anorm_b = nullptr;
  idx->codes = nullptr;
  idx->norms = nullptr;
  idx->fscale = nullptr;
  idx->anorm = nullptr;
  idx->capacity = 0;
}

// Room for n more rows: tombstones are packed first when the rows in place
// would otherwise outgrow the storage, then the storage grows if it must.
int make_room(vs_index* idx, int64_t n, hipStream_t st) {
  if (!idx->dead.empty() && idx->ntotal + n + 256 > idx->capacity) {
    const int rc = pack_dead(idx);
    if (rc) return rc;
  }
  return ensure_capacity(idx, idx->ntotal + n, st);
}

// Stable compaction of the sorted physical rows `rm` out of the index (rows,
// norms, filter planes re-derived over the moved rows), on the writer stream
// `st`, after the index's readers have drained; synchronises.
int compact_rows(vs_index* idx, const std::vector<int64_t>& rm, hipStream_t st) {
  const int64_t nrem = (int64_t)rm.size();
  if (nrem == 0) return VS_OK;
  Scratch scr(st);
  int64_t* drm = nullptr;
  VS_HIP(scr.alloc((void**)&drm, (size_t)nrem * sizeof(int64_t)), "vs_remove_ids: scratch");
  VS_HIP(hipMemcpyAsync(drm, rm.data(), (size_t)nrem * sizeof(int64_t), hipMemcpyHostToDevice, st),
         "vs_remove_ids: upload");
  // Chunked stable compaction from the first removed row on.  A chunk whose
  // rows move down by at least its own length (`before`, the removed rows
  // below it, >= its row count) is packed straight to its final position: its
  // destinations lie below its sources, in rows earlier chunks have already
  // consumed (stream order).  Otherwise (near the first removed row, where the
  // shift is small) the kept rows are packed into scratch, then copied down.
  // Once the shift reaches kDirectMin rows, chunks are cut to the shift so
  // every later chunk takes the direct path (half the bytes moved).
  const int64_t chunk = std::max<int64_t>(1024, (int64_t)(256ull << 20) / idx->rowbytes());
  constexpr int64_t kDirectMin = 16384;
  char* tmp = nullptr;
  float* tmpn = nullptr;
  const int64_t first = rm[0];
  for (int64_t s0 = first, cn = 0; s0 < idx->ntotal; s0 += cn) {
    const int64_t before = std::lower_bound(rm.begin(), rm.end(), s0) - rm.begin();
    cn = std::min(chunk, idx->ntotal - s0);
    const bool direct = before >= cn || before >= kDirectMin;
    if (direct) cn = std::min(cn, before);
    const int64_t in_chunk = std::lower_bound(rm.begin(), rm.end(), s0 + cn) - rm.begin() - before;
    const int64_t kept = cn - in_chunk;
    const int64_t dst = s0 - before;
    if (direct) {
      VS_HIP(launch_gather_kept(idx->codes, idx->norms, idx->rowbytes(), s0, cn, drm + before,
                                in_chunk, idx->row(dst), idx->norms + dst, st),
             "vs_remove_ids: move rows");
      continue;
    }
    if (!tmp) {
      VS_HIP(scr.alloc((void**)&tmp, (size_t)chunk * idx->rowbytes()), "vs_remove_ids: scratch");
      VS_HIP(scr.alloc((void**)&tmpn, (size_t)chunk * sizeof(float)), "vs_remove_ids: scratch");
    }
    VS_HIP(launch_gather_kept(idx->codes, idx->norms, idx->rowbytes(), s0, cn, drm + before,
                              in_chunk, tmp, tmpn, st),
           "vs_remove_ids: gather");
    if (kept > 0) {
      VS_HIP(hipMemcpyAsync(idx->row(dst), tmp, (size_t)kept * idx->rowbytes(),
                            hipMemcpyDeviceToDevice, st),
             "vs_remove_ids: move rows");
      VS_HIP(hipMemcpyAsync(idx->norms + dst, tmpn, (size_t)kept * sizeof(float),
                            hipMemcpyDeviceToDevice, st),
             "vs_remove_ids: move norms");
    }
  }
  const int64_t nt = idx->ntotal - nrem;
  VS_HIP(hipMemsetAsync(idx->row(nt), 0, (size_t)nrem * idx->rowbytes(), st),
         "vs_remove_ids: zero tail");
  VS_HIP(hipMemsetAsync(idx->norms + nt, 0, (size_t)nrem * sizeof(float), st),
         "vs_remove_ids: zero tail");
  // the filter planes are re-derived from the moved rows (one pass over
  // them), and their tails zeroed like the rows'; the bound maxima are
  // recomputed over the remaining rows (a removal can lower them)
  int rc = derive_plane(idx, first, nt - first, st);
  if (rc) return rc;
  for (int p = 0; p < 2; ++p)
    if (idx->plane_on[p] && idx->bstats[p])
      VS_HIP(launch_bound_stats(plane_norms(idx, p), idx->rn2[p], nt, idx->bstats[p], st),
             "vs_remove_ids: bound maxima");
  for (int p = 0; p < 2; ++p) {
    if (!idx->plane_on[p]) continue;
    VS_HIP(launch_plane_zero_rows(idx->fplane[p], idx->planebytes(p), nt, nrem, st),
           "vs_remove_ids: zero tail");
    VS_HIP(hipMemsetAsync(idx->rn2[p] + nt, 0, (size_t)nrem * sizeof(float), st),
           "vs_remove_ids: zero tail");
  }
  if (idx->fscale)
    VS_HIP(hipMemsetAsync(idx->fscale + nt, 0, (size_t)nrem * sizeof(float), st),
           "vs_remove_ids: zero tail");
  if (idx->anorm)
    VS_HIP(hipMemsetAsync(idx->anorm + nt, 0, (size_t)nrem * sizeof(float), st),
           "vs_remove_ids: zero tail");
  if (idx->anorm_b)
    VS_HIP(hipMemsetAsync(idx->anorm_b + nt, 0, (size_t)nrem * sizeof(float), st),
           "vs_remove_ids: zero tail");
  VS_HIP(hipStreamSynchronize(st), "vs_remove_ids: synchronise");
  idx->ntotal = nt;
  return VS_OK;
}

// Tombstoned rows -> packed storage (the same compaction as an immediate
// removal); the labels do not change.
int pack_dead(vs_index* idx) {
  if (idx->dead.empty()) return VS_OK;
  DeviceGuard g(idx->device);
  VS_HIP(wait_readers(idx), "vs: pack");
  hipStream_t st = nullptr;
  VS_HIP(writer_stream(idx, &st), "vs: pack");
  ++idx->gen;
  const int rc = compact_rows(idx, idx->dead, st);
  if (rc) return rc;
  idx->dead.clear();
  return VS_OK;
}

// Dead fraction at which a removal packs the tombstones (1 / kPackDen of the
// rows in place; env VS_PACK_DEN overrides, 1 = pack at every removal).  A
// dead row costs every search its bytes until the pack, a pack moves every
// row after the first dead one: at C5's 1 % per mutation round a pack comes
// every ~6 rounds.
int pack_den() {
  const char* e = getenv("VS_PACK_DEN");
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : 16;
}

// Live label l -> its row in place (the sorted dead list skipped).
int64_t row_of_label(const vs_index* idx, int64_t l) {
  int64_t p = l;
  for (int64_t d : idx->dead) {
    if (d <= p) ++p;
    else break;
  }
  return p;
}

}  // namespace host
}  // namespace vs
