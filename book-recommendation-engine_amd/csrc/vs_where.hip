// vs_where.hip — where searches (vs_search_where; DESIGN.md "Where searches"):
// exact top-k over the rows that pass a per-query attribute predicate.
//
// A predicate (WherePred, vs_internal.h) is up to four closed float ranges
// over the numeric columns and three 64-bit tag masks; the attributes
// (WhereAttrs) are indexed by the row in place.  where_pass (vs_where_device.h)
// is the one definition every kernel of this unit tests with.
//
// Kernels:
//  - attrs_spread: the attributes by label -> by row in place through the
//    sorted dead list (as sel_row_bits, vs_select.hip);
//  - attrs_count: the live rows that pass each of nq predicates, one stream
//    over the by-row arrays;
//  - where_drop: route A's stable drop of a raw window's entries whose row
//    fails the slot's predicate (sel_drop with one predicate per slot and
//    distinct_collapse's unsettled flag);
//  - route B: gemm_topk_pred / gemv_topk_pred (vs_pred_scan.h, the text the
//    boosted scan shares) without specs, behind launch_gemm_topk_where /
//    launch_gemv_topk_where.
#include <algorithm>

#include "vs_pred_scan.h"

namespace vs {

__device__ __forceinline__ int where_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------------------
// One thread per row in place: its position among the live rows is its label.
__global__ __launch_bounds__(256) void attrs_spread_kernel(
    const float* __restrict__ lcols, const unsigned long long* __restrict__ ltags, int64_t nlab,
    int ncol, const int64_t* __restrict__ dead, int64_t ndead, int64_t ntotal,
    float* __restrict__ rcols, unsigned long long* __restrict__ rtags, uint8_t* __restrict__ live) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= ntotal) return;
  int64_t lo = 0, hi = ndead;  // dead rows below r
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (dead[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  const bool alive = !(lo < ndead && dead[lo] == r) && r - lo < nlab;
  const int64_t p = r - lo;
  live[r] = alive ? 1 : 0;
  for (int c = 0; c < ncol; ++c)
    rcols[(int64_t)c * ntotal + r] = alive ? lcols[(int64_t)c * nlab + p] : __int_as_float(0x7fc00000);
  if (rtags) rtags[r] = alive ? ltags[p] : 0ull;
}

hipError_t launch_attrs_spread(const float* lcols, const unsigned long long* ltags, int64_t nlab,
                               int ncol, const int64_t* dead, int64_t ndead, int64_t ntotal,
                               float* rcols, unsigned long long* rtags, uint8_t* live,
                               hipStream_t st) {
  if (ntotal < 1 || ncol < 0 || ncol > kWhereMaxCols || ndead < 1 || !dead || !live ||
      (ncol > 0 && (!lcols || !rcols)) || ((ltags == nullptr) != (rtags == nullptr)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(attrs_spread_kernel, dim3((unsigned)((ntotal + 255) / 256)), dim3(256), 0, st,
                     lcols, ltags, nlab, ncol, dead, ndead, ntotal, rcols, rtags, live);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Counts: blockIdx.y owns the predicates [8 y, 8 y + 8), held in LDS; the
// blocks of one y stream the rows once (grid-stride), a thread keeps its 8
// counts in registers (32 of them cost the kernel its occupancy: 255 VGPRs),
// a wave adds its sums to out[q].
constexpr int kWhereCountQ = 8;

__global__ __launch_bounds__(256) void attrs_count_kernel(WhereAttrs at, int64_t nrows,
                                                          const WherePred* __restrict__ preds,
                                                          int nq,
                                                          unsigned long long* __restrict__ out) {
  __shared__ WherePred sp[kWhereCountQ];
  const int q0 = blockIdx.y * kWhereCountQ;
  const int nc = min(kWhereCountQ, nq - q0);
  for (int i = threadIdx.x; i < nc * (int)(sizeof(WherePred) / 4); i += 256)
    ((unsigned*)sp)[i] = ((const unsigned*)(preds + q0))[i];
  __syncthreads();
  int cnt[kWhereCountQ];
#pragma unroll
  for (int q = 0; q < kWhereCountQ; ++q) cnt[q] = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nrows;
       r += (int64_t)gridDim.x * 256) {
    if (at.live && !at.live[r]) continue;
    float v[kWhereMaxCols];
#pragma unroll
    for (int c = 0; c < kWhereMaxCols; ++c) v[c] = c < at.ncol ? at.cols[(int64_t)c * at.stride + r] : 0.0f;
    const unsigned long long t = at.tags ? at.tags[r] : 0ull;
#pragma unroll
    for (int q = 0; q < kWhereCountQ; ++q) {
      if (q < nc) {
        const WherePred& p = sp[q];
        bool ok = p.on != 0;
#pragma unroll
        for (int c = 0; c < kWhereMaxCols; ++c)
          if (c < at.ncol && ((p.cmask >> c) & 1u)) ok = ok && p.lo[c] <= v[c] && v[c] <= p.hi[c];
        ok = ok && (p.any_of == 0ull || (t & p.any_of) != 0ull) && (t & p.all_of) == p.all_of &&
             (t & p.none_of) == 0ull;
        cnt[q] += ok ? 1 : 0;
      }
    }
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < kWhereCountQ; ++q) {
    if (q < nc) {
      const int s = where_wave_sum_int(cnt[q]);
      if (lane == 0 && s) atomicAdd(out + q0 + q, (unsigned long long)s);
    }
  }
}

hipError_t launch_attrs_count(const WhereAttrs& at, int64_t nrows, const WherePred* preds, int nq,
                              unsigned long long* out, hipStream_t st) {
  if (nq < 0 || nrows < 0 || !out || (nq > 0 && !preds)) return hipErrorInvalidValue;
  if (nq == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)nq * sizeof(unsigned long long), st);
  if (e != hipSuccess || nrows == 0) return e;
  const unsigned bx = (unsigned)std::min<int64_t>(1024, (nrows + 255) / 256);
  const unsigned by = (unsigned)((nq + kWhereCountQ - 1) / kWhereCountQ);
  if (by > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attrs_count_kernel, dim3(bx, by), dim3(256), 0, st, at, nrows, preds, nq, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Route A: one wave per slot s of a round's batch.  Din / Iin [ns][w] are the
// raw entries as the engine wrote them (ascending (key, label), labels = row +
// id_base, -1 after the end); the slot's query is q = qmap ? qmap[s] : s and
// its predicate preds[q].  The entries whose row passes go out in order, at
// most `need` of them, as the first entries of row s of Dout / Iout
// ([ns][kout], padded with the empty result); unsettled[q] = the window was
// too short: fewer than `need` kept, no -1 entry seen and not w_is_all.
__global__ __launch_bounds__(64) void where_drop_kernel(
    int asc, const float* __restrict__ Din, const int64_t* __restrict__ Iin, int w, WhereAttrs at,
    const WherePred* __restrict__ preds, const int* __restrict__ qmap, int64_t id_base, int need,
    int w_is_all, float* __restrict__ Dout, int64_t* __restrict__ Iout, int kout,
    int* __restrict__ unsettled) {
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int q = qmap ? qmap[s] : (int)s;
  const WherePred p = preds[q];
  int kept = 0;
  bool end_seen = false;
  for (int j0 = 0; j0 < w && kept < need && !end_seen; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false, end = false;
    float sc = 0.0f;
    int64_t id = -1;
    if (j < w) {
      id = Iin[s * w + j];
      sc = Din[s * w + j];
      if (id >= 0) keep = where_pass(p, at, id - id_base);
      else end = true;
    }
    const unsigned long long m = __ballot(keep);
    end_seen = __ballot(end) != 0ull;
    const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < need && pos < kout) {
      Dout[s * kout + pos] = sc;
      Iout[s * kout + pos] = id;
    }
    kept += __popcll(m);
  }
  for (int j = min(min(kept, need), kout) + lane; j < kout; j += 64) {
    Dout[s * kout + j] = asc ? FLT_MAX : -FLT_MAX;
    Iout[s * kout + j] = -1;
  }
  if (lane == 0) unsettled[q] = (kept >= need || end_seen || w_is_all) ? 0 : 1;
}

hipError_t launch_where_drop(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                             const WhereAttrs& at, const WherePred* preds, const int* qmap,
                             int64_t id_base, int need, bool w_is_all, float* Dout, int64_t* Iout,
                             int kout, int* unsettled, hipStream_t st) {
  if (ns < 0 || w < 1 || kout < 1 || need < 1 || !Din || !Iin || !preds || !Dout || !Iout ||
      !unsettled)
    return hipErrorInvalidValue;
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(where_drop_kernel, dim3(ns), dim3(64), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, w, at, preds, qmap,
                     id_base, need, w_is_all ? 1 : 0, Dout, Iout, kout, unsettled);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Route B: this unit's instantiations of the predicated scan (vs_pred_scan.h),
// ranking by the key.
hipError_t launch_gemm_topk_where(int mode, const GemmWhereArgs& a, Partials part,
                                  hipStream_t st) {
  return launch_gemm_topk_pred(mode, a, part, st);
}

hipError_t launch_gemv_topk_where(int mode, int nq, const GemvWhereArgs& a, Partials part,
                                  hipStream_t st) {
  return launch_gemv_topk_pred(mode, nq, a, part, st);
}

}  // namespace vs
