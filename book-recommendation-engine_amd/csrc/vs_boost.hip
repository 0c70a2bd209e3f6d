// vs_boost.hip — boosted searches (vs_search_boost; DESIGN.md "Boosted
// searches"): exact top-k by final_key = fl32(key - b(q, r)), b a per-query
// function of the row's attributes (boost_value, vs_boost_value.h).
//
// Kernels:
//  - boost_rerank: route A's re-rank of a raw window, with the test that
//    proves the window sufficient;
//  - route B: gemm_topk_pred / gemv_topk_pred (vs_pred_scan.h, the text the
//    where scan shares) with the queries' specs, so that lists, floors and
//    partials hold final keys, behind launch_gemm_topk_boost /
//    launch_gemv_topk_boost.
// This unit is built with a correctly rounded division (csrc/Makefile).
#include <algorithm>

#include "vs_pred_scan.h"

namespace vs {

// ---------------------------------------------------------------------------
// Route A: one workgroup per slot s of a round's batch.  Din / Iin [ns][w] are
// the raw entries as the engine wrote them with raw = 1 (ascending (key,
// label), labels = row + id_base, -1 after the end), w <= 1023, P = w padded
// to a power of two.  An entry whose row fails the slot's predicate is dropped
// (its LDS entry sorts last); the others get their final key, an LDS bitonic
// sort orders (final_key, label), and the first k go out.
//
// The proof of sufficiency.  Let (K_w, l_w) be the window's last real entry.
// A live row outside the window has a raw (key, label) above it, so key >= K_w;
// b <= U and rounded subtraction is monotone in both operands, so its final
// key fl32(key - b) >= fl32(K_w - U).  If k entries were kept and
// final_key[k-1] < fl32(K_w - U) (strictly: an outside row that ties could
// carry a lower label), no outside row can enter the first k: the slot is
// settled.  It is settled too when the window held every row (a -1 entry, or
// w_is_all).  Otherwise state[q] = 1, or 2 when the deficit final_key[k-1] -
// fl32(K_w - U) exceeds giveup * (K_w - K_0): a longer window is then unlikely
// to settle it (a cost rule only; the scan answers those queries exactly).
__global__ __launch_bounds__(256) void boost_rerank_kernel(
    int asc, const float* __restrict__ Din, const int64_t* __restrict__ Iin, int w, int P,
    WhereAttrs at, const WherePred* __restrict__ preds, const BoostSpec* __restrict__ specs,
    const int* __restrict__ qmap, int64_t id_base, int k, int w_is_all, float giveup,
    float* __restrict__ Dout, int64_t* __restrict__ Iout, int* __restrict__ state,
    float* __restrict__ deficit, float* __restrict__ spread) {
  __shared__ float sk[1024];
  __shared__ long long si[1024];
  __shared__ int s_end, s_real, s_kept;
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int q = qmap ? qmap[s] : (int)s;
  const WherePred p = preds[q];
  const BoostSpec sp = specs[q];
  if (tid == 0) {
    s_end = 0;
    s_real = 0;
    s_kept = 0;
  }
  __syncthreads();
  for (int j = tid; j < P; j += 256) {
    float key = INFINITY;
    long long id = LLONG_MAX;
    if (j < w) {
      const int64_t lab = Iin[s * w + j];
      if (lab >= 0) {
        atomicMax(&s_real, j + 1);
        const int64_t row = lab - id_base;
        if (where_pass(p, at, row)) {
          const float d = Din[s * w + j];
          key = boost_final(asc ? d : -d, boost_of_row(sp, at, row));
          id = lab;
          atomicAdd(&s_kept, 1);
        }
      } else {
        s_end = 1;
      }
    }
    sk[j] = key;
    si[j] = id;
  }
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (P >> 1); i += 256) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const float ka = sk[lo], kb = sk[hi];
        const long long ia = si[lo], ib = si[hi];
        const bool gt = lex_less(kb, ib, ka, ia);  // (lo) after (hi)
        if (gt == up) {
          sk[lo] = kb;
          sk[hi] = ka;
          si[lo] = ib;
          si[hi] = ia;
        }
      }
    }
  }
  __syncthreads();
  const int kept = s_kept;
  for (int j = tid; j < k; j += 256) {
    const bool have = j < kept;  // (kept <= w <= P)
    Dout[s * k + j] = have ? (asc ? sk[j] : -sk[j]) : (asc ? FLT_MAX : -FLT_MAX);
    Iout[s * k + j] = have ? (int64_t)si[j] : -1;
  }
  if (tid == 0) {
    const int nreal = s_real;
    int st = 0;
    float def = 0.0f, spr = 0.0f;
    if (!(s_end || w_is_all || nreal < w)) {
      const float d0 = Din[s * w], dw = Din[s * w + nreal - 1];
      const float K0 = asc ? d0 : -d0, Kw = asc ? dw : -dw;
      const float bound = boost_final(Kw, sp.U);
      spr = Kw - K0;
      def = kept >= k ? sk[k - 1] - bound : INFINITY;
      if (!(kept >= k && sk[k - 1] < bound)) st = (giveup >= 0.0f && def > giveup * spr) ? 2 : 1;
    }
    state[q] = st;
    if (deficit) deficit[q] = def;
    if (spread) spread[q] = spr;
  }
}

hipError_t launch_boost_rerank(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                               const WhereAttrs& at, const WherePred* preds,
                               const BoostSpec* specs, const int* qmap, int64_t id_base, int k,
                               bool w_is_all, float giveup, float* Dout, int64_t* Iout,
                               int* state, float* deficit, float* spread, hipStream_t st) {
  if (ns < 0 || w < 1 || w > kBoostMaxWindow || k < 1 || !Din || !Iin || !preds || !specs ||
      !Dout || !Iout || !state)
    return hipErrorInvalidValue;
  if (ns == 0) return hipSuccess;
  int P = 2;
  while (P < w) P <<= 1;
  hipLaunchKernelGGL(boost_rerank_kernel, dim3(ns), dim3(256), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, w, P, at, preds,
                     specs, qmap, id_base, k, w_is_all ? 1 : 0, giveup, Dout, Iout, state, deficit,
                     spread);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Route B: this unit's instantiations of the predicated scan (vs_pred_scan.h),
// ranking by the final key (a.specs given).
hipError_t launch_gemm_topk_boost(int mode, const GemmWhereArgs& a, Partials part,
                                  hipStream_t st) {
  return launch_gemm_topk_pred(mode, a, part, st, a.specs);
}

hipError_t launch_gemv_topk_boost(int mode, int nq, const GemvWhereArgs& a, Partials part,
                                  hipStream_t st) {
  return launch_gemv_topk_pred(mode, nq, a, part, st, a.specs);
}

}  // namespace vs
