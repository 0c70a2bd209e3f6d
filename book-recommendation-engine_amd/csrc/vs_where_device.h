// vs_where_device.h — the per-row tests that the predicated kernels of
// vs_where.hip and vs_boost.hip share: one definition of "row r passes
// predicate p" and of "row r is in a query's exclusion segment".
#pragma once

#include "vs_device.h"

namespace vs {

__device__ __forceinline__ bool where_pass(const WherePred& p, const WhereAttrs& a, int64_t r) {
  if (!p.on) return false;
  if (a.live && !a.live[r]) return false;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < kWhereMaxCols; ++c) {
    if (c < a.ncol && ((p.cmask >> c) & 1u)) {
      const float v = a.cols[(int64_t)c * a.stride + r];
      ok = ok && p.lo[c] <= v && v <= p.hi[c];  // a NaN value fails a tested column
    }
  }
  if (p.any_of | p.all_of | p.none_of) {
    const unsigned long long t = a.tags ? a.tags[r] : 0ull;
    ok = ok && (p.any_of == 0ull || (t & p.any_of) != 0ull) && (t & p.all_of) == p.all_of &&
         (t & p.none_of) == 0ull;
  }
  return ok;
}

// row is in the ascending segment rows[b .. e)
__device__ __forceinline__ bool where_excluded(const int64_t* __restrict__ rows, int64_t b,
                                               int64_t e, int64_t row) {
  while (b < e) {
    const int64_t mid = (b + e) >> 1;
    const int64_t v = rows[mid];
    if (v == row) return true;
    if (v < row) b = mid + 1;
    else e = mid;
  }
  return false;
}

}  // namespace vs
