// vs_boost_value.h — the boost of a boosted search (DESIGN.md "Boosted
// searches"), defined once for the device kernels (vs_boost.hip) and the host
// (vs_boost_eval, vs_api_boost.hip).  Every operation is one float32 operation
// rounded to nearest: nothing is contracted into an FMA, and the units that
// include this are built with a correctly rounded division, so the value is
// the same bits on both sides and in numpy.
#pragma once

#include "vs_internal.h"

namespace vs {

// One column's term: kind 0 none, 1 near, 2 ramp; a NaN value is `miss`.
// max(0, x) and min(1, y) are written as selections so that the sign of a zero
// result is fixed (x > 0 ? x : +0).
__host__ __device__ inline float boost_term(int kind, float v, float t, float s, float w,
                                            float miss) {
#pragma clang fp contract(off)
  if (kind == 0) return 0.0f;
  if (v != v) return miss;
  const float d = v - t;
  if (kind == 1) {
    const float x = 1.0f - __builtin_fabsf(d) / s;
    return w * (x > 0.0f ? x : 0.0f);
  }
  const float y = d / s;
  const float z = y > 0.0f ? y : 0.0f;
  return w * (z < 1.0f ? z : 1.0f);
}

// b = (((c0 + c1) + c2) + c3) + g0 + g1 + g2 + g3, left to right.
__host__ __device__ inline float boost_value(const BoostSpec& sp, const float (&v)[kWhereMaxCols],
                                             unsigned long long tags) {
#pragma clang fp contract(off)
  float b = boost_term(sp.kind[0], v[0], sp.t[0], sp.s[0], sp.w[0], sp.miss[0]);
#pragma unroll
  for (int c = 1; c < kWhereMaxCols; ++c)
    b = b + boost_term(sp.kind[c], v[c], sp.t[c], sp.s[c], sp.w[c], sp.miss[c]);
#pragma unroll
  for (int j = 0; j < kBoostMaxTags; ++j) b = b + ((tags & sp.mask[j]) != 0ull ? sp.bonus[j] : 0.0f);
  return b;
}

// b of row r in place (device; vs_boost.hip and vs_bonus.hip): only the columns
// and the tag word the spec reads are loaded.
__device__ __forceinline__ float boost_of_row(const BoostSpec& sp, const WhereAttrs& a,
                                              int64_t r) {
  float v[kWhereMaxCols];
#pragma unroll
  for (int c = 0; c < kWhereMaxCols; ++c)
    v[c] = (c < a.ncol && sp.kind[c] != 0) ? a.cols[(int64_t)c * a.stride + r] : 0.0f;
  const unsigned long long any = sp.mask[0] | sp.mask[1] | sp.mask[2] | sp.mask[3];
  const unsigned long long t = (a.tags && any) ? a.tags[r] : 0ull;
  return boost_value(sp, v, t);
}

// final_key = fl32(key - b)
__host__ __device__ inline float boost_final(float key, float b) {
#pragma clang fp contract(off)
  return key - b;
}

// U >= b >= L for every row: the same sum over each term's largest and
// smallest value (rounded addition is monotone in both operands).
__host__ __device__ inline void boost_bounds(BoostSpec* sp) {
#pragma clang fp contract(off)
  float U = 0.0f, L = 0.0f;
  for (int c = 0; c < kWhereMaxCols; ++c) {
    float hi = 0.0f, lo = 0.0f;
    if (sp->kind[c] != 0) {
      hi = sp->w[c] > hi ? sp->w[c] : hi;
      hi = sp->miss[c] > hi ? sp->miss[c] : hi;
      lo = sp->w[c] < lo ? sp->w[c] : lo;
      lo = sp->miss[c] < lo ? sp->miss[c] : lo;
    }
    U = U + hi;
    L = L + lo;
  }
  for (int j = 0; j < kBoostMaxTags; ++j) {
    const float g = sp->bonus[j];
    U = U + (g > 0.0f ? g : 0.0f);
    L = L + (g < 0.0f ? g : 0.0f);
  }
  sp->U = U;
  sp->L = L;
}

}  // namespace vs
