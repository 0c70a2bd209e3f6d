// vs_x1_planes.hip — the kernels that build what a filter pass (vs_gemm_x1.hip)
// reads: the filter planes of rows and queries (int8 codes and scales, the
// augmented L2 planes), their residual norms and per-index maxima for the
// bound, and the small array kernels of the staged engine's gathered batches.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "vs_x1_device.h"

namespace vs {

// ---------------------------------------------------------------------------
// Per-index maxima for the bound: max |x|^2, max |x - hi(x)|^2 and
// max |x - hi(x)|^2 / |x|^2 over rows [0, n) (non-negative floats order as their
// bits; NaN sorts above every number and makes the bound non-finite).
__global__ __launch_bounds__(256) void bound_stats_kernel(const float* __restrict__ norms,
                                                          const float* __restrict__ rn2, int64_t n,
                                                          unsigned* __restrict__ out) {
  unsigned m0 = 0, m1 = 0, m2 = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = norms[i], r = rn2[i];
    m0 = max(m0, __float_as_uint(a) & 0x7FFFFFFFu);
    m1 = max(m1, __float_as_uint(r) & 0x7FFFFFFFu);
    if (a > 0.0f) m2 = max(m2, __float_as_uint(r / a) & 0x7FFFFFFFu);
    else if (r > 0.0f || a != a) m2 = 0x7F800000u;  // a residual without a norm: no bound
  }
  for (int o = 32; o > 0; o >>= 1) {
    m0 = max(m0, (unsigned)__shfl_xor((int)m0, o));
    m1 = max(m1, (unsigned)__shfl_xor((int)m1, o));
    m2 = max(m2, (unsigned)__shfl_xor((int)m2, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(out + 0, m0);
    atomicMax(out + 1, m1);
    atomicMax(out + 2, m2);
  }
}

hipError_t launch_bound_stats(const float* norms, const float* rn2, int64_t n, unsigned* out,
                              hipStream_t st, bool accumulate) {
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(out, 0, 3 * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
  }
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(bound_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, norms, rn2, n,
                     out);
  return hipGetLastError();
}

// |x - hi(x)|^2 of rows [r0, r0+n) (fp32 rows, stride ld), one wave per row,
// fp64 sums rounded up to float (an upper bound, as the verification needs).
__global__ __launch_bounds__(256) void resid_norms_kernel(const float* __restrict__ X, int64_t ld,
                                                          int64_t r0, int64_t n,
                                                          float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* xr = X + (r0 + row) * ld;
  double s = 0.0;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x = v[i];
      const float hi = __uint_as_float((uint32_t)f32_to_bf16_rne(x) << 16);
      const double r = (double)x - (double)hi;
      s += r * r;
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) {
    float f = (float)s;
    if ((double)f < s) f = nextafterf(f, INFINITY);
    out[r0 + row] = f;
  }
}

hipError_t launch_resid_norms(const float* X, int64_t ld, int64_t r0, int64_t n, float* out,
                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(resid_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X, ld,
                     r0, n, out);
  return hipGetLastError();
}

// int8 plane: code = rint(x / s), s = max|x| / 127 per row, clamped to +-127
// (a zero row has s = 0 and zero codes).  One wave per row: the row's maximum
// and finiteness, then the codes (4 per lane-store) and, when rn2 is given, the
// residual |x - s code|^2 in fp64 (s * code and x - s * code are exact there),
// rounded up to float; a non-finite row gets rn2 = +inf, which makes every
// bound non-finite (every query then goes to the exact engine).
template <typename RT>
__global__ __launch_bounds__(256) void quantize_i8_kernel(const RT* __restrict__ X, int64_t ld,
                                                          int64_t r0, int64_t n,
                                                          int8_t* __restrict__ codes,
                                                          float* __restrict__ scale,
                                                          float* __restrict__ rn2) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const RT* xr = X + (r0 + row) * ld;
  float m = 0.0f;
  bool bad = false;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 v = row4(xr + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bad |= !isfinite(v[i]);
      m = fmaxf(m, fabsf(v[i]));
    }
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  bad = __any(bad);
  const float s = bad ? 0.0f : m / 127.0f;
  double acc = 0.0;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 v = row4(xr + c);
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int code = 0;
      if (s > 0.0f) code = (int)fminf(fmaxf(rintf(v[i] / s), -127.0f), 127.0f);
      packed |= (uint32_t)(code & 0xFF) << (8 * i);
      const double r = (double)v[i] - (double)s * (double)code;
      acc += r * r;
    }
    *(uint32_t*)(codes + plane_offset(r0 + row, c, ld)) = packed;  // tile-major
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    scale[r0 + row] = s;
    if (rn2) {
      float f = (float)acc;
      if ((double)f < acc) f = nextafterf(f, INFINITY);
      rn2[r0 + row] = bad ? INFINITY : f;
    }
  }
}

// ---------------------------------------------------------------------------
// L2 on the int8 plane: the augmented inner product (vs_internal.h,
// launch_quantize_i8_l2aug).  faiss ranks an L2 index's rows by
// fl(fl(|q|^2 + n_x) - 2 fl(q.x)) (exhaustive_L2sqr_blas), i.e. by
// q.x - n_x / 2 up to rounding; with x' = [x, e_1 .. e_m], q' = [q, C .. C] and
// sum_j e_j = -n_x / (2 C), that is x'.q', an inner product the int8 filter
// pass runs unchanged (list and dump launches, cuts, replays).  After the pass
// the lane lists' keys A ~ n_x / 2 - q.x become L2 keys qn + 2A
// (launch_l2aug_map) and the verification runs in the L2 metric with the
// augmented bound (bound_key).  One wave per row; the codes are written four per
// lane-store, the extra block (m a multiple of 64) after the ld row columns.
__global__ __launch_bounds__(256) void quantize_i8_l2aug_kernel(
    const float* __restrict__ X, int64_t ld, int64_t r0, int64_t n, int64_t pld, int m, float C,
    float nref, const float* __restrict__ norms, int8_t* __restrict__ codes,
    float* __restrict__ scale, float* __restrict__ rn2, float* __restrict__ anorm) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* xr = X + (r0 + row) * ld;
  float mx = 0.0f;
  bool bad = false;
  double sq = 0.0;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bad |= !isfinite(v[i]);
      mx = fmaxf(mx, fabsf(v[i]));
      sq += (double)v[i] * (double)v[i];
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o));
    sq += __shfl_xor(sq, o);
  }
  bad = __any(bad);
  const bool rows = norms != nullptr;
  // the scale and the extra block's codes: rows an even split of T = rint(E / s)
  // (base + 1 on the first |rem| columns), queries c everywhere
  double E = 0.0;
  float s = 0.0f;
  int64_t T = 0;
  int cq = 0;
  if (rows) {
    E = ((double)nref - (double)norms[r0 + row]) / (2.0 * (double)C);
    bad |= !isfinite(E);
    const double sd = fmax((double)mx, fabs(E) / m) / 127.0;
    s = (float)sd;
    if ((double)s < sd) s = nextafterf(s, INFINITY);
    if (bad) s = 0.0f;
    if (s > 0.0f) {
      const double t = rint(E / (double)s);
      T = (int64_t)fmin(fmax(t, -127.0 * m), 127.0 * m);
    }
  } else {
    cq = mx > C ? max(1, min(127, (int)floorf(127.0f * (C / mx)))) : 127;
    s = bad ? 0.0f : C / (float)cq;
  }
  const int64_t base = T / m, rem = T - base * m;  // |rem| < m, the sign of T
  const int64_t sg = rem < 0 ? -1 : 1, nrem = rem < 0 ? -rem : rem;
  double acc = 0.0;
  for (int64_t c = lane * 4; c < pld; c += 256) {
    uint32_t packed = 0;
    if (c < ld) {
      const f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int code = 0;
        if (s > 0.0f) code = (int)fminf(fmaxf(rintf(v[i] / s), -127.0f), 127.0f);
        packed |= (uint32_t)(code & 0xFF) << (8 * i);
        const double r = (double)v[i] - (double)s * (double)code;
        acc += r * r;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t j = c + i - ld;  // extra column j (0 .. m-1; pld = ld + m)
        int code = 0;
        if (j < m) {
          if (rows) {
            code = (int)(base + (j < nrem ? sg : 0));
          } else if (s > 0.0f) {
            code = cq;
            const double r = (double)C - (double)s * (double)cq;
            acc += r * r;
          }
        }
        packed |= (uint32_t)(code & 0xFF) << (8 * i);
      }
    }
    *(uint32_t*)(codes + plane_offset(r0 + row, c, pld)) = packed;  // tile-major
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    scale[r0 + row] = s;
    auto up = [](double v) {
      float f = (float)v;
      if ((double)f < v) f = nextafterf(f, INFINITY);
      return f;
    };
    if (rows) {
      // the extra block: e_j = s c_j + delta, delta = (E - s T) / m (E's fp64
      // rounding folded into the margin); |e|^2 = s^2 sum c_j^2 + 2 delta s T + m delta^2
      const double dlt = fabs(E - (double)s * (double)T) + fabs(E) * 1e-15;
      const double d1 = (E - (double)s * (double)T) / m;
      const double cc = (double)(m - nrem) * (double)(base * base) +
                        (double)nrem * (double)((base + sg) * (base + sg));
      const double e2 = (double)s * (double)s * cc + 2.0 * d1 * (double)s * (double)T + m * d1 * d1;
      rn2[r0 + row] = bad ? INFINITY : up((acc + dlt * dlt / m) * (1.0 + 1e-12));
      if (anorm) anorm[r0 + row] = bad ? INFINITY : up((sq + fmax(e2, 0.0)) * (1.0 + 1e-12) + 1e-30);
    } else {
      rn2[r0 + row] = bad ? INFINITY : up(acc * (1.0 + 1e-12));
    }
  }
}

hipError_t launch_quantize_i8_l2aug(const float* X, int64_t ld, int64_t r0, int64_t n,
                                    const L2Aug& g, const float* norms, int8_t* codes,
                                    float* scale, float* rn2, float* anorm, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (ld % 64 != 0 || g.m <= 0 || g.m % 64 != 0 || !(g.C > 0.0f) || !std::isfinite(g.nref) ||
      !rn2)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantize_i8_l2aug_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X,
                     ld, r0, n, ld + g.m, g.m, g.C, g.nref, norms, codes, scale, rn2, anorm);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void bf16_plane_l2aug_kernel(
    const float* __restrict__ X, int64_t ld, int64_t r0, int64_t n, float Cb, float nref,
    const float* __restrict__ norms, uint16_t* __restrict__ plane, float* __restrict__ rn2,
    float* __restrict__ anorm) {
  constexpr int m = kAugBf16;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* xr = X + (r0 + row) * ld;
  const int64_t pld = ld + m;
  char* base = (char*)plane;
  const bool rows = norms != nullptr;
  const double E = rows ? ((double)nref - (double)norms[r0 + row]) / (2.0 * (double)Cb) : 0.0;
  const uint16_t eb = rows ? f32_to_bf16_rne((float)(E / m)) : f32_to_bf16_rne(Cb);
  const double es = (double)__uint_as_float((uint32_t)eb << 16);  // a stored extra entry
  double acc = 0.0, sq = 0.0;
  bool bad = !isfinite(E);
  for (int64_t c = lane * 4; c < pld; c += 256) {
    uint32_t lo, hi;
    if (c < ld) {
      const f32x4 v = *(const f32x4*)(xr + c);
      uint16_t b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        b[i] = f32_to_bf16_rne(v[i]);
        bad |= !isfinite(v[i]);
        const double h = (double)__uint_as_float((uint32_t)b[i] << 16);
        const double r = (double)v[i] - h;
        acc += r * r;
        sq += (double)v[i] * (double)v[i];
      }
      lo = (uint32_t)b[0] | ((uint32_t)b[1] << 16);
      hi = (uint32_t)b[2] | ((uint32_t)b[3] << 16);
    } else {  // the extra block (pld = ld + m)
      lo = (uint32_t)eb | ((uint32_t)eb << 16);
      hi = lo;
    }
    *(uint2*)(base + plane_offset(r0 + row, 2 * c, 2 * pld)) = make_uint2(lo, hi);
  }
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o);
    sq += __shfl_xor(sq, o);
  }
  bad = __any(bad);
  if (lane == 0 && rows) {
    auto up = [](double v) {
      float f = (float)v;
      if ((double)f < v) f = nextafterf(f, INFINITY);
      return f;
    };
    // e_j = es + delta, delta = (E - m es) / m: the extra block's residual is
    // m delta^2 (E's fp64 rounding in the margin)
    const double d1 = (E - m * es) / m;
    const double dlt = fabs(d1) + fabs(E) * 1e-15 / m;
    rn2[r0 + row] = bad ? INFINITY : up((acc + m * dlt * dlt) * (1.0 + 1e-12));
    anorm[r0 + row] = bad ? INFINITY : up((sq + m * (es + d1) * (es + d1)) * (1.0 + 1e-12) + 1e-30);
  }
}

hipError_t launch_bf16_plane_l2aug(const float* X, int64_t ld, int64_t r0, int64_t n,
                                   const L2Aug& g, const float* norms, uint16_t* plane, float* rn2,
                                   float* anorm, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (ld % 64 != 0 || !(g.Cb > 0.0f) || !std::isfinite(g.nref) || (norms && (!rn2 || !anorm)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bf16_plane_l2aug_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X,
                     ld, r0, n, g.Cb, g.nref, norms, plane, rn2, anorm);
  return hipGetLastError();
}

// The augmentation's statistics, two passes over the first rows: nref < 0:
// acc[0] += max|x| over the nonzero rows, acc[1] += their count, acc[2] = the
// largest norm; nref >= 0: acc[3] = max |nref - n_x| / max|x| (bits of a
// non-negative double order as its unsigned image).  One wave per row, one
// atomic set per block.
__global__ __launch_bounds__(256) void l2aug_stats_kernel(const float* __restrict__ X, int64_t ld,
                                                          int64_t r0, int64_t n,
                                                          const float* __restrict__ norms,
                                                          float nref, double* __restrict__ acc) {
  __shared__ double part[4][3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wv;
  float mx = 0.0f;
  if (row < n) {
    const float* xr = X + (r0 + row) * ld;
    for (int64_t c = lane * 4; c < ld; c += 256) {
      const f32x4 v = *(const f32x4*)(xr + c);
      mx = fmaxf(fmaxf(fmaxf(mx, fabsf(v[0])), fmaxf(fabsf(v[1]), fabsf(v[2]))), fabsf(v[3]));
    }
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (lane == 0) {
    const bool on = row < n && mx > 0.0f && isfinite(mx);
    const double nx = on ? (double)norms[r0 + row] : 0.0;
    part[wv][0] = on ? (double)mx : 0.0;
    part[wv][1] = on ? 1.0 : 0.0;
    const double r = nref < 0.0f ? nx : fabs((double)nref - nx) / (double)mx;
    part[wv][2] = on && isfinite(r) ? r : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = 0; i < 4; ++i) {
      a += part[i][0];
      b += part[i][1];
      c = fmax(c, part[i][2]);
    }
    if (b > 0.0) {
      if (nref < 0.0f) {
        atomicAdd(acc + 0, a);
        atomicAdd(acc + 1, b);
      }
      atomicMax((unsigned long long*)(acc + (nref < 0.0f ? 2 : 3)),
                (unsigned long long)__double_as_longlong(c));
    }
  }
}

hipError_t l2aug_params(const float* X, int64_t ld, int64_t r0, int64_t n, const float* norms,
                        L2Aug* out, hipStream_t st) {
  out->m = 64;
  out->C = 1.0f;
  out->nref = 0.0f;
  out->Cb = 1.0f;
  if (n <= 0) return hipSuccess;
  double* acc = nullptr;
  hipError_t e = hipMalloc(&acc, 4 * sizeof(double));
  if (e != hipSuccess) return e;
  double h[4] = {0.0, 0.0, 0.0, 0.0};
  const dim3 grid((unsigned)((n + 3) / 4));
  e = hipMemsetAsync(acc, 0, 4 * sizeof(double), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(l2aug_stats_kernel, grid, dim3(256), 0, st, X, ld, r0, n, norms, -1.0f, acc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const float nref = (float)h[2];
  if (e == hipSuccess && h[1] > 0.0 && h[0] > 0.0 && std::isfinite(nref)) {
    hipLaunchKernelGGL(l2aug_stats_kernel, grid, dim3(256), 0, st, X, ld, r0, n, norms, nref, acc);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
      const double c = h[0] / h[1];
      // a row's extra entries stay within its own max|x| when
      // m >= |nref - n_x| / (2 C max|x|)
      const double need = h[3] / (2.0 * c);
      out->C = (float)c;
      out->nref = nref;
      out->Cb = std::ldexp(1.0f, (int)std::lround(std::log2(c)));
      // capped at ld / 8 (at least 64 columns): a few tiny-but-nonzero rows
      // would otherwise widen every row of the plane (up to 4096 columns);
      // past the cap a row's extra entries exceed its max|x| and only its own
      // scale coarsens (quantize_i8_l2aug_kernel: s = max(max|x|, |E| / m) / 127)
      const double cap = std::max(64.0, std::ceil((double)ld / 8.0 / 64.0) * 64.0);
      out->m = (int)std::min<double>(cap, std::max(64.0, std::ceil(need / 64.0) * 64.0));
    }
  }
  (void)hipFree(acc);
  return e;
}

__global__ __launch_bounds__(256) void l2aug_map_kernel(float* __restrict__ key,
                                                        const int* __restrict__ id,
                                                        int64_t per_query, int nq,
                                                        const float* __restrict__ qn, float nref,
                                                        float* __restrict__ qcut) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)nq * per_query && id[i] >= 0) {
    const float v = (qn[i / per_query] + nref) + 2.0f * key[i];
    key[i] = v < 0.0f ? 0.0f : v;
  }
  if (qcut && i < nq) {
    const float c = qcut[i];
    if (c < FLT_MAX && c > -FLT_MAX) {
      const float v = (qn[i] + nref) + 2.0f * c;
      qcut[i] = v < 0.0f ? 0.0f : v;
    }
  }
}

hipError_t launch_l2aug_map(float* key, const int* id, int64_t per_query, int nq, const float* qn,
                            float nref, float* qcut, hipStream_t st) {
  const int64_t tot = std::max<int64_t>((int64_t)nq * per_query, nq);
  if (tot <= 0) return hipSuccess;
  hipLaunchKernelGGL(l2aug_map_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, key, id,
                     per_query, nq, qn, nref, qcut);
  return hipGetLastError();
}

// Gathered batch of a later filter stage: slot s < *count takes query gl[s]
// (its fp32 row of `src`, stride ld, and its aux value; self row self0 + gl[s]
// when self0 >= 0); slots past the count are zero rows (aux 0, no self row).
// One wave per slot.
__global__ __launch_bounds__(256) void gather_queries_kernel(
    const float* __restrict__ src, int64_t ld, const float* __restrict__ aux,
    const int* __restrict__ gl, const int* __restrict__ count, int nslot, int64_t self0,
    float* __restrict__ dst, float* __restrict__ daux, int* __restrict__ drow) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= nslot) return;
  const bool on = s < *count;
  const int q = on ? gl[s] : 0;
  const f32x4* in = (const f32x4*)(src + (int64_t)q * ld);
  f32x4* out = (f32x4*)(dst + (int64_t)s * ld);
  for (int64_t c = lane; c < ld / 4; c += 64) out[c] = on ? in[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  if (lane == 0) {
    if (daux) daux[s] = on && aux ? aux[q] : 0.0f;
    if (drow) drow[s] = on && self0 >= 0 ? (int)(self0 + q) : -1;
  }
}

hipError_t launch_gather_queries(const float* src, int64_t ld, const float* aux, const int* gl,
                                 const int* count, int nslot, int64_t self0, float* dst,
                                 float* daux, int* drow, hipStream_t st) {
  if (nslot <= 0) return hipSuccess;
  if (ld % 4 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_queries_kernel, dim3((unsigned)((nslot + 3) / 4)), dim3(256), 0, st,
                     src, ld, aux, gl, count, nslot, self0, dst, daux, drow);
  return hipGetLastError();
}

// out[j] = outer[inner[j]] for j < *count (query ids of a gathered batch's
// flagged slots), one thread per slot of a fixed grid.
__global__ __launch_bounds__(256) void compose_list_kernel(const int* __restrict__ outer,
                                                           const int* __restrict__ inner,
                                                           const int* __restrict__ count, int n,
                                                           int* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n && j < *count) out[j] = outer[inner[j]];
}

hipError_t launch_compose_list(const int* outer, const int* inner, const int* count, int n,
                               int* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(compose_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     outer, inner, count, n, out);
  return hipGetLastError();
}

__global__ void window_count_kernel(const int* __restrict__ count, int w0, int cap,
                                    int* __restrict__ out) {
  const int c = *count - w0;
  *out = c < 0 ? 0 : (c > cap ? cap : c);
}

hipError_t launch_window_count(const int* count, int w0, int cap, int* out, hipStream_t st) {
  hipLaunchKernelGGL(window_count_kernel, dim3(1), dim3(1), 0, st, count, w0, cap, out);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void mul_arrays_kernel(const float* __restrict__ a,
                                                         const float* __restrict__ b, int64_t n,
                                                         float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] * b[i];
}

// out[2 g + b] = max of f[r] over the rows r of 32-row group g with bit 2 of r
// equal to b (f >= 0); n a multiple of 32.  outmin (optional): the minimum
// over the rows below nvalid (FLT_MAX for a part with none: padding rows,
// whose zero factors would otherwise make every dump launch's minimum 0).
__global__ __launch_bounds__(256) void group_max_kernel(const float* __restrict__ f, int64_t ngrp,
                                                        int64_t nvalid, float* __restrict__ out,
                                                        float* __restrict__ outmin) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (group, bit)
  if (i >= 2 * ngrp) return;
  const int64_t r0 = (i >> 1) * 32 + (i & 1) * 4;
  const float* p = f + r0;
  float m = 0.0f, mn = FLT_MAX;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 v = *(const f32x4*)(p + 8 * j);
    m = fmaxf(fmaxf(fmaxf(m, v[0]), fmaxf(v[1], v[2])), v[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (r0 + 8 * j + e < nvalid) mn = fminf(mn, v[e]);
  }
  out[i] = m;
  if (outmin) outmin[i] = mn;
}

hipError_t launch_group_max(const float* f, int64_t n, float* out, hipStream_t st, int64_t nvalid,
                            float* outmin) {
  if (n <= 0) return hipSuccess;
  if (n % 32 != 0) return hipErrorInvalidValue;
  const int64_t m = 2 * (n / 32);
  hipLaunchKernelGGL(group_max_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, f,
                     n / 32, nvalid, out, outmin);
  return hipGetLastError();
}

hipError_t launch_mul_arrays(const float* a, const float* b, int64_t n, float* out,
                             hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mul_arrays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b,
                     n, out);
  return hipGetLastError();
}

hipError_t launch_quantize_i8(const void* X, int64_t ld, int64_t r0, int64_t n, int8_t* codes,
                              float* scale, float* rn2, hipStream_t st, int xesize) {
  if (n <= 0) return hipSuccess;
  if (ld % 4 != 0 || (xesize != 4 && xesize != 2)) return hipErrorInvalidValue;
  if (xesize == 4)
    hipLaunchKernelGGL(quantize_i8_kernel<float>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st,
                       (const float*)X, ld, r0, n, codes, scale, rn2);
  else
    hipLaunchKernelGGL(quantize_i8_kernel<uint16_t>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0,
                       st, (const uint16_t*)X, ld, r0, n, codes, scale, rn2);
  return hipGetLastError();
}

}  // namespace vs
