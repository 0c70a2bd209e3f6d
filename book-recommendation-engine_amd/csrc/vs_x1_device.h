// vs_x1_device.h — device helpers shared by the filter pass's units
// (vs_gemm_x1.hip, vs_x1_cuts.hip, vs_x1_planes.hip, vs_x1_verify.hip): only
// what more than one of them uses.  The exactness argument needs several
// expressions to be the same wherever they appear — a row's approximate key,
// the replay's admission, the exact key, the rounded-up cut — so each is one
// definition here.
#pragma once

#include "vs_device.h"

namespace vs {

// Four elements of a stored row as floats: fp32 rows, or bf16 rows widened
// (exactly) — the verification of a bf16 index's int8 plane rescores the
// stored bf16 values.
__device__ __forceinline__ f32x4 row4(const float* __restrict__ p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 row4(const uint16_t* __restrict__ p) {
  const uint2 u = *(const uint2*)p;
  return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u),
               __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xFFFF0000u)};
}

// The approximate key of a row from its raw sum (int8: the exact int32 sum
// times the two factors, three fp32 roundings, five with the cosine's folded
// inverse norms — xs holds s_x (IP) or s_x / |x| (COS), qsc s_q or s_q / |q|;
// bf16 inner product: -sum exactly).  One expression for the list epilogue and
// the replay, so both produce the same bits.
template <int EL>
__device__ __forceinline__ float x1_key(int sum_bits, float qsc, float fx) {
  if constexpr (EL == FILTER_I8) return -((float)sum_bits * (qsc * fx));
  else return -__int_as_float(sum_bits);
}

__device__ __forceinline__ uint32_t key_order(float f) {  // float order as unsigned order
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_unorder(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// exact dot product of two fp32 rows (fp64 accumulation across the wave);
// DIFF: the exact sum of (x - q)^2 instead (faiss's sequential L2 formula,
// MODE_L2D: each difference of two floats is exact in fp64, its square too)
template <bool DIFF = false, typename RT = float>
__device__ __forceinline__ double wave_dot(const RT* __restrict__ x, const float* __restrict__ q,
                                           int64_t ld, int lane) {
  double acc = 0.0;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 xv = row4(x + c);
    const f32x4 qv = *(const f32x4*)(q + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (DIFF) {
        const double t = (double)xv[e] - (double)qv[e];
        acc = fma(t, t, acc);
      } else {
        acc = fma((double)xv[e], (double)qv[e], acc);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// The same sums for two rows at once against a query whose slice of this lane
// sits in registers (ld <= 256 kQV): every load of both rows is issued before
// the first FMA (one memory round trip per pair instead of one per 1 KB), and
// each row's terms are added in wave_dot's order (identical results).  (Four
// rows per step: the first check 51 vs 54 us at C2, the wide check 194 vs 130
// us at one wave per SIMD, profiles/r06tl2: both are bound by the rows' HBM
// gathers, ~3-4 TB/s.)
constexpr int kQV = 8;
struct QSlice {
  f32x4 v[kQV];
};
__device__ __forceinline__ void load_qslice(const float* __restrict__ q, int64_t ld, int lane,
                                            QSlice& qs) {
#pragma unroll
  for (int i = 0; i < kQV; ++i) {
    const int64_t c = lane * 4 + 256 * i;
    qs.v[i] = c < ld ? *(const f32x4*)(q + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
template <bool DIFF = false, typename RT = float>
__device__ __forceinline__ void wave_dot2(const RT* __restrict__ xa, const RT* __restrict__ xb,
                                          const QSlice& qs, int64_t ld, int lane, double& ra,
                                          double& rb) {
  f32x4 va[kQV], vb[kQV];
#pragma unroll
  for (int i = 0; i < kQV; ++i) {
    const int64_t c = lane * 4 + 256 * i;
    va[i] = c < ld ? row4(xa + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    vb[i] = c < ld ? row4(xb + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int i = 0; i < kQV; ++i) {
    if (lane * 4 + 256 * i >= ld) break;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (DIFF) {
        const double ta = (double)va[i][e] - (double)qs.v[i][e];
        const double tb = (double)vb[i][e] - (double)qs.v[i][e];
        a = fma(ta, ta, a);
        b = fma(tb, tb, b);
      } else {
        a = fma((double)va[i][e], (double)qs.v[i][e], a);
        b = fma((double)vb[i][e], (double)qs.v[i][e], b);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
  }
  ra = a;
  rb = b;
}

template <int MODE>
__device__ __forceinline__ float exact_key(float ip, int q, int r, const float* __restrict__ qn,
                                           const float* __restrict__ xn,
                                           const float* __restrict__ qinv,
                                           const float* __restrict__ xinv) {
  return MODE == MODE_L2    ? l2_from_ip(qn[q], xn[r], ip)
         : MODE == MODE_COS ? -(ip * (qinv[q] * xinv[r]))
         : MODE == MODE_L2D ? ip  // the rounded exact sum of (x - q)^2
                            : -ip;
}

// ---------------------------------------------------------------------------
// The replay of a lane list's dumps (x1_replay_kernel and x1_replay_cut_kernel,
// vs_x1_cuts.hip): one definition of every step, so both kernels leave the
// same lists, counters and statistics.

// dump statistics, one atomic per wave: stats[0] += dumps replayed, stats[1] +=
// lists with more dumps than slots (cnt = this thread's list's dump count)
__device__ __forceinline__ void replay_stats(int cnt, int dR,
                                             unsigned long long* __restrict__ stats) {
  unsigned long long a = (unsigned long long)cnt, b = cnt > dR ? 1ull : 0ull;
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
  }
  if ((threadIdx.x & 63) == 0 && a && stats) {
    atomicAdd(stats, a);
    if (b) atomicAdd(stats + 1, b);
  }
}

// a lane list of KR entries at offset o of the partial lists, as 16-B pieces
// (o a multiple of 4: KP is one)
template <int KR>
__device__ __forceinline__ void lane_list_load(const float* __restrict__ pkey,
                                               const int* __restrict__ pid, int64_t o,
                                               float (&lk)[KR], int (&li)[KR]) {
  static_assert(KR % 4 == 0, "lane lists move as 16-B pieces");
#pragma unroll
  for (int e = 0; e < KR; e += 4) {
    const f32x4 kv = *(const f32x4*)(pkey + o + e);
    const int4 iv = *(const int4*)(pid + o + e);
    lk[e] = kv.x, lk[e + 1] = kv.y, lk[e + 2] = kv.z, lk[e + 3] = kv.w;
    li[e] = iv.x, li[e + 1] = iv.y, li[e + 2] = iv.z, li[e + 3] = iv.w;
  }
}
template <int KR>
__device__ __forceinline__ void lane_list_store(float* __restrict__ pkey, int* __restrict__ pid,
                                                int64_t o, const float (&lk)[KR],
                                                const int (&li)[KR]) {
#pragma unroll
  for (int e = 0; e < KR; e += 4) {
    *(f32x4*)(pkey + o + e) = f32x4{lk[e], lk[e + 1], lk[e + 2], lk[e + 3]};
    *(int4*)(pid + o + e) = make_int4(li[e], li[e + 1], li[e + 2], li[e + 3]);
  }
}

// Admits list i's cnt dumped rows into (lk, li) in dump order: the list's
// slots c = 0 .. cnt-1 at dslot[c * nl + i] (slot-major), eight at a time —
// their loads, then their rows' factors, then the admissions (independent
// loads in flight together instead of a chain) — each with the key the list
// epilogue computes (x1_key) and its admission: key < min(last entry, cut),
// the row inside the corpus and not the query's own.  x1_replay_cut_kernel
// replays a list exactly as x1_replay_kernel does: both call this.
template <int KR, int EL>
__device__ __forceinline__ void replay_admit(float (&lk)[KR], int (&li)[KR],
                                             const int* __restrict__ dslot, int64_t i, int64_t nl,
                                             int cnt, float qsc, const float* __restrict__ xs,
                                             int selfrow, int ntotal, float cut) {
  const i32x2* sl = (const i32x2*)dslot + i;
  constexpr int kB = 8;
  for (int c0 = 0; c0 < cnt; c0 += kB) {
    i32x2 e[kB];
    float fx[kB];
#pragma unroll
    for (int j = 0; j < kB; ++j) e[j] = c0 + j < cnt ? sl[(int64_t)(c0 + j) * nl] : i32x2{-1, 0};
#pragma unroll
    for (int j = 0; j < kB; ++j)
      fx[j] = EL == FILTER_I8 && e[j][0] >= 0 && e[j][0] < ntotal ? xs[e[j][0]] : 0.0f;
#pragma unroll
    for (int j = 0; j < kB; ++j) {
      const int row = e[j][0];
      if (!(row >= 0 && row < ntotal && row != selfrow)) continue;
      const float key = x1_key<EL>(e[j][1], qsc, fx[j]);
      if (key < fminf(lk[KR - 1], cut)) list_insert<KR, int>(lk, li, key, row);
    }
  }
}

// The cut base + factor B rounded up to a float, if that is finite, below
// FLT_MAX and below `old`; `old` otherwise (a cut never rises).  The cut
// kernels pass factor 2.000001 with base a_M ("Query cuts") and 1.000001 with
// base e_M ("Exact-key cuts", vs_x1_cuts.hip).
__device__ __forceinline__ float lower_cut(float base, double factor, double B, float old) {
  const double tp = (double)base + factor * B;
  if (isfinite(tp) && tp < (double)FLT_MAX) {
    float t = (float)tp;
    if ((double)t < tp) t = nextafterf(t, INFINITY);
    if (t < old) return t;
  }
  return old;
}

// Launchers of vs_x1_cuts.hip that x1_launch (vs_gemm_x1.hip) calls between
// the launches of a pass; launch_x1_replay is declared in vs_internal.h.
hipError_t launch_qcut(const X1Args& a, Partials part, hipStream_t st);
hipError_t launch_x1_replay_cut(const X1Args& a, Partials part, hipStream_t st);
hipError_t launch_x1_ecut(const X1Args& a, Partials part, hipStream_t st);

}  // namespace vs
