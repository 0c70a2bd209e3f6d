// vs_mmr.hip — maximal-marginal-relevance re-rank of a query's candidate rows
// (vs_mmr_select, vs_search_mmr; DESIGN.md "MMR searches"): LangChain's
// maximal_marginal_relevance over cosine similarities, on the rows in HBM.
//
// Every cosine is dot(a, b) / sqrt(dot(a, a) * dot(b, b)) with the three dot
// products summed in fp64 over the exact products of the fp32 values (a product
// of two 24-bit significands is exact in fp64), a non-finite quotient counting
// as 0.  One wave computes one dot product, always in the same order (wave_dot
// below): lane l owns the elements 4l .. 4l + 3 of every 256-element step and
// adds them in ascending order into its own accumulator, then a fixed xor
// butterfly adds the 64 accumulators.  The order depends on nothing but the
// element's index, so equal rows give equal bits whatever their position in
// the list or the batch, cos(x, x) is exactly 1, and no atomics are involved.
//
// Kernel shape (the "on demand" form): mmr_sims_kernel computes the query
// cosines s and the squared norms of the F candidates of each query (one wave
// per candidate), mmr_pick_kernel runs the greedy selection, one workgroup per
// query: per pick a workgroup-wide argmax (lowest position wins ties), then the
// cosines of the new pick to every candidate still free (F dot products, one
// wave each) folded into the running maximum.  k picks cost (k - 1) * F dot
// products; the full F x F Gram (F^2 / 2 of them, on f64 MFMA tiles) is untried.
#include "vs_device.h"

namespace vs {

namespace {

constexpr int kMmrThreads = 256;
constexpr int kMmrWaves = kMmrThreads / 64;
constexpr int kMmrAhead = 4;  // candidates a wave of the pick kernel scores at once

// Four consecutive elements of a stored row (stride a multiple of 64 elements,
// zero padded: the vector load stays inside the row) widened to fp32.
template <typename T>
__device__ __forceinline__ f32x4 mmr_row4(const T* __restrict__ row, int c) {
  if constexpr (sizeof(T) == 4) {
    return *(const f32x4*)(row + c);
  } else {
    const uint2 u = *(const uint2*)(row + c);
    f32x4 v;
    v.x = __uint_as_float(u.x << 16);
    v.y = __uint_as_float(u.x & 0xFFFF0000u);
    v.z = __uint_as_float(u.y << 16);
    v.w = __uint_as_float(u.y & 0xFFFF0000u);
    return v;
  }
}

// The same of a caller's query row: d elements, no padding, any alignment.
__device__ __forceinline__ f32x4 mmr_query4(const float* __restrict__ q, int c, int d) {
  f32x4 v;
  v.x = c < d ? q[c] : 0.0f;
  v.y = c + 1 < d ? q[c + 1] : 0.0f;
  v.z = c + 2 < d ? q[c + 2] : 0.0f;
  v.w = c + 3 < d ? q[c + 3] : 0.0f;
  return v;
}

__device__ __forceinline__ double mmr_fma4(f32x4 a, f32x4 b, double acc) {
  acc = fma((double)a.x, (double)b.x, acc);
  acc = fma((double)a.y, (double)b.y, acc);
  acc = fma((double)a.z, (double)b.z, acc);
  acc = fma((double)a.w, (double)b.w, acc);
  return acc;
}

// The fixed butterfly: every lane ends with the same bits (fp64 addition commutes).
__device__ __forceinline__ double mmr_wave_sum(double v) {
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// dot / sqrt(na * nb), 0 where that is not finite (a zero-norm row or query:
// LangChain's similarity[isnan | isinf] = 0).
__device__ __forceinline__ double mmr_cosine(double dot, double na, double nb) {
  const double c = dot / sqrt(na * nb);
  return isfinite(c) ? c : 0.0;
}

}  // namespace

// ---------------------------------------------------------------------------
// Candidate labels -> rows in place.  -1 stays -1 (an empty slot); any other
// label that is not a live label of the index becomes -1 as well and raises
// *bad (vs_mmr_select reports it; the candidates of vs_search_mmr are the
// search's own labels).  A live label l is row l + #{i : dead[i] - i <= l}
// (the host's row_of_label; dead[i] - i does not decrease).
__global__ __launch_bounds__(256) void mmr_rows_kernel(const int64_t* __restrict__ lab, int64_t n,
                                                       const int64_t* __restrict__ dead,
                                                       int64_t ndead, int64_t id_base,
                                                       int64_t live, int64_t* __restrict__ rows,
                                                       int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t v = lab[i];
  int64_t r = -1;
  if (v != -1) {
    const int64_t l = v - id_base;
    if (l >= 0 && l < live) {
      int64_t lo = 0, hi = ndead;  // the first i with dead[i] - i > l
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (dead[mid] - mid <= l) lo = mid + 1;
        else hi = mid;
      }
      r = l + lo;
    } else if (bad) {
      *bad = 1;  // (every writer stores the same value)
    }
  }
  rows[i] = r;
}

hipError_t launch_mmr_rows(const int64_t* labels, int64_t n, const int64_t* dead, int64_t ndead,
                           int64_t id_base, int64_t live, int64_t* rows, int* bad,
                           hipStream_t st) {
  if (n < 0 || !labels || !rows || (ndead > 0 && !dead)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mmr_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, labels,
                     n, dead, ndead, id_base, live, rows, bad);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Query cosines and candidate norms.  Grid (ceil(F / 4), queries), one wave per
// candidate: S[q][i] = cos(query q, candidate i), NN[q][i] = |candidate i|^2;
// an empty slot gets NN = -1 (a squared norm is never negative) and S = 0.
template <typename T>
__global__ __launch_bounds__(kMmrThreads) void mmr_sims_kernel(
    const T* __restrict__ X, int64_t ld, int d, const float* __restrict__ Q,
    const int64_t* __restrict__ rows, int F, double* __restrict__ S, double* __restrict__ NN) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kMmrWaves + (threadIdx.x >> 6);
  if (i >= F) return;  // (whole waves; the kernel has no barrier)
  const int64_t q = blockIdx.y;
  const int64_t r = rows[q * F + i];
  if (r < 0) {
    if (lane == 0) {
      S[q * F + i] = 0.0;
      NN[q * F + i] = -1.0;
    }
    return;
  }
  const T* __restrict__ row = X + r * ld;
  const float* __restrict__ qv = Q + q * (int64_t)d;
  double qc = 0.0, cc = 0.0, qq = 0.0;
  for (int c = lane * 4; c < d; c += 256) {
    const f32x4 a = mmr_query4(qv, c, d);
    const f32x4 b = mmr_row4<T>(row, c);
    qc = mmr_fma4(a, b, qc);
    cc = mmr_fma4(b, b, cc);
    qq = mmr_fma4(a, a, qq);
  }
  qc = mmr_wave_sum(qc);
  cc = mmr_wave_sum(cc);
  qq = mmr_wave_sum(qq);
  if (lane == 0) {
    S[q * F + i] = mmr_cosine(qc, qq, cc);
    NN[q * F + i] = cc;
  }
}

hipError_t launch_mmr_sims(const void* X, int esize, int64_t ld, int d, const float* Q,
                           const int64_t* rows, int nq, int F, double* S, double* NN,
                           hipStream_t st) {
  if (nq < 0 || nq > 65535 || F < 1 || F > kMmrMaxFetch || d < 1 || ld < d || ld % 64 != 0 ||
      (esize != 4 && esize != 2) || !Q || !rows || !S || !NN)
    return hipErrorInvalidValue;
  if (nq == 0) return hipSuccess;
  const dim3 grid((unsigned)((F + kMmrWaves - 1) / kMmrWaves), (unsigned)nq);
  if (esize == 4)
    hipLaunchKernelGGL((mmr_sims_kernel<float>), grid, dim3(kMmrThreads), 0, st, (const float*)X,
                       ld, d, Q, rows, F, S, NN);
  else
    hipLaunchKernelGGL((mmr_sims_kernel<uint16_t>), grid, dim3(kMmrThreads), 0, st,
                       (const uint16_t*)X, ld, d, Q, rows, F, S, NN);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The greedy selection, one workgroup per query.  LDS: s, |c|^2 and the running
// maximum cosine to the picks of every candidate (3 F doubles) and its state.
// Score of a free candidate: s (first pick), lambda * s - (1 - lambda) * max
// cos (later ones), in fp64 without contraction; a NaN score (an overflowing
// lambda) ranks as -inf; the best score wins, the lowest position among equals.
// pos[q][t] = the t-th pick's position, -1 past min(k, candidates); with Dc
// (the candidates' scores and labels, [q][F]) also Dout / Iout[q][t] = the
// pick's score and label, padded with (pad, -1).
template <typename T>
__global__ __launch_bounds__(kMmrThreads) void mmr_pick_kernel(
    const T* __restrict__ X, int64_t ld, const int64_t* __restrict__ rows, int F, int k,
    double lambda, const double* __restrict__ S, const double* __restrict__ NN,
    int* __restrict__ pos, const float* __restrict__ Dc, const int64_t* __restrict__ Ic,
    float pad, float* __restrict__ Dout, int64_t* __restrict__ Iout) {
#pragma clang fp contract(off)
  extern __shared__ double mmr_lds[];
  double* s = mmr_lds;
  double* nn = s + F;
  double* mx = nn + F;
  unsigned char* state = (unsigned char*)(mx + F);  // 0 empty, 1 free, 2 picked
  __shared__ double wbest[kMmrWaves];
  __shared__ int wpos[kMmrWaves];
  __shared__ int pick;
  __shared__ int wcount[kMmrWaves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  rows += q * F;
  int mine = 0;
  for (int i = tid; i < F; i += kMmrThreads) {
    const double n2 = NN[q * F + i];
    s[i] = S[q * F + i];
    nn[i] = n2;
    mx[i] = lambda == 1.0 ? 0.0 : -INFINITY;
    state[i] = n2 >= 0.0 ? 1 : 0;
    mine += n2 >= 0.0 ? 1 : 0;
  }
  // the candidates of the list (a wave sum of small integers, then 4 waves)
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if (lane == 0) wcount[wave] = mine;
  __syncthreads();
  int ncand = 0;
  for (int w = 0; w < kMmrWaves; ++w) ncand += wcount[w];
  const int steps = k < ncand ? k : ncand;

  for (int t = 0; t < steps; ++t) {
    double best = -INFINITY;
    int bpos = INT_MAX;
    for (int i = tid; i < F; i += kMmrThreads) {
      if (state[i] != 1) continue;
      double sc = t == 0 ? s[i] : lambda * s[i] - (1.0 - lambda) * mx[i];
      if (!(sc == sc)) sc = -INFINITY;
      if (sc > best || bpos == INT_MAX) {  // ascending i: the first of equals stays
        best = sc;
        bpos = i;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const int op = __shfl_xor(bpos, o);
      if (op != INT_MAX && (bpos == INT_MAX || ob > best || (ob == best && op < bpos))) {
        best = ob;
        bpos = op;
      }
    }
    if (lane == 0) {
      wbest[wave] = best;
      wpos[wave] = bpos;
    }
    __syncthreads();
    if (tid == 0) {
      double b = wbest[0];
      int p = wpos[0];
      for (int w = 1; w < kMmrWaves; ++w) {
        const double ob = wbest[w];
        const int op = wpos[w];
        if (op != INT_MAX && (p == INT_MAX || ob > b || (ob == b && op < p))) {
          b = ob;
          p = op;
        }
      }
      // (steps <= candidates: a free one exists, p is a position)
      pick = p;
      state[p] = 2;
      pos[q * k + t] = p;
      if (Dout) {
        Dout[q * k + t] = Dc[q * F + p];
        Iout[q * k + t] = Ic[q * F + p];
      }
    }
    __syncthreads();
    if (t + 1 == steps || lambda == 1.0) continue;  // (lambda 1: the maxima have no weight)
    // the new pick's cosines: wave w scores the free candidates among positions
    // w, w + 4, ..., kMmrAhead of them per pass over the pick's row
    const int p = pick;
    const T* __restrict__ prow = X + rows[p] * ld;
    const double pn = nn[p];
    for (int i0 = wave; i0 < F; i0 += kMmrWaves * kMmrAhead) {
      const T* crow[kMmrAhead];
      bool on[kMmrAhead];
      bool any = false;
#pragma unroll
      for (int u = 0; u < kMmrAhead; ++u) {
        const int i = i0 + u * kMmrWaves;
        on[u] = i < F && state[i] == 1;
        crow[u] = on[u] ? X + rows[i] * ld : prow;  // (an idle slot rereads the pick's row)
        any |= on[u];
      }
      if (!any) continue;
      double acc[kMmrAhead];
#pragma unroll
      for (int u = 0; u < kMmrAhead; ++u) acc[u] = 0.0;
      for (int c = lane * 4; c < (int)ld; c += 256) {
        const f32x4 a = mmr_row4<T>(prow, c);
#pragma unroll
        for (int u = 0; u < kMmrAhead; ++u) acc[u] = mmr_fma4(mmr_row4<T>(crow[u], c), a, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < kMmrAhead; ++u) {
        const double dot = mmr_wave_sum(acc[u]);
        const int i = i0 + u * kMmrWaves;
        if (on[u] && lane == 0) {
          const double c = mmr_cosine(dot, nn[i], pn);
          if (c > mx[i]) mx[i] = c;
        }
      }
    }
    __syncthreads();
  }
  for (int t = steps + tid; t < k; t += kMmrThreads) {
    pos[q * k + t] = -1;
    if (Dout) {
      Dout[q * k + t] = pad;
      Iout[q * k + t] = -1;
    }
  }
}

hipError_t launch_mmr_pick(const void* X, int esize, int64_t ld, const int64_t* rows, int nq,
                           int F, int k, double lambda, const double* S, const double* NN,
                           int* pos, const float* Dc, const int64_t* Ic, float pad, float* Dout,
                           int64_t* Iout, hipStream_t st) {
  if (nq < 0 || F < 1 || F > kMmrMaxFetch || k < 1 || ld < 1 || ld % 64 != 0 ||
      (esize != 4 && esize != 2) || !rows || !S || !NN || !pos || (Dout && (!Dc || !Ic || !Iout)))
    return hipErrorInvalidValue;
  if (nq == 0) return hipSuccess;
  const size_t lds = (size_t)F * (3 * sizeof(double) + 1);  // at most 25 KB
  if (esize == 4)
    hipLaunchKernelGGL((mmr_pick_kernel<float>), dim3((unsigned)nq), dim3(kMmrThreads), lds, st,
                       (const float*)X, ld, rows, F, k, lambda, S, NN, pos, Dc, Ic, pad, Dout,
                       Iout);
  else
    hipLaunchKernelGGL((mmr_pick_kernel<uint16_t>), dim3((unsigned)nq), dim3(kMmrThreads), lds, st,
                       (const uint16_t*)X, ld, rows, F, k, lambda, S, NN, pos, Dc, Ic, pad, Dout,
                       Iout);
  return hipGetLastError();
}

}  // namespace vs
