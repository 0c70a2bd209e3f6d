// vs_profile.hip — profile searches (vs_search_excl, vs_mean_rows,
// vs_search_profiles; DESIGN.md "Profile searches"): top-k with one exclusion
// list per query, and queries built on the device as weighted means of stored
// rows.  The engines are untouched: a class of queries whose lists hold at most
// c rows runs the unselected engine in raw order for need + c entries, and
// excl_drop below drops every query's own excluded rows from its entries
// (route (b) of the selector search, vs_select.hip sel_drop_kernel, with the
// row bitmap replaced by the query's sorted segment of a CSR).
#include "vs_device.h"

namespace vs {

// ---------------------------------------------------------------------------
// Class batches: slot s of a class is query qmap[s] of the chunk.  dst row s =
// src row qmap[s] (rows of row16 16-byte pieces) for s < cnt, zeros for the
// padding slots [cnt, nslot); daux[s] = saux[qmap[s]] or 0 likewise.
__global__ __launch_bounds__(256) void excl_gather_kernel(const uint4* __restrict__ src,
                                                          int64_t row16,
                                                          const float* __restrict__ saux,
                                                          const int* __restrict__ qmap, int cnt,
                                                          uint4* __restrict__ dst,
                                                          float* __restrict__ daux) {
  const int s = blockIdx.x;
  const bool real = s < cnt;
  const int64_t q = real ? qmap[s] : 0;
  for (int64_t c = threadIdx.x; c < row16; c += 256)
    dst[(int64_t)s * row16 + c] = real ? src[q * row16 + c] : make_uint4(0u, 0u, 0u, 0u);
  if (daux && threadIdx.x == 0) daux[s] = real ? saux[q] : 0.0f;
}

hipError_t launch_excl_gather(const void* src, int64_t rowbytes, const float* saux,
                              const int* qmap, int cnt, int nslot, void* dst, float* daux,
                              hipStream_t st) {
  if (cnt < 0 || nslot < cnt || rowbytes < 16 || rowbytes % 16 != 0 || !src || !dst || !qmap)
    return hipErrorInvalidValue;
  if (nslot == 0) return hipSuccess;
  hipLaunchKernelGGL(excl_gather_kernel, dim3(nslot), dim3(256), 0, st, (const uint4*)src,
                     rowbytes / 16, saux, qmap, cnt, (uint4*)dst, daux);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The drop.  One wave per class slot; each lane takes one raw entry, looks its
// row up in the query's sorted segment, and a ballot over the 64 entries gives
// every kept one its stable position.
__global__ __launch_bounds__(64) void excl_drop_kernel(int asc, const float* __restrict__ Din,
                                                       const int64_t* __restrict__ Iin, int k_in,
                                                       const int64_t* __restrict__ offs,
                                                       const int64_t* __restrict__ rows,
                                                       const int* __restrict__ qmap,
                                                       int64_t id_base, float* __restrict__ Dout,
                                                       int64_t* __restrict__ Iout, int k_out) {
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t q = qmap ? qmap[s] : s;
  const int64_t e0 = offs[q], e1 = offs[q + 1];
  int kept = 0;
  for (int j0 = 0; j0 < k_in && kept < k_out; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false;
    float sc = 0.0f;
    int64_t id = -1;
    if (j < k_in) {
      id = Iin[s * k_in + j];
      sc = Din[s * k_in + j];
      if (id >= 0) {
        const int64_t r = id - id_base;
        int64_t lo = e0, hi = e1;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (rows[mid] < r) lo = mid + 1;
          else hi = mid;
        }
        keep = !(lo < e1 && rows[lo] == r);
      }
    }
    const unsigned long long m = __ballot(keep);
    const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < k_out) {
      Dout[q * k_out + pos] = sc;
      Iout[q * k_out + pos] = id;
    }
    kept += __popcll(m);
  }
  for (int j = min(kept, k_out) + lane; j < k_out; j += 64) {
    Dout[q * k_out + j] = asc ? FLT_MAX : -FLT_MAX;
    Iout[q * k_out + j] = -1;
  }
}

hipError_t launch_excl_drop(int mode, const float* Din, const int64_t* Iin, int nq, int k_in,
                            const int64_t* offs, const int64_t* rows, const int* qmap,
                            int64_t id_base, float* Dout, int64_t* Iout, int k_out,
                            hipStream_t st) {
  if (nq < 0 || k_in < 1 || k_out < 1 || !offs) return hipErrorInvalidValue;
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(excl_drop_kernel, dim3(nq), dim3(64), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, k_in, offs, rows,
                     qmap, id_base, Dout, Iout, k_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Weighted means of stored rows.  Query q over its segment [offs[q], offs[q+1])
// of (row, weight) pairs, in list order and in fp32:
//   acc = x[r0] * w0;  acc = fl(acc + fl(x[ri] * wi));  out = fl(acc / W[q])
// with no contraction into FMA and a correctly rounded division (the unit is
// built with hipcc's correctly rounded fp32 division, csrc/Makefile), which is
// numpy's np.sum([x_i * w_i], axis=0) / W bit for bit.  Grid (query, chunk of
// 512 columns); a lane owns 4 consecutive columns: one 16-byte load per fp32
// row, 8 bytes per bf16 row.  The row stride is padded to a multiple of 64
// elements, so the vector load of a lane whose first column is below d stays
// inside the row; only the stores of the last lane are cut at d.  The loads of
// kMeanAhead rows are issued before their adds.
constexpr int kMeanAhead = 4;
constexpr int kMeanCols = 512;  // columns per block: 128 lanes x 4

template <typename T>
__device__ __forceinline__ f32x4 mean_load4(const T* __restrict__ X, int64_t ld, int64_t row,
                                            int c0) {
  if constexpr (sizeof(T) == 4) {
    return *(const f32x4*)(X + row * ld + c0);
  } else {
    const uint2 u = *(const uint2*)(X + row * ld + c0);
    f32x4 v;
    v.x = __uint_as_float(u.x << 16);
    v.y = __uint_as_float(u.x & 0xFFFF0000u);
    v.z = __uint_as_float(u.y << 16);
    v.w = __uint_as_float(u.y & 0xFFFF0000u);
    return v;
  }
}

template <typename T>
__global__ __launch_bounds__(128) void mean_rows_kernel(const T* __restrict__ X, int64_t ld, int d,
                                                        const int64_t* __restrict__ offs,
                                                        const int64_t* __restrict__ rows,
                                                        const float* __restrict__ wts,
                                                        const float* __restrict__ W,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t q = blockIdx.x;
  const int c0 = (blockIdx.y * 128 + threadIdx.x) * 4;
  if (c0 >= d) return;
  const int64_t s0 = offs[q], s1 = offs[q + 1];
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t j = s0; j < s1; j += kMeanAhead) {
    f32x4 v[kMeanAhead];
    float w[kMeanAhead];
#pragma unroll
    for (int i = 0; i < kMeanAhead; ++i) {
      const int64_t e = j + i < s1 ? j + i : s1 - 1;  // the tail re-reads the last entry
      v[i] = mean_load4<T>(X, ld, rows[e], c0);
      w[i] = wts[e];
    }
#pragma unroll
    for (int i = 0; i < kMeanAhead; ++i) {
      if (j + i < s1) {
        const f32x4 p = v[i] * w[i];
        acc = (j + i == s0) ? p : acc + p;
      }
    }
  }
  const float wq = W[q];
  const f32x4 r = acc / wq;
  float* o = out + q * (int64_t)d + c0;
  if ((d & 3) == 0 && ((uintptr_t)out & 15) == 0) {
    *(f32x4*)o = r;
  } else {
    o[0] = r.x;
    if (c0 + 1 < d) o[1] = r.y;
    if (c0 + 2 < d) o[2] = r.z;
    if (c0 + 3 < d) o[3] = r.w;
  }
}

hipError_t launch_mean_rows(const void* X, int esize, int64_t ld, int d, const int64_t* offs,
                            const int64_t* rows, const float* wts, const float* W, int64_t nq,
                            float* out, hipStream_t st) {
  if (nq < 0 || d < 1 || ld < d || ld % 64 != 0 || (esize != 4 && esize != 2) || !X || !offs ||
      !rows || !wts || !W || !out)
    return hipErrorInvalidValue;
  const unsigned gy = (unsigned)((d + kMeanCols - 1) / kMeanCols);
  // the x dimension of a grid holds any batch; chunk anyway to keep the launch small
  const int64_t step = 1 << 20;
  for (int64_t q0 = 0; q0 < nq; q0 += step) {
    const int64_t nc = nq - q0 < step ? nq - q0 : step;
    if (esize == 4)
      hipLaunchKernelGGL((mean_rows_kernel<float>), dim3((unsigned)nc, gy), dim3(128), 0, st,
                         (const float*)X, ld, d, offs + q0, rows, wts, W + q0, out + q0 * d);
    else
      hipLaunchKernelGGL((mean_rows_kernel<uint16_t>), dim3((unsigned)nc, gy), dim3(128), 0, st,
                         (const uint16_t*)X, ld, d, offs + q0, rows, wts, W + q0, out + q0 * d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace vs
