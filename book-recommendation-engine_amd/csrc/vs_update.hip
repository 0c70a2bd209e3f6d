// vs_update.hip — the scattered write of an in-place update (vs_update_rows,
// DESIGN.md §3 "In-place updates").  The host stages the new rows as one
// contiguous block and runs the derivation kernels of an add over it; this
// kernel then moves staged row i of every array to row rows[i] of the index's.
#include "vs_internal.h"

namespace vs {

// One wave per staged row, 16-byte loads and stores: the row's elements (a
// contiguous line of rowbytes), each plane's bytes (tile-major on both sides:
// every 64-byte step of a row is contiguous, so a 16-byte piece never crosses
// one) and the per-row scalars, one lane each.  The rows of one call are
// distinct, so no two waves write the same bytes.
__global__ __launch_bounds__(256) void update_scatter_kernel(UpdateScatter a,
                                                             const int64_t* __restrict__ rows,
                                                             int64_t n) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t r = rows[i];
  if (a.codes) {
    const char* src = a.s_codes + i * a.rowbytes;
    char* dst = a.codes + r * a.rowbytes;
    for (int64_t b = (int64_t)lane * 16; b < a.rowbytes; b += 1024)
      *(uint4*)(dst + b) = *(const uint4*)(src + b);
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (!a.plane[p]) continue;
    const int64_t ldb = a.ldb[p];
    for (int64_t b = (int64_t)lane * 16; b < ldb; b += 1024)
      *(uint4*)(a.plane[p] + plane_offset(r, b, ldb)) =
          *(const uint4*)(a.s_plane[p] + plane_offset(i, b, ldb));
  }
#pragma unroll
  for (int s = 0; s < UpdateScatter::kScalars; ++s)
    if (lane == s && a.scal[s]) a.scal[s][r] = a.s_scal[s][i];
}

hipError_t launch_update_scatter(const UpdateScatter& a, const int64_t* rows, int64_t n,
                                 hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!rows || (a.codes && (!a.s_codes || a.rowbytes <= 0 || a.rowbytes % 16 != 0)))
    return hipErrorInvalidValue;
  for (int p = 0; p < 2; ++p)
    if (a.plane[p] && (!a.s_plane[p] || a.ldb[p] <= 0 || a.ldb[p] % 64 != 0))
      return hipErrorInvalidValue;
  for (int s = 0; s < UpdateScatter::kScalars; ++s)
    if (a.scal[s] && !a.s_scal[s]) return hipErrorInvalidValue;
  hipLaunchKernelGGL(update_scatter_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, a,
                     rows, n);
  return hipGetLastError();
}

}  // namespace vs
