// vs_distinct.hip — distinct searches (vs_search_distinct; DESIGN.md "Distinct
// searches"): the k nearest groups, one best row per group.  The engines are
// untouched: a round runs the unselected engine in raw order for a window of w
// entries per query, and distinct_collapse below keeps, in window order, the
// first entry of every group (a row whose group is -1 is a group of its own).
// If the window holds `need` groups their first entries are the `need` best
// representatives in order; if it holds fewer but also the end of the rows
// there are no more groups; otherwise the host searches the query again with a
// longer window (vs_api_distinct.hip run_distinct).
#include "vs_device.h"

namespace vs {

// Slots of the LDS table of the groups seen: a power of two, at least
// 2 * need and at least need + 256 (a chunk can add 256 groups to the fewer
// than `need` kept before it), so the probing always finds a free slot.
// need <= 2047 (k <= 1024 under faiss's inner-product rule): 4096 slots.
constexpr int kDistinctTable = 4096;
constexpr int kDistinctMaxNeed = kDistinctTable / 2 - 1;

// One 256-thread workgroup per slot s of a batch: Din / Iin [ns][w] are the raw
// entries as the engine wrote them (ascending (key, label), labels = row +
// id_base, -1 after the end).  group[row] (ngroup rows) is the row's group or
// -1.  The window is walked in chunks of 256 entries, in order.  A thread
// claims or finds its group's slot (atomicCAS on the key) and records the
// smallest window position that carries the group (atomicMin): the smallest
// position wins whatever order the atomics land in, and a group kept by an
// earlier chunk holds a position before this chunk, so no entry of this chunk
// equals it.  The kept entries of a chunk go out in window order: a ballot per
// wave and a prefix over the four waves.  The walk stops at `need` kept or at
// the first -1.  Outputs: row s of Dout / Iout ([ns][kout], padded with the
// empty result), kept[s] (may be null) and unsettled[qmap ? qmap[s] : s] = the
// window was too short: fewer than `need` kept, no end of the rows seen, and
// the window is not every allowed row (w_is_all).
__global__ __launch_bounds__(256) void distinct_collapse_kernel(
    int asc, const float* __restrict__ Din, const int64_t* __restrict__ Iin, int w,
    const int32_t* __restrict__ group, int64_t ngroup, int64_t id_base, int need, int tmask,
    int tshift, int w_is_all, const int* __restrict__ qmap, float* __restrict__ Dout,
    int64_t* __restrict__ Iout, int kout, int* __restrict__ kept_out,
    int* __restrict__ unsettled) {
  __shared__ int tkey[kDistinctTable];
  __shared__ int tpos[kDistinctTable];
  __shared__ int wsum[4];
  __shared__ int s_end;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t s = blockIdx.x;
  for (int i = tid; i <= tmask; i += 256) {
    tkey[i] = -1;
    tpos[i] = INT_MAX;
  }
  if (tid == 0) s_end = 0;
  __syncthreads();
  int kept = 0;
  bool end_seen = false;
  for (int c0 = 0; c0 < w && kept < need && !end_seen; c0 += 256) {
    const int pos = c0 + tid;
    int64_t id = -1;
    float sc = 0.0f;
    if (pos < w) {
      id = Iin[s * w + pos];
      sc = Din[s * w + pos];
      if (id < 0) s_end = 1;  // (every writer stores the same value)
    }
    int slot = -1;
    if (id >= 0) {
      const int64_t r = id - id_base;
      const int g = (r >= 0 && r < ngroup) ? group[r] : -1;
      if (g >= 0) {
        unsigned h = ((unsigned)g * 2654435761u) >> tshift;
        for (;;) {
          const int old = atomicCAS(&tkey[h], -1, g);
          if (old == -1 || old == g) break;
          h = (h + 1u) & (unsigned)tmask;
        }
        slot = (int)h;
        atomicMin(&tpos[slot], pos);
      }
    }
    __syncthreads();
    const bool keep = id >= 0 && (slot < 0 || tpos[slot] == pos);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wv] = __popcll(m);
    end_seen = s_end != 0;
    __syncthreads();
    int before = kept + __popcll(m & ((1ull << lane) - 1ull));
    int total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < wv) before += wsum[j];
      total += wsum[j];
    }
    if (keep && before < need && before < kout) {
      Dout[s * kout + before] = sc;
      Iout[s * kout + before] = id;
    }
    kept += total;
    __syncthreads();  // wsum and the table are reused by the next chunk
  }
  const int filled = min(min(kept, need), kout);
  for (int j = filled + tid; j < kout; j += 256) {
    Dout[s * kout + j] = asc ? FLT_MAX : -FLT_MAX;
    Iout[s * kout + j] = -1;
  }
  if (tid == 0) {
    if (kept_out) kept_out[s] = min(kept, need);
    unsettled[qmap ? qmap[s] : s] = (kept >= need || end_seen || w_is_all) ? 0 : 1;
  }
}

hipError_t launch_distinct_collapse(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                                    const int32_t* group, int64_t ngroup, int64_t id_base,
                                    int need, bool w_is_all, const int* qmap, float* Dout,
                                    int64_t* Iout, int kout, int* kept, int* unsettled,
                                    hipStream_t st) {
  if (ns < 0 || w < 1 || kout < 1 || need < 1 || need > kDistinctMaxNeed || !Din || !Iin ||
      !group || !Dout || !Iout || !unsettled)
    return hipErrorInvalidValue;
  if (ns == 0) return hipSuccess;
  int bits = 9;  // at least 512 slots: need - 1 + 256 groups fit for need <= 256
  while ((1 << bits) < 2 * need) ++bits;
  hipLaunchKernelGGL(distinct_collapse_kernel, dim3(ns), dim3(256), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, w, group, ngroup,
                     id_base, need, (1 << bits) - 1, 32 - bits, w_is_all ? 1 : 0, qmap, Dout, Iout,
                     kout, kept, unsettled);
  return hipGetLastError();
}

// A later round's results into the rows of the original queries: row qmap[s]
// of Dout / Iout = row s of Din / Iin ([ns][k]).
__global__ __launch_bounds__(256) void distinct_scatter_kernel(const float* __restrict__ Din,
                                                               const int64_t* __restrict__ Iin,
                                                               int k,
                                                               const int* __restrict__ qmap,
                                                               float* __restrict__ Dout,
                                                               int64_t* __restrict__ Iout) {
  const int64_t s = blockIdx.x;
  const int64_t q = qmap[s];
  for (int j = threadIdx.x; j < k; j += 256) {
    Dout[q * k + j] = Din[s * k + j];
    Iout[q * k + j] = Iin[s * k + j];
  }
}

hipError_t launch_distinct_scatter(const float* Din, const int64_t* Iin, int ns, int k,
                                   const int* qmap, float* Dout, int64_t* Iout, hipStream_t st) {
  if (ns < 0 || k < 1 || !Din || !Iin || !qmap || !Dout || !Iout) return hipErrorInvalidValue;
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(distinct_scatter_kernel, dim3(ns), dim3(256), 0, st, Din, Iin, k, qmap, Dout,
                     Iout);
  return hipGetLastError();
}

}  // namespace vs
