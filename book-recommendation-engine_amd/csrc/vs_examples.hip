// vs_examples.hip — example searches (vs_search_examples; DESIGN.md "Example
// searches"): the rows nearest to ANY of a user's liked examples that are not
// at least as near to a disliked one.  The engines are untouched: a round runs
// the unselected engine in raw order for a window of w entries per positive
// example (vs_api_examples.hip run_examples), and the kernels below turn the
// a windows of a user into its answer:
//   merge    every row of the windows once, with its best (key, position)
//   select   F = the smallest last entry of the user's windows, and the set
//            S = {rows with (p, row) <= F}: exactly the allowed rows up to F
//   keys     the exact key of every member of S against its deciding positive
//            and against each negative
//   emit     the first k favoured members of S in (p, row) order, or the flag
//            that sends the user to a longer window
// A key is compared and ordered as the pair (key_order(key + 0.0f), row) packed
// in 64 bits: + 0.0f makes -0.0 and +0.0 one key, as the float comparison of
// the definition does.
#include <algorithm>

#include "vs_x1_device.h"

namespace vs {

namespace {

constexpr unsigned long long kExNone = ~0ull;

__device__ __forceinline__ unsigned long long ex_pack(float key, uint32_t lo) {
  return ((unsigned long long)key_order(key + 0.0f) << 32) | lo;
}

}  // namespace

// Rows in place -> fp32 rows of stride d (bf16 widened exactly, as
// vs_reconstruct_n returns them).  One workgroup per row.
template <typename RT>
__global__ __launch_bounds__(256) void examples_gather_kernel(const RT* __restrict__ X, int64_t ld,
                                                              int d,
                                                              const int64_t* __restrict__ rows,
                                                              float* __restrict__ out) {
  const int64_t i = blockIdx.x;
  const RT* src = X + rows[i] * ld;
  for (int c = threadIdx.x; c < d; c += 256) {
    if constexpr (sizeof(RT) == 4) out[i * d + c] = src[c];
    else out[i * d + c] = __uint_as_float((uint32_t)src[c] << 16);
  }
}

hipError_t launch_examples_gather(const void* X, int esize, int64_t ld, int d, const int64_t* rows,
                                  int64_t n, float* out, hipStream_t st) {
  if (n < 0 || n > INT_MAX || d < 1 || !X || !out || (n > 0 && !rows) ||
      (esize != 4 && esize != 2))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (esize == 4)
    hipLaunchKernelGGL(examples_gather_kernel<float>, dim3((unsigned)n), dim3(256), 0, st,
                       (const float*)X, ld, d, rows, out);
  else
    hipLaunchKernelGGL(examples_gather_kernel<uint16_t>, dim3((unsigned)n), dim3(256), 0, st,
                       (const uint16_t*)X, ld, d, rows, out);
  return hipGetLastError();
}

// The merge.  Entry e of user u is position t = e % w of the window of its
// positive j = e / w (Din / Iin [slots][w]: raw entries, labels = row +
// id_base, -1 after the end).  A thread claims or finds its row's slot of the
// user's table (trow, 1 << tbits slots from toff, -1 empty; atomicCAS) and
// folds (key, j) into the slot's value with a 64-bit atomicMin: the smallest
// key wins, among equal keys the lowest position, whatever order the atomics
// land in.  The probe visits at most every slot once; a table without a free
// slot (a sizing mistake) raises *err instead of spinning.
__global__ __launch_bounds__(256) void examples_merge_kernel(
    const ExamplesUser* __restrict__ users, int nu, int asc, const float* __restrict__ Din,
    const int64_t* __restrict__ Iin, int w, int64_t id_base, int* __restrict__ trow,
    unsigned long long* __restrict__ tval, int* __restrict__ err) {
  for (int u = blockIdx.y; u < nu; u += gridDim.y) {
    const ExamplesUser U = users[u];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)U.a * w) continue;
    const int j = (int)(e / w);
    const int64_t at = (int64_t)(U.pos0 + j) * w + (e - (int64_t)j * w);
    const int64_t id = Iin[at];
    if (id < 0) continue;
    const int r = (int)(id - id_base);
    const float sc = Din[at];
    const unsigned long long val = ex_pack(asc ? sc : -sc, (uint32_t)j);
    const unsigned mask = (1u << U.tbits) - 1u;
    unsigned h = ((unsigned)r * 2654435761u) >> (32 - U.tbits);
    bool found = false;
    for (unsigned probe = 0; probe <= mask; ++probe) {
      const int old = atomicCAS(&trow[U.toff + h], -1, r);
      if (old == -1 || old == r) {
        found = true;
        break;
      }
      h = (h + 1u) & mask;
    }
    if (found) atomicMin(&tval[U.toff + h], val);
    else atomicExch(err, 1);
  }
}

// F and S.  f_j = the last entry of positive j's window, or +inf when the
// window ended before it (a -1 entry) or is every live row (w_is_all); F =
// their minimum as a packed (key, row).  Every table slot whose (p, row) <= F
// becomes a candidate: ckey = the packed (p, row), cpos = the deciding
// positive.  A user's candidates are at most its window entries (cap = a * w);
// more than that raises *err.  Their order in ckey is not fixed (an atomic
// counter); the emit sorts them by their unique keys.
__global__ __launch_bounds__(256) void examples_select_kernel(
    const ExamplesUser* __restrict__ users, int nu, int asc, const float* __restrict__ Din,
    const int64_t* __restrict__ Iin, int w, int w_is_all, int64_t id_base,
    const int* __restrict__ trow, const unsigned long long* __restrict__ tval,
    unsigned long long* __restrict__ Fout, int* __restrict__ ccount,
    unsigned long long* __restrict__ ckey, int* __restrict__ cpos, int* __restrict__ err) {
  __shared__ unsigned long long sF;
  for (int u = blockIdx.y; u < nu; u += gridDim.y) {
    const ExamplesUser U = users[u];
    const int64_t tsize = (int64_t)1 << U.tbits;
    if ((int64_t)blockIdx.x * 256 >= tsize) continue;  // (block-uniform)
    if (threadIdx.x == 0) sF = kExNone;
    __syncthreads();
    if ((int)threadIdx.x < U.a && !w_is_all) {
      const int64_t at = (int64_t)(U.pos0 + (int)threadIdx.x) * w + (w - 1);
      const int64_t id = Iin[at];
      if (id >= 0) {
        const float sc = Din[at];
        atomicMin(&sF, ex_pack(asc ? sc : -sc, (uint32_t)(id - id_base)));
      }
    }
    __syncthreads();
    const unsigned long long F = sF;
    if (blockIdx.x == 0 && threadIdx.x == 0) Fout[u] = F;
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h < tsize) {
      const int r = trow[U.toff + h];
      if (r >= 0) {
        const unsigned long long v = tval[U.toff + h];
        const unsigned long long key = (v & 0xFFFFFFFF00000000ull) | (uint32_t)r;
        if (key <= F) {
          const int c = atomicAdd(&ccount[u], 1);
          if ((int64_t)c < (int64_t)U.a * w) {
            ckey[U.coff + c] = key;
            cpos[U.coff + c] = (int)(v & 0xFFFFFFFFull);
          } else {
            atomicExch(err, 1);
          }
        }
      }
    }
    __syncthreads();  // sF is reused by the next user of this block
  }
}

// Exact keys: one wave per candidate, one dot product at a time.  Every key
// here is the rescoring's (wave_dot's fp64 sum and butterfly, rounded once,
// exact_key<MODE>; verify_rescore_kernel).  First p, against the deciding
// positive: where the engine's own key is that key already (the staged engine
// of an fp32 index) nothing changes, where it is not (the bf16 GEMM's fp32
// accumulation) D, the comparison with n and the final order use the exact
// key.  Then the negatives: the same arithmetic, so a liked and a disliked copy
// of one vector give p == n bit for bit.  A candidate that is not favoured
// (some negative with !(p < key); a NaN key among them) has its ckey set to
// kExNone.  Qp / qp: the round's positives (stride ld, |e|^2), Qn / qn: the
// staged negatives.
template <int MODE, typename RT>
__global__ __launch_bounds__(256) void examples_keys_kernel(
    const ExamplesUser* __restrict__ users, int nu, const int* __restrict__ ccount,
    const RT* __restrict__ X, const float* __restrict__ xn, const float* __restrict__ Qp,
    const float* __restrict__ qp, const float* __restrict__ Qn, const float* __restrict__ qn,
    int64_t ld, int w, unsigned long long* __restrict__ ckey, const int* __restrict__ cpos) {
  const int lane = threadIdx.x & 63;
  for (int u = blockIdx.y; u < nu; u += gridDim.y) {
    const ExamplesUser U = users[u];
    const int cnt = min(ccount[u], (int)min((int64_t)U.a * w, (int64_t)INT_MAX));
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < cnt;
         c += (int64_t)gridDim.x * 4) {
      const int r = (int)(uint32_t)ckey[U.coff + c];
      const RT* xr = X + (int64_t)r * ld;
      const int qe = U.pos0 + min(max(cpos[U.coff + c], 0), U.a - 1);
      const double pacc = wave_dot<false, RT>(xr, Qp + (int64_t)qe * ld, ld, lane);
      const float p = exact_key<MODE>((float)pacc, qe, r, qp, xn, nullptr, nullptr) + 0.0f;
      bool favoured = p == p;  // (a NaN key is no key)
      for (int e = 0; e < U.b && favoured; ++e) {
        const int q = U.neg0 + e;
        const double acc = wave_dot<false, RT>(xr, Qn + (int64_t)q * ld, ld, lane);
        const float nk = exact_key<MODE>((float)acc, q, r, qn, xn, nullptr, nullptr) + 0.0f;
        favoured = p < nk;  // (wave-uniform: every lane holds the butterfly's sum)
      }
      if (lane == 0) ckey[U.coff + c] = favoured ? ex_pack(p, (uint32_t)r) : kExNone;
    }
  }
}

// The emit: one workgroup per user.  The candidates are walked in chunks of KB
// (a power of two >= k, at least 256) next to the KB best so far; a bitonic
// sort of the 2 KB packed keys keeps the best KB.  The first k favoured go out
// as D (p as a score), I (row + id_base) and E (the deciding positive), padded
// with (+-FLT_MAX, -1, -1).  unsettled[out] = the window was too short: fewer
// than k favoured members of S and F is an entry (not +inf).
constexpr int kExEmitMax = 2048;
__global__ __launch_bounds__(256) void examples_emit_kernel(
    const ExamplesUser* __restrict__ users, int asc, int k, int KB, int w,
    const unsigned long long* __restrict__ Fin, const int* __restrict__ ccount,
    const unsigned long long* __restrict__ ckey, const int* __restrict__ cpos, int64_t id_base,
    float* __restrict__ D, int64_t* __restrict__ I, int* __restrict__ E,
    int* __restrict__ unsettled) {
  __shared__ unsigned long long sk[kExEmitMax];
  __shared__ int sv[kExEmitMax];
  __shared__ int s_fav;
  const int tid = threadIdx.x;
  const int u = blockIdx.x;
  const ExamplesUser U = users[u];
  const int cnt = min(ccount[u], (int)min((int64_t)U.a * w, (int64_t)INT_MAX));
  for (int i = tid; i < KB; i += 256) {
    sk[i] = kExNone;
    sv[i] = -1;
  }
  if (tid == 0) s_fav = 0;
  __syncthreads();
  for (int c0 = 0; c0 < cnt; c0 += KB) {
    int fav = 0;
    for (int i = tid; i < KB; i += 256) {
      const int c = c0 + i;
      const unsigned long long key = c < cnt ? ckey[U.coff + c] : kExNone;
      sk[KB + i] = key;
      sv[KB + i] = c < cnt ? cpos[U.coff + c] : -1;
      fav += key != kExNone ? 1 : 0;
    }
    if (fav) atomicAdd(&s_fav, fav);
    __syncthreads();
    const int n2 = 2 * KB;
    for (int size = 2; size <= n2; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < KB; t += 256) {  // KB pairs
          const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const unsigned long long a = sk[lo], b = sk[hi];
          if ((a > b) == up) {
            sk[lo] = b;
            sk[hi] = a;
            const int va = sv[lo];
            sv[lo] = sv[hi];
            sv[hi] = va;
          }
        }
        __syncthreads();
      }
    }
  }
  const int64_t o = (int64_t)U.out * k;
  for (int i = tid; i < k; i += 256) {
    const unsigned long long key = sk[i];
    if (key != kExNone) {
      const float p = key_unorder((uint32_t)(key >> 32));
      D[o + i] = asc ? p : 0.0f - p;
      I[o + i] = (int64_t)(uint32_t)key + id_base;
      E[o + i] = sv[i];
    } else {
      D[o + i] = asc ? FLT_MAX : -FLT_MAX;
      I[o + i] = -1;
      E[o + i] = -1;
    }
  }
  if (tid == 0) unsettled[U.out] = (s_fav >= k || Fin[u] == kExNone) ? 0 : 1;
}

hipError_t launch_examples_collapse(const ExamplesCollapse& c, hipStream_t st) {
  if (c.nu < 0 || c.w < 1 || c.k < 1 || c.k > kExamplesMaxK || c.amax < 1 ||
      c.amax > kExamplesMaxList || c.tbits_max < 1 || c.tbits_max > 31 || !c.users || !c.Din ||
      !c.Iin || !c.trow || !c.tval || !c.F || !c.ccount || !c.ckey || !c.cpos || !c.err || !c.X ||
      !c.D || !c.I || !c.E || !c.unsettled || c.ld % 4 != 0 || (c.xesize != 4 && c.xesize != 2) ||
      (c.mode != MODE_IP && c.mode != MODE_L2) || !c.Qp || (c.mode == MODE_L2 && !c.qp) ||
      (c.any_neg && (!c.Qn || (c.mode == MODE_L2 && !c.qn))))
    return hipErrorInvalidValue;
  if (c.nu == 0) return hipSuccess;
  const int asc = c.mode == MODE_L2 ? 1 : 0;
  const unsigned gy = (unsigned)std::min(c.nu, 65535);
  const int64_t cap = (int64_t)c.amax * c.w;  // the most entries (and candidates) of a user
  if ((cap + 255) / 256 > INT_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(examples_merge_kernel, dim3((unsigned)((cap + 255) / 256), gy), dim3(256), 0,
                     st, c.users, c.nu, asc, c.Din, c.Iin, c.w, c.id_base, c.trow, c.tval, c.err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t tmax = (int64_t)1 << c.tbits_max;
  hipLaunchKernelGGL(examples_select_kernel, dim3((unsigned)((tmax + 255) / 256), gy), dim3(256), 0,
                     st, c.users, c.nu, asc, c.Din, c.Iin, c.w, c.w_is_all ? 1 : 0, c.id_base,
                     c.trow, c.tval, c.F, c.ccount, c.ckey, c.cpos, c.err);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  {
    // a wave per candidate while that stays a modest grid; longer lists stride
    const unsigned gx = (unsigned)std::min<int64_t>((cap + 3) / 4, 4096);
#define VS_EX_KEYS(MD, RT)                                                                    \
  hipLaunchKernelGGL((examples_keys_kernel<MD, RT>), dim3(gx, gy), dim3(256), 0, st, c.users, \
                     c.nu, c.ccount, (const RT*)c.X, c.xn, c.Qp, c.qp, c.Qn, c.qn, c.ld, c.w,  \
                     c.ckey, c.cpos)
    if (c.mode == MODE_L2) {
      if (c.xesize == 4) VS_EX_KEYS(MODE_L2, float);
      else VS_EX_KEYS(MODE_L2, uint16_t);
    } else {
      if (c.xesize == 4) VS_EX_KEYS(MODE_IP, float);
      else VS_EX_KEYS(MODE_IP, uint16_t);
    }
#undef VS_EX_KEYS
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  int KB = 256;
  while (KB < c.k) KB <<= 1;
  hipLaunchKernelGGL(examples_emit_kernel, dim3((unsigned)c.nu), dim3(256), 0, st, c.users, asc,
                     c.k, KB, c.w, c.F, c.ccount, c.ckey, c.cpos, c.id_base, c.D, c.I, c.E, c.unsettled);
  return hipGetLastError();
}

}  // namespace vs
