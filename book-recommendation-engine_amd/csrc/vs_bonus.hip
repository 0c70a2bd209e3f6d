// vs_bonus.hip — bonus searches (vs_search_bonus; DESIGN.md "Bonus
// searches"): exact top-k by final_key = fl32(fl32(key - b(q, r)) - s(q, r)),
// s a number the caller lists per (query, row) for at most kBonusMaxList rows
// of a query, b the boost of a boosted search (+0 without one).
//
// Kernels:
//  - bonus_score: the final key of every listed (query, row), one wave each;
//  - bonus_merge: per query, the base search's result without the listed rows,
//    merged with the query's scored list.
// This unit evaluates boost_value: it is built with a correctly rounded
// division (csrc/Makefile).
#include "vs_boost_value.h"
#include "vs_where_device.h"
#include "vs_x1_device.h"

namespace vs {

// the last q in [0, nq) with offs[q] <= e (offs ascending, offs[0] <= e)
__device__ __forceinline__ int bonus_query_of(const int64_t* __restrict__ offs, int nq,
                                              int64_t e) {
  int lo = 0, hi = nq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------------------
// One wave per list entry e (four per workgroup).  The base key is the
// rescoring's (verify_rescore_kernel, range_verify_kernel): the row gathered,
// the fp64 sum across the wave rounded once, exact_key<MODE>.  Lane 0 then
// tests the row against the query's predicate and exclusion segment and
// subtracts the boost and the bonus, each with one rounding.
template <int MODE, typename RT>
__global__ __launch_bounds__(256) void bonus_score_kernel(BonusScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.lists.total) return;  // wave-uniform
  const int64_t e = a.lists.e0 + c;
  const int q = bonus_query_of(a.lists.offs, a.lists.nq, e);
  const int64_t r = a.lists.rows[e];
  const RT* X = (const RT*)a.X;
  const double acc =
      wave_dot<MODE == MODE_L2D, RT>(X + r * a.ld, a.Q + (int64_t)q * a.ld, a.ld, lane);
  const float key = exact_key<MODE>((float)acc, q, (int)r, a.qn, a.xn, nullptr, nullptr);
  if (lane != 0) return;
  bool cand = true;
  if (a.preds) cand = where_pass(a.preds[q], a.at, r);
  if (cand && a.xoffs) cand = !where_excluded(a.xrows, a.xoffs[q], a.xoffs[q + 1], r);
  float fin = FLT_MAX;
  if (cand) {
    const float b = a.specs ? boost_of_row(a.specs[q], a.at, r) : 0.0f;
    fin = boost_final(boost_final(key, b), a.lists.vals[e]);
  }
  a.skey[c] = fin;
  a.srow[c] = cand ? r : -1;
}

hipError_t launch_bonus_score(const BonusScoreArgs& a, hipStream_t st) {
  if (a.lists.total <= 0) return hipSuccess;
  if (a.lists.nq < 1 || !a.lists.offs || !a.lists.rows || !a.lists.vals || !a.X || !a.Q ||
      !a.skey || !a.srow || a.ld % 4 != 0 || (a.esize != 4 && a.esize != 2) ||
      (a.mode == MODE_L2 && (!a.qn || !a.xn)) || ((a.xoffs == nullptr) != (a.xrows == nullptr)) ||
      a.lists.total > (int64_t)INT_MAX)
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((a.lists.total + 3) / 4);
#define VS_BS_T(MD, RT) \
  hipLaunchKernelGGL((bonus_score_kernel<MD, RT>), dim3(blocks), dim3(256), 0, st, a)
#define VS_BS(MD)            \
  do {                       \
    if (a.esize == 4)        \
      VS_BS_T(MD, float);    \
    else                     \
      VS_BS_T(MD, uint16_t); \
  } while (0)
  if (a.mode == MODE_IP)
    VS_BS(MODE_IP);
  else if (a.mode == MODE_L2)
    VS_BS(MODE_L2);
  else if (a.mode == MODE_L2D)
    VS_BS(MODE_L2D);
  else
    return hipErrorInvalidValue;
#undef VS_BS
#undef VS_BS_T
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// One workgroup per query q with m <= kBonusMaxList list entries.
//
// 1. The scored entries go to LDS (a row that is no candidate sorts last) and
//    boost_rerank's bitonic sort orders them by (final_key, row) over a
//    power-of-two pad; nv of them are candidates and Lc = min(nv, k) can reach
//    the result.
// 2. The base entries are read 256 at a time.  An entry whose row is in the
//    query's list segment (ascending rows: a binary search) is dropped and its
//    index goes to dj[] (ascending, at most m of them); a kept entry's place is
//    its rank among the kept ones (a running workgroup scan) plus the number of
//    the first Lc list entries that sort before it (a binary search in LDS).
// 3. List entry t < Lc goes to t + (base entries that sort before it: a binary
//    search over the base row, which is ascending with its dropped entries
//    still in place) - (dropped entries among those: a binary search in dj).
// A list entry and a kept base entry never compare equal (their rows differ),
// so the places are those of a stable two-way merge; places >= k are not
// written, and what the two sets leave of the k places is padded.
__global__ __launch_bounds__(256) void bonus_merge_kernel(
    int asc, const float* __restrict__ Din, const int64_t* __restrict__ Iin, int k,
    BonusLists lists, const float* __restrict__ skey, const int64_t* __restrict__ srow,
    int64_t id_base, float* __restrict__ Dout, int64_t* __restrict__ Iout,
    unsigned long long* __restrict__ entered) {
  __shared__ float sk[kBonusMaxList];
  __shared__ long long si[kBonusMaxList];
  __shared__ int dj[kBonusMaxList];
  __shared__ int s_nv, s_wsum[4], s_entered;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int64_t q = blockIdx.x;
  const int64_t lb = lists.offs[q];
  const int m = (int)(lists.offs[q + 1] - lb);
  const float* din = Din + q * k;
  const int64_t* iin = Iin + q * k;
  float* dout = Dout + q * k;
  int64_t* iout = Iout + q * k;
  if (m == 0) {  // uniform: the base result as it is
    for (int j = tid; j < k; j += 256) {
      dout[j] = din[j];
      iout[j] = iin[j];
    }
    return;
  }
  int P = 2;
  while (P < m) P <<= 1;
  if (tid == 0) {
    s_nv = 0;
    s_entered = 0;
  }
  __syncthreads();
  for (int j = tid; j < P; j += 256) {
    float key = INFINITY;
    long long id = LLONG_MAX;
    if (j < m) {
      const int64_t r = srow[lb - lists.e0 + j];
      if (r >= 0) {
        key = skey[lb - lists.e0 + j];
        id = r;
        atomicAdd(&s_nv, 1);
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
  const int Lc = min(s_nv, k);

  // 2. the base entries
  int nkept = 0, ndrop = 0;  // uniform running counts
  for (int c0 = 0; c0 < k && nkept < k; c0 += 256) {
    const int j = c0 + tid;
    int64_t lab = -1;
    float key = 0.0f;
    if (j < k) lab = iin[j];
    bool drop = false;
    if (lab >= 0) {
      const float d = din[j];
      key = asc ? d : -d;
      drop = where_excluded(lists.rows, lb, lb + m, lab - id_base);
    }
    const bool keep = lab >= 0 && !drop;
    // exclusive scan of (keep, drop) over the workgroup, both packed in one int
    const int mine = (keep ? 1 : 0) | (drop ? 1 << 16 : 0);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) s_wsum[wv] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
      const int v = s_wsum[w2];
      if (w2 < wv) before += v;
      all += v;
    }
    const int excl = before + incl - mine;
    // (at most m dropped: a result holds a row once)
    if (drop && ndrop + (excl >> 16) < kBonusMaxList) dj[ndrop + (excl >> 16)] = j;
    if (keep) {
      const int ci = nkept + (excl & 0xFFFF);
      int lo = 0, hi = Lc;  // list entries [0, lo) sort before this one
      const long long row = lab - id_base;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lex_less(sk[mid], si[mid], key, row)) lo = mid + 1;
        else hi = mid;
      }
      const int p = ci + lo;
      if (p < k) {
        dout[p] = din[j];
        iout[p] = lab;
      }
    }
    nkept += all & 0xFFFF;
    ndrop += all >> 16;
    __syncthreads();  // s_wsum is written again; dj is read below
  }

  // 3. the list entries
  for (int t = tid; t < Lc; t += 256) {
    const float key = sk[t];
    const long long row = si[t];
    int lo = 0, hi = k;  // base entries [0, lo) sort before this one
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int64_t lab = iin[mid];
      const float d = din[mid];
      if (lab >= 0 && lex_less(asc ? d : -d, (long long)(lab - id_base), key, row)) lo = mid + 1;
      else hi = mid;
    }
    int dl = 0, dh = min(ndrop, kBonusMaxList);  // dropped entries with an index below lo
    while (dl < dh) {
      const int mid = (dl + dh) >> 1;
      if (dj[mid] < lo) dl = mid + 1;
      else dh = mid;
    }
    const int p = t + lo - dl;
    if (p < k) {
      dout[p] = asc ? key : -key;
      iout[p] = (int64_t)row + id_base;
      atomicAdd(&s_entered, 1);
    }
  }
  // the padding (nkept is short only when it reached k: no padding then)
  for (int j = min(k, nkept + Lc) + tid; j < k; j += 256) {
    dout[j] = asc ? FLT_MAX : -FLT_MAX;
    iout[j] = -1;
  }
  __syncthreads();
  if (tid == 0 && entered && s_entered) atomicAdd(entered, (unsigned long long)s_entered);
}

hipError_t launch_bonus_merge(int mode, const float* Din, const int64_t* Iin, int k,
                              const BonusLists& lists, const float* skey, const int64_t* srow,
                              int64_t id_base, float* Dout, int64_t* Iout,
                              unsigned long long* entered, hipStream_t st) {
  if (lists.nq < 0 || k < 1 || !Din || !Iin || !Dout || !Iout || Din == Dout || Iin == Iout ||
      !lists.offs || (lists.total > 0 && (!lists.rows || !skey || !srow)))
    return hipErrorInvalidValue;
  if (lists.nq == 0) return hipSuccess;
  hipLaunchKernelGGL(bonus_merge_kernel, dim3(lists.nq), dim3(256), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, k, lists, skey, srow,
                     id_base, Dout, Iout, entered);
  return hipGetLastError();
}

}  // namespace vs
