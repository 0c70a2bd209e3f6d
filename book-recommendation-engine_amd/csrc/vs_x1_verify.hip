// vs_x1_verify.hip — what follows a filter pass (vs_gemm_x1.hip): the selection
// of each query's best approximate candidates from the lane lists, their exact
// rescoring, and the bound that proves the exact top-M is among them.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "vs_x1_device.h"

namespace vs {

// ---------------------------------------------------------------------------
// Verification (engines VS_ENGINE_I8_VERIFY / VS_ENGINE_BF16_VERIFY).  Written
// for the bf16 plane; the int8 plane is the same argument with hi(.) the
// dequantized row s * code and gam its three scaling roundings (the int32 sum is
// exact), see make_bound_args.  With x = hi(x) + r(x) and
// q = hi(q) + r(q) (bf16 round-to-nearest-even, residuals exact in fp32):
//   x.q - hi(x).hi(q) = hi(x).r(q) + r(x).hi(q) + r(x).r(q)
// and the MFMA sums ld exact products in fp32 (each add off by <= 1 ulp), so
// for every row (Cauchy-Schwarz on each term)
//   |approx - x.q| <= gam |hi(x)||hi(q)| + |hi(x)||r(q)| + |r(x)||hi(q)| + |r(x)||r(q)|,
// gam = n u / (1 - n u), n = ld + 1, u = 2^-23; the exact key is the fp32
// rounding of x.q (one more 2^-23 |x||q|).  |hi(x)| <= |x| + |r(x)|, and the
// verification takes the maxima of |x| and |r(x)| over the index.  Let a = the
// sorted approximate keys of the KF candidates of a query and E their exact
// keys, sorted; E[M-1] bounds the true M-th best key from above, and every row
// outside the candidates has approximate key >= T (the KF-th candidate, or a
// full lane list's last entry, whichever is smaller), so whenever
//     T - B > E[M-1]
// the exact top-M (ties included) is among the candidates and E's first M
// entries are it.  Otherwise the query is flagged for the exact engine.


__device__ __forceinline__ double bound_key(int mode, const BoundArgs& ba, double qh2, double qr2,
                                            double qn2, const unsigned* stats) {
  if (ba.l2aug) {
    // L2 through the augmented int8 plane: stats are the maxima of |x'|^2 and
    // |x' - plane(x')|^2, qh2 / qr2 the query's |plane(q')|^2 bound and
    // |q' - plane(q')|^2, qn2 = |q|^2 as staged.  The pass's key A differs from
    // n_x / 2 - q.x by at most the inner-product bound b of the augmented
    // vectors (no fp32 key rounding inside: A is not rounded again); the list
    // key is max(0, fl(fl(qn + nref) + 2A)) (two more roundings, at most
    // 2u (qn + nref + 2 |A|)) and
    // the exact key fl(fl(qn + n_x) - fl(2 fl(q.x))) is within 8u (qn + n_x) of
    // qn + n_x - 2 q.x (as for the other L2 passes); max(0, .) is 1-Lipschitz.
    const double ax2 = (double)__uint_as_float(stats[0]);  // >= max |x|^2 too
    const double hx = sqrt(ax2) + sqrt((double)__uint_as_float(stats[1]));
    const double rx = sqrt((double)__uint_as_float(stats[1]));
    const double hq = sqrt(qh2), rq = sqrt(qr2);
    const double u = ldexp(1.0, -24);
    double b = ba.gam * hx * hq + hx * rq + rx * hq + rx * rq;
    b *= 1.0 + 1e-6;
    double B = 2.0 * b + 8.0 * u * (qn2 + ax2) + 2.0 * u * (qn2 + ba.aug_nref + 2.01 * hx * hq);
    // MODE_L2D (faiss's sequential formula, keys the rounded exact sum of
    // (x - q)^2): the pass's keys follow the stored fp32 norms, each within
    // norm_inf / 2 (relative) of the exact one, and the key's own rounding
    if (mode == MODE_L2D) B += (ba.norm_inf + 4.0 * u) * (qn2 + ax2);
    return B * (1.0 + 1e-6);
  }
  const double xm = sqrt((double)__uint_as_float(stats[0]) * (1.0 + ba.norm_inf));
  const double rx = ba.rows_exact ? 0.0 : sqrt((double)__uint_as_float(stats[1]));
  const double hx = xm + rx;
  const double hq = sqrt(qh2), rq = sqrt(qr2), qn = sqrt(qn2);
  double b = ba.gam * hx * hq + hx * rq + rx * hq + rx * rq + 2.0 * ldexp(1.0, -24) * xm * qn;
  b *= 1.0 + 1e-6;
  if (mode == MODE_L2 || mode == MODE_L2D) {  // key = (|q|^2 + |x|^2) - 2 ip, every step rounded
    const double xm2 = (double)__uint_as_float(stats[0]);
    b = 2.0 * b + 8.0 * ldexp(1.0, -24) * (qn2 + xm2);
    if (mode == MODE_L2D) b += (ba.norm_inf + 4.0 * ldexp(1.0, -24)) * (qn2 + xm2);
  } else if (mode == MODE_COS) {
    // keys -(s qinv xinv) with qinv, xinv from the stored norms (relative error
    // ~gam(ld) each, 1.5 norm_inf together); |s_a - s_e| / (|x||q|) <=
    // gam (1+rho)^2 + 2 rho (1+rho) + rho^2 + 2^-23, rho = max |r(x)| / |x| (the queries are stored rows); two roundings
    // of a key of magnitude <= 1 add 2^-22
    const double rho =
        ba.rows_exact ? 0.0 : sqrt((double)__uint_as_float(stats[2]) * (1.0 + ba.norm_inf));
    const double rel = ba.gam * (1 + rho) * (1 + rho) + 2 * rho * (1 + rho) + rho * rho +
                       ldexp(1.0, -23);
    b = (rel * (1.0 + 1.5 * ba.norm_inf) + ldexp(1.0, -22)) * (1.0 + 1e-6);
  }
  return b;
}

// the query's split norms |hi(q)|^2, |r(q)|^2, |q|^2 (fp64, across the wave);
// int8 plane (qr2i8 = the query's stored residual norm, rounded up):
// |hi(q)| <= |q| + |r(q)|
__device__ __forceinline__ void query_split_norms(const float* __restrict__ qrow, int64_t ld,
                                                  int lane, const float* __restrict__ qr2i8,
                                                  double& qh2, double& qr2, double& qn2,
                                                  double aug = 0.0) {
  double a = 0.0, r = 0.0, n = 0.0;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 v = *(const f32x4*)(qrow + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x = v[i];
      const float hi = __uint_as_float((uint32_t)f32_to_bf16_rne(x) << 16);
      const double rr = (double)x - (double)hi;
      a += (double)hi * hi;
      r += rr * rr;
      n += (double)x * x;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    r += __shfl_xor(r, o);
    n += __shfl_xor(n, o);
  }
  qh2 = a + aug;  // aug: |q'|^2 = |q|^2 + m C^2 (the augmented L2 planes; exact
  qr2 = r;        // in bf16, whose extra entries are a power of two)
  qn2 = n;
  if (qr2i8) {
    qr2 = (double)*qr2i8;
    const double hq = sqrt(n + aug) + sqrt(qr2);
    qh2 = hq * hq;
  }
}

// One wave per query.  Dk/Ik: the KF best approximate keys (ascending) and
// local rows; X/xn: fp32 rows (stride ld) and squared norms; Q: query rows
// (stride ld); qn: |q|^2 as staged for L2.  Writes KF exact (key, row) entries
// sorted, padded to KP, and fail[q].  NE = candidates per lane (KF <= 64 NE).
template <int MODE, int NE, typename RT>
__global__ __launch_bounds__(64) void verify_rescore_kernel(
    int KF, int M, const float* __restrict__ Dk, const int64_t* __restrict__ Ik,
    const RT* __restrict__ X, const float* __restrict__ xn, const float* __restrict__ Q,
    const float* __restrict__ qn, int64_t ld, BoundArgs ba, const unsigned* __restrict__ stats,
    const float* __restrict__ lkey, const int* __restrict__ lid, int P, int LKP, int L,
    float* __restrict__ okey, int* __restrict__ oid, int KP, int* __restrict__ fail,
    const float* __restrict__ qinv, const float* __restrict__ xinv, const float* __restrict__ qr2i8,
    const int* __restrict__ qcount, const float* __restrict__ qcut) {
  __shared__ float ek[64 * NE];
  __shared__ int sid[64 * NE];
  __shared__ float eMs;
  const int lane = threadIdx.x;
  const int q = blockIdx.x;
  if (qcount && q >= *qcount) {  // gathered batch: slots past the count are not flagged
    if (lane == 0) fail[q] = 0;
    return;
  }
  int id[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int j = lane + 64 * e;
    id[e] = j < KF ? (int)Ik[(int64_t)q * KF + j] : -1;
    sid[j] = id[e];
  }
  if (lane == 0) eMs = FLT_MAX;
  const float aK = Dk[(int64_t)q * KF + KF - 1];
  const int idK = (int)Ik[(int64_t)q * KF + KF - 1];
  // T: the KF-th merged key (if the merge found KF) and the last key of every
  // full lane list; `bounded` = false when neither exists (the candidates are
  // every admissible row)
  bool bounded = idK >= 0;
  float T = idK >= 0 ? aK : FLT_MAX;
  for (int j = lane; j < P; j += 64) {
    const int64_t o = ((int64_t)q * P + j) * LKP + L - 1;
    if (lid[o] >= 0) {
      bounded = true;
      T = fminf(T, lkey[o]);
    }
  }
  for (int o = 32; o > 0; o >>= 1) T = fminf(T, __shfl_xor(T, o));
  bounded = __any(bounded);
  if (qcut && qcut[q] < FLT_MAX) {  // the pass dropped every row at or above the cut
    bounded = true;
    T = fminf(T, qcut[q]);
  }

  const float* qrow = Q + (int64_t)q * ld;
  double qh2, qr2, qn2;
  query_split_norms(qrow, ld, lane, qr2i8 ? qr2i8 + q : nullptr, qh2, qr2, qn2, ba.aug_q2);
  if (ba.rows_exact) {  // the fp32 GEMM multiplied q itself
    qh2 = qn2;
    qr2 = 0.0;
  }
  __syncthreads();  // sid
  if (ld <= 256 * kQV) {  // two candidates per step, the query in registers
    QSlice qsl;
    load_qslice(qrow, ld, lane, qsl);
    for (int j = 0; j < KF; j += 2) {
      const int ra = sid[j], rb = j + 1 < KF ? sid[j + 1] : -1;
      double da, db;
      wave_dot2<MODE == MODE_L2D, RT>(X + (int64_t)max(ra, 0) * ld, X + (int64_t)max(rb, 0) * ld,
                                      qsl, ld, lane, da, db);
      if (lane == 0) {
        ek[j] = ra < 0 ? FLT_MAX : exact_key<MODE>((float)da, q, ra, qn, xn, qinv, xinv);
        if (j + 1 < KF) ek[j + 1] = rb < 0 ? FLT_MAX : exact_key<MODE>((float)db, q, rb, qn, xn, qinv, xinv);
      }
    }
  } else {
    for (int j = 0; j < KF; ++j) {
      const int r = sid[j];
      if (r < 0) {
        if (lane == 0) ek[j] = FLT_MAX;
        continue;
      }
      const double acc = wave_dot<MODE == MODE_L2D, RT>(X + (int64_t)r * ld, qrow, ld, lane);
      if (lane == 0) ek[j] = exact_key<MODE>((float)acc, q, r, qn, xn, qinv, xinv);
    }
  }
  __syncthreads();
  // rank sort of (key, row); empty slots last, in slot order among themselves
  float* ok = okey + (int64_t)q * KP;
  int* oi = oid + (int64_t)q * KP;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int s = lane + 64 * e;
    if (s < KF) {
      const float k0 = ek[s];
      const int i0 = id[e] < 0 ? INT_MAX : id[e];
      int rank = 0;
      for (int j = 0; j < KF; ++j) {
        const float kj = ek[j];
        const int ij = sid[j] < 0 ? INT_MAX : sid[j];
        rank += (lex_less(kj, ij, k0, i0) || (kj == k0 && ij == i0 && j < s)) ? 1 : 0;
      }
      ok[rank] = k0;
      oi[rank] = id[e];  // -1 for empty slots
      if (rank == M - 1) eMs = k0;  // the M-th exact key
    } else if (s < KP) {
      ok[s] = FLT_MAX;
      oi[s] = -1;
    }
  }
  __syncthreads();
  const float eM = eMs;
  const double bkey = bound_key(MODE, ba, qh2, qr2,
                                MODE == MODE_L2 || MODE == MODE_L2D ? (double)qn[q] : qn2, stats);
  const bool pass = !bounded || ((double)T - bkey > (double)eM && isfinite(T) && isfinite(eM) &&
                                  isfinite(bkey));
  if (lane == 0) fail[q] = pass ? 0 : 1;
}

hipError_t launch_verify_rescore(const VerifyArgs& v, int nq, const float* Dk, const int64_t* Ik,
                                 const int* qcount, hipStream_t st) {
  const int KF = v.KF;
  if (KF > kVerifyMaxKF || v.KP > kVerifyMaxKF || KF > v.KP || v.M < 1 || v.M > KF ||
      v.ld % 4 != 0 || v.L < 1 || v.L > v.lists.KP || (v.xesize != 4 && v.xesize != 2))
    return hipErrorInvalidValue;
  if (nq <= 0) return hipSuccess;
#define VS_VERIFY_T(MD, NE, RT)                                                                   \
  hipLaunchKernelGGL((verify_rescore_kernel<MD, NE, RT>), dim3(nq), dim3(64), 0, st, KF, v.M, Dk, \
                     Ik, (const RT*)v.X, v.xn, v.Q, v.qn, v.ld, v.ba, v.stats, v.lists.key,       \
                     v.lists.id, v.lists.P, v.lists.KP, v.L, v.okey, v.oid, v.KP, v.fail, v.qinv, \
                     v.xinv, v.qr2i8, qcount, v.qcut)
#define VS_VERIFY(MD, NE)                  \
  do {                                     \
    if (v.xesize == 4)                     \
      VS_VERIFY_T(MD, NE, float);          \
    else                                   \
      VS_VERIFY_T(MD, NE, uint16_t);       \
  } while (0)
#define VS_VERIFY_NE(MD)   \
  do {                     \
    if (KF <= 64)          \
      VS_VERIFY(MD, 1);    \
    else if (KF <= 128)    \
      VS_VERIFY(MD, 2);    \
    else if (KF <= 256)    \
      VS_VERIFY(MD, 4);    \
    else if (KF <= 512)    \
      VS_VERIFY(MD, 8);    \
    else                   \
      VS_VERIFY(MD, 16);   \
  } while (0)
  if (v.mode == MODE_IP)
    VS_VERIFY_NE(MODE_IP);
  else if (v.mode == MODE_L2)
    VS_VERIFY_NE(MODE_L2);
  else if (v.mode == MODE_L2D)
    VS_VERIFY_NE(MODE_L2D);
  else if (v.mode == MODE_COS && v.qinv && v.xinv)
    VS_VERIFY_NE(MODE_COS);
  else
    return hipErrorInvalidValue;
#undef VS_VERIFY_NE
#undef VS_VERIFY
#undef VS_VERIFY_T
  return hipGetLastError();
}

// Flagged queries -> ascending list qlist[0 .. *count) (one workgroup; a
// block-wide prefix count per 1024-query chunk).  Running statistics: adds
// the count to *total and n to *total_n (when not null).
__global__ __launch_bounds__(1024) void compact_flags_kernel(const int* __restrict__ flags, int n,
                                                             int* __restrict__ list,
                                                             int* __restrict__ count,
                                                             unsigned long long* __restrict__ total,
                                                             unsigned long long* __restrict__ total_n) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + tid;
    const int f = i < n && flags[i] != 0 ? 1 : 0;
    const uint64_t bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int j = 0; j < wv; ++j) off += wsum[j];
    if (f) list[off + before] = i;
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int j = 0; j < 16; ++j) s += wsum[j];
      base += s;
    }
    __syncthreads();
  }
  if (tid == 0) {
    *count = base;
    if (total) atomicAdd(total, (unsigned long long)base);
    if (total_n) atomicAdd(total_n, (unsigned long long)n);
  }
}

// acc[0] += n, acc[1] += *count (one thread; a per-index record of a stage)
__global__ void add_counts_kernel(const int* __restrict__ count, int n,
                                  unsigned long long* __restrict__ acc) {
  // atomic: searches of one index on two streams may run this concurrently
  atomicAdd(acc + 0, (unsigned long long)n);
  atomicAdd(acc + 1, (unsigned long long)*count);
}

hipError_t launch_add_counts(const int* count, int n, unsigned long long* acc, hipStream_t st) {
  hipLaunchKernelGGL(add_counts_kernel, dim3(1), dim3(1), 0, st, count, n, acc);
  return hipGetLastError();
}

hipError_t launch_compact_flags(const int* flags, int n, int* list, int* count,
                                unsigned long long* total, unsigned long long* total_n,
                                hipStream_t st) {
  if (n < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compact_flags_kernel, dim3(1), dim3(1024), 0, st, flags, n, list, count,
                     total, total_n);
  return hipGetLastError();
}

// Wide verification of the flagged queries qlist[0 .. *count) (one 256-thread
// workgroup per flagged query, a fixed grid striding over the device-side
// count, so the host never reads it).  The condition above only needs a
// threshold T such that every row outside the rescored set has approximate key
// >= T: the smallest last entry of the full lane lists is one (a full list
// dropped only rows lexicographically after its last entry), and then the set
// may be *all* list entries below T, not just the KF merged ones.  More than
// kWideCap entries below T, fewer than M, or a non-finite key: the query stays
// flagged.  The KF merged candidates the first check rescored (Dk/Ik, exact
// keys in okey/oid) keep their exact keys: an entry lexicographically at or
// before the KF-th merged one is one of them, and only the others are read
// from HBM again (C4: ~40 % of the wide set).
template <int MODE, typename RT>
__global__ __launch_bounds__(256) void verify_wide_kernel(
    const int* __restrict__ qlist, const int* __restrict__ count, int KF, int M,
    const RT* __restrict__ X, const float* __restrict__ xn, const float* __restrict__ Q,
    const float* __restrict__ qn, int64_t ld, BoundArgs ba, const unsigned* __restrict__ stats,
    const float* __restrict__ lkey, const int* __restrict__ lid, int P, int LKP, int L,
    float* __restrict__ okey, int* __restrict__ oid, int KP, int* __restrict__ fail,
    const float* __restrict__ qinv, const float* __restrict__ xinv, const float* __restrict__ qr2i8,
    const float* __restrict__ Dk, const int64_t* __restrict__ Ik,
    unsigned long long* __restrict__ sizes, const float* __restrict__ qcut) {
  __shared__ float ck[kWideCap];
  __shared__ int cid[kWideCap];
  // the first check's exact keys (KP <= kVerifyMaxKF) / the reused ones
  __shared__ float rk[kVerifyMaxKF], kk[kVerifyMaxKF];
  __shared__ int ri[kVerifyMaxKF], ki[kVerifyMaxKF];
  __shared__ int cntk;
  __shared__ float wT[4];
  __shared__ int wB[4];
  __shared__ int cnt, bad;
  __shared__ float eMs;
  __shared__ double qs[3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nflag = *count;
  for (int jq = blockIdx.x; jq < nflag; jq += gridDim.x) {
    const int q = qlist[jq];
    const int64_t lbase = (int64_t)q * P * LKP;
    float T = FLT_MAX;
    bool bounded = false;
    for (int j = tid; j < P; j += 256) {
      const int64_t o = lbase + (int64_t)j * LKP + L - 1;
      if (lid[o] >= 0) {
        bounded = true;
        T = fminf(T, lkey[o]);
      }
    }
    for (int o = 32; o > 0; o >>= 1) T = fminf(T, __shfl_xor(T, o));
    bounded = __any(bounded);
    if (lane == 0) {
      wT[wv] = T;
      wB[wv] = bounded ? 1 : 0;
    }
    if (tid == 0) {
      cnt = 0;
      cntk = 0;
      bad = 0;
      eMs = FLT_MAX;
    }
    for (int t = tid; t < kVerifyMaxKF; t += 256) {  // the first check's output (KP entries)
      rk[t] = t < KP ? okey[(int64_t)q * KP + t] : FLT_MAX;
      ri[t] = t < KP ? oid[(int64_t)q * KP + t] : -1;
    }
    const float* qrow = Q + (int64_t)q * ld;
    if (wv == 0) {
      double a, b, c;
      query_split_norms(qrow, ld, lane, qr2i8 ? qr2i8 + q : nullptr, a, b, c, ba.aug_q2);
      if (lane == 0) {
        qs[0] = a;
        qs[1] = b;
        qs[2] = c;
      }
    }
    __syncthreads();
    T = fminf(fminf(wT[0], wT[1]), fminf(wT[2], wT[3]));
    bounded = (wB[0] | wB[1] | wB[2] | wB[3]) != 0;
    if (qcut && qcut[q] < FLT_MAX) {  // the pass dropped every row at or above the cut
      bounded = true;
      T = fminf(T, qcut[q]);
    }
    const double bkey =
        bound_key(MODE, ba, qs[0], qs[1],
                  MODE == MODE_L2 || MODE == MODE_L2D ? (double)qn[q] : qs[2], stats);
    // Any threshold T' <= T works (every row outside the set still has an
    // approximate key >= T'): with a_M the M-th smallest approximate key (the
    // merge's Dk), the M best-approximate rows have exact keys <= a_M + B, so
    // T' = a_M + 2B passes the check whenever it is below T, and rescoring only
    // the entries below T' keeps the set small when the lists reach deep (many
    // lists per query: T far behind the top).
    // Tighter still: e1_M, the M-th exact key among the first check's KF rows,
    // bounds E_M from above, and every row with approximate key >= e1_M + B has
    // an exact key > e1_M >= E_M; those M rows (approximate keys <= e1_M + B)
    // stay in the set.  T' = e1_M + B is ~a_M + B: half the window of a_M + 2B.
    if (bounded && Dk) {
      const float aM = Dk[(int64_t)q * KF + M - 1];
      double tp = (double)aM + 2.000001 * bkey;
      if (ri[M - 1] >= 0 && isfinite(rk[M - 1]))
        tp = fmin(tp, (double)rk[M - 1] + 1.000001 * bkey);
      if (isfinite(tp) && tp < (double)T) {
        float t = (float)tp;
        if ((double)t < tp) t = nextafterf(t, INFINITY);
        T = fminf(T, t);
      }
    }
    // the KF-th merged entry: entries up to it were rescored by the first check
    // (all of them when the merge found fewer than KF)
    const float kfk = Dk ? Dk[(int64_t)q * KF + KF - 1] : -FLT_MAX;
    const int kfi = Dk ? (int)Ik[(int64_t)q * KF + KF - 1] : INT_MIN;
    // gather every entry below T (all entries when no list is full)
    for (int j = tid; j < P * L; j += 256) {
      const int64_t o = lbase + (int64_t)(j / L) * LKP + j % L;
      const int r = lid[o];
      const float lk = lkey[o];
      if (r >= 0 && (!bounded || lk < T)) {
        int hit = -1;
        if (Dk && (kfi < 0 || !lex_less(kfk, kfi, lk, r)))
          for (int t = 0; t < KP; ++t) hit = ri[t] == r ? t : hit;
        if (hit >= 0) {
          const int s = atomicAdd(&cntk, 1);
          if (s < kVerifyMaxKF) {
            kk[s] = rk[hit];
            ki[s] = r;
          }
        } else {
          const int s = atomicAdd(&cnt, 1);
          if (s < kWideCap) cid[s] = r;
        }
      }
    }
    __syncthreads();
    const int nu = cnt;  // rows to rescore
    const int nk = min(cntk, kVerifyMaxKF);
    const int n = nu + cntk;
    if (sizes && tid == 0) {
      atomicAdd(sizes, (unsigned long long)n);
      atomicAdd(sizes + 1, (unsigned long long)nu);
    }
    if (!(n > kWideCap || n < M || !isfinite(T))) {  // uniform
      auto put = [&](int j, int r, double acc) {
        if (lane == 0) {
          const float key = exact_key<MODE>((float)acc, q, r, qn, xn, qinv, xinv);
          ck[j] = key;
          if (!isfinite(key)) bad = 1;
        }
      };
      if (ld <= 256 * kQV) {  // two rows per wave step, the query in registers
        QSlice qsl;
        load_qslice(qrow, ld, lane, qsl);
        for (int j = wv; j < nu; j += 8) {
          const int ra = cid[j], rb = j + 4 < nu ? cid[j + 4] : ra;
          double da, db;
          wave_dot2<MODE == MODE_L2D, RT>(X + (int64_t)ra * ld, X + (int64_t)rb * ld, qsl, ld, lane, da,
                                      db);
          put(j, ra, da);
          if (j + 4 < nu) put(j + 4, rb, db);
        }
      } else {
        for (int j = wv; j < nu; j += 4) {
          const int r = cid[j];
          put(j, r, wave_dot<MODE == MODE_L2D, RT>(X + (int64_t)r * ld, qrow, ld, lane));
        }
      }
      for (int t = tid; t < nk; t += 256) {  // the reused exact keys after the rescored ones
        ck[nu + t] = kk[t];
        cid[nu + t] = ki[t];
        if (!isfinite(kk[t])) bad = 1;
      }
      __syncthreads();
      if (!bad) {  // uniform
        // rank of each (key, row) among the n (rows are distinct: the lists are disjoint)
        float* ok = okey + (int64_t)q * KP;
        int* oi = oid + (int64_t)q * KP;
        for (int j = tid; j < n; j += 256) {
          const float kj = ck[j];
          const int ij = cid[j];
          int rank = 0;
          for (int t = 0; t < n; ++t) rank += lex_less(ck[t], cid[t], kj, ij) ? 1 : 0;
          if (rank < KF) {
            ok[rank] = kj;
            oi[rank] = ij;
          }
          if (rank == M - 1) eMs = kj;
        }
        for (int j = min(n, KF) + tid; j < KP; j += 256) {
          ok[j] = FLT_MAX;
          oi[j] = -1;
        }
        __syncthreads();
        const float eM = eMs;
        const bool pass =
            !bounded || ((double)T - bkey > (double)eM && isfinite(eM) && isfinite(bkey));
        if (tid == 0 && pass) fail[q] = 0;
      }
    }
    __syncthreads();  // the shared state is reused by the next flagged query
  }
}

hipError_t launch_verify_wide(const VerifyArgs& v, int nq_max, const int* qlist, const int* count,
                              const float* Dk, const int64_t* Ik, unsigned long long* sizes,
                              hipStream_t st) {
  if (v.KF > v.KP || v.KP > kVerifyMaxKF || (Dk && !Ik) || v.M < 1 || v.M > v.KF ||
      v.ld % 4 != 0 || v.L < 1 || v.L > v.lists.KP || (v.xesize != 4 && v.xesize != 2))
    return hipErrorInvalidValue;
  if (nq_max <= 0) return hipSuccess;
  const int grid = std::min(nq_max, 2048);
#define VS_WIDE_T(MD, RT)                                                                        \
  hipLaunchKernelGGL((verify_wide_kernel<MD, RT>), dim3(grid), dim3(256), 0, st, qlist, count,   \
                     v.KF, v.M, (const RT*)v.X, v.xn, v.Q, v.qn, v.ld, v.ba, v.stats,            \
                     v.lists.key, v.lists.id, v.lists.P, v.lists.KP, v.L, v.okey, v.oid, v.KP,   \
                     v.fail, v.qinv, v.xinv, v.qr2i8, Dk, Ik, sizes, v.qcut)
#define VS_WIDE(MD)             \
  do {                          \
    if (v.xesize == 4)          \
      VS_WIDE_T(MD, float);     \
    else                        \
      VS_WIDE_T(MD, uint16_t);  \
  } while (0)
  if (v.mode == MODE_IP)
    VS_WIDE(MODE_IP);
  else if (v.mode == MODE_L2)
    VS_WIDE(MODE_L2);
  else if (v.mode == MODE_L2D)
    VS_WIDE(MODE_L2D);
  else if (v.mode == MODE_COS && v.qinv && v.xinv)
    VS_WIDE(MODE_COS);
  else
    return hipErrorInvalidValue;
#undef VS_WIDE
#undef VS_WIDE_T
  return hipGetLastError();
}

// bkey[q]: the bound B of query q (bound_key over its split norms, the same
// double the verification computes).
template <int MODE>
__global__ __launch_bounds__(64) void qbound_kernel(const float* __restrict__ Q, int64_t ld,
                                                    const float* __restrict__ qn, BoundArgs ba,
                                                    const unsigned* __restrict__ stats,
                                                    const float* __restrict__ qr2i8, int nq,
                                                    double* __restrict__ bkey) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  if (q >= nq) return;
  double qh2, qr2, qn2;
  query_split_norms(Q + (int64_t)q * ld, ld, lane, qr2i8 ? qr2i8 + q : nullptr, qh2, qr2, qn2,
                    ba.aug_q2);
  if (ba.rows_exact) {  // the fp32 GEMM multiplied q itself (as verify_rescore_kernel)
    qh2 = qn2;
    qr2 = 0.0;
  }
  double b = bound_key(MODE, ba, qh2, qr2,
                                MODE == MODE_L2 || MODE == MODE_L2D ? (double)qn[q] : qn2, stats);
  // the augmented L2 pass cuts its lists in the inner-product keys A, whose
  // map qn + 2A doubles distances: half the L2 bound there
  if (ba.l2aug) b *= 0.5;
  if (lane == 0) bkey[q] = b;
}

hipError_t launch_qbound(int mode, const float* Q, int64_t ld, const float* qn, int filter,
                         const unsigned* stats, const float* qr2i8, int nq, double* bkey,
                         hipStream_t st, const BoundArgs* bap) {
  if (nq <= 0) return hipSuccess;
  if (ld % 4 != 0) return hipErrorInvalidValue;
  const BoundArgs ba = bap ? *bap : make_bound_args(ld, filter);
#define VS_QB(MD) \
  hipLaunchKernelGGL(qbound_kernel<MD>, dim3(nq), dim3(64), 0, st, Q, ld, qn, ba, stats, qr2i8, nq, bkey)
  if (mode == MODE_IP)
    VS_QB(MODE_IP);
  else if (mode == MODE_L2)
    VS_QB(MODE_L2);
  else if (mode == MODE_COS)
    VS_QB(MODE_COS);
  else if (mode == MODE_L2D)  // the range search's small L2 calls (the extra norm term)
    VS_QB(MODE_L2D);
  else
    return hipErrorInvalidValue;
#undef VS_QB
  return hipGetLastError();
}

// The KF = 128 or 256 best approximate candidates of each query (KF <= 64 goes
// through merge_lists_kernel, whose register lists would not hold 128): one
// 256-thread workgroup per query finds the KF-th smallest 64-bit image
// (key order << 32 | row; a query's lists hold distinct rows) of its P lists of
// L entries by a radix select, keeps the entries at or below it and ranks
// them.  Writes Dk/Ik [nq][KF] ascending (FLT_MAX / -1 padding).
__global__ __launch_bounds__(256) void select_lists_kernel(const float* __restrict__ lkey,
                                                           const int* __restrict__ lid, int P,
                                                           int LKP, int L, int KF,
                                                           float* __restrict__ Dk,
                                                           int64_t* __restrict__ Ik,
                                                           const int* __restrict__ qcount) {
  __shared__ int wsum[4];
  __shared__ unsigned long long sel[kVerifyMaxKF];
  __shared__ int nsel;
  __shared__ int hist[256];
  __shared__ int sel_digit, sel_before;
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (qcount && q >= *qcount) return;  // gathered batch: slots past the count
  const int64_t base = (int64_t)q * P * LKP;
  const int n = P * L;
  constexpr int kR = 16;
  constexpr unsigned long long kNone = ~0ull;
  unsigned long long v[kR];
  const bool regs = n <= 256 * kR;  // uniform
  auto image = [&](int j) -> unsigned long long {
    const int64_t o = base + (int64_t)(j / L) * LKP + j % L;
    const int r = lid[o];
    return r >= 0 ? ((unsigned long long)key_order(lkey[o]) << 32) | (uint32_t)r : kNone;
  };
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const int j = tid + 256 * i;
    v[i] = regs && j < n ? image(j) : kNone;
  }
  auto count_le = [&](unsigned long long y) {  // entries with image <= y (workgroup-wide)
    int c = 0;
    if (regs) {
#pragma unroll
      for (int i = 0; i < kR; ++i) c += v[i] <= y && v[i] != kNone ? 1 : 0;
    } else {
      for (int j = tid; j < n; j += 256) {
        const unsigned long long x = image(j);
        c += x <= y && x != kNone ? 1 : 0;
      }
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __syncthreads();
    if (lane == 0) wsum[wv] = c;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
  };
  const int total = count_le(kNone - 1);
  const int M = total < KF ? total : KF;
  // the M-th smallest image y, by a radix select over its eight bytes from the
  // top: per byte a 256-bin histogram of the entries that share the bytes
  // chosen so far, the bin where the running count reaches the rank left
  // (8 passes over the entries instead of a bitwise search's 64: one query's
  // select is one workgroup's latency, a batch-1 search waits for all of it)
  unsigned long long y = kNone - 1;
  if (M > 0 && M < total) {
    unsigned long long pre = 0;
    int want = M;  // rank of y among the entries that share pre's chosen bytes
    for (int sh = 56; sh >= 0; sh -= 8) {
      hist[tid] = 0;  // 256 threads, 256 bins
      __syncthreads();
      auto add = [&](unsigned long long x) {
        if (x != kNone && (sh == 56 || (x >> (sh + 8)) == (pre >> (sh + 8))))
          atomicAdd(&hist[(int)((x >> sh) & 0xFF)], 1);
      };
      if (regs) {
#pragma unroll
        for (int i = 0; i < kR; ++i) add(v[i]);
      } else {
        for (int j = tid; j < n; j += 256) add(image(j));
      }
      __syncthreads();
      if (wv == 0) {  // the bin where the running count reaches `want`
        const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2],
                  h3 = hist[4 * lane + 3];
        const int own = h0 + h1 + h2 + h3;
        int inc = own;  // inclusive prefix over the lanes
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(inc, o);
          if (lane >= o) inc += t;
        }
        const int before = inc - own;
        if (before < want && want <= inc) {
          int c = before, d = 4 * lane;
          const int hh[4] = {h0, h1, h2, h3};
          for (int e = 0; e < 4; ++e) {
            if (c + hh[e] >= want) {
              d = 4 * lane + e;
              break;
            }
            c += hh[e];
          }
          sel_digit = d;
          sel_before = c;
        }
      }
      __syncthreads();
      pre |= (unsigned long long)sel_digit << sh;
      want -= sel_before;
      __syncthreads();  // hist and the broadcast are rewritten by the next byte
    }
    y = pre;  // the entries are distinct: y is the M-th smallest image
  }
  if (tid == 0) nsel = 0;
  __syncthreads();
  auto take = [&](unsigned long long x) {
    if (x != kNone && x <= y) {
      const int s = atomicAdd(&nsel, 1);
      if (s < kVerifyMaxKF) sel[s] = x;
    }
  };
  if (M > 0) {
    if (regs) {
#pragma unroll
      for (int i = 0; i < kR; ++i) take(v[i]);
    } else {
      for (int j = tid; j < n; j += 256) take(image(j));
    }
  }
  __syncthreads();
  float* dk = Dk + (int64_t)q * KF;
  int64_t* ik = Ik + (int64_t)q * KF;
  for (int t = tid; t < KF; t += 256) {
    if (t < M) {
      const unsigned long long x = sel[t];
      int rank = 0;
      for (int j = 0; j < M; ++j) rank += sel[j] < x ? 1 : 0;
      dk[rank] = key_unorder((uint32_t)(x >> 32));
      ik[rank] = (int64_t)(uint32_t)(x & 0xFFFFFFFFull);
    } else {
      dk[t] = FLT_MAX;
      ik[t] = -1;
    }
  }
}

hipError_t launch_select_lists(Partials part, int L, int nq, int KF, float* Dk, int64_t* Ik,
                               hipStream_t st, const int* qcount) {
  if (KF < 1 || KF > kVerifyMaxKF || L < 1 || L > part.KP || part.P < 1) return hipErrorInvalidValue;
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(select_lists_kernel, dim3(nq), dim3(256), 0, st, part.key, part.id, part.P,
                     part.KP, L, KF, Dk, Ik, qcount);
  return hipGetLastError();
}

// The KF <= 64 best approximate candidates of each query from its P sorted
// lane lists of 8 entries (stride 8), by a bound from the lists' heads instead
// of merge_lists_kernel's six rounds of 32-entry merges (C2: 35-38 us vs the
// merge's 94 in two levels, profiles/r06tl2).  The KF-th smallest head U (lexicographic (key, row);
// a query's lists hold distinct rows) bounds the KF-th smallest entry: the KF
// lists of the smallest heads hold KF entries <= U.  Only those lists can hold
// an entry <= U, so at most 8 KF entries (<= 512) are kept and ranked.  Fewer
// than KF non-empty lists: every entry is kept.  Same output as the merge:
// Dk/Ik [nq][KF] ascending, (FLT_MAX, -1) padding.
constexpr int kHeadsMaxP = 512;
constexpr int kHeadsMaxKF = 64;
__global__ __launch_bounds__(256) void select_heads_kernel(const float* __restrict__ lkey,
                                                           const int* __restrict__ lid, int P,
                                                           int KF, float* __restrict__ Dk,
                                                           int64_t* __restrict__ Ik,
                                                           const int* __restrict__ qcount) {
  __shared__ float hk[kHeadsMaxP];
  __shared__ int hi[kHeadsMaxP];
  __shared__ float ck[8 * kHeadsMaxKF];
  __shared__ int ci[8 * kHeadsMaxKF];
  __shared__ int cnt, ui;
  __shared__ float uk;
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  if (qcount && q >= *qcount) return;  // gathered batch: slots past the count
  const int64_t base = (int64_t)q * P * 8;
  for (int p = tid; p < P; p += 256) {
    hk[p] = lkey[base + (int64_t)p * 8];
    hi[p] = lid[base + (int64_t)p * 8];
  }
  if (tid == 0) {
    cnt = 0;
    ui = -1;  // no bound: fewer than KF non-empty lists
    uk = FLT_MAX;
  }
  __syncthreads();
  for (int p = tid; p < P; p += 256) {
    const float k0 = hk[p];
    const int i0 = hi[p];
    if (i0 < 0) continue;
    int r = 0;
    for (int t = 0; t < P; ++t) r += hi[t] >= 0 && lex_less(hk[t], hi[t], k0, i0) ? 1 : 0;
    if (r == KF - 1) {
      uk = k0;
      ui = i0;
    }
  }
  __syncthreads();
  const float U = uk;
  const int Ui = ui;
  for (int p = tid; p < P; p += 256) {
    if (Ui >= 0 && lex_less(U, Ui, hk[p], hi[p])) continue;  // head above the bound
    const f32x4* kp = (const f32x4*)(lkey + base + (int64_t)p * 8);
    const int4* ip = (const int4*)(lid + base + (int64_t)p * 8);
    const f32x4 ka = kp[0], kb = kp[1];
    const int4 ia = ip[0], ib = ip[1];
    const float kk[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
    const int ii[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (ii[j] < 0 || (Ui >= 0 && lex_less(U, Ui, kk[j], ii[j]))) break;  // sorted: the rest too
      const int s = atomicAdd(&cnt, 1);
      if (s < 8 * kHeadsMaxKF) {
        ck[s] = kk[j];
        ci[s] = ii[j];
      }
    }
  }
  __syncthreads();
  // <= 8 KF: at most KF lists pass the head test when bounded
  const int n = min(cnt, 8 * kHeadsMaxKF);
  float* dk = Dk + (int64_t)q * KF;
  int64_t* ik = Ik + (int64_t)q * KF;
  for (int j = tid; j < n; j += 256) {
    const float k0 = ck[j];
    const int i0 = ci[j];
    int r = 0;
    for (int t = 0; t < n; ++t) r += lex_less(ck[t], ci[t], k0, i0) ? 1 : 0;
    if (r < KF) {
      dk[r] = k0;
      ik[r] = i0;
    }
  }
  for (int j = n + tid; j < KF; j += 256) {
    dk[j] = FLT_MAX;
    ik[j] = -1;
  }
}

bool select_heads_applies(const Partials& part, int L, int KF) {
  const char* e = getenv("VS_SELECT_HEADS");  // =0: the list merge (A/B; read at every search)
  if (e && atoi(e) == 0) return false;
  return L == 8 && part.KP == 8 && KF >= 1 && KF <= kHeadsMaxKF && part.P >= KF &&
         part.P <= kHeadsMaxP;
}

hipError_t launch_select_heads(Partials part, int nq, int KF, float* Dk, int64_t* Ik,
                               hipStream_t st, const int* qcount) {
  if (!select_heads_applies(part, 8, KF)) return hipErrorInvalidValue;
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(select_heads_kernel, dim3(nq), dim3(256), 0, st, part.key, part.id, part.P,
                     KF, Dk, Ik, qcount);
  return hipGetLastError();
}

// Bound constants for `ld` K elements (see "Verification" above).  bf16: the MFMA's fp32
// accumulation.  int8: the int32 sum is exact (|code| <= 127, ld <= kI8MaxLd),
// and the approximate score fl(fl(float(sum)) * fl(f_q * f_x)) carries three
// roundings for IP (f = s), five for the cosine (f = fl(s * inverse norm)), so
// approx = hi(x).hi(q) (1 + d), |d| <= (1 + 2^-24)^5 - 1 < 6 * 2^-24; for the
// cosine the key then needs no further rounding term (the 2^-22 kept below is
// slack).
BoundArgs make_bound_args(int64_t ld, int filter) {
  BoundArgs ba;
  ba.filter = filter;
  const double u = std::ldexp(1.0, -23);
  const double n = (double)ld + 1.0;
  ba.gam = filter == FILTER_I8 ? 6.0 * std::ldexp(1.0, -24) : n * u / (1.0 - n * u);
  // the stored norms are fp32 sums of ld squares: they undercount by at most
  // ~gam(ld), whatever the plane
  ba.norm_inf = 2.0 * (n * u / (1.0 - n * u));
  return ba;
}

BoundArgs make_bound_args_l2aug(int64_t ld, const L2Aug& g, int filter) {
  const bool i8 = filter == FILTER_I8;
  BoundArgs ba = make_bound_args(ld + (i8 ? g.m : kAugBf16), filter);
  ba.l2aug = 1;
  const double c = i8 ? (double)g.C : (double)g.Cb;
  ba.aug_q2 = (i8 ? (double)g.m : (double)kAugBf16) * c * c;
  ba.aug_nref = (double)g.nref;
  return ba;
}

}  // namespace vs
