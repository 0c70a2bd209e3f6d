// vs_range.hip — range search (faiss IndexFlat::range_search): every row whose
// exact key passes the radius, as many as there are ("Range
// search").  The fp32 / bf16 MFMA GEMM of vs_gemm.hip preselects candidates
// against a per-query threshold (the radius widened by the GEMM's rigorous
// error bound), in two passes that take identical decisions — one counts, a
// scan turns the counts into offsets, one fills — and the verification decides
// every candidate by the rescoring's exact key (vs_x1_device.h exact_key).
// The range self-join (vs_range_selfjoin, "Range self-join") runs the same
// passes with the stored rows as queries and the cosine key.
#include <algorithm>
#include <cmath>

#include "vs_exact_tile.h"
#include "vs_x1_device.h"

namespace vs {

// ---------------------------------------------------------------------------
// The candidate passes.  gemm_range runs the exact tile described in
// vs_exact_tile.h (gemm_topk's 128 x 128 tile, glds staging, swizzle and MFMAs;
// the mapping and the keys are that header's) and adds the UPPER tile range and
// an epilogue that tests a row's key against its query's threshold instead of
// keeping lists.  After the K loop a lane holds, for ONE query, the keys of rows
// 32 s + 8 j + 4 h + i of subtile s (h = its lane half, register (j, i)), so a
// query's hits of a subtile are two 16-bit masks, one per lane half.
//
// FILL = false: cnt[q][split] = the query's candidates among the split's rows
// (the two halves' popcounts, summed in registers across tiles; one store).
// FILL = true: the halves exchange their masks, a hit's rank inside the
// subtile follows ascending row order (j, then h, then i), and the lane writes
// its rows at cand[off[q][split] + hits so far + rank]: a (query, split)
// segment is ascending by row, and the scan is query-major, so a query's
// candidates are contiguous and ascending.  Both passes run the same
// arithmetic on the same grid; should they ever disagree, the fill pass writes
// nothing outside its segment and raises *err (the host fails the call).
//
// MODE_COS (the range self-join): Q is the index's own rows, read in place from
// the call's first query row, qaux / xaux their inverse norms, and the key is
// gemm_topk's cosine expression.  UPPER (a query reports only the rows after
// it): query tile qt starts its row tiles at the one that holds its first
// query row, row qrow0 + qt * kBQ, and its splits divide that range — a row
// tile wholly below the diagonal is never loaded; both passes derive the range
// from this one expression.  The rows r <= q of the tiles on the diagonal are
// left to the verification.
template <int MODE, typename T, bool FILL, bool UPPER = false>
__global__ __launch_bounds__(256, 2) void gemm_range(
    const T* __restrict__ X, const float* __restrict__ xaux, const T* __restrict__ Q,
    const float* __restrict__ qaux, int64_t ld, int nstage, int ntotal, int ntiles, int nsplit,
    int nqt, const float* __restrict__ thr, int* __restrict__ cnt,
    const int64_t* __restrict__ off, int* __restrict__ cand, int* __restrict__ err,
    int qrow0) {
  static_assert(!UPPER || MODE == MODE_COS, "the triangle is the self-join's");
  static_assert(sizeof(T) == 4 || sizeof(T) == 2, "fp32 or bf16 rows");
  // [buf][X|Q][128 rows][128 B]; viewed as floats (32 per row) for addressing.
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * kBN * kBK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int h = lane >> 5;
  const int c32 = lane & 31;

  const int lb = tile_logical_block();
  const int qt = lb % nqt;
  const int sp = lb / nqt;
  int t0, t1;
  if constexpr (UPPER) {
    const int tlo = min((qrow0 + qt * kBQ) / kBN, ntiles);
    tile_split_range(sp, ntiles - tlo, nsplit, t0, t1);
    t0 += tlo;
    t1 += tlo;
  } else {
    tile_split_range(sp, ntiles, nsplit, t0, t1);
  }

  const int qloc = 32 * w + c32;
  const int gq = qt * kBQ + qloc;
  float qa = 0.0f;
  if constexpr (MODE == MODE_L2 || MODE == MODE_COS) qa = qaux[gq];
  const float th = thr[gq];
  const int64_t seg = (int64_t)gq * nsplit + sp;
  int64_t base = 0, end = 0;
  if constexpr (FILL) {
    base = off[seg];
    end = off[seg + 1];
  }
  int run = 0;  // count pass: this half's hits; fill pass: the query's hits so far

  const T* Qblk = Q + (int64_t)qt * kBQ * ld;
  // glds geometry: a wave instruction moves 8 rows x 128 B; wave w stages row
  // groups g = 4w..4w+3 of both operands.  The per-lane source offset is 32-bit
  // on a wave-uniform base (saddr form); the swizzle (row >> 1) & 7 depends on
  // the group only through g & 1, so two lane offsets cover all four groups.
  const int srow = lane >> 3;
  const int sphys = lane & 7;
  const uint32_t ldb = (uint32_t)ld * (uint32_t)sizeof(T);  // row stride in bytes
  uint32_t soff[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int row = par * 8 + srow;  // any group with g & 1 == par has this swizzle
    soff[par] = (uint32_t)(w * 32 + srow) * ldb + tile_chunk(sphys, row);
  }
  // fragment-read geometry: (row >> 1) & 7 is the same for every subtile.
  const int fsw = (c32 >> 1) & 7;

  for (int t = t0; t < t1; ++t) {
    const char* Xblk = (const char*)(X + (int64_t)t * kBN * ld);
    f32x16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;
    }

    auto stage = [&](int buf, int kb) {
      float* dX = smem + buf * (2 * kBN * kBK);
      float* dQ = dX + kBN * kBK;
      const char* xs = Xblk + kb;
      const char* qs = (const char*)Qblk + kb;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g = w * 4 + i;
        const uint32_t o = soff[i & 1] + (uint32_t)(i * 8) * ldb;
        __builtin_amdgcn_global_load_lds(xs + o, VS_LDS(dX + g * 256), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(qs + o, VS_LDS(dQ + g * 256), 16, 0, 0);
      }
    };

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int st = 0; st < nstage; ++st) {
      if (st + 1 < nstage) stage((st + 1) & 1, (st + 1) * 128);
      const float* cX = smem + (st & 1) * (2 * kBN * kBK);
      const float* cQ = cX + kBN * kBK;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int coff = ((kc * 2 + h) ^ fsw) * 4;
        const f32x4 bq = *(const f32x4*)(cQ + qloc * kBK + coff);
        f32x4 ax[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) ax[s] = *(const f32x4*)(cX + (32 * s + c32) * kBK + coff);
        if constexpr (sizeof(T) == 4) {
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
              acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[s][tt], bq[tt], acc[s], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ax[s]),
                                                            __builtin_bit_cast(bf16x8, bq),
                                                            acc[s], 0, 0, 0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }

    // Epilogue, one 32-row subtile at a time: scores -> keys (gemm_key) -> the
    // 16-bit mask of the rows at or below the threshold.
    const int r0 = t * kBN;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint32_t m = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rb = r0 + 32 * s + 8 * j + 4 * h;
        f32x4 xa = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE == MODE_L2 || MODE == MODE_COS) xa = *(const f32x4*)(xaux + rb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rb + i;
          const float v = acc[s][j * 4 + i];
          const float key = gemm_key<MODE>(v, qa, xa[i]);
          const bool hit = row < ntotal && key <= th;  // a NaN key or threshold: no
          m |= (uint32_t)hit << (j * 4 + i);
        }
      }
      if constexpr (!FILL) {
        run += __popc(m);
      } else {
        const uint32_t mo = (uint32_t)__shfl_xor((int)m, 32);  // the other half's mask
        uint32_t mm = m;
        while (mm) {
          const int bi = __builtin_ctz(mm);
          mm &= mm - 1;
          // the rows before this one: this half's lower bits, and the other
          // half's rows of the groups j' < j (h = 0) or j' <= j (h = 1)
          const int rank = __popc(m & ((1u << bi) - 1u)) +
                           __popc(mo & ((1u << (4 * ((bi >> 2) + h))) - 1u));
          const int64_t pos = base + run + rank;
          const int row = r0 + 32 * s + (bi & 3) + 8 * (bi >> 2) + 4 * h;
          if (pos < end) cand[pos] = row;
          else *err = 1;
        }
        run += __popc(m) + __popc(mo);
      }
    }
  }

  if constexpr (!FILL) {
    const int tot = run + __shfl_xor(run, 32);
    if (h == 0) cnt[seg] = tot;
  } else {
    if (base + run != end) *err = 1;
  }
}

template <int MODE, bool UPPER = false>
static hipError_t gemm_range_mode(bool fill, const void* X, const float* xaux, const void* Q,
                                  const float* qaux, int64_t ld, int esize, int ntotal,
                                  int nq_pad, int nsplit, const float* thr, int* cnt,
                                  const int64_t* off, int* cand, int* err, hipStream_t st,
                                  int qrow0 = 0) {
  const int ntiles = (ntotal + kBN - 1) / kBN;
  const int nqt = nq_pad / kBQ;
  const int nblk = nqt * nsplit;
  const int nstage = (int)(ld * esize / 128);
#define VS_RANGE_GO(T, FILL)                                                                   \
  hipLaunchKernelGGL((gemm_range<MODE, T, FILL, UPPER>), dim3(nblk), dim3(256), 0, st,         \
                     (const T*)X, xaux, (const T*)Q, qaux, ld, nstage, ntotal, ntiles, nsplit, \
                     nqt, thr, cnt, off, cand, err, qrow0)
  if (esize == 4) {
    if (fill) VS_RANGE_GO(float, true);
    else VS_RANGE_GO(float, false);
  } else {
    if (fill) VS_RANGE_GO(uint16_t, true);
    else VS_RANGE_GO(uint16_t, false);
  }
#undef VS_RANGE_GO
  return hipGetLastError();
}

hipError_t launch_gemm_range(bool fill, int mode, const void* X, const float* xaux, const void* Q,
                             const float* qaux, int64_t ld, int esize, int ntotal, int nq_pad,
                             int nsplit, const float* thr, int* cnt, const int64_t* off,
                             int* cand, int* err, hipStream_t st, int64_t upper_q0) {
  if (nq_pad <= 0 || nq_pad % kBQ != 0 || (ld * esize) % 128 != 0 || (esize != 4 && esize != 2) ||
      ntotal <= 0 || nsplit < 1 || !thr || (fill ? (!off || !cand || !err) : !cnt))
    return hipErrorInvalidValue;
  if (upper_q0 >= 0 && mode != MODE_COS) return hipErrorInvalidValue;
  if (mode == MODE_IP)
    return gemm_range_mode<MODE_IP>(fill, X, xaux, Q, qaux, ld, esize, ntotal, nq_pad, nsplit, thr,
                                    cnt, off, cand, err, st);
  if (mode == MODE_L2)
    return gemm_range_mode<MODE_L2>(fill, X, xaux, Q, qaux, ld, esize, ntotal, nq_pad, nsplit, thr,
                                    cnt, off, cand, err, st);
  if (mode == MODE_COS) {
    if (!xaux || !qaux || upper_q0 >= ntotal) return hipErrorInvalidValue;
    if (upper_q0 >= 0)
      return gemm_range_mode<MODE_COS, true>(fill, X, xaux, Q, qaux, ld, esize, ntotal, nq_pad,
                                             nsplit, thr, cnt, off, cand, err, st, (int)upper_q0);
    return gemm_range_mode<MODE_COS>(fill, X, xaux, Q, qaux, ld, esize, ntotal, nq_pad, nsplit,
                                     thr, cnt, off, cand, err, st);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// The bound's index maximum where no plane keeps it: out[0] = the bits of the
// largest stored norm (non-negative floats order as their bits), out[1] =
// out[2] = 0.  NaN norms (tombstoned rows, which never match) are left out.
// Two launches, no atomics: per-block maxima, then their maximum.
constexpr int kNormMaxBlocks = 256;

__device__ __forceinline__ unsigned block_max_256(unsigned m, unsigned* sh) {
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  return max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

__global__ __launch_bounds__(256) void range_norm_max_kernel(const float* __restrict__ norms,
                                                             int64_t n,
                                                             unsigned* __restrict__ part) {
  __shared__ unsigned sh[4];
  unsigned m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = norms[i];
    if (a == a) m = max(m, __float_as_uint(a) & 0x7FFFFFFFu);
  }
  m = block_max_256(m, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void range_norm_max_final(const unsigned* __restrict__ part,
                                                            int nparts,
                                                            unsigned* __restrict__ out) {
  __shared__ unsigned sh[4];
  unsigned m = (int)threadIdx.x < nparts ? part[threadIdx.x] : 0u;
  m = block_max_256(m, sh);
  if (threadIdx.x == 0) {
    out[0] = m;
    out[1] = 0u;
    out[2] = 0u;
  }
}

int range_norm_max_parts() { return kNormMaxBlocks; }

hipError_t launch_range_norm_max(const float* norms, int64_t n, unsigned* part, unsigned* out,
                                 hipStream_t st) {
  if (n <= 0 || !part || !out) return hipErrorInvalidValue;
  const int blocks = (int)std::min<int64_t>(kNormMaxBlocks, (n + 255) / 256);
  hipLaunchKernelGGL(range_norm_max_kernel, dim3(blocks), dim3(256), 0, st, norms, n, part);
  hipLaunchKernelGGL(range_norm_max_final, dim3(1), dim3(256), 0, st, part, blocks, out);
  return hipGetLastError();
}

// thr[q] = the radius key + B_q rounded up (a row whose exact key passes the
// radius has its GEMM key within B_q of it, so at or below thr[q]).  A NaN
// radius admits nothing (NaN); a bound that is not finite admits every row
// with a key (+inf); padding queries admit nothing.  bstride = 0: one bound
// for every query (the self-join's cosine bound is a constant).
__global__ __launch_bounds__(256) void range_thr_kernel(const double* __restrict__ bkey, int nq,
                                                        int nq_pad, float radkey,
                                                        float* __restrict__ thr, int bstride) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq_pad) return;
  float t = __builtin_nanf("");
  if (q < nq && radkey == radkey) {
    const double tp = (double)radkey + bkey[(int64_t)q * bstride];
    if (tp == tp) {
      t = (float)tp;
      if ((double)t < tp) t = nextafterf(t, INFINITY);
    } else {
      t = INFINITY;
    }
  }
  thr[q] = t;
}

hipError_t launch_range_thr(const double* bkey, int nq, int nq_pad, float radkey, float* thr,
                            hipStream_t st, int bstride) {
  if (nq < 0 || nq_pad < nq || nq_pad <= 0 || (bstride != 0 && bstride != 1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_thr_kernel, dim3((nq_pad + 255) / 256), dim3(256), 0, st, bkey, nq,
                     nq_pad, radkey, thr, bstride);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Exclusive scan of n counts into n + 1 int64 offsets (off[n] = the total).
// One workgroup (launch_sel_scan's scheme): thread t owns a segment.
__global__ __launch_bounds__(256) void range_scan_kernel(const int* __restrict__ cnt, int64_t n,
                                                         int64_t* __restrict__ off) {
  __shared__ int64_t sh[256];
  const int tid = threadIdx.x;
  const int64_t seg = (n + 255) / 256;
  const int64_t b0 = tid * seg < n ? tid * seg : n, b1 = b0 + seg < n ? b0 + seg : n;
  int64_t s = 0;
  for (int64_t i = b0; i < b1; ++i) s += cnt[i];
  sh[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int i = 0; i < 256; ++i) {
      const int64_t v = sh[i];
      sh[i] = run;
      run += v;
    }
    off[n] = run;
  }
  __syncthreads();
  int64_t run = sh[tid];
  for (int64_t i = b0; i < b1; ++i) {
    off[i] = run;
    run += cnt[i];
  }
}

hipError_t launch_range_scan(const int* cnt, int64_t n, int64_t* off, hipStream_t st) {
  if (n < 0 || !off || (n > 0 && !cnt)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(256), 0, st, cnt, n, off);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Verification: one wave per candidate.  Candidate c belongs to the query q
// with off[q * nsplit] <= c < off[(q + 1) * nsplit]; its exact key is the
// rescoring's (fp64 sum across the wave, rounded once, exact_key<MODE>), and
// the row is a hit iff that key passes faiss's strict comparison (L2: key <
// radius; inner product: score > radius) and, with a selector, its bit is set.
// ekey[c] = the key as a score (distance, or inner product); flag[c] = hit.
template <int MODE, typename RT>
__global__ __launch_bounds__(256) void range_verify_kernel(
    const int* __restrict__ cand, int64_t total, const int64_t* __restrict__ off, int nsplit,
    int nq, const RT* __restrict__ X, const float* __restrict__ xn, const float* __restrict__ Q,
    const float* __restrict__ qn, int64_t ld, int ntotal, float radius,
    const uint32_t* __restrict__ rbits, float* __restrict__ ekey, uint8_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= total) return;
  int lo = 0, hi = nq - 1;  // the last query whose segment starts at or before c
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[(int64_t)mid * nsplit] <= c) lo = mid;
    else hi = mid - 1;
  }
  const int q = lo;
  const int r = cand[c];
  bool live = r >= 0 && r < ntotal;
  if (live && rbits) live = (rbits[r >> 5] >> (r & 31)) & 1u;
  if (!live) {  // wave-uniform
    if (lane == 0) {
      ekey[c] = 0.0f;
      flag[c] = 0;
    }
    return;
  }
  const double acc = wave_dot<MODE == MODE_L2D, RT>(X + (int64_t)r * ld, Q + (int64_t)q * ld, ld, lane);
  const float key = exact_key<MODE>((float)acc, q, r, qn, xn, nullptr, nullptr);
  const float score = MODE == MODE_IP ? -key : key;
  const bool hit = MODE == MODE_IP ? score > radius : score < radius;  // NaN: no
  if (lane == 0) {
    ekey[c] = score;
    flag[c] = hit ? 1 : 0;
  }
}

hipError_t launch_range_verify(int mode, const int* cand, int64_t total, const int64_t* off,
                               int nsplit, int nq, const void* X, int xesize, const float* xn,
                               const float* Q, const float* qn, int64_t ld, int ntotal,
                               float radius, const uint32_t* rbits, float* ekey, uint8_t* flag,
                               hipStream_t st) {
  if (total <= 0) return hipSuccess;
  if (nq < 1 || nsplit < 1 || ld % 4 != 0 || (xesize != 4 && xesize != 2) || total > INT_MAX)
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 3) / 4);
#define VS_RV_T(MD, RT)                                                                          \
  hipLaunchKernelGGL((range_verify_kernel<MD, RT>), dim3(blocks), dim3(256), 0, st, cand, total, \
                     off, nsplit, nq, (const RT*)X, xn, Q, qn, ld, ntotal, radius, rbits, ekey, \
                     flag)
#define VS_RV(MD)                   \
  do {                              \
    if (xesize == 4)                \
      VS_RV_T(MD, float);           \
    else                            \
      VS_RV_T(MD, uint16_t);        \
  } while (0)
  if (mode == MODE_IP)
    VS_RV(MODE_IP);
  else if (mode == MODE_L2)
    VS_RV(MODE_L2);
  else if (mode == MODE_L2D)
    VS_RV(MODE_L2D);
  else
    return hipErrorInvalidValue;
#undef VS_RV
#undef VS_RV_T
  return hipGetLastError();
}

// The self-join's verification (MODE_COS): one wave per candidate, both
// operands stored rows (fp32 x fp32, or bf16 x bf16 widened exactly), summed in
// wave_dot's order.  Every product of two stored values is exact in fp64 and
// commutes, and exact_key<MODE_COS> multiplies the two inverse norms with each
// other first, so the key of (a, b) is the key of (b, a) bit for bit.  Query q
// is row q0 + q; a candidate is a hit iff sim >= min_sim (not strict: the
// comparison of vs_selfjoin's min_sim; NaN never passes) and the row is not
// the query's own (exclude_self) / comes after it (upper).
template <typename RT>
__device__ __forceinline__ double wave_dot_rows(const RT* __restrict__ x, const RT* __restrict__ y,
                                                int64_t ld, int lane) {
  double acc = 0.0;
  for (int64_t c = lane * 4; c < ld; c += 256) {
    const f32x4 xv = row4(x + c);
    const f32x4 yv = row4(y + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fma((double)xv[e], (double)yv[e], acc);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

template <typename RT>
__global__ __launch_bounds__(256) void range_join_verify_kernel(
    const int* __restrict__ cand, int64_t total, const int64_t* __restrict__ off, int nsplit,
    int nq, const RT* __restrict__ X, const float* __restrict__ rinv, int64_t ld, int ntotal,
    int q0, float min_sim, int exclude_self, int upper, float* __restrict__ ekey,
    uint8_t* __restrict__ flag, const int* __restrict__ qrows) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= total) return;
  int lo = 0, hi = nq - 1;  // the last query whose segment starts at or before c
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[(int64_t)mid * nsplit] <= c) lo = mid;
    else hi = mid - 1;
  }
  const int qr = qrows ? qrows[lo] : q0 + lo;  // the row-list join: any row, any order
  const int r = cand[c];
  bool live = r >= 0 && r < ntotal;
  if (exclude_self) live = live && r != qr;
  if (upper) live = live && r > qr;
  if (!live) {  // wave-uniform
    if (lane == 0) {
      ekey[c] = 0.0f;
      flag[c] = 0;
    }
    return;
  }
  const double acc = wave_dot_rows<RT>(X + (int64_t)r * ld, X + (int64_t)qr * ld, ld, lane);
  const float sim = -exact_key<MODE_COS>((float)acc, qr, r, nullptr, nullptr, rinv, rinv);
  if (lane == 0) {
    ekey[c] = sim;
    flag[c] = sim >= min_sim ? 1 : 0;  // NaN (a zero row, a NaN threshold): no
  }
}

hipError_t launch_range_join_verify(const int* cand, int64_t total, const int64_t* off, int nsplit,
                                    int nq, const void* X, int xesize, const float* rinv,
                                    int64_t ld, int ntotal, int64_t q0, float min_sim,
                                    int exclude_self, int upper, float* ekey, uint8_t* flag,
                                    hipStream_t st, const int* qrows) {
  if (total <= 0) return hipSuccess;
  if (nq < 1 || nsplit < 1 || ld % 4 != 0 || (xesize != 4 && xesize != 2) || total > INT_MAX ||
      !rinv || q0 < 0 || (qrows ? upper != 0 : q0 + nq > ntotal))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((total + 3) / 4);
  if (xesize == 4)
    hipLaunchKernelGGL(range_join_verify_kernel<float>, dim3(blocks), dim3(256), 0, st, cand, total,
                       off, nsplit, nq, (const float*)X, rinv, ld, ntotal, (int)q0, min_sim,
                       exclude_self, upper, ekey, flag, qrows);
  else
    hipLaunchKernelGGL(range_join_verify_kernel<uint16_t>, dim3(blocks), dim3(256), 0, st, cand,
                       total, off, nsplit, nq, (const uint16_t*)X, rinv, ld, ntotal, (int)q0,
                       min_sim, exclude_self, upper, ekey, flag, qrows);
  return hipGetLastError();
}

// The row-list join's query block: one wave per slot, 16-byte pieces; slot i <
// nq takes row qrows[i] and its inverse norm, the padding slots zeros (their
// thresholds are NaN: they admit nothing).
__global__ __launch_bounds__(256) void range_gather_rows_kernel(
    const char* __restrict__ X, int64_t rowbytes, const float* __restrict__ rinv,
    const int* __restrict__ qrows, int nq, int nq_pad, char* __restrict__ Q,
    float* __restrict__ qaux) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nq_pad) return;
  char* dst = Q + (int64_t)i * rowbytes;
  if (i < nq) {
    const int r = qrows[i];
    const char* src = X + (int64_t)r * rowbytes;
    for (int64_t b = (int64_t)lane * 16; b < rowbytes; b += 1024)
      *(uint4*)(dst + b) = *(const uint4*)(src + b);
    if (lane == 0) qaux[i] = rinv[r];
  } else {
    for (int64_t b = (int64_t)lane * 16; b < rowbytes; b += 1024)
      *(uint4*)(dst + b) = make_uint4(0u, 0u, 0u, 0u);
    if (lane == 0) qaux[i] = 0.0f;
  }
}

hipError_t launch_range_gather_rows(const void* X, int64_t rowbytes, const float* rinv,
                                    const int* qrows, int nq, int nq_pad, void* Q, float* qaux,
                                    hipStream_t st) {
  if (nq < 1 || nq_pad < nq || rowbytes <= 0 || rowbytes % 16 != 0 || !X || !rinv || !qrows ||
      !Q || !qaux)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_gather_rows_kernel, dim3((unsigned)((nq_pad + 3) / 4)), dim3(256), 0,
                     st, (const char*)X, rowbytes, rinv, qrows, nq, nq_pad, (char*)Q, qaux);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Emission.  hits[q] = the flags set in query q's segment (one workgroup per
// query); after their scan into lims, the same walk compacts the segment
// stably into D (score) and I (row + id_base) at lims[q].
__device__ __forceinline__ int block_scan_flags(bool f, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  __syncthreads();  // wsum's readers of the previous round are done
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int before = __popcll(m & ((1ull << lane) - 1ull));
  for (int i = 0; i < w; ++i) before += wsum[i];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return before;
}

__global__ __launch_bounds__(256) void range_hits_kernel(const uint8_t* __restrict__ flag,
                                                         const int64_t* __restrict__ off,
                                                         int nsplit, int* __restrict__ hits) {
  __shared__ int wsum[4];
  const int64_t q = blockIdx.x;
  const int64_t c0 = off[q * nsplit], c1 = off[(q + 1) * nsplit];
  int s = 0;
  for (int64_t c = c0 + threadIdx.x; c < c1; c += 256) s += flag[c];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) hits[q] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

hipError_t launch_range_hits(const uint8_t* flag, const int64_t* off, int nsplit, int nq,
                             int* hits, hipStream_t st) {
  if (nq < 1 || nsplit < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_hits_kernel, dim3(nq), dim3(256), 0, st, flag, off, nsplit, hits);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void range_emit_kernel(
    const int* __restrict__ cand, const float* __restrict__ ekey, const uint8_t* __restrict__ flag,
    const int64_t* __restrict__ off, int nsplit, const int64_t* __restrict__ lims,
    int64_t id_base, float* __restrict__ D, int64_t* __restrict__ I) {
  __shared__ int wsum[4];
  const int64_t q = blockIdx.x;
  const int64_t c0 = off[q * nsplit], c1 = off[(q + 1) * nsplit];
  const int64_t o1 = lims[q + 1];
  int64_t out = lims[q];
  for (int64_t b = c0; b < c1; b += 256) {  // uniform trip count
    const int64_t c = b + threadIdx.x;
    const bool f = c < c1 && flag[c] != 0;
    int total;
    const int64_t pos = out + block_scan_flags(f, wsum, &total);
    if (f && pos < o1) {
      D[pos] = ekey[c];
      I[pos] = (int64_t)cand[c] + id_base;
    }
    out += total;
  }
}

hipError_t launch_range_emit(const int* cand, const float* ekey, const uint8_t* flag,
                             const int64_t* off, int nsplit, int nq, const int64_t* lims,
                             int64_t id_base, float* D, int64_t* I, hipStream_t st) {
  if (nq < 1 || nsplit < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_emit_kernel, dim3(nq), dim3(256), 0, st, cand, ekey, flag, off, nsplit,
                     lims, id_base, D, I);
  return hipGetLastError();
}

}  // namespace vs
