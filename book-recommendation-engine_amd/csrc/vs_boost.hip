// vs_boost.hip — boosted searches (vs_search_boost; DESIGN.md "Boosted
// searches"): exact top-k by final_key = fl32(key - b(q, r)), b a per-query
// function of the row's attributes (boost_value, vs_boost_value.h).
//
// Kernels:
//  - boost_rerank: route A's re-rank of a raw window, with the test that
//    proves the window sufficient;
//  - gemm_topk_boost / gemv_topk_boost: route B, restatements of
//    gemm_topk_where / gemv_topk_where (vs_where.hip) whose lists, floors and
//    partials hold final keys.  Tile geometry, LDS layout, swizzle and list
//    discipline are those kernels'; only the differences are noted.
// This unit is built with a correctly rounded division (csrc/Makefile).
#include <algorithm>

#include "vs_boost_value.h"
#include "vs_exact_tile.h"
#include "vs_where_device.h"

namespace vs {

// ---------------------------------------------------------------------------
// Route A: one workgroup per slot s of a round's batch.  Din / Iin [ns][w] are
// the raw entries as the engine wrote them with raw = 1 (ascending (key,
// label), labels = row + id_base, -1 after the end), w <= 1023, P = w padded
// to a power of two.  An entry whose row fails the slot's predicate is dropped
// (its LDS entry sorts last); the others get their final key, an LDS bitonic
// sort orders (final_key, label), and the first k go out.
//
// The proof of sufficiency.  Let (K_w, l_w) be the window's last real entry.
// A live row outside the window has a raw (key, label) above it, so key >= K_w;
// b <= U and rounded subtraction is monotone in both operands, so its final
// key fl32(key - b) >= fl32(K_w - U).  If k entries were kept and
// final_key[k-1] < fl32(K_w - U) (strictly: an outside row that ties could
// carry a lower label), no outside row can enter the first k: the slot is
// settled.  It is settled too when the window held every row (a -1 entry, or
// w_is_all).  Otherwise state[q] = 1, or 2 when the deficit final_key[k-1] -
// fl32(K_w - U) exceeds giveup * (K_w - K_0): a longer window is then unlikely
// to settle it (a cost rule only; the scan answers those queries exactly).
__global__ __launch_bounds__(256) void boost_rerank_kernel(
    int asc, const float* __restrict__ Din, const int64_t* __restrict__ Iin, int w, int P,
    WhereAttrs at, const WherePred* __restrict__ preds, const BoostSpec* __restrict__ specs,
    const int* __restrict__ qmap, int64_t id_base, int k, int w_is_all, float giveup,
    float* __restrict__ Dout, int64_t* __restrict__ Iout, int* __restrict__ state,
    float* __restrict__ deficit, float* __restrict__ spread) {
  __shared__ float sk[1024];
  __shared__ long long si[1024];
  __shared__ int s_end, s_real, s_kept;
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int q = qmap ? qmap[s] : (int)s;
  const WherePred p = preds[q];
  const BoostSpec sp = specs[q];
  if (tid == 0) {
    s_end = 0;
    s_real = 0;
    s_kept = 0;
  }
  __syncthreads();
  for (int j = tid; j < P; j += 256) {
    float key = INFINITY;
    long long id = LLONG_MAX;
    if (j < w) {
      const int64_t lab = Iin[s * w + j];
      if (lab >= 0) {
        atomicMax(&s_real, j + 1);
        const int64_t row = lab - id_base;
        if (where_pass(p, at, row)) {
          const float d = Din[s * w + j];
          key = boost_final(asc ? d : -d, boost_of_row(sp, at, row));
          id = lab;
          atomicAdd(&s_kept, 1);
        }
      } else {
        s_end = 1;
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
  const int kept = s_kept;
  for (int j = tid; j < k; j += 256) {
    const bool have = j < kept;  // (kept <= w <= P)
    Dout[s * k + j] = have ? (asc ? sk[j] : -sk[j]) : (asc ? FLT_MAX : -FLT_MAX);
    Iout[s * k + j] = have ? (int64_t)si[j] : -1;
  }
  if (tid == 0) {
    const int nreal = s_real;
    int st = 0;
    float def = 0.0f, spr = 0.0f;
    if (!(s_end || w_is_all || nreal < w)) {
      const float d0 = Din[s * w], dw = Din[s * w + nreal - 1];
      const float K0 = asc ? d0 : -d0, Kw = asc ? dw : -dw;
      const float bound = boost_final(Kw, sp.U);
      spr = Kw - K0;
      def = kept >= k ? sk[k - 1] - bound : INFINITY;
      if (!(kept >= k && sk[k - 1] < bound)) st = (giveup >= 0.0f && def > giveup * spr) ? 2 : 1;
    }
    state[q] = st;
    if (deficit) deficit[q] = def;
    if (spread) spread[q] = spr;
  }
}

hipError_t launch_boost_rerank(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                               const WhereAttrs& at, const WherePred* preds,
                               const BoostSpec* specs, const int* qmap, int64_t id_base, int k,
                               bool w_is_all, float giveup, float* Dout, int64_t* Iout,
                               int* state, float* deficit, float* spread, hipStream_t st) {
  if (ns < 0 || w < 1 || w > kBoostMaxWindow || k < 1 || !Din || !Iin || !preds || !specs ||
      !Dout || !Iout || !state)
    return hipErrorInvalidValue;
  if (ns == 0) return hipSuccess;
  int P = 2;
  while (P < w) P <<= 1;
  hipLaunchKernelGGL(boost_rerank_kernel, dim3(ns), dim3(256), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, w, P, at, preds,
                     specs, qmap, id_base, k, w_is_all ? 1 : 0, giveup, Dout, Iout, state, deficit,
                     spread);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gemm_topk_boost: gemm_topk_where with the boost applied where a row enters
// a list.  Each lane also holds its query's BoostSpec.  Phase A knows no
// attribute and admits a superset by the spec's bounds: final >= fl32(key - U)
// and final <= fl32(key - L), so an entry that can pass the exact tests has
// fl32(key - U) <= tail and fl32(key - L) >= floor.  Phase B computes the
// row's b and final key and applies the exact tests against the live tail and
// the floor, the predicate and the exclusion search, and only then inserts.
template <int MODE, typename T>
__global__ __launch_bounds__(256, 1) void gemm_topk_boost(
    const T* __restrict__ X, const float* __restrict__ xaux, const T* __restrict__ Q,
    const float* __restrict__ qaux, int64_t ld, int nstage, int ntotal, int ntiles, int nsplit,
    int nqt, float* __restrict__ pkey, int* __restrict__ pid, const int* __restrict__ qlist,
    const int* __restrict__ qcount, const float* __restrict__ fkey, const int* __restrict__ fid,
    WhereAttrs at, const WherePred* __restrict__ preds, const BoostSpec* __restrict__ specs,
    const int64_t* __restrict__ xoffs, const int64_t* __restrict__ xrows) {
  constexpr int KP = 64;
  static_assert(sizeof(T) == 4 || sizeof(T) == 2, "fp32 or bf16 rows");
  static_assert(MODE == MODE_IP || MODE == MODE_L2, "inner product or L2");
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
  tile_split_range(sp, ntiles, nsplit, t0, t1);

  const int nf = *qcount;
  if (qt * kBQ >= nf) return;  // uniform
  const int qloc = 32 * w + c32;
  const int gq = qt * kBQ + qloc;
  const int qsrc = qlist[min(gq, nf - 1)];
  float qa = 0.0f;
  if constexpr (MODE == MODE_L2) qa = qaux[qsrc];
  const float fk = fkey[qsrc];
  const int fi = fid[qsrc];
  const WherePred pred = preds[qsrc];
  const BoostSpec spec = specs[qsrc];
  int64_t xb = 0, xe = 0;
  if (xoffs) {
    xb = xoffs[qsrc];
    xe = xoffs[qsrc + 1];
  }

  float lk[KP];
  int li[KP];
  list_init<KP, int>(lk, li);

  const int srow = lane >> 3;
  const int sphys = lane & 7;
  const uint32_t ldb = (uint32_t)ld * (uint32_t)sizeof(T);
  uint32_t soff[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int row = par * 8 + srow;
    soff[par] = (uint32_t)(w * 32 + srow) * ldb + tile_chunk(sphys, row);
  }
  uint64_t qoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int slot = qt * kBQ + w * 32 + i * 8 + srow;
    const int src = qlist[min(slot, nf - 1)];
    const int row = (w * 4 + i) * 8 + srow;  // the LDS row decides the swizzle
    qoff[i] = (uint64_t)src * ldb + tile_chunk(sphys, row);
  }
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
      const char* qs = (const char*)Q + kb;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g = w * 4 + i;
        const uint32_t o = soff[i & 1] + (uint32_t)(i * 8) * ldb;
        __builtin_amdgcn_global_load_lds(xs + o, VS_LDS(dX + g * 256), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(qs + qoff[i], VS_LDS(dQ + g * 256), 16, 0, 0);
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

    // Epilogue as in gemm_topk_where; phase A by the bounds, phase B exact.
    const int r0 = t * kBN;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float tk = lk[KP - 1];
      uint32_t m = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rb = r0 + 32 * s + 8 * j + 4 * h;
        f32x4 xa = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE == MODE_L2) xa = *(const f32x4*)(xaux + rb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rb + i;
          const float v = acc[s][j * 4 + i];
          const float key = gemm_key<MODE>(v, qa, xa[i]);
          acc[s][j * 4 + i] = key;
          const bool cand = row < ntotal && boost_final(key, spec.U) <= tk &&
                            boost_final(key, spec.L) >= fk;
          m |= (uint32_t)cand << (j * 4 + i);
        }
      }
      if (m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) smem[r * 256 + tid] = acc[s][r];
        do {
          const int bi = __builtin_ctz(m);
          m &= m - 1;
          const int row = r0 + 32 * s + (bi & 3) + 8 * (bi >> 2) + 4 * h;
          if (where_pass(pred, at, row)) {
            const float fin = boost_final(smem[bi * 256 + tid], boost_of_row(spec, at, row));
            if (lex_less(fin, row, lk[KP - 1], li[KP - 1]) && lex_less(fk, fi, fin, row) &&
                !where_excluded(xrows, xb, xe, row))
              list_insert<KP, int>(lk, li, fin, row);
          }
        } while (m);
      }
    }
    __syncthreads();
  }

  const int P = nsplit * 2;
  float* ok = pkey + ((int64_t)gq * P + sp * 2 + h) * KP;
  int* oi = pid + ((int64_t)gq * P + sp * 2 + h) * KP;
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    ok[j] = lk[j];
    oi[j] = li[j];
  }
}

template <int MODE>
static hipError_t gemm_boost_dispatch(const GemmWhereArgs& a, const BoostSpec* specs,
                                      Partials part, hipStream_t st) {
  const int ntiles = (a.ntotal + kBN - 1) / kBN;
  const int nqt = a.nq_pad / kBQ;
  const int nblk = nqt * a.nsplit;
  const int nstage = (int)(a.ld * a.esize / 128);
  if (a.esize == 4)
    hipLaunchKernelGGL((gemm_topk_boost<MODE, float>), dim3(nblk), dim3(256), 0, st,
                       (const float*)a.X, a.xaux, (const float*)a.Q, a.qaux, a.ld, nstage,
                       a.ntotal, ntiles, a.nsplit, nqt, part.key, part.id, a.qlist, a.qcount,
                       a.fkey, a.fid, a.at, a.preds, specs, a.xoffs, a.xrows);
  else
    hipLaunchKernelGGL((gemm_topk_boost<MODE, uint16_t>), dim3(nblk), dim3(256), 0, st,
                       (const uint16_t*)a.X, a.xaux, (const uint16_t*)a.Q, a.qaux, a.ld, nstage,
                       a.ntotal, ntiles, a.nsplit, nqt, part.key, part.id, a.qlist, a.qcount,
                       a.fkey, a.fid, a.at, a.preds, specs, a.xoffs, a.xrows);
  return hipGetLastError();
}

hipError_t launch_gemm_topk_boost(int mode, const GemmWhereArgs& a, const BoostSpec* specs,
                                  Partials part, hipStream_t st) {
  const int ntiles = (a.ntotal + kBN - 1) / kBN;
  if (a.nq_pad < kBQ || a.nq_pad % kBQ != 0 || (a.ld * a.esize) % 128 != 0 || part.KP != 64 ||
      part.P != 2 * a.nsplit || (a.esize != 4 && a.esize != 2) || !a.qlist || !a.qcount ||
      !a.fkey || !a.fid || !a.preds || !specs || a.ntotal < 1 || a.nsplit < 1 ||
      a.nsplit > ntiles || ((a.xoffs == nullptr) != (a.xrows == nullptr)))
    return hipErrorInvalidValue;
  if (mode == MODE_IP) return gemm_boost_dispatch<MODE_IP>(a, specs, part, st);
  if (mode == MODE_L2) return gemm_boost_dispatch<MODE_L2>(a, specs, part, st);
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// gemv_topk_boost: gemv_topk_where whose lanes q < NQ also hold their query's
// BoostSpec and insert a row by its final key.  The 4-row step skipping is
// where's: a step is loaded when some lane's predicate passes one of its rows,
// so a call without predicates (every lane's predicate passes every live row)
// loads every step that holds a live row.
template <int NQ, int MODE, typename T>
__global__ __launch_bounds__(256) void gemv_topk_boost(
    const T* __restrict__ X, const float* __restrict__ Q, int64_t ld, int ntotal,
    int rows_per_block, float* __restrict__ pkey, int* __restrict__ pid,
    const float* __restrict__ fkey, const int* __restrict__ fid, const int* __restrict__ run,
    WhereAttrs at, const WherePred* __restrict__ preds, const BoostSpec* __restrict__ specs,
    const int64_t* __restrict__ xoffs, const int64_t* __restrict__ xrows) {
  constexpr int KP = 64;
  constexpr int EPC = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) float sq[];  // [NQ][ld]
  if (run && *run == 0) return;  // uniform
  const int tid = threadIdx.x;
  for (int64_t i = (int64_t)tid * 4; i < (int64_t)NQ * ld; i += 1024)
    *(f32x4*)(sq + i) = *(const f32x4*)(Q + i);
  __syncthreads();

  const int lane = tid & 63;
  const int w = tid >> 6;
  const int cpr = (int)(ld / EPC);
  const int rb0 = blockIdx.x * rows_per_block;
  const int ntot16 = (ntotal + 15) & ~15;
  const int rb1 = min(rb0 + rows_per_block, ntot16);

  float lk[KP];
  int li[KP];
  list_init<KP, int>(lk, li);
  const int ql = lane < NQ ? lane : 0;
  const float fk = fkey[ql];
  const int fi = fid[ql];
  WherePred pred = preds[ql];
  if (lane >= NQ) pred.on = 0;
  const BoostSpec spec = specs[ql];
  int64_t xb = 0, xe = 0;
  if (xoffs && pred.on) {
    xb = xoffs[ql];
    xe = xoffs[ql + 1];
  }

  for (int r = rb0 + 4 * w; r < rb1; r += 16) {
    unsigned mine4 = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (pred.on && r + a < ntotal && where_pass(pred, at, r + a)) mine4 |= 1u << a;
    if (__ballot(mine4 != 0) == 0ull) continue;  // uniform: nobody wants these rows

    float acc[4][NQ];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[a][q] = 0.0f;

    const T* xr = X + (int64_t)r * ld;
    for (int c = lane; c < cpr; c += 64) {
      uint4 xv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = __builtin_nontemporal_load((const u32x4*)(xr + a * ld) + c);
        xv[a] = make_uint4(v.x, v.y, v.z, v.w);
      }
      float xf[4][EPC];
#pragma unroll
      for (int a = 0; a < 4; ++a) widen_chunk<T>(xv[a], xf[a]);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float qf[EPC];
#pragma unroll
        for (int e = 0; e < EPC; e += 4) {
          const f32x4 qv = *(const f32x4*)(sq + q * ld + c * EPC + e);
          qf[e] = qv.x;
          qf[e + 1] = qv.y;
          qf[e + 2] = qv.z;
          qf[e + 3] = qv.w;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float sacc = 0.0f;
#pragma unroll
          for (int e = 0; e < EPC; ++e) {
            if constexpr (MODE == MODE_L2D) {
              const float dv = xf[a][e] - qf[e];
              sacc += dv * dv;
            } else {
              sacc += xf[a][e] * qf[e];
            }
          }
          acc[a][q] += sacc;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float mine = 0.0f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float s = wave_sum(acc[a][q]);
        if (q == lane) mine = s;
      }
      const int row = r + a;
      if ((mine4 >> a) & 1u) {
        const float key = (MODE == MODE_L2D) ? mine : -mine;
        const float fin = boost_final(key, boost_of_row(spec, at, row));
        if (lex_less(fk, fi, fin, row) && !where_excluded(xrows, xb, xe, row))
          list_insert<KP, int>(lk, li, fin, row);
      }
    }
  }

  float* mk = sq + (int64_t)NQ * ld;   // [4][NQ][KP]
  int* mi = (int*)(mk + 4 * NQ * KP);  // [4][NQ][KP]
  if (lane < NQ) {
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      mk[(w * NQ + lane) * KP + j] = lk[j];
      mi[(w * NQ + lane) * KP + j] = li[j];
    }
  }
  __syncthreads();
  if (w == 0 && lane < NQ) {
#pragma unroll
    for (int o = 1; o < 4; ++o) {
      merge2_sorted<KP, int>(mk + lane * KP, mi + lane * KP, mk + (o * NQ + lane) * KP,
                             mi + (o * NQ + lane) * KP, lk, li);
      if (o < 3) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          mk[lane * KP + j] = lk[j];
          mi[lane * KP + j] = li[j];
        }
      }
    }
    float* ok = pkey + ((int64_t)lane * gridDim.x + blockIdx.x) * KP;
    int* oi = pid + ((int64_t)lane * gridDim.x + blockIdx.x) * KP;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      ok[j] = lk[j];
      oi[j] = li[j];
    }
  }
}

template <int NQ, typename T>
static hipError_t gemv_boost_dispatch_t(int mode, const GemvWhereArgs& a, const BoostSpec* specs,
                                        Partials part, hipStream_t st) {
  const int ntot16 = (a.ntotal + 15) & ~15;
  int rpb = (ntot16 + a.nblocks - 1) / a.nblocks;
  rpb = (rpb + 15) & ~15;
  const size_t lds = (size_t)NQ * a.ld * sizeof(float) + (size_t)4 * NQ * 64 * 8;
  if (mode == MODE_IP)
    hipLaunchKernelGGL((gemv_topk_boost<NQ, MODE_IP, T>), dim3(a.nblocks), dim3(256), lds, st,
                       (const T*)a.X, a.Q, a.ld, a.ntotal, rpb, part.key, part.id, a.fkey, a.fid,
                       a.run, a.at, a.preds, specs, a.xoffs, a.xrows);
  else
    hipLaunchKernelGGL((gemv_topk_boost<NQ, MODE_L2D, T>), dim3(a.nblocks), dim3(256), lds, st,
                       (const T*)a.X, a.Q, a.ld, a.ntotal, rpb, part.key, part.id, a.fkey, a.fid,
                       a.run, a.at, a.preds, specs, a.xoffs, a.xrows);
  return hipGetLastError();
}

template <int NQ>
static hipError_t gemv_boost_dispatch(int mode, const GemvWhereArgs& a, const BoostSpec* specs,
                                      Partials part, hipStream_t st) {
  if (a.esize == 4) return gemv_boost_dispatch_t<NQ, float>(mode, a, specs, part, st);
  return gemv_boost_dispatch_t<NQ, uint16_t>(mode, a, specs, part, st);
}

hipError_t launch_gemv_topk_boost(int mode, int nq, const GemvWhereArgs& a,
                                  const BoostSpec* specs, Partials part, hipStream_t st) {
  if (nq < 1 || nq > kGemvMaxQ || part.KP != 64 || part.P != a.nblocks || a.nblocks < 1 ||
      (a.ld * a.esize) % 16 != 0 || (a.esize != 4 && a.esize != 2) || !a.fkey || !a.fid ||
      !a.preds || !specs || a.ntotal < 1 || (mode != MODE_IP && mode != MODE_L2D) ||
      ((a.xoffs == nullptr) != (a.xrows == nullptr)) ||
      (size_t)kGemvMaxQ * a.ld * sizeof(float) + (size_t)4 * kGemvMaxQ * 64 * 8 > 64 * 1024)
    return hipErrorInvalidValue;
  switch (nq) {
    case 1:
      return gemv_boost_dispatch<1>(mode, a, specs, part, st);
    case 2:
      return gemv_boost_dispatch<2>(mode, a, specs, part, st);
    case 3:
    case 4:
      return gemv_boost_dispatch<4>(mode, a, specs, part, st);
    default:
      return gemv_boost_dispatch<8>(mode, a, specs, part, st);
  }
}

}  // namespace vs
