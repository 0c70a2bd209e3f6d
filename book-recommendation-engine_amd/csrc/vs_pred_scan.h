// vs_pred_scan.h — the predicated scan's two kernels (route B of the where and
// the boosted searches; DESIGN.md "Where searches", "Boosted searches"), one
// text each, with their dispatch and argument checks:
//  - gemm_topk_pred<MODE, T, Specs...>: gemm_topk (vs_gemm.hip) at KP = 64 with
//    FLOOR always on, over a gathered batch;
//  - gemv_topk_pred<NQ, MODE, T, Specs...>: gemv_topk (vs_gemv.hip) at KP = 64
//    with FLOOR always on and row skipping.
// Every page of the paged engine runs one instantiation, so a row's key is
// bit-identical in all pages.  Tile geometry, LDS layout, swizzle, list
// discipline and keys are those files'; only the differences are noted.
//
// Specs is empty or one `const BoostSpec*`: the kernels of a boosted scan take
// the queries' specs as one more argument after preds (BOOST in the text
// below), the where scan's take none, so each kind's kernels keep exactly the
// argument list they had as two texts (an unused pointer in the middle of the
// where kernels' list cost each of them a wait; profiles/pred_scan).  Without
// specs a kernel ranks by the key (vs_where.hip instantiates those), with them
// by final_key = fl32(key - b(q, r)) (vs_boost.hip, built with a correctly
// rounded division): lists, floors and partials then hold final keys.  The two
// share text by the template parameters only: the K loop and the epilogue stay
// written out in the kernel (profiles/exact_tile/code_objects.txt: as callees
// they moved the KP = 64 kernels' waits and occupancy), and each unit compiles
// its own instantiations under its own flags (profiles/pred_scan).
#pragma once

#include "vs_boost_value.h"
#include "vs_exact_tile.h"
#include "vs_where_device.h"

namespace vs {

// the one element of a kernel's Specs pack
__device__ __forceinline__ const BoostSpec* scan_specs(const BoostSpec* specs) { return specs; }

// ---------------------------------------------------------------------------
// gemm_topk_pred: qlist / qcount always given, no self-join.  Each lane owns
// one query and holds that query's predicate and exclusion segment in
// registers; an entry that passed the key test (phase A, whose threshold admits
// a superset) is tested in phase B against the by-row attributes and, by binary
// search, against the query's excluded rows, and only then inserted.  The test
// is exact there because the threshold only tightens through insertions of rows
// that passed.
//
// BOOST: each lane also holds its query's BoostSpec.  Phase A knows no
// attribute and admits a superset by the spec's bounds: final >= fl32(key - U)
// and final <= fl32(key - L), so an entry that can pass the exact tests has
// fl32(key - U) <= tail and fl32(key - L) >= floor.  Phase B computes the
// row's b and final key and applies the exact tests against the live tail and
// the floor before the exclusion search.
template <int MODE, typename T, typename... Specs>
__global__ __launch_bounds__(256, 1) void gemm_topk_pred(
    const T* __restrict__ X, const float* __restrict__ xaux, const T* __restrict__ Q,
    const float* __restrict__ qaux, int64_t ld, int nstage, int ntotal, int ntiles, int nsplit,
    int nqt, float* __restrict__ pkey, int* __restrict__ pid, const int* __restrict__ qlist,
    const int* __restrict__ qcount, const float* __restrict__ fkey, const int* __restrict__ fid,
    WhereAttrs at, const WherePred* __restrict__ preds, Specs __restrict__... specs,
    const int64_t* __restrict__ xoffs, const int64_t* __restrict__ xrows) {
  constexpr bool BOOST = sizeof...(Specs) == 1;
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
  BoostSpec spec = {};
  if constexpr (BOOST) spec = scan_specs(specs...)[qsrc];
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

    // Epilogue as in gemm_topk; phase B adds the predicate and exclusion tests
    // (BOOST: phase A by the bounds, phase B exact on the final key).
    const int r0 = t * kBN;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float tk = lk[KP - 1];
      const int ti = li[KP - 1];
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
          bool cand;
          if constexpr (BOOST)
            cand = row < ntotal && boost_final(key, spec.U) <= tk && boost_final(key, spec.L) >= fk;
          else
            cand = row < ntotal && lex_less(key, row, tk, ti) && lex_less(fk, fi, key, row);
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
          if constexpr (BOOST) {
            if (where_pass(pred, at, row)) {
              const float fin = boost_final(smem[bi * 256 + tid], boost_of_row(spec, at, row));
              if (lex_less(fin, row, lk[KP - 1], li[KP - 1]) && lex_less(fk, fi, fin, row) &&
                  !where_excluded(xrows, xb, xe, row))
                list_insert<KP, int>(lk, li, fin, row);
            }
          } else {
            if (where_pass(pred, at, row) && !where_excluded(xrows, xb, xe, row))
              list_insert<KP, int>(lk, li, smem[bi * 256 + tid], row);
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

template <int MODE, typename... Specs>
hipError_t gemm_pred_dispatch(const GemmWhereArgs& a, Partials part, hipStream_t st,
                              Specs... specs) {
  const int ntiles = (a.ntotal + kBN - 1) / kBN;
  const int nqt = a.nq_pad / kBQ;
  const int nblk = nqt * a.nsplit;
  const int nstage = (int)(a.ld * a.esize / 128);
  if (a.esize == 4)
    hipLaunchKernelGGL((gemm_topk_pred<MODE, float, Specs...>), dim3(nblk), dim3(256), 0, st,
                       (const float*)a.X, a.xaux, (const float*)a.Q, a.qaux, a.ld, nstage,
                       a.ntotal, ntiles, a.nsplit, nqt, part.key, part.id, a.qlist, a.qcount,
                       a.fkey, a.fid, a.at, a.preds, specs..., a.xoffs, a.xrows);
  else
    hipLaunchKernelGGL((gemm_topk_pred<MODE, uint16_t, Specs...>), dim3(nblk), dim3(256), 0, st,
                       (const uint16_t*)a.X, a.xaux, (const uint16_t*)a.Q, a.qaux, a.ld, nstage,
                       a.ntotal, ntiles, a.nsplit, nqt, part.key, part.id, a.qlist, a.qcount,
                       a.fkey, a.fid, a.at, a.preds, specs..., a.xoffs, a.xrows);
  return hipGetLastError();
}

// launch_gemm_topk_where (no specs: a.specs null) / launch_gemm_topk_boost (a.specs)
template <typename... Specs>
hipError_t launch_gemm_topk_pred(int mode, const GemmWhereArgs& a, Partials part, hipStream_t st,
                                 Specs... specs) {
  const int ntiles = (a.ntotal + kBN - 1) / kBN;
  if (a.nq_pad < kBQ || a.nq_pad % kBQ != 0 || (a.ld * a.esize) % 128 != 0 || part.KP != 64 ||
      part.P != 2 * a.nsplit || (a.esize != 4 && a.esize != 2) || !a.qlist || !a.qcount ||
      !a.fkey || !a.fid || !a.preds || (sizeof...(Specs) == 1) != (a.specs != nullptr) ||
      a.ntotal < 1 ||
      a.nsplit < 1 || a.nsplit > ntiles || ((a.xoffs == nullptr) != (a.xrows == nullptr)))
    return hipErrorInvalidValue;
  if (mode == MODE_IP) return gemm_pred_dispatch<MODE_IP>(a, part, st, specs...);
  if (mode == MODE_L2) return gemm_pred_dispatch<MODE_L2>(a, part, st, specs...);
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// gemv_topk_pred: lane q < NQ owns query q of the group: its predicate, floor
// and exclusion segment.  Before a wave streams a 4-row step those lanes test
// the four rows against their predicates; a ballot gives the wave-uniform
// "someone wants a row of this step", and a step nobody wants is not loaded
// (a call without predicates loads every step that holds a live row).  A lane
// inserts a row only if its own test passed.  streamed (optional, read only
// without BOOST): += 4 per step a wave loaded.
//
// BOOST: the lanes q < NQ also hold their query's BoostSpec and insert a row
// by its final key.
template <int NQ, int MODE, typename T, typename... Specs>
__global__ __launch_bounds__(256) void gemv_topk_pred(
    const T* __restrict__ X, const float* __restrict__ Q, int64_t ld, int ntotal,
    int rows_per_block, float* __restrict__ pkey, int* __restrict__ pid,
    const float* __restrict__ fkey, const int* __restrict__ fid, const int* __restrict__ run,
    WhereAttrs at, const WherePred* __restrict__ preds, Specs __restrict__... specs,
    const int64_t* __restrict__ xoffs, const int64_t* __restrict__ xrows,
    unsigned long long* __restrict__ streamed) {
  constexpr bool BOOST = sizeof...(Specs) == 1;
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
  BoostSpec spec = {};
  if constexpr (BOOST) spec = scan_specs(specs...)[ql];
  int64_t xb = 0, xe = 0;
  if (xoffs && pred.on) {
    xb = xoffs[ql];
    xe = xoffs[ql + 1];
  }
  int steps = 0;

  for (int r = rb0 + 4 * w; r < rb1; r += 16) {
    unsigned mine4 = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (pred.on && r + a < ntotal && where_pass(pred, at, r + a)) mine4 |= 1u << a;
    if (__ballot(mine4 != 0) == 0ull) continue;  // uniform: nobody wants these rows
    if constexpr (!BOOST) ++steps;

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
        float key = (MODE == MODE_L2D) ? mine : -mine;
        if constexpr (BOOST) key = boost_final(key, boost_of_row(spec, at, row));
        if (lex_less(fk, fi, key, row) && !where_excluded(xrows, xb, xe, row))
          list_insert<KP, int>(lk, li, key, row);
      }
    }
  }
  if constexpr (!BOOST)
    if (streamed && lane == 0 && steps) atomicAdd(streamed, (unsigned long long)(4 * steps));

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

template <int NQ, typename T, typename... Specs>
hipError_t gemv_pred_dispatch(int mode, const GemvWhereArgs& a, Partials part, hipStream_t st,
                              Specs... specs) {
  const int ntot16 = (a.ntotal + 15) & ~15;
  int rpb = (ntot16 + a.nblocks - 1) / a.nblocks;
  rpb = (rpb + 15) & ~15;
  const size_t lds = (size_t)NQ * a.ld * sizeof(float) + (size_t)4 * NQ * 64 * 8;
  if (mode == MODE_IP)
    hipLaunchKernelGGL((gemv_topk_pred<NQ, MODE_IP, T, Specs...>), dim3(a.nblocks), dim3(256), lds,
                       st, (const T*)a.X, a.Q, a.ld, a.ntotal, rpb, part.key, part.id, a.fkey,
                       a.fid, a.run, a.at, a.preds, specs..., a.xoffs, a.xrows, a.streamed);
  else
    hipLaunchKernelGGL((gemv_topk_pred<NQ, MODE_L2D, T, Specs...>), dim3(a.nblocks), dim3(256), lds,
                       st, (const T*)a.X, a.Q, a.ld, a.ntotal, rpb, part.key, part.id, a.fkey,
                       a.fid, a.run, a.at, a.preds, specs..., a.xoffs, a.xrows, a.streamed);
  return hipGetLastError();
}

// launch_gemv_topk_where (no specs: a.specs null) / launch_gemv_topk_boost (a.specs)
template <typename... Specs>
hipError_t launch_gemv_topk_pred(int mode, int nq, const GemvWhereArgs& a, Partials part,
                                 hipStream_t st, Specs... specs) {
  if (nq < 1 || nq > kGemvMaxQ || part.KP != 64 || part.P != a.nblocks || a.nblocks < 1 ||
      (a.ld * a.esize) % 16 != 0 || (a.esize != 4 && a.esize != 2) || !a.fkey || !a.fid ||
      !a.preds || (sizeof...(Specs) == 1) != (a.specs != nullptr) || a.ntotal < 1 ||
      (mode != MODE_IP && mode != MODE_L2D) || ((a.xoffs == nullptr) != (a.xrows == nullptr)) ||
      (size_t)kGemvMaxQ * a.ld * sizeof(float) + (size_t)4 * kGemvMaxQ * 64 * 8 > 64 * 1024)
    return hipErrorInvalidValue;
  const bool f32 = a.esize == 4;
  switch (nq) {
    case 1:
      return f32 ? gemv_pred_dispatch<1, float>(mode, a, part, st, specs...)
                 : gemv_pred_dispatch<1, uint16_t>(mode, a, part, st, specs...);
    case 2:
      return f32 ? gemv_pred_dispatch<2, float>(mode, a, part, st, specs...)
                 : gemv_pred_dispatch<2, uint16_t>(mode, a, part, st, specs...);
    case 3:
    case 4:
      return f32 ? gemv_pred_dispatch<4, float>(mode, a, part, st, specs...)
                 : gemv_pred_dispatch<4, uint16_t>(mode, a, part, st, specs...);
    default:
      return f32 ? gemv_pred_dispatch<8, float>(mode, a, part, st, specs...)
                 : gemv_pred_dispatch<8, uint16_t>(mode, a, part, st, specs...);
  }
}

}  // namespace vs
