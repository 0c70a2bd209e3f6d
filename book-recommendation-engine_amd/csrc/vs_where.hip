// vs_where.hip — where searches (vs_search_where; DESIGN.md "Where searches"):
// exact top-k over the rows that pass a per-query attribute predicate.
//
// A predicate (WherePred, vs_internal.h) is up to four closed float ranges
// over the numeric columns and three 64-bit tag masks; the attributes
// (WhereAttrs) are indexed by the row in place.  where_pass (vs_where_device.h)
// is the one definition every kernel of this unit tests with.
//
// Kernels:
//  - attrs_spread: the attributes by label -> by row in place through the
//    sorted dead list (as sel_row_bits, vs_select.hip);
//  - attrs_count: the live rows that pass each of nq predicates, one stream
//    over the by-row arrays;
//  - where_drop: route A's stable drop of a raw window's entries whose row
//    fails the slot's predicate (sel_drop with one predicate per slot and
//    distinct_collapse's unsettled flag);
//  - gemm_topk_where / gemv_topk_where: route B, restatements of gemm_topk
//    (vs_gemm.hip) and gemv_topk (vs_gemv.hip) at KP = 64 with FLOOR always on
//    (every page of the paged engine runs one instantiation, so a row's key
//    is bit-identical in all pages).  Tile geometry, LDS layout, swizzle, list
//    discipline and keys are those files'; only the differences are noted.
#include <algorithm>

#include "vs_exact_tile.h"
#include "vs_where_device.h"

namespace vs {

__device__ __forceinline__ int where_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------------------
// One thread per row in place: its position among the live rows is its label.
__global__ __launch_bounds__(256) void attrs_spread_kernel(
    const float* __restrict__ lcols, const unsigned long long* __restrict__ ltags, int64_t nlab,
    int ncol, const int64_t* __restrict__ dead, int64_t ndead, int64_t ntotal,
    float* __restrict__ rcols, unsigned long long* __restrict__ rtags, uint8_t* __restrict__ live) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= ntotal) return;
  int64_t lo = 0, hi = ndead;  // dead rows below r
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (dead[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  const bool alive = !(lo < ndead && dead[lo] == r) && r - lo < nlab;
  const int64_t p = r - lo;
  live[r] = alive ? 1 : 0;
  for (int c = 0; c < ncol; ++c)
    rcols[(int64_t)c * ntotal + r] = alive ? lcols[(int64_t)c * nlab + p] : __int_as_float(0x7fc00000);
  if (rtags) rtags[r] = alive ? ltags[p] : 0ull;
}

hipError_t launch_attrs_spread(const float* lcols, const unsigned long long* ltags, int64_t nlab,
                               int ncol, const int64_t* dead, int64_t ndead, int64_t ntotal,
                               float* rcols, unsigned long long* rtags, uint8_t* live,
                               hipStream_t st) {
  if (ntotal < 1 || ncol < 0 || ncol > kWhereMaxCols || ndead < 1 || !dead || !live ||
      (ncol > 0 && (!lcols || !rcols)) || ((ltags == nullptr) != (rtags == nullptr)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(attrs_spread_kernel, dim3((unsigned)((ntotal + 255) / 256)), dim3(256), 0, st,
                     lcols, ltags, nlab, ncol, dead, ndead, ntotal, rcols, rtags, live);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Counts: blockIdx.y owns the predicates [8 y, 8 y + 8), held in LDS; the
// blocks of one y stream the rows once (grid-stride), a thread keeps its 8
// counts in registers (32 of them cost the kernel its occupancy: 255 VGPRs),
// a wave adds its sums to out[q].
constexpr int kWhereCountQ = 8;

__global__ __launch_bounds__(256) void attrs_count_kernel(WhereAttrs at, int64_t nrows,
                                                          const WherePred* __restrict__ preds,
                                                          int nq,
                                                          unsigned long long* __restrict__ out) {
  __shared__ WherePred sp[kWhereCountQ];
  const int q0 = blockIdx.y * kWhereCountQ;
  const int nc = min(kWhereCountQ, nq - q0);
  for (int i = threadIdx.x; i < nc * (int)(sizeof(WherePred) / 4); i += 256)
    ((unsigned*)sp)[i] = ((const unsigned*)(preds + q0))[i];
  __syncthreads();
  int cnt[kWhereCountQ];
#pragma unroll
  for (int q = 0; q < kWhereCountQ; ++q) cnt[q] = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nrows;
       r += (int64_t)gridDim.x * 256) {
    if (at.live && !at.live[r]) continue;
    float v[kWhereMaxCols];
#pragma unroll
    for (int c = 0; c < kWhereMaxCols; ++c) v[c] = c < at.ncol ? at.cols[(int64_t)c * at.stride + r] : 0.0f;
    const unsigned long long t = at.tags ? at.tags[r] : 0ull;
#pragma unroll
    for (int q = 0; q < kWhereCountQ; ++q) {
      if (q < nc) {
        const WherePred& p = sp[q];
        bool ok = p.on != 0;
#pragma unroll
        for (int c = 0; c < kWhereMaxCols; ++c)
          if (c < at.ncol && ((p.cmask >> c) & 1u)) ok = ok && p.lo[c] <= v[c] && v[c] <= p.hi[c];
        ok = ok && (p.any_of == 0ull || (t & p.any_of) != 0ull) && (t & p.all_of) == p.all_of &&
             (t & p.none_of) == 0ull;
        cnt[q] += ok ? 1 : 0;
      }
    }
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < kWhereCountQ; ++q) {
    if (q < nc) {
      const int s = where_wave_sum_int(cnt[q]);
      if (lane == 0 && s) atomicAdd(out + q0 + q, (unsigned long long)s);
    }
  }
}

hipError_t launch_attrs_count(const WhereAttrs& at, int64_t nrows, const WherePred* preds, int nq,
                              unsigned long long* out, hipStream_t st) {
  if (nq < 0 || nrows < 0 || !out || (nq > 0 && !preds)) return hipErrorInvalidValue;
  if (nq == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)nq * sizeof(unsigned long long), st);
  if (e != hipSuccess || nrows == 0) return e;
  const unsigned bx = (unsigned)std::min<int64_t>(1024, (nrows + 255) / 256);
  const unsigned by = (unsigned)((nq + kWhereCountQ - 1) / kWhereCountQ);
  if (by > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attrs_count_kernel, dim3(bx, by), dim3(256), 0, st, at, nrows, preds, nq, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Route A: one wave per slot s of a round's batch.  Din / Iin [ns][w] are the
// raw entries as the engine wrote them (ascending (key, label), labels = row +
// id_base, -1 after the end); the slot's query is q = qmap ? qmap[s] : s and
// its predicate preds[q].  The entries whose row passes go out in order, at
// most `need` of them, as the first entries of row s of Dout / Iout
// ([ns][kout], padded with the empty result); unsettled[q] = the window was
// too short: fewer than `need` kept, no -1 entry seen and not w_is_all.
__global__ __launch_bounds__(64) void where_drop_kernel(
    int asc, const float* __restrict__ Din, const int64_t* __restrict__ Iin, int w, WhereAttrs at,
    const WherePred* __restrict__ preds, const int* __restrict__ qmap, int64_t id_base, int need,
    int w_is_all, float* __restrict__ Dout, int64_t* __restrict__ Iout, int kout,
    int* __restrict__ unsettled) {
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int q = qmap ? qmap[s] : (int)s;
  const WherePred p = preds[q];
  int kept = 0;
  bool end_seen = false;
  for (int j0 = 0; j0 < w && kept < need && !end_seen; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false, end = false;
    float sc = 0.0f;
    int64_t id = -1;
    if (j < w) {
      id = Iin[s * w + j];
      sc = Din[s * w + j];
      if (id >= 0) keep = where_pass(p, at, id - id_base);
      else end = true;
    }
    const unsigned long long m = __ballot(keep);
    end_seen = __ballot(end) != 0ull;
    const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < need && pos < kout) {
      Dout[s * kout + pos] = sc;
      Iout[s * kout + pos] = id;
    }
    kept += __popcll(m);
  }
  for (int j = min(min(kept, need), kout) + lane; j < kout; j += 64) {
    Dout[s * kout + j] = asc ? FLT_MAX : -FLT_MAX;
    Iout[s * kout + j] = -1;
  }
  if (lane == 0) unsettled[q] = (kept >= need || end_seen || w_is_all) ? 0 : 1;
}

hipError_t launch_where_drop(int mode, const float* Din, const int64_t* Iin, int ns, int w,
                             const WhereAttrs& at, const WherePred* preds, const int* qmap,
                             int64_t id_base, int need, bool w_is_all, float* Dout, int64_t* Iout,
                             int kout, int* unsettled, hipStream_t st) {
  if (ns < 0 || w < 1 || kout < 1 || need < 1 || !Din || !Iin || !preds || !Dout || !Iout ||
      !unsettled)
    return hipErrorInvalidValue;
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(where_drop_kernel, dim3(ns), dim3(64), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, w, at, preds, qmap,
                     id_base, need, w_is_all ? 1 : 0, Dout, Iout, kout, unsettled);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gemm_topk_where: gemm_topk<64, MODE, T, FLOOR = true> over a gathered batch
// (qlist / qcount always given, no self-join).  Each lane owns one query and
// holds that query's predicate and exclusion segment in registers; an entry
// that passed the key test (phase A, whose threshold admits a superset) is
// tested in phase B against the by-row attributes and, by binary search,
// against the query's excluded rows, and only then inserted.  The test is
// exact there because the threshold only tightens through insertions of rows
// that passed.
template <int MODE, typename T>
__global__ __launch_bounds__(256, 1) void gemm_topk_where(
    const T* __restrict__ X, const float* __restrict__ xaux, const T* __restrict__ Q,
    const float* __restrict__ qaux, int64_t ld, int nstage, int ntotal, int ntiles, int nsplit,
    int nqt, float* __restrict__ pkey, int* __restrict__ pid, const int* __restrict__ qlist,
    const int* __restrict__ qcount, const float* __restrict__ fkey, const int* __restrict__ fid,
    WhereAttrs at, const WherePred* __restrict__ preds, const int64_t* __restrict__ xoffs,
    const int64_t* __restrict__ xrows) {
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

    // Epilogue as in gemm_topk; phase B adds the predicate and exclusion tests.
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
          const bool cand =
              row < ntotal && lex_less(key, row, tk, ti) && lex_less(fk, fi, key, row);
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
          if (where_pass(pred, at, row) && !where_excluded(xrows, xb, xe, row))
            list_insert<KP, int>(lk, li, smem[bi * 256 + tid], row);
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
static hipError_t gemm_where_dispatch(const GemmWhereArgs& a, Partials part, hipStream_t st) {
  const int ntiles = (a.ntotal + kBN - 1) / kBN;
  const int nqt = a.nq_pad / kBQ;
  const int nblk = nqt * a.nsplit;
  const int nstage = (int)(a.ld * a.esize / 128);
  if (a.esize == 4)
    hipLaunchKernelGGL((gemm_topk_where<MODE, float>), dim3(nblk), dim3(256), 0, st,
                       (const float*)a.X, a.xaux, (const float*)a.Q, a.qaux, a.ld, nstage,
                       a.ntotal, ntiles, a.nsplit, nqt, part.key, part.id, a.qlist, a.qcount,
                       a.fkey, a.fid, a.at, a.preds, a.xoffs, a.xrows);
  else
    hipLaunchKernelGGL((gemm_topk_where<MODE, uint16_t>), dim3(nblk), dim3(256), 0, st,
                       (const uint16_t*)a.X, a.xaux, (const uint16_t*)a.Q, a.qaux, a.ld, nstage,
                       a.ntotal, ntiles, a.nsplit, nqt, part.key, part.id, a.qlist, a.qcount,
                       a.fkey, a.fid, a.at, a.preds, a.xoffs, a.xrows);
  return hipGetLastError();
}

hipError_t launch_gemm_topk_where(int mode, const GemmWhereArgs& a, Partials part,
                                  hipStream_t st) {
  const int ntiles = (a.ntotal + kBN - 1) / kBN;
  if (a.nq_pad < kBQ || a.nq_pad % kBQ != 0 || (a.ld * a.esize) % 128 != 0 || part.KP != 64 ||
      part.P != 2 * a.nsplit || (a.esize != 4 && a.esize != 2) || !a.qlist || !a.qcount ||
      !a.fkey || !a.fid || !a.preds || a.ntotal < 1 || a.nsplit < 1 || a.nsplit > ntiles ||
      ((a.xoffs == nullptr) != (a.xrows == nullptr)))
    return hipErrorInvalidValue;
  if (mode == MODE_IP) return gemm_where_dispatch<MODE_IP>(a, part, st);
  if (mode == MODE_L2) return gemm_where_dispatch<MODE_L2>(a, part, st);
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// gemv_topk_where: gemv_topk<NQ, 64, MODE, T, FLOOR = true> with row skipping.
// Lane q < NQ owns query q of the group: its predicate, floor and exclusion
// segment.  Before a wave streams a 4-row step those lanes test the four rows
// against their predicates; a ballot gives the wave-uniform "someone wants a
// row of this step", and a step nobody wants is not loaded.  A lane inserts a
// row only if its own test passed.  streamed (optional): += 4 per step a wave
// loaded.
template <int NQ, int MODE, typename T>
__global__ __launch_bounds__(256) void gemv_topk_where(
    const T* __restrict__ X, const float* __restrict__ Q, int64_t ld, int ntotal,
    int rows_per_block, float* __restrict__ pkey, int* __restrict__ pid,
    const float* __restrict__ fkey, const int* __restrict__ fid, const int* __restrict__ run,
    WhereAttrs at, const WherePred* __restrict__ preds, const int64_t* __restrict__ xoffs,
    const int64_t* __restrict__ xrows, unsigned long long* __restrict__ streamed) {
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
    ++steps;

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
        if (lex_less(fk, fi, key, row) && !where_excluded(xrows, xb, xe, row))
          list_insert<KP, int>(lk, li, key, row);
      }
    }
  }
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

template <int NQ, typename T>
static hipError_t gemv_where_dispatch_t(int mode, const GemvWhereArgs& a, Partials part,
                                        hipStream_t st) {
  const int ntot16 = (a.ntotal + 15) & ~15;
  int rpb = (ntot16 + a.nblocks - 1) / a.nblocks;
  rpb = (rpb + 15) & ~15;
  const size_t lds = (size_t)NQ * a.ld * sizeof(float) + (size_t)4 * NQ * 64 * 8;
  if (mode == MODE_IP)
    hipLaunchKernelGGL((gemv_topk_where<NQ, MODE_IP, T>), dim3(a.nblocks), dim3(256), lds, st,
                       (const T*)a.X, a.Q, a.ld, a.ntotal, rpb, part.key, part.id, a.fkey, a.fid,
                       a.run, a.at, a.preds, a.xoffs, a.xrows, a.streamed);
  else
    hipLaunchKernelGGL((gemv_topk_where<NQ, MODE_L2D, T>), dim3(a.nblocks), dim3(256), lds, st,
                       (const T*)a.X, a.Q, a.ld, a.ntotal, rpb, part.key, part.id, a.fkey, a.fid,
                       a.run, a.at, a.preds, a.xoffs, a.xrows, a.streamed);
  return hipGetLastError();
}

template <int NQ>
static hipError_t gemv_where_dispatch(int mode, const GemvWhereArgs& a, Partials part,
                                      hipStream_t st) {
  if (a.esize == 4) return gemv_where_dispatch_t<NQ, float>(mode, a, part, st);
  return gemv_where_dispatch_t<NQ, uint16_t>(mode, a, part, st);
}

hipError_t launch_gemv_topk_where(int mode, int nq, const GemvWhereArgs& a, Partials part,
                                  hipStream_t st) {
  if (nq < 1 || nq > kGemvMaxQ || part.KP != 64 || part.P != a.nblocks || a.nblocks < 1 ||
      (a.ld * a.esize) % 16 != 0 || (a.esize != 4 && a.esize != 2) || !a.fkey || !a.fid ||
      !a.preds || a.ntotal < 1 || (mode != MODE_IP && mode != MODE_L2D) ||
      ((a.xoffs == nullptr) != (a.xrows == nullptr)) ||
      (size_t)kGemvMaxQ * a.ld * sizeof(float) + (size_t)4 * kGemvMaxQ * 64 * 8 > 64 * 1024)
    return hipErrorInvalidValue;
  switch (nq) {
    case 1:
      return gemv_where_dispatch<1>(mode, a, part, st);
    case 2:
      return gemv_where_dispatch<2>(mode, a, part, st);
    case 3:
    case 4:
      return gemv_where_dispatch<4>(mode, a, part, st);
    default:
      return gemv_where_dispatch<8>(mode, a, part, st);
  }
}

}  // namespace vs
