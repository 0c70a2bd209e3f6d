// vs_select.hip — selector searches (vs_search_sel): exact top-k over a subset
// of the rows, faiss's SearchParameters(sel=IDSelector...).
//
// A selector holds, on the device, a bitmap over the rows in place and the
// ascending int32 list of the selected rows, padded to a multiple of 128 with
// its last row (a valid row: the kernels read it and mask its entries).  Both
// come from the compaction below: the label bitmap mapped to rows in place
// (through the sorted dead list of a tombstoned index), block popcounts, an
// exclusive scan, a scatter.
//
// gemm_topk_rows / gemv_topk_rows are gemm_topk (vs_gemm.hip) and gemv_topk
// (vs_gemv.hip) with the database rows taken from the list: the same tile
// geometry, LDS layout, swizzle and list discipline (vs_device.h), so what
// those files' headers say holds here and only the differences are noted.
// The lists keep rows in place as ids; the row list is ascending, so a tile's
// entries come in (key, row) order as in the unselected kernels, and the
// merges (launch_merge_partials) and the label map are used unchanged.
//
// L2: the streaming kernel computes sum (x - q)^2 (MODE_L2D) — faiss-cpu 1.11
// takes its sequential branch for a search with a selector, whatever the batch
// (distances.cpp knn_L2sqr, as recalled: faiss is not vendored); the MFMA
// kernel uses the norm expansion |q|^2 + |x|^2 - 2 q.x clamped at 0, as
// gemm_topk does (the two agree within the fp32 tolerance the tests document
// for gemm_topk).
#include "vs_exact_tile.h"

namespace vs {

// ---------------------------------------------------------------------------
// Compaction.
__device__ __forceinline__ int64_t sel_count_less(const int64_t* a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One thread per row; a wave's ballot is two words of the row bitmap.
__global__ __launch_bounds__(256) void sel_row_bits_kernel(const uint8_t* __restrict__ lbits,
                                                           int64_t nbits,
                                                           const int64_t* __restrict__ dead,
                                                           int64_t ndead, int ntotal,
                                                           uint32_t* __restrict__ rbits) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool sel = false;
  if (r < ntotal) {
    int64_t p = r;
    bool live = true;
    if (ndead > 0) {
      const int64_t nd = sel_count_less(dead, ndead, r);  // dead rows below r
      live = !(nd < ndead && dead[nd] == r);
      p = r - nd;
    }
    if (live && p < nbits) sel = (lbits[p >> 3] >> (p & 7)) & 1;
  }
  const unsigned long long m = __ballot(sel);
  const int lane = threadIdx.x & 63;
  if ((lane & 31) == 0) rbits[r >> 5] = (uint32_t)(m >> (lane & 32));
}

__global__ __launch_bounds__(256) void sel_block_counts_kernel(const uint32_t* __restrict__ rbits,
                                                               int* __restrict__ bsum) {
  __shared__ int sw[4];
  const int tid = threadIdx.x;
  int c = __popc(rbits[(int64_t)blockIdx.x * 256 + tid]);
  c = (int)wave_sum((float)c);  // at most 2048 per wave: exact in fp32
  if ((tid & 63) == 0) sw[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) bsum[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// Inclusive scan of one int per thread over a 256-thread block (Hillis-Steele
// in LDS); returns the inclusive prefix, *total = the block's sum.
__device__ __forceinline__ int block_scan_256(int v, int* sh, int* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < 256; o <<= 1) {
    const int add = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  const int incl = sh[tid];
  *total = sh[255];
  __syncthreads();
  return incl;
}

// One block: thread t owns the segment [t * seg, (t + 1) * seg) of bsum.
__global__ __launch_bounds__(256) void sel_scan_kernel(int* __restrict__ bsum, int nblocks,
                                                       int* __restrict__ count) {
  __shared__ int sh[256];
  const int tid = threadIdx.x;
  const int seg = (nblocks + 255) / 256;
  const int b0 = min(tid * seg, nblocks), b1 = min(b0 + seg, nblocks);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += bsum[b];
  int total;
  int run = block_scan_256(s, sh, &total) - s;
  for (int b = b0; b < b1; ++b) {
    const int v = bsum[b];
    bsum[b] = run;
    run += v;
  }
  if (tid == 0) *count = total;
}

__global__ __launch_bounds__(256) void sel_scatter_kernel(const uint32_t* __restrict__ rbits,
                                                          const int* __restrict__ boff,
                                                          const int* __restrict__ count,
                                                          int* __restrict__ list) {
  __shared__ int sh[256];
  const int tid = threadIdx.x;
  const int64_t word = (int64_t)blockIdx.x * 256 + tid;
  uint32_t w = rbits[word];
  const int c = __popc(w);
  int total;
  int pos = boff[blockIdx.x] + block_scan_256(c, sh, &total) - c;
  const int n = *count;
  const int npad = (n + kBN - 1) / kBN * kBN;
  while (w) {
    const int bit = __builtin_ctz(w);
    w &= w - 1;
    const int row = (int)(word * 32 + bit);
    list[pos] = row;
    if (pos == n - 1)  // the last selected row pads the list
      for (int j = n; j < npad; ++j) list[j] = row;
    ++pos;
  }
}

hipError_t launch_sel_row_bits(const uint8_t* lbits, int64_t nbits, const int64_t* dead,
                               int64_t ndead, int ntotal, uint32_t* rbits, int64_t nwords,
                               hipStream_t st) {
  if (nwords <= 0 || nwords % (kSelBlockRows / 32) != 0 || (int64_t)ntotal > nwords * 32 ||
      nbits < 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sel_row_bits_kernel, dim3((unsigned)(nwords * 32 / 256)), dim3(256), 0, st,
                     lbits, nbits, dead, ndead, ntotal, rbits);
  return hipGetLastError();
}

hipError_t launch_sel_block_counts(const uint32_t* rbits, int nblocks, int* bsum, hipStream_t st) {
  if (nblocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sel_block_counts_kernel, dim3(nblocks), dim3(256), 0, st, rbits, bsum);
  return hipGetLastError();
}

hipError_t launch_sel_scan(int* bsum, int nblocks, int* count, hipStream_t st) {
  if (nblocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(256), 0, st, bsum, nblocks, count);
  return hipGetLastError();
}

hipError_t launch_sel_scatter(const uint32_t* rbits, int nblocks, const int* boff,
                              const int* count, int* list, hipStream_t st) {
  if (nblocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sel_scatter_kernel, dim3(nblocks), dim3(256), 0, st, rbits, boff, count,
                     list);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Route (b): stable drop of the unselected entries.  One wave per query; a
// ballot over 64 entries gives every kept one its output position.
__global__ __launch_bounds__(64) void sel_drop_kernel(int asc, const float* __restrict__ Din,
                                                      const int64_t* __restrict__ Iin, int k_in,
                                                      const uint32_t* __restrict__ rbits,
                                                      int64_t id_base, float* __restrict__ Dout,
                                                      int64_t* __restrict__ Iout, int k_out) {
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  int kept = 0;
  for (int j0 = 0; j0 < k_in && kept < k_out; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false;
    float s = 0.0f;
    int64_t id = -1;
    if (j < k_in) {
      id = Iin[q * k_in + j];
      s = Din[q * k_in + j];
      if (id >= 0) {
        const int64_t r = id - id_base;
        keep = (rbits[r >> 5] >> (r & 31)) & 1;
      }
    }
    const unsigned long long m = __ballot(keep);
    const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < k_out) {
      Dout[q * k_out + pos] = s;
      Iout[q * k_out + pos] = id;
    }
    kept += __popcll(m);
  }
  for (int j = min(kept, k_out) + lane; j < k_out; j += 64) {
    Dout[q * k_out + j] = asc ? FLT_MAX : -FLT_MAX;
    Iout[q * k_out + j] = -1;
  }
}

hipError_t launch_sel_drop(int mode, const float* Din, const int64_t* Iin, int nq, int k_in,
                           const uint32_t* rbits, int64_t id_base, float* Dout, int64_t* Iout,
                           int k_out, hipStream_t st) {
  if (nq < 0 || k_in < 1 || k_out < 1) return hipErrorInvalidValue;
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(sel_drop_kernel, dim3(nq), dim3(64), 0, st,
                     (mode == MODE_L2 || mode == MODE_L2D) ? 1 : 0, Din, Iin, k_in, rbits, id_base,
                     Dout, Iout, k_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gemm_topk_rows: the exact tile of vs_exact_tile.h (its mapping and keys)
// with a database tile of 128 consecutive list entries.  What it adds: each
// lane's X source offset is its list row times the row stride (64-bit, a row
// can sit past 4 GiB) plus the swizzled chunk, reloaded per tile; the epilogue
// reads the tile's rows from the list again, gathers xaux[row] and masks the
// entries past `count` (the list's padding).
template <int KP, int MODE, typename T>
__global__ __launch_bounds__(256, (KP >= 64 ? 1 : 2)) void gemm_topk_rows(
    const T* __restrict__ X, const float* __restrict__ xaux, const T* __restrict__ Q,
    const float* __restrict__ qaux, int64_t ld, int nstage, const int* __restrict__ list,
    int count, int ntiles, int nsplit, int nqt, float* __restrict__ pkey,
    int* __restrict__ pid) {
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

  const int qloc = 32 * w + c32;
  const int gq = qt * kBQ + qloc;
  float qa = 0.0f;
  if constexpr (MODE == MODE_L2) qa = qaux[gq];

  float lk[KP];
  int li[KP];
  list_init<KP, int>(lk, li);

  const T* Qblk = Q + (int64_t)qt * kBQ * ld;
  const int srow = lane >> 3;
  const int sphys = lane & 7;
  const uint32_t ldb = (uint32_t)ld * (uint32_t)sizeof(T);
  uint32_t qoff[4];
  uint32_t xsw[4];  // swizzled chunk offset of staged row group i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (w * 4 + i) * 8 + srow;  // the LDS row decides the swizzle
    // tile_chunk(sphys, row), written out: through the helper this kernel's
    // instruction streams change (profiles/exact_tile/code_objects.txt)
    xsw[i] = (uint32_t)(sphys ^ ((row >> 1) & 7)) * 16u;
    qoff[i] = (uint32_t)(w * 32 + i * 8 + srow) * ldb + xsw[i];
  }
  const int fsw = (c32 >> 1) & 7;

  for (int t = t0; t < t1; ++t) {
    const int r0 = t * kBN;
    uint64_t xoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      xoff[i] = (uint64_t)list[r0 + w * 32 + i * 8 + srow] * ldb + xsw[i];
    f32x16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;
    }

    auto stage = [&](int buf, int kb) {
      float* dX = smem + buf * (2 * kBN * kBK);
      float* dQ = dX + kBN * kBK;
      const char* xs = (const char*)X + kb;
      const char* qs = (const char*)Qblk + kb;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g = w * 4 + i;
        __builtin_amdgcn_global_load_lds(xs + xoff[i], VS_LDS(dX + g * 256), 16, 0, 0);
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

    // Epilogue as in gemm_topk; entry e of the tile is row list[r0 + e].
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float tk = lk[KP - 1];
      const int ti = li[KP - 1];
      uint32_t m = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int eb = r0 + 32 * s + 8 * j + 4 * h;
        const i32x4 rows = *(const i32x4*)(list + eb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rows[i];
          const float v = acc[s][j * 4 + i];
          float xa = 0.0f;
          if constexpr (MODE == MODE_L2) xa = xaux[row];
          const float key = gemm_key<MODE>(v, qa, xa);
          acc[s][j * 4 + i] = key;
          const bool cand = eb + i < count && lex_less(key, row, tk, ti);
          m |= (uint32_t)cand << (j * 4 + i);
        }
      }
      if (m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) smem[r * 256 + tid] = acc[s][r];
        do {
          const int bi = __builtin_ctz(m);
          m &= m - 1;
          const int row = list[r0 + 32 * s + (bi & 3) + 8 * (bi >> 2) + 4 * h];
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

template <int KP, int MODE>
static hipError_t gemm_rows_dispatch_t(const void* X, const float* xaux, const void* Q,
                                       const float* qaux, int64_t ld, int esize, const int* list,
                                       int count, int nq_pad, int nsplit, Partials part,
                                       hipStream_t st) {
  const int ntiles = (count + kBN - 1) / kBN;
  const int nqt = nq_pad / kBQ;
  const int nblk = nqt * nsplit;
  const int nstage = (int)(ld * esize / 128);
  if (esize == 4)
    hipLaunchKernelGGL((gemm_topk_rows<KP, MODE, float>), dim3(nblk), dim3(256), 0, st,
                       (const float*)X, xaux, (const float*)Q, qaux, ld, nstage, list, count,
                       ntiles, nsplit, nqt, part.key, part.id);
  else
    hipLaunchKernelGGL((gemm_topk_rows<KP, MODE, uint16_t>), dim3(nblk), dim3(256), 0, st,
                       (const uint16_t*)X, xaux, (const uint16_t*)Q, qaux, ld, nstage, list,
                       count, ntiles, nsplit, nqt, part.key, part.id);
  return hipGetLastError();
}

template <int KP>
static hipError_t gemm_rows_dispatch(int mode, const void* X, const float* xaux, const void* Q,
                                     const float* qaux, int64_t ld, int esize, const int* list,
                                     int count, int nq_pad, int nsplit, Partials part,
                                     hipStream_t st) {
  if (mode == MODE_IP)
    return gemm_rows_dispatch_t<KP, MODE_IP>(X, xaux, Q, qaux, ld, esize, list, count, nq_pad,
                                             nsplit, part, st);
  return gemm_rows_dispatch_t<KP, MODE_L2>(X, xaux, Q, qaux, ld, esize, list, count, nq_pad,
                                           nsplit, part, st);
}

hipError_t launch_gemm_topk_rows(int KP, int mode, const void* X, const float* xaux,
                                 const void* Q, const float* qaux, int64_t ld, int esize,
                                 const int* list, int count, int nq_pad, int nsplit,
                                 Partials part, hipStream_t st) {
  const int ntiles = (count + kBN - 1) / kBN;
  if (nq_pad < kBQ || nq_pad % kBQ != 0 || (ld * esize) % 128 != 0 || part.KP != KP ||
      part.P != 2 * nsplit || (esize != 4 && esize != 2) || count < 1 || nsplit < 1 ||
      nsplit > ntiles || !list || (mode != MODE_IP && mode != MODE_L2) ||
      ld * esize > (int64_t)UINT32_MAX / kBQ)
    return hipErrorInvalidValue;
  switch (KP) {
    case 8:
      return gemm_rows_dispatch<8>(mode, X, xaux, Q, qaux, ld, esize, list, count, nq_pad, nsplit, part, st);
    case 16:
      return gemm_rows_dispatch<16>(mode, X, xaux, Q, qaux, ld, esize, list, count, nq_pad, nsplit, part, st);
    case 32:
      return gemm_rows_dispatch<32>(mode, X, xaux, Q, qaux, ld, esize, list, count, nq_pad, nsplit, part, st);
    case 64:
      return gemm_rows_dispatch<64>(mode, X, xaux, Q, qaux, ld, esize, list, count, nq_pad, nsplit, part, st);
    default:
      return hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------
// gemv_topk_rows: gemv_topk over list positions; position p is row list[p].
template <int NQ, int KP, int MODE, typename T>
__global__ __launch_bounds__(256) void gemv_topk_rows(const T* __restrict__ X,
                                                      const float* __restrict__ Q, int64_t ld,
                                                      const int* __restrict__ list, int count,
                                                      int rows_per_block,
                                                      float* __restrict__ pkey,
                                                      int* __restrict__ pid) {
  constexpr int EPC = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) float sq[];  // [NQ][ld]
  const int tid = threadIdx.x;
  for (int64_t i = (int64_t)tid * 4; i < (int64_t)NQ * ld; i += 1024)
    *(f32x4*)(sq + i) = *(const f32x4*)(Q + i);
  __syncthreads();

  const int lane = tid & 63;
  const int w = tid >> 6;
  const int cpr = (int)(ld / EPC);
  const int rb0 = blockIdx.x * rows_per_block;
  const int cnt16 = (count + 15) & ~15;  // inside the list's padding (a multiple of 128)
  const int rb1 = min(rb0 + rows_per_block, cnt16);

  float lk[KP];
  int li[KP];
  list_init<KP, int>(lk, li);

  for (int p = rb0 + 4 * w; p < rb1; p += 16) {
    float acc[4][NQ];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[a][q] = 0.0f;

    const i32x4 rows = *(const i32x4*)(list + p);
    const T* xr[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xr[a] = X + (int64_t)rows[a] * ld;
    for (int c = lane; c < cpr; c += 64) {
      uint4 xv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = __builtin_nontemporal_load((const u32x4*)xr[a] + c);
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
      if (lane < NQ && p + a < count) {
        const float key = (MODE == MODE_L2D) ? mine : -mine;
        list_insert<KP, int>(lk, li, key, rows[a]);
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

template <int NQ, int KP, typename T>
static hipError_t gemv_rows_dispatch_t(int mode, const T* X, const float* Q, int64_t ld,
                                       const int* list, int count, int nblocks, Partials part,
                                       hipStream_t st) {
  const int cnt16 = (count + 15) & ~15;
  int rpb = (cnt16 + nblocks - 1) / nblocks;
  rpb = (rpb + 15) & ~15;
  const size_t lds = (size_t)NQ * ld * sizeof(float) + (size_t)4 * NQ * KP * 8;
  if (mode == MODE_L2D)
    hipLaunchKernelGGL((gemv_topk_rows<NQ, KP, MODE_L2D, T>), dim3(nblocks), dim3(256), lds, st, X,
                       Q, ld, list, count, rpb, part.key, part.id);
  else
    hipLaunchKernelGGL((gemv_topk_rows<NQ, KP, MODE_IP, T>), dim3(nblocks), dim3(256), lds, st, X,
                       Q, ld, list, count, rpb, part.key, part.id);
  return hipGetLastError();
}

template <int NQ, int KP>
static hipError_t gemv_rows_dispatch_q(int mode, const void* X, int esize, const float* Q,
                                       int64_t ld, const int* list, int count, int nblocks,
                                       Partials part, hipStream_t st) {
  if (esize == 4)
    return gemv_rows_dispatch_t<NQ, KP, float>(mode, (const float*)X, Q, ld, list, count, nblocks,
                                               part, st);
  return gemv_rows_dispatch_t<NQ, KP, uint16_t>(mode, (const uint16_t*)X, Q, ld, list, count,
                                                nblocks, part, st);
}

template <int KP>
static hipError_t gemv_rows_dispatch(int mode, int nq, const void* X, int esize, const float* Q,
                                     int64_t ld, const int* list, int count, int nblocks,
                                     Partials part, hipStream_t st) {
  switch (nq) {
    case 1:
      return gemv_rows_dispatch_q<1, KP>(mode, X, esize, Q, ld, list, count, nblocks, part, st);
    case 2:
      return gemv_rows_dispatch_q<2, KP>(mode, X, esize, Q, ld, list, count, nblocks, part, st);
    case 3:
    case 4:
      return gemv_rows_dispatch_q<4, KP>(mode, X, esize, Q, ld, list, count, nblocks, part, st);
    default:
      return gemv_rows_dispatch_q<8, KP>(mode, X, esize, Q, ld, list, count, nblocks, part, st);
  }
}

hipError_t launch_gemv_topk_rows(int KP, int mode, int nq, const void* X, int esize,
                                 const float* Q, int64_t ld, const int* list, int count,
                                 int nblocks, Partials part, hipStream_t st) {
  if (nq < 1 || nq > kGemvMaxQ || part.KP != KP || part.P != nblocks || nblocks < 1 ||
      (ld * esize) % 16 != 0 || (esize != 4 && esize != 2) || count < 1 || !list ||
      (mode != MODE_IP && mode != MODE_L2D) ||
      (size_t)kGemvMaxQ * ld * sizeof(float) + (size_t)4 * kGemvMaxQ * KP * 8 > 64 * 1024)
    return hipErrorInvalidValue;
  switch (KP) {
    case 8:
      return gemv_rows_dispatch<8>(mode, nq, X, esize, Q, ld, list, count, nblocks, part, st);
    case 16:
      return gemv_rows_dispatch<16>(mode, nq, X, esize, Q, ld, list, count, nblocks, part, st);
    case 32:
      return gemv_rows_dispatch<32>(mode, nq, X, esize, Q, ld, list, count, nblocks, part, st);
    case 64:
      return gemv_rows_dispatch<64>(mode, nq, X, esize, Q, ld, list, count, nblocks, part, st);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace vs
