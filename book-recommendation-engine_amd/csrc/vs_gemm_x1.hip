// vs_gemm_x1.hip — the filter pass of the filter-and-verify engine: one
// low-precision MFMA product per fp32 product, fused with per-lane candidate
// lists.
//
// Every fp32 index keeps, beside its fp32 rows, a "filter plane" copy of every
// row (tile-major: the 64-B step s of the 256 rows of tile t is one contiguous
// 16-KB block, plane_offset in vs_internal.h) and the squared norm of each
// row's residual x - plane(x).  Two planes exist (vs_internal.h, Filter):
//   int8 (default): code = rint(x / s) with one scale s = max|x| / 127 per row;
//     the kernel multiplies codes on v_mfma_i32_32x32x32_i8 (exact int32 sums,
//     twice the bf16 MFMA rate, 64 elements per 64-B step) and scales the sum
//     by s_q * s_x in the epilogue;
//   bf16: round-to-nearest-even copies on v_mfma_f32_32x32x16_bf16.
// A search converts its queries the same way and the kernel below scores every
// (query, row) pair with the one product plane(q) . plane(x) — a plain GEMM over
// Q (nq x d) and X (N x d) whose output never leaves the chip: each lane keeps
// the best approximate keys of its queries.  The exact answer is then proved and
// produced by verify_rescore_kernel (vs_x1_verify.hip): the candidates are
// rescored in fp64 from the fp32 rows, and a rigorous bound on |approx - exact|
// decides whether the candidate set must contain the exact top-M (DESIGN.md
// §4.2).
//
// Tile: 256 database rows x 256 queries per workgroup of 8 waves (two per SIMD,
// one workgroup per CU).  Wave w owns rows [128 (w&1), +128) and queries
// [64 (w>>1), +64): 4 x 2 accumulators of 32x32 (128 registers); lane l sees
// queries c = l&31 of its two 32-query blocks and keeps one sorted list of KR
// entries per query (lanes l and l+32 hold disjoint rows of the same query).
// K advances 64 B per row per step (32 bf16 / 64 int8 elements) through a ring of NBUF LDS
// images (both operand tiles of one step, 32 KB), filled by
// global_load_lds_dwordx4 (LDS-DMA) NBUF-1 steps ahead; see gemm_topk_x1
// below for the step schedule.
//
// Two kinds of launch (template flag DUMP), per search:
//  * list launches (the first launch of a pass, gathered batches, the bf16
//    L2 / cosine kernels): the epilogue of every 256-row tile reduces each
//    lane's 16 keys of a 32-row block to their maximum and, only when the
//    block can enter the lane's list, inserts its rows one by one;
//  * dump launches (every later launch of an int8 or bf16 inner-product
//    pass): the lists stay in memory; the epilogue compares each block with
//    its list's floor (the query's CUT, x1_qcut, set from the first launch's
//    lists and taken again after every replay, or the list's own last entry)
//    and, for the rare block that may
//    hold a row below it, stores one (row, raw sum) pair per row that clears
//    the per-row threshold to the list's next dump slot; x1_replay (between
//    segments of launches) admits the dumped rows into the lists exactly as a
//    list launch would have — same keys, same order, same admission rule — so
//    both kinds leave the same lists.
// The int8 inner-product dump launches (the augmented L2 among them) run on
// v_mfma_i32_16x16x64_i8 instead (template flag S16, the default; env
// VS_X1_DUMP_MFMA=32 keeps the 32x32x32 form): 8 x 4 accumulators of 16 rows
// x 16 queries per wave, one MFMA each per step — the same tile, cycles,
// accumulator and fragment registers, LDS images and DMA pieces; the chip
// holds a higher clock on that shape (tools/mfma_ceiling.hip: 1.14x by wall
// with no loads).  Lane l then holds query l & 15 of four 16-query blocks, and
// lanes l and l ^ 32 feed the same lane list: the dump epilogue exchanges
// their candidate counts so that the lists, slots and dump order are exactly
// the 32x32 form's (epilogue16 below).
// The lists are per lane, so a list launch pays for a wave's rows whenever ANY
// of its 64 lanes admits one (an exec-masked insertion chain per block that
// passes somewhere): about a sixth of the int8 pass (profiles/r04a/x1_probes.txt:
// 3.45 ms per dispatch with the candidate work, 2.86 ms with the epilogue's
// per-block test alone).  A dump costs one 8-B store per candidate row on the
// lanes that pass, and the scan that finds the row: the scan is what is paid
// for (the stores add nothing measurable).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "vs_x1_device.h"

// Diagnostic builds only (tools/x1_probe.sh; wrong results by design): a mask
// of ablations — 1 no LDS-DMA, 2 no fragment reads, 4 no mid-step barrier,
// 8 no epilogue, 16 no database pieces, 32 no query pieces, 64 no vmcnt wait in
// the loop, 128 the epilogue's per-block test alone (no block ever passes),
// 256 the dump branch in full (pass test, masks, count exchange, running
// counts) without its stores (the launch leaves dcount as it found it, so the
// replay reads no slot that was never written).
#ifndef VS_X1_PROBE
#define VS_X1_PROBE 0
#endif
#define VS_X1_P(bit) ((VS_X1_PROBE & (bit)) != 0)

namespace vs {

// Diagnostic builds only (VS_X1_STAMP=1, tools/build_variant.sh): per-segment
// s_memtime sums of the step schedules, [group (waves 0-3 | 4-7)][segment]
// (segments: load issue, vmcnt wait, barrier 1, matrix issue, barrier 2,
// epilogue), added once per wave at the end; read by vs_x1_stamps.  The real
// kernel has no stamp.
#ifndef VS_X1_STAMP
#define VS_X1_STAMP 0
#endif
constexpr int kStampSeg = 9;  // + inside the epilogue: reject, factor loads, keys/inserts
constexpr int kStampCnt = 3;  // epilogue counts: factor loads, blocks inserting, inserts
// + the 16x16x64 dump launches' events (rows that take a slot) per lane and
// launch, as a histogram of 0 .. 15+ [the pass's first dump launch | the rest]
constexpr int kStampHist = 16;
constexpr int kStampN = 2 * (kStampSeg + kStampCnt) + 2 + 2 * kStampHist;
__device__ unsigned long long g_x1_stamps[kStampN];

namespace {

constexpr int kT = 256;               // rows (and queries) per tile
constexpr int kNbuf = 5;              // LDS images in the ring (4: -1 %, profiles/r02y)
constexpr int kX1ChunkTiles = 64;     // database tiles per workgroup per launch
// dump slots (candidate rows) per lane list and segment: a segment of
// doubling data meets ~8 rows below a list's floor, a split pass's dump launch
// more (by the lists' own last entries alone; the cut only lowers the floor):
// after a list launch over a quarter of the tiles, three times as many rows
// follow, ~24 below the floor, with a tail: the dump launch beats the list
// launch's 8th row at least n times when at most 7 of the best 8 + n rows lie
// in the list launch's tiles, Binomial(8 + n, 1/4) <= 7: ~2e-4 per list at
// n = 64 (a fifth of C2's queries, with 512 lists each, handed on), ~1e-8 at
// n = 128
constexpr int kDumpMaxR = 128;
// The step schedule of a launch: 1 = fragment reads half a step ahead, DMA
// pieces between the MFMAs; 2 = separate load and matrix segments.  Measured
// per plane and launch kind: int8 list launches are faster on 1 (C2 390k vs
// 337k queries/s, C4 465k vs 437k students/s), int8 dump launches on 2 (C3
// 70.8k vs 68.9k; profiles/r04a/r04e_sched_dump_ab.txt), bf16 on 2 (clustered
// 34.4k vs 32.5k, profiles/r03_ab_sched.txt).
constexpr int x1_sched(int el, bool dump) { return el != FILTER_I8 || dump ? 2 : 1; }
// The passes with a dump form: inner product on either plane (every key
// follows from the raw sum and, for int8, the row factor the replay reads).
// Not the cosine: its bound is relative (B ~ 2 rho, ~0.02 at d = 1536 for
// int8), wide beside the similarity spread of high-dimensional rows, so its
// cut lies behind the lists' own floors, and its row factors (s_x / |x|)
// spread widely, so a launch-wide factor bound passes ~70 rows per list and
// segment; the bf16 L2 / cosine keys also need the row norms in the kernel.
// An int8 cosine dump form (the folded factors in the place of s_x) stored
// about as many rows as list launches insert: C4 440-469k vs 471k students/s
// (profiles/r05o).
constexpr bool x1_has_dump(int mode, int el) { return mode == MODE_IP; }
// The dump launches on v_mfma_i32_16x16x64_i8 (template flag S16; default):
// int8 inner-product passes (the augmented L2 among them) under the segmented
// schedule.  The same cycles per step as the 32x32x32 form, but the chip holds
// a higher clock on the 16x16 shape (tools/mfma_ceiling.hip).
// List launches, the cosine and every bf16 kernel stay on 32x32
// (the two bf16 shapes add their fp32 partial sums in different orders, so a
// list launch and a dump launch would not give a row the same key bits).
constexpr bool x1_has_s16(int mode, int el) {
  return mode == MODE_IP && el == FILTER_I8 && x1_sched(el, true) == 2;
}

__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

__device__ __forceinline__ bf16x8 as_bf(const uint4& u) { return __builtin_bit_cast(bf16x8, u); }
__device__ __forceinline__ i32x4 as_i4(const uint4& u) { return __builtin_bit_cast(i32x4, u); }

// One 32x32 block of one 64-B sub-step: C (+)= A . B on the plane's MFMA.
template <int EL>
using AccT = typename std::conditional<EL == FILTER_I8, i32x16, f32x16>::type;
template <int EL>
__device__ __forceinline__ AccT<EL> mfma_blk(const uint4& a, const uint4& b, const AccT<EL>& c) {
  if constexpr (EL == FILTER_I8)
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(as_i4(a), as_i4(b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a), as_bf(b), c, 0, 0, 0);
}

// LDS-DMA of 16 B per lane into the wave-uniform LDS byte address `lds` (M0 is
// written and restored inside the statement; cdna_hip_programming.md §5.7).
// hipcc does not count it, so it inserts no waits of its own around it: the
// caller retires it with a counted vmcnt before the barrier that precedes the
// ds_reads of that image (the builtin form makes hipcc assume every later LDS
// read may alias it and drain vmcnt to 0 before them).  No VGPR destination,
// so no register hazard.
// The source is a uniform base (SGPR pair) plus a 32-bit per-lane offset: no
// 64-bit address VGPRs beside the accumulators.
__device__ __forceinline__ void glds16(const void* sbase, uint32_t voff, uint32_t lds) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds)
      : "memory");
}

// Row order inside database tile t: LDS slot s holds tile row s ^ tile_perm(t)
// (bits 2..7, so 4-row groups stay contiguous).  The slot decides which lane
// list sees a row; without the permutation a row's list would depend only on
// row % 256, and data laid out periodically (rows of one cluster every 1024
// rows, say) would crowd a quarter of a query's lists, pulling the wide
// check's floor T toward the top and failing its bound.
__device__ __forceinline__ int tile_perm(int t) {
  return (int)(((uint32_t)t * 2654435761u) >> 24) & 0xFC;
}

__device__ __forceinline__ int sel16i(const i32x16& v, int i) {
  int r = v[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) r = i == j ? v[j] : r;
  return r;
}

__device__ __forceinline__ float sel4x4(const f32x4 (&v)[4], int i) {
  float r = v[0][0];
#pragma unroll
  for (int j = 1; j < 16; ++j) r = i == j ? v[j >> 2][j & 3] : r;
  return r;
}

// int8 candidate threshold: an integer T with fl(fl(float(a)) * c) <= lim for
// every int32 a <= T (c > 0; the scaled score is monotone in a), from an
// approximate quotient minus a margin, then checked: INT_MIN (every row a
// candidate) when the check fails.  A smaller T only admits more candidates.
__device__ __forceinline__ int i8_threshold(float lim, float c) {
  const float q = lim * __builtin_amdgcn_rcpf(c);
  const float qm = q > 0.0f ? q * (1.0f - 0x1p-20f) : q * (1.0f + 0x1p-20f);
  float fl = floorf(qm) - 2.0f;
  fl = fminf(fmaxf(fl, -2147483520.0f), 2147483520.0f);  // in int range (NaN -> lower bound)
  const int T = (int)fl;
  return (float)T * c <= lim ? T : INT_MIN;
}

__device__ __forceinline__ float sel16(const f32x16& v, int i) {
  float r = v[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) r = i == j ? v[j] : r;
  return r;
}

}  // namespace

// ---------------------------------------------------------------------------
// The step schedule.  Each 32-element step is two sub-steps of 16 (8 MFMAs per
// wave each), cut at its middle by the one barrier of the step, and the
// fragment reads run one half-step ahead of the MFMAs:
//     MFMAs of sub-step 0 (fragments read during the previous step)
//     ds_read the sub-step 1 fragments
//     wait for this wave's pieces of step s+1, s_barrier
//     LDS-DMA of step s+NBUF-1 into the image step s-1 used (every wave has
//       passed this barrier, so every read of that image is done)
//     MFMAs of sub-step 1, then ds_read sub-step 0 of step s+1 (its image is
//       complete: every wave's pieces were retired before this barrier)
// so the LDS read latency after a barrier hides under MFMAs instead of
// stalling both waves of a SIMD at every step.  The LDS-DMA steps are retired
// with a COUNTED vmcnt (the younger NBUF-2 steps stay in flight across the raw
// s_barrier; cdna_hip_programming.md "Pipelining across barriers"); loads past
// the last step re-read it (unconditional loads keep the count fixed).  64-B
// LDS rows: chunk c of row r at c ^ ((r >> 2) & 3) — conflict-free ds_read_b128
// for the 32x32x16 fragments, and one per-lane source offset for every 16-row
// group.  The first sub-step of every tile multiplies into a zero accumulator
// (the MFMA's inline-constant C), so no register clearing between tiles.  Load
// and position cursors are incremental (no divisions in the loop).
// A dump launch's stores (rare: a block below the cut) are vector-memory
// operations younger than the DMA pieces in flight: a counted wait after them
// retires more than its step needs (over-waits), never less.
//
// XCD blocking (grids of 8 S workgroups; workgroup b runs on XCD b % 8, in slot
// order b / 8 there): the S workgroups of an XCD take QG query tiles x DG
// database splits (QG = min(nqt, qg)), so each XCD's L2 holds QG query tiles'
// slices (QG x 16 KB per step) and serves a database tile to QG workgroups;
// slot / QG orders the splits, so with two rounds of workgroups per CU each
// round covers its own DG / 2 splits.  Other grids: a plain dealing.
template <int KR, int MODE, bool DUMP, int EL, bool S16 = false>
__global__ __launch_bounds__(512, 1) void gemm_topk_x1(
    const char* __restrict__ XH, const float* __restrict__ xs, const float* __restrict__ xaux,
    const char* __restrict__ QH, const float* __restrict__ qs, const float* __restrict__ qaux,
    int nqa, int nksteps, int ntotal, int ntiles, int nsplit, int nqt, int qtile0, int64_t self0,
    const int* __restrict__ qrow, const int* __restrict__ qcount, int chunk, int chunk_end,
    int nchunk, int KP, int qg, float* __restrict__ pkey, int* __restrict__ pid,
    const float* __restrict__ xgmax, const float* __restrict__ xgmin, const float* __restrict__ qcut,
    int* __restrict__ dcount, int* __restrict__ dslot, int dR, int qskip) {
  static_assert(!DUMP || x1_has_dump(MODE, EL), "dump form");
  static_assert(!S16 || (DUMP && x1_has_s16(MODE, EL)), "16x16x64 form");
  // query blocks per lane: two of 32 queries, or (S16) four of 16
  constexpr int NQB = S16 ? 4 : 2;
  constexpr int NBUF = kNbuf;
  constexpr int kStepB = kT * 64;  // one operand tile of one 32-element step: 16 KB
  constexpr int D = NBUF - 1;      // steps in flight
  static_assert(NBUF * 2 * kStepB <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[NBUF * 2 * kStepB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5;
  const int c32 = lane & 31;
  const int wr = w & 1;
  const int wq = w >> 1;

  int qt, sp;
  {
    const int nblk = gridDim.x;
    const int b = blockIdx.x;
    const int qga = qg < 0 ? -qg : qg;  // qg < 0: no rounds of groups (A/B)
    const int QG = nqt < qga ? nqt : qga;
    const int G = nqt / QG;
    const int S = nblk >> 3;
    if ((nblk & 7) == 0 && nqt * nsplit == nblk && nqt % QG == 0 && G <= 8 && 8 % G == 0 &&
        S % QG == 0) {
      const int xcd = b & 7, slot = b >> 3, DG = S / QG;
      qt = (xcd % G) * QG + slot % QG;
      sp = (xcd / G) * DG + slot / QG;
    } else if (qg > 0 && (nblk & 7) == 0 && nqt * nsplit == nblk && nqt % QG == 0 && G % 8 == 0) {
      // more query-tile groups than XCDs (C4's 65,536-student chunks: 256 query
      // tiles): XCD x takes groups x, x + 8, ... one after another, each as QG
      // query tiles x every split in slot order, so the workgroups an XCD runs
      // together share their database tiles and their QG query tiles in its L2
      // (a plain dealing put 32 different query tiles on an XCD at once)
      const int xcd = b & 7, slot = b >> 3, per = QG * nsplit;
      const int gi = slot / per, rem = slot - gi * per;
      qt = (gi * 8 + xcd) * QG + rem % QG;
      sp = rem / QG;
    } else {
      const int xcd = b & 7, slot = b >> 3, qq = nblk >> 3, rr = nblk & 7;
      const int lb = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + slot;
      qt = lb % nqt;
      sp = lb / nqt;
    }
  }
  // a gathered batch (device-side count): query tiles past it have nothing to do
  // (qskip: a gathered stage of at most qskip queries is skinny_plane_topk's)
  if (qcount && (qt * kT >= *qcount || *qcount <= qskip)) return;  // uniform
  const int s0 = (int)((int64_t)sp * ntiles / nsplit);
  const int s1 = (int)((int64_t)(sp + 1) * ntiles / nsplit);
  const int t0 = s0 + (int)((int64_t)(s1 - s0) * chunk / nchunk);
  // parts [chunk, chunk_end) of the split's nchunk (a launch usually covers one)
  const int t1 = s0 + (int)((int64_t)(s1 - s0) * chunk_end / nchunk);

  int gq[NQB], selfrow[NQB];
  float qa[NQB], qsc[NQB];
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    gq[qb] = qt * kT + 64 * wq + (S16 ? 16 * qb + (lane & 15) : 32 * qb + c32);
    qa[qb] = 0.0f;
    if constexpr (MODE == MODE_L2 || (MODE == MODE_COS && EL != FILTER_I8))
      qa[qb] = gq[qb] < nqa ? qaux[gq[qb]] : 0.0f;
    qsc[qb] = 0.0f;
    if constexpr (EL == FILTER_I8) qsc[qb] = gq[qb] < nqa ? qs[gq[qb]] : 0.0f;
    selfrow[qb] = qrow ? (gq[qb] < nqa ? qrow[gq[qb]] : -1) : self0 >= 0 ? (int)(self0 + gq[qb]) : -1;
  }
  const int P = nsplit * 4;
  // (S16: the list of a row is still bit 2 of its slot, here bit 4 of the lane)
  const int pl = sp * 4 + wr * 2 + (S16 ? (lane >> 4) & 1 : h);
  // List launches: the lane's sorted lists (admission limit: the last entry).
  // Dump launches: the query's cut (padding queries: nothing passes) and the
  // lane list's running dump count over the search's launches.
  // dump launches keep no list (the arrays are never touched there: no
  // registers)
  constexpr int KL = KR;
  float lk[2][KL];
  int li[2][KL];
  float tq[NQB] = {};
  int dc[NQB] = {};
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    if constexpr (DUMP) {
      // the cut, or the list's own last entry after the first launch when
      // that is lower (a row at or above it can never enter this list: its
      // last entry only falls)
      const int64_t o = ((int64_t)gq[qb] * P + pl) * KP + KR - 1;
      float tl = qcut[gq[qb]];
      if (pid[o] >= 0) tl = fminf(tl, pkey[o]);
      tq[qb] = gq[qb] < nqa ? tl : -FLT_MAX;
      dc[qb] = dcount[(int64_t)gq[qb] * P + pl];
      asm volatile("" ::"v"(tq[qb]), "v"(dc[qb]));
    } else {
      const int64_t o = ((int64_t)gq[qb] * P + pl) * KP;
      if (chunk == 0) {
        list_init<KR, int>(lk[qb], li[qb]);
      } else {
#pragma unroll
        for (int e = 0; e < KR; ++e) {
          lk[qb][e] = pkey[o + e];
          li[qb][e] = pid[o + e];
        }
      }
#pragma unroll
      for (int e = 0; e < KR; ++e) asm volatile("" ::"v"(lk[qb][e]), "v"(li[qb][e]));
    }
    asm volatile("" ::"v"(qa[qb]));
    if constexpr (EL == FILTER_I8) asm volatile("" ::"v"(qsc[qb]));
  }

  if (t1 > t0) {  // uniform over the workgroup
    // Planes are tile-major (vs_internal.h plane_offset): the 64-B step s of
    // the 256 rows of tile t is one contiguous 16-KB block, so a DMA piece (16
    // rows x 64 B) reads 1 KB of consecutive bytes — eight whole 128-B lines,
    // not sixteen half lines of sixteen row-major rows.
    // per-lane DMA source: row (lane >> 2) of a 16-row piece, 16-B chunk
    // swizzled by the LDS slot (c ^ ((slot >> 2) & 3))
    const uint32_t soff = (uint32_t)(lane >> 2) * 64u + (uint32_t)((lane & 3) ^ (lane >> 4)) * 16u;
    const int fsw = (c32 >> 2) & 3;
    const char* qtile = QH + (int64_t)(qtile0 + qt) * nksteps * kStepB + (uint32_t)(32 * w) * 64u;
    const uint32_t lds0 = (uint32_t)(uintptr_t)VS_LDS(smem);
    const int nsteps = (t1 - t0) * nksteps;

    // load cursor: the step it issues next (past the end it keeps re-reading
    // the last step: unconditional loads keep the vmcnt counts fixed)
    int ls = 0, lt = t0, lk_ = 0, lbuf = 0;
    // the load tile's permuted source rows: slot 32 w + 16 p + (lane >> 2) of
    // piece p reads row (32 w + 16 p) ^ (f & 0xF0) + ((lane >> 2) ^ (f & 0x0C))
    // (the two parts occupy disjoint bits): one lane offset, a uniform rest
    uint32_t xlane = 0;
    int xhi = 0;
    auto set_xoff = [&](int tt) {  // once per tile; the lane id is re-derived
      const int f = tile_perm(tt);
      const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      xhi = f & 0xF0;
      xlane = (uint32_t)((ln >> 2) ^ (f & 0x0C)) * 64u + (uint32_t)((ln & 3) ^ (ln >> 4)) * 16u;
    };
    set_xoff(t0);
    // Segmented schedule: the load cursor's step as two running uniform
    // pointers (X: the lower of the wave's two permuted 16-row groups; Q: the
    // wave's query rows) and a lane offset per X group (both >= 0: the groups
    // differ in bit 4 of the row), so a step's four pieces cost two 64-bit
    // adds and one asm block (stage_step) instead of ~40 scalar instructions
    // of address arithmetic and M0 saves
    // (inner product only: the bf16 L2 / cosine list kernels have no registers
    // to spare for the two lane offsets)
    constexpr bool kSeg = x1_sched(EL, DUMP) == 2 && MODE == MODE_IP;
    const char* xstep = nullptr;
    const char* qstep = nullptr;
    uint32_t xl0 = 0, xl2 = 0;
    auto set_step_ptrs = [&]() {
      const int r0 = (32 * w) ^ xhi, r2 = (32 * w + 16) ^ xhi;
      xstep = XH + ((int64_t)lt * nksteps + lk_) * kStepB + (uint32_t)(r0 & ~16) * 64u;
      qstep = qtile + (int64_t)lk_ * kStepB;
      xl0 = xlane + (uint32_t)(r0 & 16) * 64u;
      xl2 = xlane + (uint32_t)(r2 & 16) * 64u;
    };
    if constexpr (kSeg) set_step_ptrs();

    // int8 dump launches: one integer threshold per list for the whole launch
    // (its floor is fixed, and the factor bound is the launch's: the maximum
    // of its tiles' group maxima), so the per-block test is a maximum and a
    // compare with no per-tile loads or threshold arithmetic
    // A floor above 0 (every row of the list so far scored below 0: queries
    // pointing away from the data) needs the SMALLEST factor instead: a row
    // with a negative sum scores highest with its smallest factor, so it can
    // clear the limit only if fl(sum * fl(s_q * fmin)) does (rows with sums
    // >= 0 always clear it, and the threshold is below 0).
    int Tq[NQB] = {};
    float fm = 0.0f, fn = FLT_MAX;  // the dump tiles' largest and smallest row factors
    auto set_Tq = [&]() {
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) {
        const float c = qsc[qb] * fm, cn = qsc[qb] * fn, last = tq[qb];
        Tq[qb] = (c > 0.0f && -last >= 0.0f)                    ? i8_threshold(-last, c)
                 : (cn > 0.0f && cn <= FLT_MAX && -last < 0.0f) ? min(i8_threshold(-last, cn), -1)
                 : (c > 0.0f || -0.0f < last)                   ? INT_MIN
                                                                : INT_MAX;
        asm volatile("" ::"v"(Tq[qb]));
      }
    };
    // the launch's largest and smallest row factor
    auto set_factor_bounds = [&]() {
      const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      for (int g = 16 * t0 + ln; g < 16 * t1; g += 64) {
        fm = fmaxf(fm, xgmax[g]);
        fn = fminf(fn, xgmin[g]);
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        fm = fmaxf(fm, __shfl_xor(fm, m));
        fn = fminf(fn, __shfl_xor(fn, m));
      }
    };
    if constexpr (DUMP && EL == FILTER_I8) {
      set_factor_bounds();
      set_Tq();
    }

    AccT<EL> acc[4][2];
    // fragments of one sub-step: A (database rows) x4, B (queries) x2
    uint4 fa0[4], fb0[2], fa1[4], fb1[2];
    auto rd = [&](int buf, int s2, uint4 (&fa)[4], uint4 (&fb)[2]) {
      const char* base = smem + buf * 2 * kStepB;
      const int co = ((2 * s2 + h) ^ fsw) * 16;
      const char* cX = base + (128 * wr + c32) * 64 + co;
      const char* cQ = base + kStepB + (64 * wq + c32) * 64 + co;
      if constexpr (!VS_X1_P(2)) {
        fb[0] = *(const uint4*)cQ;
        fb[1] = *(const uint4*)(cQ + 32 * 64);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) fa[rb] = *(const uint4*)(cX + rb * 32 * 64);
      } else {
        auto opq = [](uint4& u) { asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w)); };
        asm volatile("" ::"v"(cX), "v"(cQ));
        opq(fb[0]);
        opq(fb[1]);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) opq(fa[rb]);
      }
    };
    auto mfma_rb = [&](int rb, const uint4 (&fa)[4], const uint4 (&fb)[2]) {
      acc[rb][0] = mfma_blk<EL>(fa[rb], fb[0], acc[rb][0]);
      acc[rb][1] = mfma_blk<EL>(fa[rb], fb[1], acc[rb][1]);
    };
    // the first sub-step of a tile: C = 0 (inline constant), no clearing pass
    auto mfma_rb_first = [&](int rb, const uint4 (&fa)[4], const uint4 (&fb)[2]) {
      const AccT<EL> z = {};
      acc[rb][0] = mfma_blk<EL>(fa[rb], fb[0], z);
      acc[rb][1] = mfma_blk<EL>(fa[rb], fb[1], z);
    };
    // The 16x16x64 form (S16): 8 x 4 accumulators of 16 rows x 16 queries, one
    // MFMA each per step (a 16x16x64 MFMA covers the whole 64-B step), the same
    // 128 accumulator registers and the same 12 fragment registers (fa0 | fa1
    // hold the 8 database fragments, fb0 | fb1 the 4 query fragments).  Lane l
    // holds query l & 15 of each 16-query block and rows 16 b + 4 (l >> 4) + e
    // (e = 0..3) of the wave's 128; as an operand it supplies row (or query)
    // l & 15 and K group l >> 4.  Both operands take data chunk pi(g) for K
    // group g, pi = (0, 3, 1, 2): a product is a sum over K, so any fixed
    // permutation serves, and this one makes the 16-row reads of the unchanged
    // images (chunk c of row r at c ^ ((r >> 2) & 3)) conflict-free — the
    // identity would put lanes 0-3 and 20-23 of a ds_read_b128 lane group on
    // the same banks (tests/test_x1_shape_model.py).
    i32x4 acc16[S16 ? 8 : 1][4];
    auto rd16 = [&](int buf) {
      const char* base = smem + buf * 2 * kStepB;
      const int c16 = lane & 15;
      const int co = (((0x9C >> (2 * (lane >> 4))) & 3) ^ ((c16 >> 2) & 3)) * 16;
      const char* cX = base + (128 * wr + c16) * 64 + co;
      const char* cQ = base + kStepB + (64 * wq + c16) * 64 + co;
      if constexpr (!VS_X1_P(2)) {
        fb0[0] = *(const uint4*)cQ;
        fb0[1] = *(const uint4*)(cQ + 16 * 64);
        fb1[0] = *(const uint4*)(cQ + 32 * 64);
        fb1[1] = *(const uint4*)(cQ + 48 * 64);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          fa0[b] = *(const uint4*)(cX + b * 16 * 64);
          fa1[b] = *(const uint4*)(cX + (b + 4) * 16 * 64);
        }
      } else {
        auto opq = [](uint4& u) { asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w)); };
        asm volatile("" ::"v"(cX), "v"(cQ));
        opq(fb0[0]), opq(fb0[1]), opq(fb1[0]), opq(fb1[1]);
#pragma unroll
        for (int b = 0; b < 4; ++b) opq(fa0[b]), opq(fa1[b]);
      }
    };
    // the four MFMAs of 16-row block b (C = 0 on a tile's first step)
    auto mfma16_b = [&](int b, auto first_tag) {
      if constexpr (S16) {
        const uint4& a = b < 4 ? fa0[b & 3] : fa1[b & 3];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
          const uint4& q = qb < 2 ? fb0[qb & 1] : fb1[qb & 1];
          const i32x4 c = decltype(first_tag)::value ? i32x4{} : acc16[b][qb];
          acc16[b][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(as_i4(a), as_i4(q), c, 0, 0, 0);
        }
      }
    };
    // the four LDS-DMA pieces of the load cursor's step, one at a time
    auto stage_piece = [&](int i) {
      // uniform bases (the piece's permuted 16-row group of the load tile, the
      // query tile's) + per-lane offsets below 256 rows
      const char* xbase = XH + ((int64_t)lt * nksteps + lk_) * kStepB +
                          (uint32_t)((32 * w + 16 * (i >> 1)) ^ xhi) * 64u;
      const char* qbase = qtile + (int64_t)lk_ * kStepB + (uint32_t)(16 * (i >> 1)) * 64u;
      const uint32_t lx = lds0 + (uint32_t)lbuf * (2 * kStepB) + (uint32_t)(2 * w) * 1024u;
      if constexpr (!VS_X1_P(1)) {
        if ((i & 1) == 0) {
          if constexpr (!VS_X1_P(16))
            glds16(xbase, xlane, __builtin_amdgcn_readfirstlane(lx + (i >> 1) * 1024u));
        } else {
          if constexpr (!VS_X1_P(32))
            glds16(qbase, soff, __builtin_amdgcn_readfirstlane(lx + kStepB + (i >> 1) * 1024u));
        }
      } else {
        asm volatile("" ::"v"(xlane), "v"(soff), "s"(xbase), "s"(qbase), "s"(lx));
      }
    };
    auto advance_cursor = [&]() {
      if (ls + 1 < nsteps) {
        ++ls;
        if constexpr (kSeg) {  // a tile change rebuilds them below
          xstep += kStepB;
          qstep += kStepB;
        }
        if (++lk_ == nksteps) {
          lk_ = 0;
          set_xoff(++lt);
          if constexpr (kSeg) set_step_ptrs();
        }
      }
      lbuf = lbuf + 1 == NBUF ? 0 : lbuf + 1;
    };
    // the four pieces of the load cursor's step in stage_piece's order (X
    // group 0, Q rows 0-15, X group 1, Q rows 16-31); M0 saved once, set per
    // piece (one wait state before each LDS-DMA reads it).  No instruction
    // offsets: an LDS-DMA adds its offset to the LDS address as well.
    auto stage_step = [&]() {
      if constexpr (!kSeg || (VS_X1_PROBE & (1 | 16 | 32)) != 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) stage_piece(i);
      } else {
        const uint32_t lx = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)lbuf * (2 * kStepB) +
                                                           (uint32_t)(2 * w) * 1024u);
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %4\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %5\n\t"
            "s_add_u32 m0, %4, 0x4000\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %3, %6\n\t"
            "s_add_u32 m0, %4, 0x400\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %2, %5\n\t"
            "s_add_u32 m0, %4, 0x4400\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %7, %6\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(xl0), "v"(xl2), "v"(soff), "s"(lx), "s"(xstep), "s"(qstep), "v"(soff + 1024u)
            : "memory");
        static_assert(kStepB == 0x4000, "stage_step's M0 offsets");
      }
    };
#if VS_X1_STAMP
    unsigned long long ecnt[kStampCnt] = {0, 0, 0};  // only [0] (wave level) is kept
    unsigned long long sg[kStampSeg] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tA = 0, tB = 0, eA = 0, eB = 0;
#define VS_X1_COUNT(i, v) (ecnt[i] += (v))
#define VS_X1_EMARK(i) (eB = stamp_now(), sg[i] += eB - eA, eA = eB)
#else
#define VS_X1_COUNT(i, v) ((void)0)
#define VS_X1_EMARK(i) ((void)0)
#endif
    auto epilogue = [&](int t) {
      // a block's admission limit: the list's last entry, or the floor
      auto lim = [&](int qb) -> float {
        if constexpr (DUMP) return tq[qb];
        else return lk[qb][KL - 1];
      };
      // uniform: every row of the tile exists and none is excluded
      const bool plain = self0 < 0 && !qrow && (t + 1) * kT <= ntotal;
      const int f = tile_perm(t);
      const int fh = (4 * h) ^ (f & 0x04);
      // slot 128 wr + 32 rb + 8 jj + 4 h + e holds row t kT + (slot ^ f); the
      // slot's fields are disjoint bits, so the XOR splits into a uniform part
      // (wr, rb, jj) and one lane part (h), and f leaves the low two bits (e)
      auto rowof = [&](int rb, int jj) {
        return t * kT + ((128 * wr + 32 * rb) ^ (f & 0xE0)) + ((8 * jj) ^ (f & 0x18)) + fh;
      };
      // Phase 1: the candidate rows of every (rb, qb) block, one bit per block,
      // against each block's limit before any insertion of this tile (a list's
      // last entry only tightens, so the bits are a superset).
      //  * int8: a row's score fl(fl(float(sum)) * fl(f_q * f_x)) is monotone
      //    in the sum and in f_x (factors >= 0), so with the lane's largest
      //    factor over its 16 rows (xgmax: the maximum per 32-row group and
      //    bit 2 of the row, a SCALAR load) a row can beat the limit only if
      //    its int32 sum exceeds one integer threshold per block (i8_threshold):
      //    a maximum and one compare;
      //  * bf16 inner product: the key is -sum, exactly: a maximum and a compare;
      //  * bf16 L2 / cosine: every row (the key needs the row's norm).
      uint32_t pass = 0;
      float fmx[4];  // int8: the lane's factor bound per row block
#if VS_X1_STAMP
      if constexpr (EL == FILTER_I8) eA = stamp_now();
#endif
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        fmx[rb] = 0.0f;
        if constexpr (EL == FILTER_I8 && !DUMP) {
          const int grp = (t * kT + ((128 * wr + 32 * rb) ^ (f & 0xE0))) >> 5;  // uniform
          const float g0 = xgmax[2 * grp], g1 = xgmax[2 * grp + 1];
          fmx[rb] = (fh & 4) ? g1 : g0;
        }
      }
#if VS_X1_STAMP
      if constexpr (EL == FILTER_I8) {
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) asm volatile("" ::"v"(fmx[rb]));
        VS_X1_EMARK(7);
      }
#endif
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          const float last = lim(qb);
          bool p;
          if constexpr (EL == FILTER_I8 && DUMP) {
            int amax = acc[rb][qb][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) amax = max(amax, acc[rb][qb][r]);
            p = amax > Tq[qb];
          } else if constexpr (EL == FILTER_I8) {
            const float c = qsc[qb] * fmx[rb];
            if (c > 0.0f && -last >= 0.0f) {
              int amax = acc[rb][qb][0];
#pragma unroll
              for (int r = 1; r < 16; ++r) amax = max(amax, acc[rb][qb][r]);
              p = amax > i8_threshold(-last, c);
            } else {
              p = c > 0.0f || -0.0f < last;
            }
          } else if constexpr (MODE == MODE_IP) {
            float amax = acc[rb][qb][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) amax = fmaxf(amax, acc[rb][qb][r]);
            p = -amax < last;  // NaN sums never enter
          } else {
            p = true;
          }
          pass |= (uint32_t)p << (2 * rb + qb);
        }
      }
      VS_X1_EMARK(6);
      if constexpr (VS_X1_P(128)) {
        asm volatile("" ::"v"(pass));
        pass = 0;
      }
      if constexpr (DUMP) {
        // Dump launch: every row of a block that passed whose sum clears the
        // limit (int8: above the launch's integer threshold; bf16: -sum below
        // the limit) goes to the lane list's
        // next slot as (row, raw sum): one 8-B store per candidate row (a
        // whole block's 16 sums took five stores and ~4 % of a C3 step,
        // profiles/r04f/stamp_c3_dump.txt; the single stores cost nothing
        // that can be measured: with them suppressed, VS_X1_PROBE=256, a C3
        // dump launch takes as long, profiles/r10gate — the branch's cost is
        // its VALU work).  A list past its dR slots counts on (the replay
        // fails its query).
        // (a block, not an early return: one exit keeps the step loop's
        // branch to the epilogue a single compare)
        if (__ballot(pass != 0) != 0) {  // uniform: rare
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) {
            if (pass & (1u << (2 * rb + qb))) {
              const float last = lim(qb);
              uint32_t cm = 0;
              if constexpr (EL == FILTER_I8) {
#pragma unroll
                for (int r = 0; r < 16; ++r) cm |= (uint32_t)(acc[rb][qb][r] > Tq[qb]) << r;
              } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) cm |= (uint32_t)(-acc[rb][qb][r] < last) << r;
              }
              while (cm) {
                const int bi = __builtin_ctz(cm);
                cm &= cm - 1;
                // rows past the corpus (the last tile's zero padding, whose sums
                // of 0 clear a floor above 0) take no slot
                const int row = rowof(rb, bi >> 2) + (bi & 3);
                if (!plain && !(row < ntotal && row != selfrow[qb])) continue;
                const int c = dc[qb]++;
                if (c < dR) {
                  int sum;
                  if constexpr (EL == FILTER_I8) sum = sel16i(acc[rb][qb], bi);
                  else sum = __float_as_int(sel16(acc[rb][qb], bi));
                  // slot-major (slot c of every list together): the replay's
                  // threads, one per list, read their c-th slots coalesced
                  const int64_t slot = (int64_t)c * ((int64_t)nqt * kT * P) + (int64_t)gq[qb] * P + pl;
                  if constexpr (!VS_X1_P(256)) *(i32x2*)(dslot + slot * 2) = i32x2{row, sum};
                  else asm volatile("" ::"v"(slot), "v"(row), "v"(sum));
                }
              }
            }
          }
        }
        }
        VS_X1_EMARK(8);
      } else {
      // Phases 2 and 3 per half tile (rb pair): the per-row values (int8
      // factors; bf16 L2 / cosine norms) of the lane's 32 rows, when any lane of
      // the wave has a candidate in the pair — eight 16-B loads in ONE asm
      // statement that also retires them (vmcnt(0), which drains the LDS-DMA
      // pieces in flight too: twice per tile at most; loads the compiler sees
      // would get a vmcnt counted without the DMA pieces, and its waits would
      // leak into the loop) — then the exact keys of the candidates, admitted
      // with key < the list's last entry (a row tied with it is left out even
      // when its label is lower: the lists are candidate pools, and the
      // verification only needs every row outside them to have an approximate
      // key >= its list's final last entry, which this keeps); list_insert
      // orders the admitted rows lexicographically.  The fragment registers
      // are dead here (reloaded by the next load segment).
      constexpr bool kRows = EL == FILTER_I8 || MODE == MODE_L2 || MODE == MODE_COS;
      // row blocks per load group: 2 under the segmented schedule; 1 under the
      // round-2 schedule, whose next-step fragments stay live across the
      // epilogue (registers)
      constexpr int G = x1_sched(EL, DUMP) != 1 ? 2 : 1;
#pragma unroll
      for (int hp = 0; hp < 4 / G; ++hp) {
        f32x4 rv[G][4];
#pragma unroll
        for (int r2 = 0; r2 < G; ++r2)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) rv[r2][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
        const uint32_t any = (pass >> (2 * G * hp)) & ((1u << (2 * G)) - 1u);
        if (__ballot(any != 0) == 0) continue;  // uniform
        if constexpr (kRows) {
          const float* src = EL == FILTER_I8 ? xs : xaux;
          if constexpr (G == 2) {
            const float* a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = src + rowof(2 * hp + (q >> 2), q & 3);
            asm volatile(
                "global_load_dwordx4 %0, %8, off\n\tglobal_load_dwordx4 %1, %9, off\n\t"
                "global_load_dwordx4 %2, %10, off\n\tglobal_load_dwordx4 %3, %11, off\n\t"
                "global_load_dwordx4 %4, %12, off\n\tglobal_load_dwordx4 %5, %13, off\n\t"
                "global_load_dwordx4 %6, %14, off\n\tglobal_load_dwordx4 %7, %15, off\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(rv[0][0]), "=&v"(rv[0][1]), "=&v"(rv[0][2]), "=&v"(rv[0][3]),
                  "=&v"(rv[G - 1][0]), "=&v"(rv[G - 1][1]), "=&v"(rv[G - 1][2]), "=&v"(rv[G - 1][3])
                : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]),
                  "v"(a[7])
                : "memory");
          } else {
            const float* a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = src + rowof(hp, q);
            asm volatile(
                "global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %5, off\n\t"
                "global_load_dwordx4 %2, %6, off\n\tglobal_load_dwordx4 %3, %7, off\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(rv[0][0]), "=&v"(rv[0][1]), "=&v"(rv[0][2]), "=&v"(rv[0][3])
                : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3])
                : "memory");
          }
          __builtin_amdgcn_sched_barrier(0);
          VS_X1_COUNT(0, 1);  // uniform: a scalar count
        }
#pragma unroll
        for (int r2 = 0; r2 < G; ++r2) {
          const int rb = G * hp + r2;
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) {
            if (!(pass & (1u << (2 * rb + qb)))) continue;
            uint32_t cm = 0;
            if constexpr ((MODE == MODE_L2 || MODE == MODE_COS) && EL != FILTER_I8) {
              // every row is a candidate: keys first, admission mask from them
              f32x16 key;
#pragma unroll
              for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const float v = acc[rb][qb][jj * 4 + e];
                  key[jj * 4 + e] = MODE == MODE_L2 ? l2_from_ip(qa[qb], rv[r2][jj][e], v)
                                                    : -(v * (qa[qb] * rv[r2][jj][e]));
                }
              const float last = lim(qb);
              cm = 0;
#pragma unroll
              for (int r = 0; r < 16; ++r) cm |= (uint32_t)(key[r] < last) << r;
              if (!plain) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                  const int row = rowof(rb, r >> 2) + (r & 3);
                  if (!(row < ntotal && row != selfrow[qb])) cm &= ~(1u << r);
                }
              }
              while (cm) {
                const int bi = __builtin_ctz(cm);
                cm &= cm - 1;
                const int row = rowof(rb, bi >> 2) + (bi & 3);
                list_insert<KR, int>(lk[qb], li[qb], sel16(key, bi), row);
              }
            } else {
              // the block's candidate rows (int8: sum above the block's integer
              // threshold; bf16: -sum below the last entry), then one at a time:
              // the exact key of the row and its admission
              const float last = lim(qb);
              if constexpr (EL == FILTER_I8) {
                const float c = qsc[qb] * fmx[rb];
                const int T = (c > 0.0f && -last >= 0.0f) ? i8_threshold(-last, c) : INT_MIN;
#pragma unroll
                for (int r = 0; r < 16; ++r) cm |= (uint32_t)(acc[rb][qb][r] > T) << r;
              } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) cm |= (uint32_t)(-acc[rb][qb][r] < last) << r;
              }
              while (cm) {
                const int bi = __builtin_ctz(cm);
                cm &= cm - 1;
                const int row = rowof(rb, bi >> 2) + (bi & 3);
                float key;
                if constexpr (EL == FILTER_I8)
                  key = x1_key<EL>(sel16i(acc[rb][qb], bi), qsc[qb], sel4x4(rv[r2], bi));
                else
                  key = -sel16(acc[rb][qb], bi);
                const bool ok = (plain || (row < ntotal && row != selfrow[qb])) && key < lim(qb);
                if (ok) list_insert<KR, int>(lk[qb], li[qb], key, row);
              }
            }
          }
        }
        VS_X1_EMARK(8);
      }
      }
    };

    // The dump epilogue of the 16x16x64 form: the same lists, slots, counts and
    // dump order as the 32x32 form's.  Slot 128 wr + 16 b + 4 g + e (g = lane >>
    // 4) holds row t kT + (slot ^ f); a row's list is bit 2 of its slot, g & 1,
    // so lanes l and l ^ 32 feed the SAME list of the same query and hold the
    // same floor, threshold and running count.  Within a list the 32x32 form
    // stores by ascending slot (32-row block, then jj, then e); here that is
    // 16-row block b, then the lane below 32, then its partner, then e: per
    // block the pair exchange their candidate counts (rows that take a slot
    // only), the lower lane stores first and both advance the count by the sum.
    // The control flow around the exchange is wave-uniform.
    // What the branch costs is its scan, not its stores (profiles/r10gate: a
    // C3 dump launch with the stores suppressed takes as long, one with no
    // block ever passing 0.1-0.6 ms less), and every wave of the workgroup
    // waits for the slowest at the next barrier: a query block that passed
    // drops each 16-row block with one maximum and one compare before any
    // per-row mask, and the count exchange stays out of the LDS pipe.
#if VS_X1_STAMP
    int nev = 0;  // the lane's events of this launch
#endif
    auto epilogue16 = [&](int t) {
      if constexpr (S16) {
        const bool plain = self0 < 0 && !qrow && (t + 1) * kT <= ntotal;
        const int f = tile_perm(t);
        const int fl = (4 * (lane >> 4)) ^ (f & 0x0C);
        // uniform part (wr, b) + lane part (g); f leaves the low two bits (e)
        auto rowof16 = [&](int b) { return t * kT + ((128 * wr + 16 * b) ^ (f & 0xF0)) + fl; };
        // one bit per query block: all 32 rows of the lane feed one list under
        // one threshold, so the test is one maximum and one compare per block
        uint32_t pass = 0;
#if VS_X1_STAMP
        eA = stamp_now();
#endif
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
          int amax = acc16[0][qb][0];
#pragma unroll
          for (int r = 1; r < 32; ++r) amax = max(amax, acc16[r >> 2][qb][r & 3]);
          pass |= (uint32_t)(amax > Tq[qb]) << qb;
        }
        VS_X1_EMARK(6);
        if constexpr (VS_X1_P(128)) {
          asm volatile("" ::"v"(pass));
          pass = 0;
        }
        if (__ballot(pass != 0) != 0) {  // uniform: rare
          const int64_t nl = (int64_t)nqt * kT * P;
#pragma unroll
          for (int qb = 0; qb < 4; ++qb) {
            if (__ballot((pass >> qb) & 1u) == 0) continue;  // uniform
            int* const dst = dslot + ((int64_t)gq[qb] * P + pl) * 2;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
              // most 16-row blocks of a query block that passed hold no
              // candidate: one maximum and one compare (the ballot) drops them
              // before the per-row masks
              const int m4 = max(max(acc16[b][qb][0], acc16[b][qb][1]),
                                 max(acc16[b][qb][2], acc16[b][qb][3]));
              if (__ballot(m4 > Tq[qb]) == 0) continue;  // uniform
              uint32_t cm = 0;
#pragma unroll
              for (int e = 0; e < 4; ++e) cm |= (uint32_t)(acc16[b][qb][e] > Tq[qb]) << e;
              const int row0 = rowof16(b);
              // rows past the corpus (the last tile's zero padding, whose sums
              // of 0 clear a floor above 0) and the query's own row take no slot
              // and are not counted
              if (!plain) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (!(row0 + e < ntotal && row0 + e != selfrow[qb])) cm &= ~(1u << e);
              }
              if (__ballot(cm != 0) == 0) continue;  // uniform
              const int n = __popc(cm);
              // the partner's count (every lane active): v_permlane32_swap
              // puts the lower lanes' n into the upper lanes of sw[0] and the
              // upper lanes' n into the lower lanes of sw[1] — one VALU
              // instruction, where a shuffle is a trip through the LDS pipe
              // (ds_bpermute) and a wait for it
              const auto sw = __builtin_amdgcn_permlane32_swap(n, n, false, false);
              const int np = (int)(lane < 32 ? sw[1] : sw[0]);
              int c = dc[qb] + (lane >= 32 ? np : 0);
              dc[qb] += n + np;  // counts on past dR (the replay fails the query)
#if VS_X1_STAMP
              nev += min(n, max(dR - c, 0));
#endif
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (cm & (1u << e)) {
                  if constexpr (VS_X1_P(256)) {
                    if (c < dR) asm volatile("" ::"v"(dst + (int64_t)c * nl * 2), "v"(row0 + e),
                                             "v"(acc16[b][qb][e]));
                  } else {
                    // slot-major, as in the 32x32 form
                    if (c < dR) *(i32x2*)(dst + (int64_t)c * nl * 2) = i32x2{row0 + e, acc16[b][qb][e]};
                  }
                  ++c;
                }
              }
            }
          }
        }
        VS_X1_EMARK(8);
      }
    };

    constexpr int kSched = x1_sched(EL, DUMP);
    if constexpr (kSched == 1) {
    static_assert(EL == FILTER_I8 && !DUMP, "the round-2 schedule: int8 list launches only");

    // prologue: steps 0 .. D-1 in flight, retire step 0, read its first fragments
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) stage_piece(j);
      advance_cursor();
    }
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // step 0 of the D in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    rd(0, 0, fa0, fb0);
    int buf = 0;
    // The instruction order inside a step is pinned with sched_barrier(0): hipcc
    // would otherwise move the MFMAs across the barrier and the fragment reads
    // next to their first use, undoing the half-step lookahead.
    // Stagger: waves 4-7 take the step's barrier at its start instead of its
    // middle, so they run half a step behind their SIMD partners (the LDS-DMA
    // issue of one wave beside the other's MFMAs).  Every condition above
    // still holds for them: they retire DMA(s+1) before barrier s and read
    // image s+1 only after it, and their last reads of image s-1 are consumed
    // before barrier s, after which DMA(s+D) may overwrite it.
    const bool lag = w >= 4;
#if VS_X1_STAMP
    tA = stamp_now();
#define VS_X1_MARK1(i) (tB = stamp_now(), sg[i] += tB - tA, tA = tB)
#else
#define VS_X1_MARK1(i) ((void)0)
#endif
    // one step; `first` as in the segmented schedule's seg_step (peeled)
    auto s1_step = [&](auto first_tag) {
      constexpr bool first = decltype(first_tag)::value;
      const int nbuf = buf + 1 == NBUF ? 0 : buf + 1;
      // this wave's pieces of step s+1: the steps s+2 .. s+D-1 stay in flight
      // (the lagging waves wait before this step's first pieces, the others
      // after them)
      if (lag) {  // uniform
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      __builtin_amdgcn_sched_barrier(0);
      // first half: sub-step 0 (fragments read during the previous step), with
      // the sub-step 1 reads of this step's image issued behind two MFMAs
      if constexpr (first) {  // a tile's first step starts its accumulators
        mfma_rb_first(0, fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        rd(buf, 1, fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_rb_first(1, fa0, fb0);
        mfma_rb_first(2, fa0, fb0);
        mfma_rb_first(3, fa0, fb0);
      } else {
        mfma_rb(0, fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        rd(buf, 1, fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_rb(1, fa0, fb0);
        mfma_rb(2, fa0, fb0);
        mfma_rb(3, fa0, fb0);
      }
      __builtin_amdgcn_sched_barrier(0);
      VS_X1_MARK1(0);
      // retire step s+1 (this wave's pieces); the younger D-2 steps stay in flight
      if (!lag) {  // uniform
        if constexpr (!VS_X1_P(64)) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        if constexpr (!VS_X1_P(4)) __builtin_amdgcn_s_barrier();
      }
      __builtin_amdgcn_sched_barrier(0);
      VS_X1_MARK1(1);
      // second half: next step's sub-step 0 reads first (their latency hides under
      // this half's MFMAs), then sub-step 1's MFMAs with the LDS-DMA of step s+D
      // (into the image of step s-1, which every wave has finished) between them
      rd(nbuf, 0, fa0, fb0);  // past the end: a harmless read of a stale image
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        mfma_rb(i, fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        stage_piece(i);
        __builtin_amdgcn_sched_barrier(0);
      }
      advance_cursor();
      VS_X1_MARK1(3);
      VS_X1_MARK1(5);
      buf = nbuf;
    };
    // the launch's tiles (a lambda called once, not a bare loop: hipcc assigns
    // the loop's registers differently for the bare loop, and every measurement
    // on record is of this form's code)
    auto s1_tiles = [&]() {
      for (int t = t0; t < t1; ++t) {
        s1_step(std::true_type{});
        for (int k = 1; k < nksteps; ++k) s1_step(std::false_type{});
        if constexpr (!VS_X1_P(8)) {
          epilogue(t);
        } else {
#pragma unroll
          for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) asm volatile("" ::"v"(acc[rb][qb]));
        }
        VS_X1_MARK1(5);
      }
    };
    s1_tiles();
#undef VS_X1_MARK1
    } else {
    // Segmented schedule: every step of a wave is a LOAD segment (the step's 12
    // fragment reads, the 4 LDS-DMA pieces of step s+3, the wait for this
    // wave's pieces of step s+1) and a MATRIX segment (the step's 16 MFMAs),
    // each closed by a barrier.  Waves 4-7 run one barrier behind waves 0-3,
    // so on every SIMD one wave's load segment — whose DMA issue stalls that
    // wave for ~100-185 cycles per piece (MI355X_MICROARCH.md, LDS-DMA piece
    // issue cost) — runs beside its partner's matrix segment, and no wave's
    // MFMA stream is cut by its own DMA issue (the 8-phase GEMM template's
    // pairing, cdna_hip_programming.md).  3 steps in flight over a ring of 5
    // images: the image a DMA refills was read two barriers earlier by every
    // wave (reads retired by the lgkmcnt wait that opens the reader's matrix
    // segment); an image is read only after the barrier that follows every
    // wave's counted wait for its pieces.
    // (4 steps in flight, each load segment closed by an lgkmcnt(0) so the
    // image a DMA refills could be the one read a barrier earlier: C3 70.2k vs
    // 70.8k queries/s, C2 -3 %, C4 -2 %: not shipped.  The query fragments
    // loaded straight into registers, one step ahead, instead of through LDS
    // (half the DMA pieces, two thirds of the fragment reads): C3 +0.3 %, so
    // the cost is the bytes entering the CU, not the LDS path; s_setprio on
    // either half: -0.1 %; profiles/r04n/ab_qreg_prio.txt: not shipped)
    static_assert(NBUF == 5, "segmented schedule: 3 steps in flight over 5 images");
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      stage_step();
      advance_cursor();
    }
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // this wave's pieces of step 0
    __builtin_amdgcn_s_barrier();
    const bool lag = w >= 4;
    if (lag) __builtin_amdgcn_s_barrier();  // uniform: one barrier behind
    int buf = 0;
#if VS_X1_STAMP
    tA = stamp_now();
#define VS_X1_MARK(i) (tB = stamp_now(), sg[i] += tB - tA, tA = tB)
#else
#define VS_X1_MARK(i) ((void)0)
#endif
    // One step; `first` (a tile's first step, which starts its accumulators)
    // is a compile-time tag: the loops below peel it, so a step carries no
    // branch on its position in the tile.
    auto seg_step = [&](auto first_tag) {
      constexpr bool first = decltype(first_tag)::value;
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (S16) {
        rd16(buf);
      } else {
        rd(buf, 0, fa0, fb0);
        rd(buf, 1, fa1, fb1);
      }
      __builtin_amdgcn_sched_barrier(0);
      stage_step();
      advance_cursor();
      __builtin_amdgcn_sched_barrier(0);
      VS_X1_MARK(0);
      // this wave's pieces of step s+1 (the younger steps stay in flight)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      VS_X1_MARK(1);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      VS_X1_MARK(2);
      if constexpr (S16) {
#pragma unroll
        for (int b = 0; b < 8; ++b) mfma16_b(b, first_tag);
      } else {
        if constexpr (first) {
#pragma unroll
          for (int rb = 0; rb < 4; ++rb) mfma_rb_first(rb, fa0, fb0);
        } else {
#pragma unroll
          for (int rb = 0; rb < 4; ++rb) mfma_rb(rb, fa0, fb0);
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) mfma_rb(rb, fa1, fb1);
      }
      __builtin_amdgcn_sched_barrier(0);
      VS_X1_MARK(3);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      VS_X1_MARK(4);
      VS_X1_MARK(5);
      buf = buf + 1 == NBUF ? 0 : buf + 1;
    };
    auto seg_tiles = [&]() {  // (a lambda called once: as s1_tiles)
      for (int t = t0; t < t1; ++t) {
        seg_step(std::true_type{});
        for (int k = 1; k < nksteps; ++k) seg_step(std::false_type{});
        // the tile's epilogue, beside the partner's matrix segment
        if constexpr (!VS_X1_P(8)) {
          if constexpr (S16) epilogue16(t);
          else epilogue(t);
        } else if constexpr (S16) {
#pragma unroll
          for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) asm volatile("" ::"v"(acc16[b][qb]));
        } else {
#pragma unroll
          for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) asm volatile("" ::"v"(acc[rb][qb]));
        }
        VS_X1_MARK(5);
      }
    };
    seg_tiles();
    if (!lag) __builtin_amdgcn_s_barrier();  // the lagging waves' extra one
#undef VS_X1_MARK
    }
#if VS_X1_STAMP
    {  // vector atomics; the counts are summed over the lanes
      const int grp = w >= 4 ? 1 : 0;
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kStampSeg; ++i)
          atomicAdd(&g_x1_stamps[grp * (kStampSeg + kStampCnt) + i], sg[i]);
        atomicAdd(&g_x1_stamps[2 * (kStampSeg + kStampCnt) + grp], (unsigned long long)nsteps);
      }
      if (lane == 0)
        atomicAdd(&g_x1_stamps[grp * (kStampSeg + kStampCnt) + kStampSeg], ecnt[0]);
      if constexpr (S16) {  // the lanes' event counts, one atomic per wave and bin
        const int bin = nev < kStampHist ? nev : kStampHist - 1;
        for (int v = 0; v < kStampHist; ++v) {
          const unsigned long long m = __ballot(bin == v);
          if (lane == 0 && m)
            atomicAdd(&g_x1_stamps[2 * (kStampSeg + kStampCnt) + 2 + (chunk == 1 ? 0 : kStampHist) + v],
                      (unsigned long long)__popcll(m));
        }
      }
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain before the workgroup exits
  }

  // the list offsets are recomputed from the lane id here (not kept live
  // across the main loop: registers)
  const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int pl0 = sp * 4 + wr * 2 + (S16 ? (ln >> 4) & 1 : ln >> 5);
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int64_t g =
        (int64_t)(qt * kT + 64 * wq + (S16 ? 16 * qb + (ln & 15) : 32 * qb + (ln & 31))) * P + pl0;
    if constexpr (VS_X1_P(256) && DUMP) {
      asm volatile("" ::"v"(dc[qb]), "v"(g));  // no stores: the count stays as it was
    } else if constexpr (S16) {
      // lanes l and l ^ 32 hold the same count of the same list: one writes it
      if (ln < 32) dcount[g] = dc[qb];
    } else if constexpr (DUMP) {
      dcount[g] = dc[qb];
    } else {
      const int64_t o = g * KP;
#pragma unroll
      for (int e = 0; e < KR; ++e) {
        pkey[o + e] = lk[qb][e];
        pid[o + e] = li[qb][e];
      }
      for (int e = KR; e < KP; ++e) {
        pkey[o + e] = FLT_MAX;
        pid[o + e] = -1;
      }
    }
  }
}

// Query tiles per XCD of the blocked grid (env VS_X1_QG for A/B; default 4).
static int x1_qg() {
  static const int v = [] {
    const char* e = getenv("VS_X1_QG");
    const int q = e ? atoi(e) : 0;
    return q > 0 ? q : 4;
  }();
  return v;
}

// XCD rounds of query-tile groups for grids of more than 8 groups (env
// VS_X1_XCDG=0 turns them off, for A/B; read at every search)
static bool x1_group_rounds() {
  const char* e = getenv("VS_X1_XCDG");
  return !e || atoi(e) != 0;
}

// split passes: a list launch over the first 1/8 of every workgroup's tiles
// (x1_split_den; C2 on one box, profiles/r05m: 426k queries/s at 1/8, 416k at
// 1/4, 410k as one list launch)
constexpr int kX1SplitDen = 8;

// Database tiles per workgroup per launch for a pass of per_block tiles per
// workgroup: 64, or 32 for a pass that can dump and has 128-192 tiles per
// workgroup, which 64-tile launches would cut into fewer than 4 (no dumps) and
// 32-tile ones into 4-6 (one list launch, the rest dumps): a 1.25M-row shard
// at 16 query tiles (C3 over 8 GPUs), 153 tiles: 435k vs 423k queries/s; with
// 305 tiles (2.5M rows) and at C3, 32-tile launches lose 2 % and 1 %
// (profiles/r04t/ab_chunk.txt).  Env VS_X1_CHUNK_TILES overrides both (read at
// every search: A/B runs, and tests that need multi-launch passes on small
// indexes).
// (round 6: 40-tile launches there, four of them for the 1.25M-row rank —
// one list launch, three dumps — instead of five 32-tile ones: 460.5k vs
// 447.6k / 451.6k queries/s, profiles/r06rc)
constexpr int kX1ShortChunkTiles = 40;
static int x1_chunk_tiles(int per_block, bool can_dump) {
  const char* e = getenv("VS_X1_CHUNK_TILES");
  const int v = e ? atoi(e) : 0;
  if (v > 0) return v;
  return can_dump && per_block >= 128 && per_block <= 3 * kX1ChunkTiles ? kX1ShortChunkTiles
                                                                        : kX1ChunkTiles;
}

// Split passes (env VS_X1_SPLIT=<den>, read at every search; 0 = off;
// default kX1SplitDen): a
// dump-capable pass too short for 4 launches (C2: one launch of 61 tiles per
// workgroup) runs as TWO launches, a list launch over the first 1/den of every
// workgroup's tiles and one dump launch over the rest, with the cut between
// them and one replay after: the dump launch's floor is min(cut, the list's
// last entry), so it stores a few rows per list.
static int x1_split_den() {
  const char* e = getenv("VS_X1_SPLIT");
  return e ? std::max(0, atoi(e)) : kX1SplitDen;
}
constexpr int kSplitMinTiles = 16;
// (default: the bf16 plane's passes only — clustered C3 +1.4 %, C3's int8
// pass -1 %, profiles/r05u)
// VS_X1_QUARTER=<F>: the list launch covers 1/F of the first chunk (0: off,
// 1: 1/4 as F = 4)
// (round 9: the int8 pass too when its cuts are exact-key cuts — the looser
// first cut then costs far fewer rows than the shorter list launch saves,
// profiles/r09ec)
static int x1_first_den(int el, bool ecut) {
  const char* e = getenv("VS_X1_QUARTER");
  if (!e) return el == FILTER_BF16 || ecut ? 4 : 0;
  const int v = atoi(e);
  return v == 1 ? 4 : v >= 2 ? v : 0;
}

// The launch plan of a pass: which launches run over which parts of every
// workgroup's tiles, of which kind, and what runs between them.  Host only and
// pure (the knobs above are its only other inputs): x1_launch executes it,
// x1_pass_dumps asks it whether a pass has dump launches (vs_engines.hip allocates
// the dump slots and cuts by that), and vs_x1_plan shows it to CPU tests.
// (the values are vs_x1_plan's; 1 was the hybrid launch, retired: never produced)
enum X1Kind : int { kX1List = 0, kX1Dump32 = 2, kX1Dump16 = 3 };
// what follows a launch, in this order (a bit mask)
enum : int {
  kX1Replay = 1,     // x1_replay
  kX1FirstCut = 2,   // x1_qcut: the pass's first cut, from launch 0's lists
  kX1ReplayCut = 4,  // the replay and a new cut (launch_x1_replay_cut)
  kX1ExactCut = 8,   // x1_ecut after the cut
};
struct X1Step {
  int p0, p1;  // parts [p0, p1) of X1Plan::nparts
  int kind;    // X1Kind; kX1Dump32 stands for either dump form (x1_dump_kind)
  int after;
};
struct X1Plan {
  int nparts = 1;
  // the first launch's lists set cuts, and launches c > 0 are dump launches
  bool cutting = false;
  std::vector<X1Step> step;
  int nlaunch() const { return (int)step.size(); }
};
// per_block: database tiles per workgroup; can_dump: the pass has a dump form
// and its buffers; ecut: its cuts are also exact-key cuts; gathered: a later
// stage's gathered batch; recut: X1Args::recut.
static X1Plan x1_plan(int per_block, bool can_dump, int el, bool ecut, bool gathered, int recut) {
  X1Plan p;
  const bool dump = can_dump && !gathered;
  const int chunk_tiles = x1_chunk_tiles(per_block, dump);
  // a gathered later stage (usually empty: its tiles exit at once) is one launch
  const int nchunk = gathered ? 1 : std::max(1, (per_block + chunk_tiles - 1) / chunk_tiles);
  // Dump launches after the first: its lists set the cuts (x1_qcut), the rest
  // of the pass stores only the blocks below them, and x1_replay folds the
  // dumps into the lists between segments (below).  Passes of at least 4
  // launches (C3: 20) cut their launches as they are; a shorter one (C2) is
  // a split pass when VS_X1_SPLIT allows it (above); otherwise list launches
  // (C2 forced to 4 equal launches lost in round 4: 308k vs 394k queries/s,
  // profiles/r04a/r04d_sched_c2_cl_ab.txt).
  const int den = x1_split_den();
  const bool split = dump && nchunk < 4 && den >= 2 && per_block >= kSplitMinTiles;
  p.cutting = dump && (nchunk >= 4 || split);
  // the launches as part ranges [p0, p1) of nparts
  // Quarter-chunk list launches (env VS_X1_QUARTER=0/1/F; default: bf16 passes
  // and int8 passes with exact-key cuts): a
  // cutting pass of nchunk launches lists only parts [0, 1) of 4 nchunk, then a
  // dump launch over [1, 4) and one launch per chunk.  The list launch runs at
  // ~2/3 of a dump launch's rate (a k = 60 pass of 5 chunks spent 15 of its
  // 58 ms in it, profiles/r05t), but cuts set from a quarter of the rows are
  // looser: C3 dumps 1.7x the rows, 76.5k vs 77.4k queries/s; k = 60 equal,
  // clustered +1.4 % (profiles/r05u).
  const int F = x1_first_den(el, ecut);
  const bool quarter =
      p.cutting && !split && nchunk >= 4 && F >= 2 && per_block / (F * nchunk) >= 2;
  p.nparts = split ? den : quarter ? F * nchunk : nchunk;
  const int nlaunch = split ? 2 : quarter ? nchunk + 1 : nchunk;
  for (int c = 0; c < nlaunch; ++c) {
    X1Step s;
    s.p0 = split     ? (c == 0 ? 0 : 1)
           : quarter ? (c == 0 ? 0 : c == 1 ? 1 : F * (c - 1))
                     : c;
    s.p1 = split     ? (c == 0 ? 1 : den)
           : quarter ? (c == 0 ? 1 : F * c)
                     : c + 1;
    s.kind = p.cutting && c > 0 ? kX1Dump32 : kX1List;
    s.after = 0;
    if (p.cutting && c == 0) s.after |= kX1FirstCut | (ecut ? kX1ExactCut : 0);
    // Segments of dump launches end where the data seen doubles (after
    // launches 1, 3, 7, 15, ... and the last): a dump launch's threshold is
    // min(cut, list last entry at its start), and the replay between segments
    // lowers the last entries, so a lane list meets ~8 blocks below its own
    // floor per segment whatever the data (a top-8 list over n rows is beaten
    // by ~8 of the next n) — the cut alone is too wide when 2B spans
    // thousands of rows (C3: ~5k, 63 % of the lists out of 32 slots in one
    // segment, profiles/r04b).
    //
    // The cuts again after every replay of a cutting pass but the last (recut;
    // "Query cuts", vs_x1_cuts.hip): the lists hold better keys than when the
    // cut was
    // taken, a_M has only fallen, and min(old cut, a_M(now) + 2B) is a valid
    // cut for the segments that follow (C3: the cut from 1/20 of the corpus let
    // 2.8k rows per query through, most of them in the later, longer segments).
    // After the last replay nothing reads a new cut but the verification,
    // which takes a_M + 2B itself.
    if (p.cutting && c > 0 && (((c + 1) & c) == 0 || c + 1 == nlaunch)) {
      const bool again = recut && c + 1 < nlaunch;
      s.after |= again ? kX1ReplayCut | (ecut ? kX1ExactCut : 0) : kX1Replay;
    }
    p.step.push_back(s);
  }
  return p;
}
// a plan's dump launches run the 16x16x64 form where the pass has one
static int x1_dump_kind(int mode, int el, bool dump32) {
  return x1_has_s16(mode, el) && !dump32 ? kX1Dump16 : kX1Dump32;
}

template <int KR, int MODE, int EL>
static hipError_t x1_launch(const X1Args& a, Partials part, hipStream_t st, int* ndispatch) {
  const int ntiles = (a.ntotal + kT - 1) / kT;
  const int nqt = a.nq_pad / kT;
  const int per_block = (ntiles + a.nsplit - 1) / a.nsplit;
  // A gathered later stage holds its few queries in the first query tile(s):
  // every XCD takes every query tile there (QG = nqt), so the working
  // workgroups of tile 0 spread over all XCDs instead of the 2 of 8 that QG = 4
  // gives it (clustered C3: 202 -> 151 ms per step, profiles/r02za).
  const int qg = a.qcount ? nqt : x1_qg() * (x1_group_rounds() ? 1 : -1);
  const bool dump = a.dump && x1_has_dump(MODE, EL) && !a.qcount && a.qcut && a.qbkey &&
                    a.qcut_m > 0 && a.dcount && a.dslot && a.dR > 0;
  const bool ecut = MODE == MODE_IP && EL == FILTER_I8 && a.ecut_x && a.qam;
  const X1Plan plan = x1_plan(per_block, dump, EL, ecut, a.qcount != nullptr, a.recut);
  const int nlaunch = plan.nlaunch();
  const int64_t ldb = a.ld * filter_bytes(EL);
  if (a.qtile0 < 0) return hipErrorInvalidValue;
  // the one launch site: list launches get no cuts and no dump buffers
  auto launch = [&](auto kernel, const X1Step& s, bool dumps) {
    hipLaunchKernelGGL(kernel, dim3(nqt * a.nsplit), dim3(512), 0, st, (const char*)a.XH, a.xs,
                       a.xaux, (const char*)a.QH, a.qs, a.qaux, a.nqa, (int)(ldb / 64), a.ntotal,
                       ntiles, a.nsplit, nqt, a.qtile0, a.self0, a.qrow, a.qcount, s.p0, s.p1,
                       plan.nparts, part.KP, qg, part.key, part.id, a.xgmax, a.xgmin,
                       dumps ? a.qcut : nullptr, dumps ? a.dcount : nullptr,
                       dumps ? a.dslot : nullptr, dumps ? a.dR : 0, a.qskip);
  };
  for (int c = 0; c < nlaunch; ++c) {
    const X1Step& s = plan.step[c];
    // the timed span of this launch alone (the cut and replay kernels between
    // launches stay outside the spans); the first launch of a pass whose later
    // launches dump is timed apart ("<name>_list")
    if (a.timing)
      a.timing->begin(st, !(plan.cutting && nlaunch > 1) || c > 0,
                      (double)(s.p1 - s.p0) / plan.nparts);
    switch (s.kind == kX1Dump32 ? x1_dump_kind(MODE, EL, a.dump32) : s.kind) {
      case kX1Dump16:
        if constexpr (x1_has_s16(MODE, EL))
          launch(gemm_topk_x1<KR, MODE, true, EL, true>, s, true);
        break;
      case kX1Dump32:
        if constexpr (x1_has_dump(MODE, EL)) launch(gemm_topk_x1<KR, MODE, true, EL>, s, true);
        break;
      default:
        launch(gemm_topk_x1<KR, MODE, false, EL>, s, false);
    }
    if (a.timing) a.timing->end(st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && (s.after & kX1Replay)) e = launch_x1_replay(a, part, st);
    if (e == hipSuccess && (s.after & kX1FirstCut)) e = launch_qcut(a, part, st);
    if (e == hipSuccess && (s.after & kX1ReplayCut)) e = launch_x1_replay_cut(a, part, st);
    if (e == hipSuccess && (s.after & kX1ExactCut)) e = launch_x1_ecut(a, part, st);
    if (e != hipSuccess) return e;
  }
  if (ndispatch) *ndispatch = nlaunch;
  return hipSuccess;
}

int x1_lane_len() { return 8; }
int x1_dump_slots() { return kDumpMaxR; }
// (ntotal, nsplit) carry neither the plane nor the exact-key cuts: whether a
// pass cuts does not depend on them (they only choose the quarter list launch).
bool x1_pass_dumps(int ntotal, int nsplit) {
  const int ntiles = (ntotal + kT - 1) / kT;
  return x1_plan((ntiles + nsplit - 1) / nsplit, true, FILTER_I8, false, false, 1).cutting;
}

bool x1_plan_describe(int mode, int filter, int64_t ntotal, int nsplit, bool can_dump, bool ecut,
                      bool gathered, int recut, bool dump32, int32_t* out, int cap,
                      int* nlaunch) {
  if ((filter != FILTER_I8 && filter != FILTER_BF16) || ntotal <= 0 || ntotal > INT_MAX ||
      nsplit < 1 || (mode != MODE_IP && mode != MODE_L2 && mode != MODE_COS))
    return false;
  const int64_t ntiles = (ntotal + kT - 1) / kT;
  const X1Plan plan =
      x1_plan((int)((ntiles + nsplit - 1) / nsplit), can_dump && x1_has_dump(mode, filter), filter,
              ecut && mode == MODE_IP && filter == FILTER_I8, gathered, recut);
  // out[2] was "launch 0 is a hybrid launch" (retired): 0, so the rest keep their indices
  out[0] = plan.nparts, out[1] = plan.cutting, out[2] = 0, out[3] = plan.cutting;
  out[4] = x1_pass_dumps((int)ntotal, nsplit);
  for (int c = 0; c < plan.nlaunch() && c < cap; ++c) {
    const X1Step& s = plan.step[c];
    int32_t* o = out + 5 + 4 * c;
    o[0] = s.p0, o[1] = s.p1, o[3] = s.after;
    o[2] = s.kind == kX1Dump32 ? x1_dump_kind(mode, filter, dump32) : s.kind;
  }
  *nlaunch = plan.nlaunch();
  return true;
}

hipError_t x1_stamps(unsigned long long* out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_x1_stamps), sizeof(g_x1_stamps));
  if (e == hipSuccess && reset) {
    unsigned long long z[kStampN] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_x1_stamps), z, sizeof(z));
  }
  return e;
}

template <int EL>
static hipError_t x1_dispatch(int mode, const X1Args& a, Partials part, hipStream_t st,
                              int* ndispatch) {
  switch (mode) {
    case MODE_IP:
      return x1_launch<8, MODE_IP, EL>(a, part, st, ndispatch);
    case MODE_L2:
      // int8: no L2 form (its key needs two per-row factors, which do not fit
      // the registers beside the accumulators); L2 indexes hold the bf16 plane
      if constexpr (EL == FILTER_I8) return hipErrorInvalidValue;
      else return x1_launch<8, MODE_L2, EL>(a, part, st, ndispatch);
    case MODE_COS:
      return x1_launch<8, MODE_COS, EL>(a, part, st, ndispatch);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_gemm_topk_x1(int mode, const X1Args& a, Partials part, hipStream_t st,
                               int* ndispatch) {
  // 64-B K-steps of plane rows padded to 64 elements; 256-query tiles; the
  // lists of a query are (split, row half, lane half)
  if (a.nq_pad % kT != 0 || a.ld % 64 != 0 || a.ld <= 0 || part.KP < x1_lane_len() ||
      part.P != 4 * a.nsplit || a.nsplit < 1 || a.ntotal <= 0)
    return hipErrorInvalidValue;
  if (a.filter == FILTER_I8) {
    if (!a.xs || !a.qs || !a.xgmax || !a.xgmin || a.ld > kI8MaxLd) return hipErrorInvalidValue;
    return x1_dispatch<FILTER_I8>(mode, a, part, st, ndispatch);
  }
  return x1_dispatch<FILTER_BF16>(mode, a, part, st, ndispatch);
}

bool x1_dump_applies(int mode, int filter) { return x1_has_dump(mode, filter); }

// Filter-pass candidate count: the merged approximate candidates for `need`
// exact entries, with a margin of at least 8 (0 = not served by the filter).
int x1_list_len(int need) {
  return need + 8 <= 24   ? 24
         : need + 8 <= 32 ? 32
         : need + 8 <= 64 ? 64
         : need < 128 ? 128  // inner product k = 29 .. 64 (2k - 1 <= 127)
         : need < 256 ? 256  // inner product k = 65 .. 128, L2 k <= 255
         : need < 512 ? 512  // inner product k = 129 .. 256
         : need < kVerifyMaxKF ? kVerifyMaxKF  // inner product k = 257 .. 512, L2 k <= 1023
                               : 0;
}

}  // namespace vs
