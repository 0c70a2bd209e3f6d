// vs_x1_cuts.hip — between the launches of a filter pass (vs_gemm_x1.hip,
// x1_launch): the replay of a segment's dumps into the lane lists and the
// query cuts the dump launches run under — a_M + 2B from the lists (qcut,
// fused with the replay after the first), e_M + B from exact keys (ecut).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "vs_x1_device.h"

namespace vs {

// ---------------------------------------------------------------------------
// Query cuts.  The verification (vs_x1_verify.hip) needs every row outside the
// rescored set to have an approximate key >= its threshold T, and only ever uses
// T' = min(T, a_M + 2.000001 B, ...) (wide check) or passes iff T - B > E_M with
// E_M <= a_M + B (first check).  Every row with approximate key >= a_M + 2 B
// is therefore useless to both, and a_M, the M-th smallest key over a query's
// lane lists, only falls while the pass runs.  After the first launch of a
// pass, x1_qcut sets cut[q] = min(cut[q], a_M(now) + 2.000001 B) (rounded up);
// the dump launches that follow keep only the blocks that may hold a row below
// the cut, x1_replay admits their rows against min(list last, cut), and the
// verification takes T = min(T, cut) as the floor of the rows dropped that way.
// Since the final a_M <= a_M(now), the cut is never below the verification's
// own a_M + 2B: no check changes its outcome, and the lists only lose rows that
// could never enter the rescored set.  What it saves: a lane list admits rows
// against its own 8th entry (the 8th best of a 1/128 slice of the corpus at C3);
// the cut is the M-th best over all of them plus 2B, so a dump launch finds a
// block below it only for ~1 in 40 (lane, block) pairs — rare enough that a
// wave almost never waits on one (tests/test_filter_argument.py models it).
// The cut is taken again after every replay but the last (x1_replay_cut_kernel
// below, env VS_X1_RECUT): cut[q] = min(cut[q], a_M(lists after the replay) +
// 2.000001 B).  It never rises, -FLT_MAX stays, a query with fewer than M
// entries gets none, and every value it ever held is >= the final a_M + 2B, so
// the final cut is a floor for every row any launch dropped
// (tests/test_cut_refresh_argument.py).
// The int8 inner-product pass of an fp32 index lowers every cut further, to
// e_M + 1.000001 B with e_M from exact keys ("Exact-key cuts", x1_ecut_kernel
// below): such a cut may be below the final a_M + 2B, and what keeps it valid is
// that no row it drops can be in the exact top M.

// The replay of a segment of dump launches: one thread per lane list (query
// q, list pl = 4 sp + 2 wr + h).  The list as the previous launches left it,
// then every row dumped since in dump order (the order the lane met them:
// tiles ascending, launch after launch) with the key the list epilogue
// computes (x1_key, the same expression) and the same admission: key <
// min(last entry, cut), the row inside the corpus and not the query's own; the
// count restarts at zero for the next segment.  A list with more dumps than
// slots lost some: its query's cut becomes -FLT_MAX, which fails both checks
// of the verification (the query goes to the next stage) and stops the
// query's dumps.
template <int KR, int EL>
__global__ __launch_bounds__(256) void x1_replay_kernel(
    int* __restrict__ dcount, const int* __restrict__ dslot, float* __restrict__ pkey,
    int* __restrict__ pid, int P, int KP, int nqa, const float* __restrict__ qs,
    const float* __restrict__ xs, int64_t self0, int ntotal, int dR, int64_t nl,
    float* __restrict__ qcut, unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cnt = i < (int64_t)nqa * P ? dcount[i] : 0;
  replay_stats(cnt, dR, stats);
  if (cnt == 0) return;
  dcount[i] = 0;  // the next segment's dumps start at slot 0
  const int q = (int)(i / P);
  if (cnt > dR) {
    qcut[q] = -FLT_MAX;
    return;
  }
  const float cut = qcut[q];
  const float qsc = EL == FILTER_I8 ? qs[q] : 0.0f;
  const int selfrow = self0 >= 0 ? (int)(self0 + q) : -1;
  float lk[KR];
  int li[KR];
  const int64_t o = i * KP;  // KP: a multiple of 4 (launch_x1_replay)
  lane_list_load<KR>(pkey, pid, o, lk, li);
  replay_admit<KR, EL>(lk, li, dslot, i, nl, cnt, qsc, xs, selfrow, ntotal, cut);
  lane_list_store<KR>(pkey, pid, o, lk, li);
}

// The replay of launch_gemm_topk_x1's dumps (a no-op when the pass had none to
// make: the counts stay zero).
hipError_t launch_x1_replay(const X1Args& a, Partials part, hipStream_t st) {
  unsigned long long* stats = a.dstats;
  if (!a.dump || !a.dcount || a.nqa <= 0) return hipSuccess;
  if (part.KP < x1_lane_len() || part.KP % 4 != 0) return hipErrorInvalidValue;
  const int64_t n = (int64_t)a.nqa * part.P;
  const dim3 grid((unsigned)((n + 255) / 256));
  const int64_t nl = (int64_t)a.nq_pad * part.P;  // lists of the pass (the slots' stride)
  if (a.filter == FILTER_I8)
    hipLaunchKernelGGL((x1_replay_kernel<8, FILTER_I8>), grid, dim3(256), 0, st, a.dcount, a.dslot,
                       part.key, part.id, part.P, part.KP, a.nqa, a.qs, a.xs, a.self0, a.ntotal,
                       a.dR, nl, a.qcut, stats);
  else
    hipLaunchKernelGGL((x1_replay_kernel<8, FILTER_BF16>), grid, dim3(256), 0, st, a.dcount,
                       a.dslot, part.key, part.id, part.P, part.KP, a.nqa, a.qs, a.xs, a.self0,
                       a.ntotal, a.dR, nl, a.qcut, stats);
  return hipGetLastError();
}

// One workgroup of 256 threads per query: a_M = the M-th smallest key over
// the query's P lists of L entries (bitwise search on the order-preserving
// integer image), then the cut.  Fewer than M entries: no cut yet.  Up to 4,096
// entries stay in registers (C2: 256 lists x 8; one wave re-reading 2,048
// entries from memory per count cost ~0.8 ms per search, profiles/r05l), more
// are read again per count.
constexpr int kQcutThreads = 256;
__global__ __launch_bounds__(kQcutThreads) void qcut_kernel(
    const float* __restrict__ lkey, const int* __restrict__ lid, int P, int LKP, int L, int M,
    const double* __restrict__ bkey, int nq, float* __restrict__ cut, float* __restrict__ qam) {
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  if (q >= nq) return;  // uniform over the workgroup
  const int64_t base = (int64_t)q * P * LKP;
  const int n = P * L;
  // order images (uint64; empty entries 2^32, never counted)
  constexpr int kR = 16;
  uint64_t v[kR];
  const bool regs = n <= kQcutThreads * kR;  // uniform
  auto image = [&](int j) -> uint64_t {
    const int64_t o = base + (int64_t)(j / L) * LKP + j % L;
    return lid[o] >= 0 ? (uint64_t)key_order(lkey[o]) : (1ull << 32);
  };
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const int j = tid + kQcutThreads * i;
    v[i] = regs && j < n ? image(j) : (1ull << 32);
  }
  __shared__ int part[kQcutThreads / 64];
  auto count_below = [&](uint64_t y) {  // entries with order image < y (uniform result)
    int c = 0;
    if (regs) {
#pragma unroll
      for (int i = 0; i < kR; ++i) c += v[i] < y ? 1 : 0;
    } else {
      for (int j = tid; j < n; j += kQcutThreads) c += image(j) < y ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __syncthreads();  // the previous count's reads of part[] are done
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < kQcutThreads / 64; ++w) t += part[w];
    return t;
  };
  if (count_below(1ull << 32) < M) return;  // uniform
  // the largest x with fewer than M entries below it: the M-th smallest image
  uint64_t x = 0;
  for (int b = 31; b >= 0; --b)
    if (count_below(x + (1ull << b)) < M) x += 1ull << b;
  const float aM = key_unorder((uint32_t)x);
  if (tid == 0 && qam) qam[q] = aM;  // x1_ecut_kernel's candidates: the entries <= a_M
  if (tid == 0) {
    const float old = cut[q];
    const float t = lower_cut(aM, 2.000001, bkey[q], old);
    if (t < old) cut[q] = t;
  }
}

hipError_t launch_qcut(const X1Args& a, Partials part, hipStream_t st) {
  const int nq = a.nqa;
  hipLaunchKernelGGL(qcut_kernel, dim3(nq), dim3(kQcutThreads), 0, st, part.key, part.id, part.P, part.KP,
                     x1_lane_len(), a.qcut_m, a.qbkey, nq, a.qcut, a.qam);
  return hipGetLastError();
}

// The replay of a segment and the query's next cut in one kernel (the cuts
// taken again after every replay, x1_launch): one workgroup per query, thread t
// the query's lane list t (P <= 256 lists; the slots of consecutive lists are
// consecutive in every slot plane, so a wave's slot reads are whole lines as
// in x1_replay_kernel).  Each thread replays its list with x1_replay_kernel's
// own steps (replay_stats, lane_list_load, replay_admit against min(last
// entry, the cut the segment's launches ran with), lane_list_store:
// vs_x1_device.h) and the same overflow rule, and keeps it in registers; the
// workgroup then finds a_M, the M-th smallest key over the P lists, by a radix select over the four bytes of
// the order image (a 256-bin histogram per byte: 4 rounds instead of the
// bitwise search's 32) and writes the cut with qcut_kernel's lower_cut.  What
// keeps the pass exact:
//  * the cut never rises: it is written only when below the stored value;
//  * a cut of -FLT_MAX (a list of the query out of slots, now or in an earlier
//    segment) stays -FLT_MAX: nothing is below it, and the selection is skipped;
//  * fewer than M entries over the lists: no cut is written;
//  * a_M only falls while the pass runs, so every cut ever written is >= the
//    final a_M + 2B: a row dropped at launch c had key >= min(cut_c, last_c) >=
//    min(final cut, final last), which is the floor the verification takes
//    (T = min(T, cut)), and the verification itself uses nothing above a_M + 2B.
template <int KR, int EL>
__global__ __launch_bounds__(256) void x1_replay_cut_kernel(
    int* __restrict__ dcount, const int* __restrict__ dslot, float* __restrict__ pkey,
    int* __restrict__ pid, int P, int KP, const float* __restrict__ qs,
    const float* __restrict__ xs, int64_t self0, int ntotal, int dR, int64_t nl,
    float* __restrict__ qcut, unsigned long long* __restrict__ stats, int M,
    const double* __restrict__ bkey, float* __restrict__ qam) {
  __shared__ int hist[256];
  __shared__ int wsum[4];
  __shared__ int s_over, sel_digit, sel_before;
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nth = blockDim.x, nwv = nth >> 6;
  const bool has = tid < P;
  const int64_t i = (int64_t)q * P + tid;
  const int cnt = has ? dcount[i] : 0;
  replay_stats(cnt, dR, stats);
  if (tid == 0) s_over = 0;
  // the cut the segment's launches ran with (written again only at the end,
  // after every thread has read it)
  const float cut = qcut[q];
  float lk[KR];
  int li[KR];
  const int64_t o = i * KP;  // KP: a multiple of 4 (launch_x1_replay_cut)
#pragma unroll
  for (int e = 0; e < KR; ++e) lk[e] = FLT_MAX, li[e] = -1;
  if (has) lane_list_load<KR>(pkey, pid, o, lk, li);
  __syncthreads();  // s_over is zero before any list reports
  if (cnt > 0) {
    dcount[i] = 0;  // the next segment's dumps start at slot 0
    if (cnt > dR) {
      s_over = 1;  // the list lost rows: its query fails (below)
    } else {
      const float qsc = EL == FILTER_I8 ? qs[q] : 0.0f;
      const int selfrow = self0 >= 0 ? (int)(self0 + q) : -1;
      replay_admit<KR, EL>(lk, li, dslot, i, nl, cnt, qsc, xs, selfrow, ntotal, cut);
      lane_list_store<KR>(pkey, pid, o, lk, li);
    }
  }
  __syncthreads();
  if (s_over) {  // uniform
    if (tid == 0) qcut[q] = -FLT_MAX;
    return;
  }
  if (cut == -FLT_MAX) return;  // uniform: failed in an earlier segment, stays failed
  // order images of the thread's entries (empty entries are never counted)
  uint32_t v[KR];
  int nv = 0;
#pragma unroll
  for (int e = 0; e < KR; ++e) {
    v[e] = key_order(lk[e]);
    nv += li[e] >= 0 ? 1 : 0;
  }
  for (int o2 = 32; o2 > 0; o2 >>= 1) nv += __shfl_xor(nv, o2);
  if (lane == 0) wsum[wv] = nv;
  __syncthreads();
  int total = 0;
  for (int w2 = 0; w2 < nwv; ++w2) total += wsum[w2];
  if (total < M) return;  // uniform: fewer than M entries, no cut yet
  // the M-th smallest image: per byte from the top, the histogram of the
  // entries that share the bytes chosen so far and the bin where the running
  // count reaches the rank left (duplicates share a bin to the end)
  uint32_t pre = 0;
  int want = M;
  for (int sh = 24; sh >= 0; sh -= 8) {
    for (int b = tid; b < 256; b += nth) hist[b] = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < KR; ++e)
      if (li[e] >= 0 && (sh == 24 || (v[e] >> (sh + 8)) == (pre >> (sh + 8))))
        atomicAdd(&hist[(v[e] >> sh) & 0xFF], 1);
    __syncthreads();
    if (wv == 0) {  // the bin where the running count reaches `want`
      const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2],
                h3 = hist[4 * lane + 3];
      const int own = h0 + h1 + h2 + h3;
      int inc = own;  // inclusive prefix over the lanes
      for (int o2 = 1; o2 < 64; o2 <<= 1) {
        const int t = __shfl_up(inc, o2);
        if (lane >= o2) inc += t;
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
    pre |= (uint32_t)sel_digit << sh;
    want -= sel_before;
    // (the next round's first barrier separates these reads from the next
    // writes of sel_digit / sel_before; hist is rewritten before it, but only
    // wave 0 read it, before the barrier above)
  }
  if (tid == 0) {
    const float aM = key_unorder(pre);
    if (qam) qam[q] = aM;
    const float t = lower_cut(aM, 2.000001, bkey[q], cut);
    if (t < cut) qcut[q] = t;
  }
}

constexpr int kReplayCutMaxP = 256;

// The replay of a segment and the cuts after it (a cutting pass, x1_launch):
// the fused kernel for up to kReplayCutMaxP lists per query, else (or with
// a.recut == 2, the A/B of the fusion) x1_replay and x1_qcut back to back.
hipError_t launch_x1_replay_cut(const X1Args& a, Partials part, hipStream_t st) {
  if (!a.dump || !a.dcount || a.nqa <= 0) return hipSuccess;
  if (part.KP < x1_lane_len() || part.KP % 4 != 0) return hipErrorInvalidValue;
  if (a.recut == 2 || part.P > kReplayCutMaxP) {
    const hipError_t e = launch_x1_replay(a, part, st);
    return e != hipSuccess ? e : launch_qcut(a, part, st);
  }
  const int64_t nl = (int64_t)a.nq_pad * part.P;  // lists of the pass (the slots' stride)
  const dim3 block((unsigned)((part.P + 63) / 64 * 64));
  if (a.filter == FILTER_I8)
    hipLaunchKernelGGL((x1_replay_cut_kernel<8, FILTER_I8>), dim3(a.nqa), block, 0, st, a.dcount,
                       a.dslot, part.key, part.id, part.P, part.KP, a.qs, a.xs, a.self0, a.ntotal,
                       a.dR, nl, a.qcut, a.dstats, a.qcut_m, a.qbkey, a.qam);
  else
    hipLaunchKernelGGL((x1_replay_cut_kernel<8, FILTER_BF16>), dim3(a.nqa), block, 0, st, a.dcount,
                       a.dslot, part.key, part.id, part.P, part.KP, a.qs, a.xs, a.self0, a.ntotal,
                       a.dR, nl, a.qcut, a.dstats, a.qcut_m, a.qbkey, a.qam);
  return hipGetLastError();
}

// Exact-key cuts (int8 inner-product passes over fp32 rows; X1Args::ecut_x).
// Let e_M be the M-th smallest EXACT key over any M (or more) distinct
// admissible rows: the true M-th best key E_M is at most e_M.  A row whose
// approximate key is >= e_M + 1.000001 B has an exact key >= e_M + 0.000001 B >
// e_M >= E_M (|a - e| <= B): it is outside the exact top M, ties included, so
// no check needs it — the window above the M-th key is B where a_M + 2B takes
// 2B (a_M <= E_M + B is all the approximate keys can say).  The verification
// already takes T = min(T, cut) and decides T - B > E_M itself, so a cut can
// only hand a query on, never change an answer.
//
// After every cut kernel (x1_qcut or the fused replay + cut, which leave a_M in
// qam[q]) one workgroup per query takes the query's list entries with key <=
// a_M — the M best approximate ones and their ties, at most kEcutCand of them
// in (list, position) order, the same set whichever kernel took a_M — adds the
// rows kept from the earlier cuts (ecut_key / ecut_id: the M best exact keys
// scored so far, so a refresh scores only rows it has not seen and e_M only
// falls), scores the new rows with the verification's own arithmetic
// (wave_dot / wave_dot2's fp64 sums, exact_key<MODE_IP>: bit-identical to
// verify_rescore_kernel), ranks the union by (key, row) and writes
// cut = min(cut, fl_up(e_M + 1.000001 B)).  -FLT_MAX stays, fewer than M rows
// give no exact cut, and list entries are admissible rows already (inside the
// corpus, not the query's own).
constexpr int kEcutCand = 64;
__global__ __launch_bounds__(256) void x1_ecut_kernel(
    const float* __restrict__ lkey, const int* __restrict__ lid, int P, int LKP, int L, int M,
    const double* __restrict__ bkey, const float* __restrict__ qam, const float* __restrict__ X,
    const float* __restrict__ Q, int64_t ld, int ntotal, float* __restrict__ ckey,
    int* __restrict__ cid, float* __restrict__ qcut) {
  constexpr int kU = kEcutMaxM + kEcutCand;
  __shared__ int cand[kEcutCand];
  __shared__ float uk[kU];
  __shared__ int ui[kU];
  __shared__ int wsum[4];
  __shared__ int un;
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float cut = qcut[q];
  const float aM = qam[q];
  // the rows kept from the earlier cuts and the query's slice, loaded beside the
  // lists (one memory round trip for the three; the kernel is a chain of them)
  float* ck = ckey + (int64_t)q * kEcutMaxM;
  int* ci = cid + (int64_t)q * kEcutMaxM;
  if (tid < kEcutMaxM) {
    ui[tid] = ci[tid];  // valid entries first (written by rank below), -1 after them
    uk[tid] = ck[tid];
  }
  const float* qrow = Q + (int64_t)q * ld;
  const bool pairs = ld <= 256 * kQV;  // two rows per step, the query in registers
  QSlice qsl;
  if (pairs) load_qslice(qrow, ld, lane, qsl);
  // uniform: a list out of slots, or no a_M yet (fewer than M entries)
  if (cut == -FLT_MAX || !(aM < FLT_MAX)) return;
  // the candidates: entries with key <= a_M, in (list, position) order
  const bool vec = L == 8 && LKP % 4 == 0;  // lane lists as 16-B pieces
  int ncand = 0;
  for (int p0 = 0; p0 < P && ncand < kEcutCand; p0 += 256) {  // uniform
    const int p = p0 + tid;
    int ids[8];  // (static indices only: registers)
    float lk[8];
    int c = 0;
    const int64_t o = ((int64_t)q * P + p) * LKP;
#pragma unroll
    for (int e = 0; e < 8; ++e) ids[e] = -1, lk[e] = FLT_MAX;
    if (p < P && vec) {
#pragma unroll
      for (int e = 0; e < 8; e += 4) {
        const f32x4 kv = *(const f32x4*)(lkey + o + e);
        const int4 iv = *(const int4*)(lid + o + e);
        lk[e] = kv.x, lk[e + 1] = kv.y, lk[e + 2] = kv.z, lk[e + 3] = kv.w;
        ids[e] = iv.x, ids[e + 1] = iv.y, ids[e + 2] = iv.z, ids[e + 3] = iv.w;
      }
    } else if (p < P) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < L) ids[e] = lid[o + e], lk[e] = lkey[o + e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (ids[e] >= 0 && ids[e] < ntotal && lk[e] <= aM)
        ++c;
      else
        ids[e] = -1;
    }
    int inc = c;  // inclusive prefix over the workgroup's lists
    for (int o2 = 1; o2 < 64; o2 <<= 1) {
      const int t = __shfl_up(inc, o2);
      if (lane >= o2) inc += t;
    }
    __syncthreads();  // the previous round's reads of wsum
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int before = ncand + inc - c;
    for (int w = 0; w < wv; ++w) before += wsum[w];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (ids[e] >= 0) {
        if (before < kEcutCand) cand[before] = ids[e];
        ++before;
      }
    ncand += wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
  ncand = min(ncand, kEcutCand);
  // the rows kept from the earlier cuts, then the candidates not among them
  __syncthreads();  // cand, ui
  int m0 = 0;
  for (int t = 0; t < kEcutMaxM; ++t) m0 += ui[t] >= 0 ? 1 : 0;
  if (tid == 0) un = m0;
  __syncthreads();
  if (tid < ncand) {
    const int r = cand[tid];
    bool found = false;
    for (int t = 0; t < m0; ++t) found |= ui[t] == r;
    if (!found) ui[atomicAdd(&un, 1)] = r;  // < m0 + ncand <= kU
  }
  __syncthreads();
  const int n = un;
  if (pairs) {
    for (int j = m0 + 2 * wv; j < n; j += 8) {
      const int ra = ui[j], rb = j + 1 < n ? ui[j + 1] : ra;
      double da, db;
      wave_dot2<false, float>(X + (int64_t)ra * ld, X + (int64_t)rb * ld, qsl, ld, lane, da, db);
      if (lane == 0) {
        uk[j] = exact_key<MODE_IP>((float)da, q, ra, nullptr, nullptr, nullptr, nullptr);
        if (j + 1 < n)
          uk[j + 1] = exact_key<MODE_IP>((float)db, q, rb, nullptr, nullptr, nullptr, nullptr);
      }
    }
  } else {
    for (int j = m0 + wv; j < n; j += 4) {
      const int r = ui[j];
      const double acc = wave_dot<false, float>(X + (int64_t)r * ld, qrow, ld, lane);
      if (lane == 0) uk[j] = exact_key<MODE_IP>((float)acc, q, r, nullptr, nullptr, nullptr, nullptr);
    }
  }
  __syncthreads();
  // rank by (key, row) (distinct rows): the M best stay for the next cut
  if (tid < n) {
    const float k0 = uk[tid];
    const int i0 = ui[tid];
    int rank = 0;
    for (int t = 0; t < n; ++t) rank += lex_less(uk[t], ui[t], k0, i0) ? 1 : 0;
    if (rank < M) {
      ck[rank] = k0;
      ci[rank] = i0;
    }
    if (rank == M - 1) {  // e_M
      const float t = lower_cut(k0, 1.000001, bkey[q], cut);
      if (t < cut) qcut[q] = t;
    }
  }
  // (n < M: the ranks 0 .. n-1 hold the rows; the entries after them are -1
  // already — the kept set only grows up to M)
}

hipError_t launch_x1_ecut(const X1Args& a, Partials part, hipStream_t st) {
  if (!a.ecut_x || !a.ecut_q || !a.qam || !a.ecut_key || !a.ecut_id || a.nqa <= 0)
    return hipSuccess;
  if (a.qcut_m < 1 || a.qcut_m > kEcutMaxM || a.ecut_ld % 4 != 0 || x1_lane_len() > 8)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(x1_ecut_kernel, dim3(a.nqa), dim3(256), 0, st, part.key, part.id, part.P,
                     part.KP, x1_lane_len(), a.qcut_m, a.qbkey, a.qam, a.ecut_x, a.ecut_q,
                     a.ecut_ld, a.ntotal, a.ecut_key, a.ecut_id, a.qcut);
  return hipGetLastError();
}

}  // namespace vs
