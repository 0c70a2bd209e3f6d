// vs_exact_tile.h — the exact fp32 / bf16 MFMA tile of gemm_topk (vs_gemm.hip),
// gemm_topk_rows (vs_select.hip) and gemm_range (vs_range.hip): what the three
// kernels share.  Defined here once: the workgroup mapping, the swizzle on the
// global source address and the score -> key expressions.  The lane geometry, the K loop and the epilogues stand in each
// kernel's own text (gemm_topk's is the one the others follow): as callees they
// change the kernels' instruction streams (profiles/exact_tile/code_objects.txt).
//
// Workgroup = 256 threads (4 waves), tile = 128 database rows x 128 queries.
// Wave w owns queries [32w, 32w+32) of the tile against all 128 rows: four
// 32x32 accumulators (database subtiles s = 0..3).  In v_mfma_f32_32x32x2_f32 the
// A operand is the database row block (row i = lane&31) and the B operand the
// query block (column j = lane&31), so after the K loop lane l holds, for query
// column l&31, the scores of rows (r&3) + 8(r>>2) + 4(l>>5) of each subtile: a
// lane sees one query only, and can keep that query's top-k in its own
// registers with no cross-lane traffic.  Each query therefore owns two lists per
// workgroup (lane halves h = 0, 1); the merge kernel combines them.
//
// K loop: BK = 32 floats per stage, double-buffered in LDS and filled with
// global_load_lds_dwordx4 (no VGPR staging).  An LDS row is 128 B = 8 chunks of
// 16 B; chunk c of row r is stored at c ^ ((r >> 1) & 7), which makes the
// ds_read_b128 fragment reads conflict-free (each 16-lane read group lands on 16
// distinct 16-B slots).  glds writes LDS lane-linearly, so the swizzle is applied
// to the per-lane GLOBAL source address instead.
//
// Fragment k-order: every lane reads one 16-B chunk per operand per step (chunk
// c = 2*step + h of the 128-B stage row).  fp32: the chunk holds 4 floats and
// feeds 4 x32x32x2 MFMAs (instruction t uses k = 4h + t of the 8-wide step);
// bf16: the chunk holds 8 bf16 = exactly the 32x32x16 operand of lane l
// (k = 8h + j).  A and B use the same mapping, so the product is the plain dot
// product; the summation order differs from faiss's sgemm, inside the
// documented fp32 tolerance.  Each stage moves 128 B per row: 32 floats or 64 bf16.
//
// Workgroup -> (query tile, split) mapping is XCD-aware: consecutive logical ids
// (which share a database split and differ in query tile) are packed onto one XCD
// so the 4 MiB L2 there serves each database tile to all query tiles in flight.
#pragma once

#include "vs_device.h"

namespace vs {

// Bijective XCD remap (blocks b and b+8 are dispatched to the same XCD): the
// logical block of this workgroup.  Query tile qt = lb % nqt, split sp = lb / nqt.
__device__ __forceinline__ int tile_logical_block() {
  const int nblk = gridDim.x;
  const int b = blockIdx.x;
  const int xcd = b & 7, slot = b >> 3, qq = nblk >> 3, rr = nblk & 7;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + slot;
}

// Split sp's share [t0, t1) of n tiles.
__device__ __forceinline__ void tile_split_range(int sp, int n, int nsplit, int& t0, int& t1) {
  t0 = (int)((int64_t)sp * n / nsplit);
  t1 = (int)((int64_t)(sp + 1) * n / nsplit);
}

// The swizzle on the global source address: the byte offset, inside a 128-B
// stage row, of the chunk that the lane writing physical chunk sphys sources
// for LDS row `row` of the tile (the LDS row decides the swizzle).
__device__ __forceinline__ uint32_t tile_chunk(int sphys, int row) {
  return (uint32_t)(sphys ^ ((row >> 1) & 7)) * 16u;
}

// The key of a score v = q.x: qa / xa are the query's and the row's squared
// norm (L2) or inverse norm (cosine).
template <int MODE>
__device__ __forceinline__ float gemm_key(float v, float qa, float xa) {
  if constexpr (MODE == MODE_IP) {
    return -v;
  } else if constexpr (MODE == MODE_L2) {
    return l2_from_ip(qa, xa, v);
  } else {
    return -(v * (qa * xa));
  }
}

}  // namespace vs
