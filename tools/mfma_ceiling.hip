// The held-clock MFMA ceiling at the filter pass's occupancy (VERDICT r04
// "next" 2): one workgroup of 8 waves per CU (two per SIMD, 160 KB of LDS
// declared so no second workgroup fits), every wave issuing the filter
// kernel's MFMAs of one 64-B (int8) / 32-element (bf16) step of K into its
// 128-row x 64-query output tile — and nothing else: no loads in the loop, no
// LDS, no barriers.  What it reaches is the most the filter kernel's tile can
// reach on this chip at the clock the chip holds under MFMA load; bench.py's
// roofline fraction against the nominal peak reads against it.
//
// Two MFMA shapes run at that same output tile per wave and the same 12
// 16-byte operand fragments per lane and step:
//   32x32: 8 accumulators of 16 registers, two K sub-steps, 16 MFMAs per step
//          (v_mfma_i32_32x32x32_i8 / v_mfma_f32_32x32x16_bf16) — the shape the
//          x1 pass runs;
//   16x16: 32 accumulators of 4 registers, one K step, 32 MFMAs per step
//          (v_mfma_i32_16x16x64_i8 / v_mfma_f32_16x16x32_bf16).
// The cycles per step are the same (16 x 16 passes against 32 x 8), so what
// differs by wall is the clock the chip holds on each shape.  Operands are
// random (int8: uniform bytes; bf16: uniform [-1, 1)), generated on the host
// and loaded once before the loop: lane-index patterns or zeros read high
// because the chip holds a higher clock on them.  The shapes run alternated in
// one process, `runs` runs each, a run being one warm launch and `launches`
// timed ones back to back.
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/mfma_ceiling tools/mfma_ceiling.hip
//   tools/mfma_ceiling [iters [runs [launches]]]
// prints one JSON line per plane and shape, then one line per plane comparing
// the shapes: the ratio of the means, both run-to-run spreads, and whether the
// 16x16 loop is faster by more than either spread.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define CHECK(x)                                                               \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

constexpr int kLds = 160 * 1024;
constexpr int kFrags = 12;  // 16-byte operand fragments per lane: 8 database + 4 query

// ops: kFrags fragments per lane, [frag][lane] — every wave loads the same 12 KB.
template <bool I8, bool S16>
__global__ __launch_bounds__(512) void mfma_loop(int iters, const i32x4* __restrict__ ops, int* out) {
  extern __shared__ char lds[];  // occupancy only: never touched
  (void)lds;
  const int lane = threadIdx.x & 63;
  i32x4 f[kFrags];
#pragma unroll
  for (int i = 0; i < kFrags; ++i) f[i] = ops[i * 64 + lane];
  if constexpr (S16) {
    // database fragment rb (16 rows x the whole K step) x query fragment qb
    if constexpr (I8) {
      i32x4 acc[8][4];
      for (int rb = 0; rb < 8; ++rb)
        for (int qb = 0; qb < 4; ++qb) acc[rb][qb] = i32x4{};
      for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rb = 0; rb < 8; ++rb)
#pragma unroll
          for (int qb = 0; qb < 4; ++qb)
            acc[rb][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(f[rb], f[8 + qb], acc[rb][qb], 0, 0, 0);
      }
      int r = 0;
      for (int rb = 0; rb < 8; ++rb)
        for (int qb = 0; qb < 4; ++qb)
          for (int e = 0; e < 4; ++e) r ^= acc[rb][qb][e];
      if (r == 0x7fffffff) out[blockIdx.x] = r;  // keeps the loop; never true in practice
    } else {
      f32x4 acc[8][4];
      for (int rb = 0; rb < 8; ++rb)
        for (int qb = 0; qb < 4; ++qb) acc[rb][qb] = f32x4{};
      for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rb = 0; rb < 8; ++rb)
#pragma unroll
          for (int qb = 0; qb < 4; ++qb)
            acc[rb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, f[rb]), __builtin_bit_cast(bf16x8, f[8 + qb]), acc[rb][qb], 0, 0, 0);
      }
      float r = 0.f;
      for (int rb = 0; rb < 8; ++rb)
        for (int qb = 0; qb < 4; ++qb)
          for (int e = 0; e < 4; ++e) r += acc[rb][qb][e];
      if (r == 1.2345f) out[blockIdx.x] = 1;
    }
  } else {
    // database fragment (rb, s): 32 rows x K sub-step s, at f[s * 4 + rb]; query
    // fragment (qb, s) at f[8 + s * 2 + qb] — the x1 kernel's fa0/fa1, fb0/fb1
    if constexpr (I8) {
      i32x16 acc[4][2];
      for (int rb = 0; rb < 4; ++rb)
        for (int qb = 0; qb < 2; ++qb) acc[rb][qb] = i32x16{};
      for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
              acc[rb][qb] =
                  __builtin_amdgcn_mfma_i32_32x32x32_i8(f[s * 4 + rb], f[8 + s * 2 + qb], acc[rb][qb], 0, 0, 0);
      }
      int r = 0;
      for (int rb = 0; rb < 4; ++rb)
        for (int qb = 0; qb < 2; ++qb)
          for (int e = 0; e < 16; ++e) r ^= acc[rb][qb][e];
      if (r == 0x7fffffff) out[blockIdx.x] = r;
    } else {
      f32x16 acc[4][2];
      for (int rb = 0; rb < 4; ++rb)
        for (int qb = 0; qb < 2; ++qb) acc[rb][qb] = f32x16{};
      for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
              acc[rb][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f[s * 4 + rb]),
                                                                    __builtin_bit_cast(bf16x8, f[8 + s * 2 + qb]),
                                                                    acc[rb][qb], 0, 0, 0);
      }
      float r = 0.f;
      for (int rb = 0; rb < 4; ++rb)
        for (int qb = 0; qb < 2; ++qb)
          for (int e = 0; e < 16; ++e) r += acc[rb][qb][e];
      if (r == 1.2345f) out[blockIdx.x] = 1;
    }
  }
}

struct Ctx {
  int cus, iters, launches;
  int* out;
  const i32x4* ops_i8;
  const i32x4* ops_bf;
  hipEvent_t e0, e1;
};

// One run: a warm launch, then `launches` timed ones back to back.  Returns TOP/s.
template <bool I8, bool S16>
double one_run(const Ctx& c) {
  const i32x4* ops = I8 ? c.ops_i8 : c.ops_bf;
  mfma_loop<I8, S16><<<c.cus, 512, kLds>>>(c.iters, ops, c.out);
  CHECK(hipGetLastError());
  CHECK(hipEventRecord(c.e0));
  for (int l = 0; l < c.launches; ++l) mfma_loop<I8, S16><<<c.cus, 512, kLds>>>(c.iters, ops, c.out);
  CHECK(hipEventRecord(c.e1));
  CHECK(hipEventSynchronize(c.e1));
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, c.e0, c.e1));
  // per wave and iteration: a 128 x 64 output tile over K = 64 (int8) / 32 (bf16), 2 ops per MAC
  const double ops_n = (double)c.cus * 8 * c.iters * c.launches * 128.0 * 64.0 * (I8 ? 64 : 32) * 2;
  return ops_n / (ms * 1e-3) / 1e12;
}

struct Stat {
  double mean, mn, mx;
};

Stat report(const char* plane, const char* shape, const Ctx& c, const std::vector<double>& t, double peak) {
  Stat s{0., 1e30, 0.};
  for (double v : t) {
    s.mean += v;
    s.mn = v < s.mn ? v : s.mn;
    s.mx = v > s.mx ? v : s.mx;
  }
  s.mean /= t.size();
  printf("{\"plane\": \"%s\", \"shape\": \"%s\", \"operands\": \"random\", \"cus\": %d, \"iters\": %d, "
         "\"launches_per_run\": %d, \"runs_tops\": [",
         plane, shape, c.cus, c.iters, c.launches);
  for (size_t i = 0; i < t.size(); ++i) printf("%s%.1f", i ? ", " : "", t[i]);
  // the implied clock: the fraction of the peak, which is quoted at 2.4 GHz
  printf("], \"tops_mean\": %.1f, \"tops_min\": %.1f, \"tops_max\": %.1f, \"spread\": %.4f, "
         "\"peak_tops\": %.1f, \"frac_of_peak\": %.4f, \"implied_clock_ghz\": %.3f, "
         "\"implied_clock_ghz_min\": %.3f}\n",
         s.mean, s.mn, s.mx, (s.mx - s.mn) / s.mean, peak, s.mean / peak, 2.4 * s.mean / peak, 2.4 * s.mn / peak);
  return s;
}

void compare(const char* plane, const Stat& a32, const Stat& a16) {
  const double sp32 = (a32.mx - a32.mn) / a32.mean, sp16 = (a16.mx - a16.mn) / a16.mean;
  const double ratio = a16.mean / a32.mean;
  const bool faster = ratio - 1.0 > (sp32 > sp16 ? sp32 : sp16) && a16.mn > a32.mx;
  printf("{\"plane\": \"%s\", \"ratio_16x16_over_32x32_mean\": %.4f, \"worst_16x16_over_best_32x32\": %.4f, "
         "\"spread_32x32\": %.4f, \"spread_16x16\": %.4f, \"faster_16x16_beyond_spread\": %s}\n",
         plane, ratio, a16.mn / a32.mx, sp32, sp16, faster ? "true" : "false");
}

int main(int argc, char** argv) {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  Ctx c{};
  c.cus = p.multiProcessorCount;
  c.iters = argc > 1 ? atoi(argv[1]) : 20000;
  const int runs = argc > 2 ? atoi(argv[2]) : 5;
  c.launches = argc > 3 ? atoi(argv[3]) : 10;
  if (c.iters < 1 || runs < 1 || c.launches < 1) {
    fprintf(stderr, "usage: mfma_ceiling [iters [runs [launches]]], all >= 1\n");
    return 2;
  }

  // random operands from the host: uniform bytes for int8, uniform [-1, 1) as bf16 (RNE)
  const size_t nbytes = (size_t)kFrags * 64 * sizeof(i32x4);
  std::mt19937 rng(20240607);
  std::vector<uint8_t> h_i8(nbytes);
  for (auto& b : h_i8) b = (uint8_t)(rng() & 0xff);
  std::vector<uint16_t> h_bf(nbytes / 2);
  std::uniform_real_distribution<float> uni(-1.f, 1.f);
  for (auto& h : h_bf) {
    const float v = uni(rng);
    uint32_t u;
    memcpy(&u, &v, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    h = (uint16_t)(u >> 16);
  }
  void *d_i8 = nullptr, *d_bf = nullptr;
  CHECK(hipMalloc(&d_i8, nbytes));
  CHECK(hipMalloc(&d_bf, nbytes));
  CHECK(hipMemcpy(d_i8, h_i8.data(), nbytes, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_bf, h_bf.data(), nbytes, hipMemcpyHostToDevice));
  c.ops_i8 = (const i32x4*)d_i8;
  c.ops_bf = (const i32x4*)d_bf;
  CHECK(hipMalloc(&c.out, sizeof(int) * c.cus));
  CHECK(hipEventCreate(&c.e0));
  CHECK(hipEventCreate(&c.e1));
  CHECK(hipFuncSetAttribute((const void*)mfma_loop<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  CHECK(hipFuncSetAttribute((const void*)mfma_loop<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  CHECK(hipFuncSetAttribute((const void*)mfma_loop<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  CHECK(hipFuncSetAttribute((const void*)mfma_loop<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));

  std::vector<double> i8_32, i8_16, bf_32, bf_16;
  for (int r = 0; r < runs; ++r) {  // alternated: every shape once per round
    i8_32.push_back(one_run<true, false>(c));
    i8_16.push_back(one_run<true, true>(c));
    bf_32.push_back(one_run<false, false>(c));
    bf_16.push_back(one_run<false, true>(c));
  }
  const Stat s_i8_32 = report("int8", "32x32x32", c, i8_32, 5000.0);
  const Stat s_i8_16 = report("int8", "16x16x64", c, i8_16, 5000.0);
  const Stat s_bf_32 = report("bf16", "32x32x16", c, bf_32, 2500.0);
  const Stat s_bf_16 = report("bf16", "16x16x32", c, bf_16, 2500.0);
  compare("int8", s_i8_32, s_i8_16);
  compare("bf16", s_bf_32, s_bf_16);

  CHECK(hipFree(c.out));
  CHECK(hipFree(d_i8));
  CHECK(hipFree(d_bf));
  CHECK(hipEventDestroy(c.e0));
  CHECK(hipEventDestroy(c.e1));
  return 0;
}
