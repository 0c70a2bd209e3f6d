// Stand-alone check of the host logic the search entry points share
// (check_search_args) and the engines' sizes (gemm_nsplit and the other sizing
// rules of vs_host.h, plan_stage): no GPU, no Python.  Build it with the
// sanitizers on the host side, against sanitized vs_api / vs_runtime objects
// and the library's other objects as they are (from csrc/, after `make`):
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $S"
//   hipcc $F -c vs_api.hip -o build/asan_vs_api.o
//   hipcc $F -c vs_runtime.hip -o build/asan_vs_runtime.o
//   hipcc $F -I. -c ../../tools/host_checks.hip -o build/asan_host_checks.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o build/host_checks \
//     build/asan_*.o $(make -s print-objs | tr ' ' '\n' | grep -v -e vs_api.o -e vs_runtime.o)
//   build/host_checks
#include <climits>
#include <cstdio>
#include <cstring>

#include "vs_host.h"

using namespace vs::host;

static int failures = 0;

static void expect(int rc, int want_rc, const char* want_msg, int line) {
  const char* got = vs_last_error();
  if (rc != want_rc || (want_msg && strcmp(got, want_msg) != 0)) {
    fprintf(stderr, "line %d: rc %d \"%s\", expected %d \"%s\"\n", line, rc, got, want_rc,
            want_msg ? want_msg : "");
    ++failures;
  }
}
#define EXPECT(call, rc, msg) expect((call), (rc), (msg), __LINE__)

static void expect_eq(long long got, long long want, const char* what, int line) {
  if (got != want) {
    fprintf(stderr, "line %d: %s = %lld, expected %lld\n", line, what, got, want);
    ++failures;
  }
}
#define EXPECT_EQ(expr, want) expect_eq((long long)(expr), (long long)(want), #expr, __LINE__)

// The sizing rules the engines share (vs_host.h), at their boundaries.
static void check_sizing_rules() {
  // streaming kernels: blocks of 256 rows, 1 .. 2048
  EXPECT_EQ(stream_blocks(0), 1);
  EXPECT_EQ(stream_blocks(1), 1);
  EXPECT_EQ(stream_blocks(255), 1);
  EXPECT_EQ(stream_blocks(256), 1);
  EXPECT_EQ(stream_blocks(257), 2);
  EXPECT_EQ(stream_blocks(2048 * 256), 2048);
  EXPECT_EQ(stream_blocks(INT_MAX), 2048);
  // exact-key stream: blocks of 1024 rows, 1 .. 256
  EXPECT_EQ(exact_stream_lists(0), 1);
  EXPECT_EQ(exact_stream_lists(1), 1);
  EXPECT_EQ(exact_stream_lists(255), 1);
  EXPECT_EQ(exact_stream_lists(256), 1);
  EXPECT_EQ(exact_stream_lists(257), 1);
  EXPECT_EQ(exact_stream_lists(1024), 1);
  EXPECT_EQ(exact_stream_lists(1025), 2);
  EXPECT_EQ(exact_stream_lists(INT_MAX), 256);
  // gathered GEMM: one split per row tile, 1 .. 256
  EXPECT_EQ(gathered_nsplit(0), 1);
  EXPECT_EQ(gathered_nsplit(1), 1);
  EXPECT_EQ(gathered_nsplit(255), 255);
  EXPECT_EQ(gathered_nsplit(256), 256);
  EXPECT_EQ(gathered_nsplit(257), 256);
  EXPECT_EQ(gathered_nsplit(INT_MAX), 256);
  // slot windows: whole query tiles (128), at least one, lists within 2^30 bytes
  EXPECT_EQ(slot_window_cap(0, 512, 64), 0);
  EXPECT_EQ(slot_window_cap(1, 512, 64), 1);
  EXPECT_EQ(slot_window_cap(128, 512, 64), 128);
  EXPECT_EQ(slot_window_cap(65536, 512, 64), 4096);  // 2^30 / (512 * 64 * 8)
  EXPECT_EQ(slot_window_cap(65536, 512, 32), 8192);
  EXPECT_EQ(slot_window_cap(65536, 2, 8), 65536);
  EXPECT_EQ(slot_window_cap(INT_MAX, 2, 8), 8388608);  // 2^30 / 128
  EXPECT_EQ(slot_window_cap(65536, 512, 1024), 256);   // 2^30 / 2^22
  EXPECT_EQ(slot_window_cap(65536, 4096, 1024), 128);  // 32 slots' worth: one tile all the same
  // GEMV: 8 query rows of ld floats + 16 KB of lists in 64 KB of LDS
  EXPECT_EQ(gemv_fits(0), 1);
  EXPECT_EQ(gemv_fits(64), 1);
  EXPECT_EQ(gemv_fits(1536), 1);  // 8 * 1536 * 4 = 48 KB
  EXPECT_EQ(gemv_fits(1537), 0);
  EXPECT_EQ(gemv_fits(INT_MAX), 0);
}

static StageShape shape(int mode, int plane, int KF, int nq, int nq_pad, int64_t ntotal) {
  StageShape s;
  s.mode = mode;
  s.plane = plane;
  s.KF = KF;
  s.nq = nq;
  s.nq_pad = nq_pad;
  s.ntotal = ntotal;
  s.L = 8;
  s.skinny_max_q = vs::skinny_plane_max_queries();
  return s;
}

// plan_stage against the rules of run_filter_verify as they stood before it
// was split, worked by hand: nqt = nq_pad / 256 query tiles, ntiles =
// ceil(ntotal / 256); base = max(min(ntiles, lpc * ceil(KF / 8)), min(ntiles,
// ceil(wg / nqt))) with lpc = 8 for inner product at KF >= 64, else 4, and wg
// = 256 up to 8 query tiles, else 512.
static void check_plan_stage() {
  using namespace vs;
  const int64_t N = 10000000;  // ntiles 39,063
  const int I8 = FILTER_I8, B16 = FILTER_BF16;
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 24, 1024, 1024, N)).nsplit, 64);    // 1: 256 / 4
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 24, 4096, 4096, N)).nsplit, 32);    // 2: 512 / 16
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 24, 2048, 2048, N)).nsplit, 32);    // 3: 256 / 8
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 24, 2304, 2304, N)).nsplit, 57);    // 4: ceil(512 / 9)
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 64, 4096, 4096, N)).nsplit, 64);    // 5: 8 * 8
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 128, 4096, 4096, N)).nsplit, 128);  // 6: 8 * 16
  EXPECT_EQ(plan_stage(shape(MODE_COS, I8, 64, 65536, 65536, N)).nsplit, 32); // 7: 4 * 8
  EXPECT_EQ(plan_stage(shape(MODE_IP, I8, 24, 4096, 4096, 1000)).nsplit, 4);  // 8: ntiles
  {
    // 9: the deep stage, max(base 32, min(ntiles, 512, 2^30 / (4096 * 4 * 8 * 8) = 1024)) =
    // 512: lane lists of 4096 * 4 * 512 * 8 * 8 B = 512 MiB.  (256 would be the
    // cap of 8,192 slots; 4,096 slots leave room for all 512.)
    StageShape s = shape(MODE_IP, B16, 24, 4096, 4096, N);
    s.gathered = s.deep = true;
    EXPECT_EQ(plan_stage(s).nsplit, 512);
    s.nq = s.nq_pad = 8192;  // 2^30 / (8192 * 256) = 512 still; 16,384 slots: 256
    EXPECT_EQ(plan_stage(s).nsplit, 512);
    s.nq = s.nq_pad = 16384;
    EXPECT_EQ(plan_stage(s).nsplit, 256);
    s.nq = s.nq_pad = 256;  // 10: base 256 / 1, deep min(ntiles, 512, 16384)
    EXPECT_EQ(plan_stage(s).nsplit, 512);
    EXPECT_EQ(plan_stage(s).small, 0);
  }
  EXPECT_EQ(plan_stage(shape(MODE_IP, B16, 24, 4096, 4096, N)).nsplit, 64);  // 11: 2 * 32
  {
    const StagePlan p = plan_stage(shape(MODE_IP, I8, 24, 8, 128, 262144));  // 12: ntiles 1024
    EXPECT_EQ(p.small, 1);
    EXPECT_EQ(p.nsplit, 256);  // (1024 + 3) / 4
    EXPECT_EQ(p.nq_pad, 256);
    const StagePlan q = plan_stage(shape(MODE_IP, I8, 24, 8, 128, N));  // 13
    EXPECT_EQ(q.small, 1);
    EXPECT_EQ(q.nsplit, 512);
  }
  {
    StageShape s = shape(MODE_IP, I8, 24, 4096, 4096, N);
    s.split_mult = 2;  // 14
    EXPECT_EQ(plan_stage(s).nsplit, 64);
    s.ntotal = 1000;  // 15: never more splits than tiles
    EXPECT_EQ(plan_stage(s).nsplit, 4);
    s = shape(MODE_IP, I8, 24, 4096, 4096, N);
    s.wgs_env = 1024;  // 16: 1024 / 16
    EXPECT_EQ(plan_stage(s).nsplit, 64);
  }
  {  // not small: no inner-product pass, a self-join, too many queries, a later stage
    EXPECT_EQ(plan_stage(shape(MODE_COS, I8, 24, 8, 128, N)).small, 0);
    StageShape s = shape(MODE_IP, I8, 24, 8, 128, N);
    s.self_join = true;
    EXPECT_EQ(plan_stage(s).small, 0);
    s = shape(MODE_L2, I8, 24, 8, 128, N);
    EXPECT_EQ(plan_stage(s).small, 0);
    s.l2aug = true;
    EXPECT_EQ(plan_stage(s).small, 1);
    s = shape(MODE_IP, I8, 24, s.skinny_max_q, 128, N);
    EXPECT_EQ(plan_stage(s).small, 1);
    s.nq = s.skinny_max_q + 1;
    EXPECT_EQ(plan_stage(s).small, 0);
    EXPECT_EQ(plan_stage(s).nsplit, 256);  // the x1 pass of one query tile
  }
  // every shape: 1 <= nsplit <= ntiles, whole query tiles, deep lists within 1 GiB
  const int64_t rows[] = {1, 255, 256, 257, 65536, ((int64_t)1 << 31) - 257};
  const int pads[] = {256, 65536};
  int last_kf = 0;
  for (int need = 1; need < kVerifyMaxKF; ++need) {
    const int KF = x1_list_len(need);
    if (KF == last_kf) continue;
    last_kf = KF;
    for (int64_t nt : rows)
      for (int pad : pads)
        for (int plane : {B16, I8})
          for (int later = 0; later < 2; ++later)
            for (int mode : {(int)MODE_IP, (int)MODE_L2, (int)MODE_COS}) {
              StageShape s = shape(mode, plane, KF, pad, pad, nt);
              s.gathered = later != 0;  // gathered alone: the base rule, nothing else
              const StagePlan base = plan_stage(s);
              s.deep = later != 0;
              const StagePlan p = plan_stage(s);
              const int64_t ntiles = (nt + 255) / 256;
              const bool ok =
                  p.nsplit >= 1 && p.nsplit <= std::max<int64_t>(1, ntiles) && p.nq_pad % 256 == 0 &&
                  p.nq_pad >= pad &&
                  (p.nsplit <= base.nsplit ||  // the deep rule raised it: within 1 GiB
                   (int64_t)p.nq_pad * 4 * p.nsplit * 8 * 8 <= ((int64_t)1 << 30));
              if (!ok) {
                fprintf(stderr, "plan_stage(mode %d plane %d KF %d nq_pad %d ntotal %lld later %d) = "
                        "nsplit %d nq_pad %d\n", mode, plane, KF, pad, (long long)nt, later, p.nsplit,
                        p.nq_pad);
                ++failures;
              }
            }
  }
  EXPECT_EQ(last_kf, kVerifyMaxKF);
}

int main() {
  // a non-null index: the checks never read it
  static char store[64];
  const vs_index* idx = reinterpret_cast<const vs_index*>(store);
  const int64_t neg = -1, zero = 0, one = 1, big = INT64_MAX, low = INT64_MIN;
  const int E = VS_E_INVALID;

  EXPECT(check_search_args("vs_search", nullptr, &neg, 0, false, false), E, "vs_search: null index");
  EXPECT(check_search_args("vs_search_sel", idx, &neg, 0, false, false), E,
         "vs_search_sel: null selector");
  EXPECT(check_search_args("vs_search", idx, &neg, 0, false), E, "vs_search: n < 0");
  EXPECT(check_search_args("vs_search", idx, &low, 1), E, "vs_search: n < 0");
  EXPECT(check_search_args("vs_search", idx, &one, 0, false), E, "vs_search: k must be > 0");
  EXPECT(check_search_args("vs_search", idx, &one, low), E, "vs_search: k must be > 0");
  EXPECT(check_search_args("vs_search", idx, &one, INT_MAX / 2 + 1), E, "vs_search: k too large");
  EXPECT(check_search_args("vs_search", idx, &big, big), E, "vs_search: k too large");
  EXPECT(check_search_args("vs_search", idx, &one, INT_MAX / 2, false), E,
         "vs_search: null buffer");
  // no queries: no buffer is needed; no count: the caller checks its own
  EXPECT(check_search_args("vs_search", idx, &zero, 1, false), VS_OK, nullptr);
  EXPECT(check_search_args("vs_search", idx, &big, INT_MAX / 2), VS_OK, nullptr);
  EXPECT(check_search_args("vs_selfjoin", idx, nullptr, 0), E, "vs_selfjoin: k must be > 0");
  EXPECT(check_search_args("vs_selfjoin", idx, nullptr, 1), VS_OK, nullptr);
  EXPECT(check_search_args("vs_selfjoin", idx, nullptr, 1, false), E, "vs_selfjoin: null buffer");
  // a prefix longer than any small-string buffer
  EXPECT(check_search_args("vs_search_profiles_with_a_long_name", nullptr, nullptr, 1), E,
         "vs_search_profiles_with_a_long_name: null index");
  // the exported entry points, on the same path
  EXPECT(vs_search(nullptr, nullptr, 1, 1, nullptr, nullptr, 0, nullptr), E, "vs_search: null index");
  EXPECT(vs_selfjoin(const_cast<vs_index*>(idx), 0, 1, INT_MAX, 1, 0.0f, nullptr, nullptr, 0,
                     nullptr),
         E, "vs_selfjoin: k too large");

  // gemm_nsplit: about 512 workgroups over the query tiles, 1 <= nsplit <= ntiles
  // (callers pass at most 512 query tiles; INT_MAX - 512 is the most its int sum holds)
  const int tiles[] = {0, 1, 2, 3, 255, 256, 511, 512, 513, 78125, INT_MAX};
  const int qtiles[] = {1, 2, 3, 4, 7, 8, 255, 256, 511, 512, 513, 65536 / 128, INT_MAX - 512};
  for (int nt : tiles)
    for (int nq : qtiles) {
      const int s = gemm_nsplit(nt, nq);
      const int64_t want =
          std::max<int64_t>(1, std::min<int64_t>(nt, ((int64_t)512 + nq - 1) / nq));
      if (s != want || s < 1 || (nt >= 1 && s > nt)) {
        fprintf(stderr, "gemm_nsplit(%d, %d) = %d, expected %lld\n", nt, nq, s, (long long)want);
        ++failures;
      }
    }
  check_sizing_rules();
  check_plan_stage();
  if (failures) return 1;
  printf("host checks ok\n");
  return 0;
}
