// Stand-alone check of the host logic the search entry points share
// (check_search_args, gemm_nsplit): no GPU, no Python.  Build it with the
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
  if (failures) return 1;
  printf("host checks ok\n");
  return 0;
}
