// vs_runtime.hip — process-wide host state of libvsearch.so, one definition
// each: the calling thread's error string, the reader marks' waits, the
// scratch chunk cache, the kernel timer and the filter statistics, with the
// exports that read them (vs_last_error, vs_timer_*, vs_filter_*_stats,
// vs_x1_stamps).
#include "vs_host.h"

using namespace vs;
using namespace vs::host;

namespace {
thread_local std::string g_err;
}  // namespace

namespace vs {
namespace host {

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? VS_E_OOM : VS_E_HIP;
}

ReaderMark::~ReaderMark() {
  std::lock_guard<std::mutex> g(idx->rd_mu);
  for (auto& r : idx->readers)
    if (r.first == st) {
      (void)hipEventRecord(r.second, st);
      return;
    }
  // a new stream: first drop the marks that have completed (a caller with a
  // stream per request would otherwise grow the list, and every writer's
  // wait_readers, without bound)
  for (size_t i = 0; i < idx->readers.size();) {
    if (hipEventQuery(idx->readers[i].second) == hipSuccess) {
      (void)hipEventDestroy(idx->readers[i].second);
      idx->readers[i] = idx->readers.back();
      idx->readers.pop_back();
    } else {
      ++i;
    }
  }
  (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);  // no mark possible: finish the work instead
    return;
  }
  (void)hipEventRecord(ev, st);
  idx->readers.emplace_back(st, ev);
}

hipError_t wait_readers(vs_index* idx) {
  std::lock_guard<std::mutex> g(idx->rd_mu);
  for (auto& r : idx->readers) {
    hipError_t e = hipEventSynchronize(r.second);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t writer_stream(vs_index* idx, hipStream_t* out) {
  if (!idx->wst) {
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    e = hipStreamCreateWithPriority(&idx->wst, hipStreamNonBlocking, greatest);
    if (e != hipSuccess) return e;
  }
  *out = idx->wst;
  return hipSuccess;
}

}  // namespace host
}  // namespace vs

// Scratch chunks (vs_internal.h): power-of-two sizes from 64 MB, kept after
// use with the event of their last use; a taker's stream waits on that event
// (a device-side wait).
namespace {
std::mutex g_chunk_mu;
std::vector<ScratchChunk> g_chunk_idle;
size_t g_chunk_idle_bytes = 0;
constexpr size_t kChunkMin = size_t(64) << 20;
constexpr size_t kChunkIdleCap = size_t(16) << 30;  // per process
}  // namespace

namespace vs {
void scratch_trim() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::vector<ScratchChunk> drop;
  {
    std::lock_guard<std::mutex> g(g_chunk_mu);
    for (size_t i = 0; i < g_chunk_idle.size();) {
      if (g_chunk_idle[i].dev == dev) {
        drop.push_back(g_chunk_idle[i]);
        g_chunk_idle_bytes -= g_chunk_idle[i].size;
        g_chunk_idle[i] = g_chunk_idle.back();
        g_chunk_idle.pop_back();
      } else {
        ++i;
      }
    }
  }
  if (drop.empty()) return;
  for (auto& c : drop) (void)hipEventSynchronize(c.ev);  // each chunk's last use
  for (auto& c : drop) {
    (void)hipFree(c.p);
    (void)hipEventDestroy(c.ev);
  }
}

hipError_t scratch_chunk_get(size_t bytes, hipStream_t st, ScratchChunk* out) {
  size_t sz = kChunkMin;
  while (sz < bytes) sz <<= 1;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  // An idle chunk last used on this stream needs no wait (stream order), one
  // whose last use has completed needs none either; a chunk still in use on
  // another stream would tie this call to that stream's queue (another
  // index's long searches, say), so a new chunk is allocated instead while
  // memory allows, and only then is the busy one taken with a device-side wait.
  int busy = -1;
  {
    std::lock_guard<std::mutex> g(g_chunk_mu);
    int pick = -1;
    for (size_t i = 0; i < g_chunk_idle.size(); ++i) {
      const ScratchChunk& c = g_chunk_idle[i];
      // the power-of-two chunk of this request, or an exact-size one (the OOM
      // fallback below) that holds it
      if (c.dev != dev || c.size < bytes || c.size > sz) continue;
      if (c.st == st || hipEventQuery(c.ev) == hipSuccess) {
        pick = (int)i;
        break;
      }
      if (busy < 0) busy = (int)i;
    }
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady
    if (pick >= 0) {
      *out = g_chunk_idle[pick];
      g_chunk_idle[pick] = g_chunk_idle.back();
      g_chunk_idle.pop_back();
      g_chunk_idle_bytes -= out->size;
      return out->st == st ? hipSuccess : hipStreamWaitEvent(st, out->ev, 0);
    }
  }
  ScratchChunk c;
  c.size = sz;
  c.dev = dev;
  e = hipMalloc(&c.p, sz);
  if (e != hipSuccess && busy >= 0) {  // short of memory: wait for the busy chunk
    (void)hipGetLastError();
    std::lock_guard<std::mutex> g(g_chunk_mu);
    for (size_t i = 0; i < g_chunk_idle.size(); ++i) {
      if (g_chunk_idle[i].dev == dev && g_chunk_idle[i].size >= bytes &&
          g_chunk_idle[i].size <= sz) {
        *out = g_chunk_idle[i];
        g_chunk_idle[i] = g_chunk_idle.back();
        g_chunk_idle.pop_back();
        g_chunk_idle_bytes -= out->size;
        return hipStreamWaitEvent(st, out->ev, 0);
      }
    }
  }
  if (e != hipSuccess) {  // idle chunks of other sizes may hold the memory
    (void)hipGetLastError();
    scratch_trim();
    e = hipMalloc(&c.p, sz);
  }
  if (e != hipSuccess) {  // the power-of-two rounding may be what does not fit
    (void)hipGetLastError();
    const size_t exact = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
    if (exact >= sz) return e;
    c.size = exact;
    e = hipMalloc(&c.p, exact);
    if (e != hipSuccess) return e;
  }
  e = hipEventCreateWithFlags(&c.ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    (void)hipFree(c.p);
    return e;
  }
  *out = c;
  return hipSuccess;
}

void scratch_chunk_put(const ScratchChunk& c0, hipStream_t st) {
  if (!c0.p) return;
  ScratchChunk c = c0;
  c.st = st;
  (void)hipEventRecord(c.ev, st);
  {
    std::lock_guard<std::mutex> g(g_chunk_mu);
    if (g_chunk_idle_bytes + c.size <= kChunkIdleCap) {
      g_chunk_idle.push_back(c);
      g_chunk_idle_bytes += c.size;
      return;
    }
  }
  (void)hipEventSynchronize(c.ev);
  (void)hipFree(c.p);
  (void)hipEventDestroy(c.ev);
}
}  // namespace vs

namespace {
std::mutex g_timer_mu;
bool g_timer_on = false;
struct TimedSpan {
  hipEvent_t a, b;
  int dispatches;
  const char* name;
  bool aux;      // an extra span over other spans' kernels: not in the unnamed total
  double share;  // the span's share of its pass's database tiles (filter passes)
};
std::vector<TimedSpan> g_timer_events;
const char* g_timer_kernel = "";

std::mutex g_stats_mu;
std::vector<unsigned long long*> g_dev_stats;
}  // namespace

namespace vs {
namespace host {

unsigned long long* device_stats(int dev) {
  std::lock_guard<std::mutex> g(g_stats_mu);
  if ((int)g_dev_stats.size() <= dev) g_dev_stats.resize(dev + 1, nullptr);
  if (!g_dev_stats[dev]) {
    unsigned long long* p = nullptr;
    if (hipMalloc(&p, kStatSlots * sizeof(unsigned long long)) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, kStatSlots * sizeof(unsigned long long)) != hipSuccess) return nullptr;
    g_dev_stats[dev] = p;
  }
  return g_dev_stats[dev];
}

KernelTimer::KernelTimer(hipStream_t s, const char* nm, bool names_kernel) : st(s), name(nm) {
  if (!name) return;
  std::lock_guard<std::mutex> g(g_timer_mu);
  if (names_kernel) g_timer_kernel = name;
  aux = !names_kernel;
  if (!g_timer_on) return;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
    a = b = nullptr;
    return;
  }
  (void)hipEventRecord(a, st);
}

void KernelTimer::stop() {
  if (!a) return;
  (void)hipEventRecord(b, st);
  std::lock_guard<std::mutex> g(g_timer_mu);
  g_timer_events.push_back({a, b, dispatches, name, aux, share});
  a = b = nullptr;
}

}  // namespace host
}  // namespace vs

extern "C" {

const char* vs_last_error(void) { return g_err.c_str(); }

// The counters live on the devices (written by the searches' own kernels); reading
// them waits for every search already queued on those devices.
static int read_filter_stats(unsigned long long out[kStatSlots], int reset) {
  for (int i = 0; i < kStatSlots; ++i) out[i] = 0;
  std::lock_guard<std::mutex> g(g_stats_mu);
  for (int dev = 0; dev < (int)g_dev_stats.size(); ++dev) {
    if (!g_dev_stats[dev]) continue;
    DeviceGuard dg(dev);
    unsigned long long h[kStatSlots] = {};
    VS_HIP(hipDeviceSynchronize(), "vs_filter_stats");
    VS_HIP(hipMemcpy(h, g_dev_stats[dev], sizeof(h), hipMemcpyDeviceToHost), "vs_filter_stats");
    for (int i = 0; i < kStatSlots; ++i) out[i] += h[i];
    if (reset) VS_HIP(hipMemset(g_dev_stats[dev], 0, sizeof(h)), "vs_filter_stats");
  }
  return VS_OK;
}

int vs_filter_stats(int64_t* queries, int64_t* fallbacks, int reset) {
  if (!queries || !fallbacks) return fail(VS_E_INVALID, "vs_filter_stats: null output");
  unsigned long long c[kStatSlots];
  int rc = read_filter_stats(c, reset);
  if (rc) return rc;
  *queries = (int64_t)c[0];
  *fallbacks = (int64_t)c[2];
  return VS_OK;
}

int vs_filter_wide_stats(int64_t* wide) {
  if (!wide) return fail(VS_E_INVALID, "vs_filter_wide_stats: null output");
  unsigned long long c[kStatSlots];
  int rc = read_filter_stats(c, 0);
  if (rc) return rc;
  *wide = (int64_t)c[1];
  return VS_OK;
}

int vs_filter_wide_sets(int64_t* entries, int64_t* rescored) {
  if (!entries || !rescored) return fail(VS_E_INVALID, "vs_filter_wide_sets: null output");
  unsigned long long c[kStatSlots];
  int rc = read_filter_stats(c, 0);
  if (rc) return rc;
  *entries = (int64_t)c[4];
  *rescored = (int64_t)c[5];
  return VS_OK;
}

int vs_filter_dump_stats(int64_t* dumps, int64_t* overflows) {
  if (!dumps || !overflows) return fail(VS_E_INVALID, "vs_filter_dump_stats: null output");
  unsigned long long c[kStatSlots];
  int rc = read_filter_stats(c, 0);
  if (rc) return rc;
  *dumps = (int64_t)c[6];
  *overflows = (int64_t)c[7];
  return VS_OK;
}

int vs_filter_second_stats(int64_t* second) {
  if (!second) return fail(VS_E_INVALID, "vs_filter_second_stats: null output");
  unsigned long long c[kStatSlots];
  int rc = read_filter_stats(c, 0);
  if (rc) return rc;
  *second = (int64_t)c[3];
  return VS_OK;
}

int vs_filter_exact_stats(int64_t* streamed) {
  if (!streamed) return fail(VS_E_INVALID, "vs_filter_exact_stats: null output");
  unsigned long long c[kStatSlots];
  int rc = read_filter_stats(c, 0);
  if (rc) return rc;
  *streamed = (int64_t)c[8];
  return VS_OK;
}

int vs_x1_stamps(unsigned long long* out, int reset) {
  if (!out) return fail(VS_E_INVALID, "vs_x1_stamps: null buffer");
  VS_HIP(x1_stamps(out, reset), "vs_x1_stamps");
  return VS_OK;
}

int vs_timer_enable(int on) {
  std::lock_guard<std::mutex> g(g_timer_mu);
  g_timer_on = on != 0;
  return VS_OK;
}

int vs_timer_reset(void) {
  std::lock_guard<std::mutex> g(g_timer_mu);
  for (auto& p : g_timer_events) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  g_timer_events.clear();
  return VS_OK;
}

const char* vs_timer_kernel(void) {
  std::lock_guard<std::mutex> g(g_timer_mu);
  return g_timer_kernel;
}

int vs_timer_read(double* total_ms, int64_t* launches) {
  return vs_timer_read_kernel(nullptr, total_ms, launches);
}

int vs_timer_read_kernel_share(const char* kernel, double* total_ms, int64_t* launches,
                               double* share) {
  if (!total_ms || !launches) return fail(VS_E_INVALID, "vs_timer_read: null output");
  std::lock_guard<std::mutex> g(g_timer_mu);
  double tot = 0.0, sh = 0.0;
  int64_t n = 0;
  for (auto& p : g_timer_events) {
    if (kernel ? strcmp(kernel, p.name) != 0 : p.aux) continue;
    VS_HIP(hipEventSynchronize(p.b), "vs_timer_read: synchronise");
    float ms = 0.0f;
    VS_HIP(hipEventElapsedTime(&ms, p.a, p.b), "vs_timer_read: elapsed");
    tot += ms;
    n += p.dispatches;
    sh += p.share;
  }
  *total_ms = tot;
  *launches = n;
  if (share) *share = sh;
  return VS_OK;
}

int vs_timer_read_kernel(const char* kernel, double* total_ms, int64_t* launches) {
  return vs_timer_read_kernel_share(kernel, total_ms, launches, nullptr);
}

}  // extern "C"
