// common.hip -- error reporting, version and the ordered sum of per-block partials for libsniper_hip.so
#include "common.h"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

static thread_local char g_err[512] = "";

void sn_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

SN_EXPORT const char *sn_last_error(void) { return g_err; }
SN_EXPORT int sn_version(void) { return 100; }

hipError_t sn_once_per_device_max_lds(const void *kernel, int bytes) {
  static std::mutex mu;
  static std::vector<std::pair<const void *, int>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  for (const auto &d : done)
    if (d.first == kernel && d.second == dev) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.emplace_back(kernel, dev);
  return e;
}

static std::atomic<int> g_debug[SN_OPT_COUNT];
static const char *const kDebugNames[SN_OPT_COUNT] = {"proposal_full_sort", "nms_full_mask", "conv_no_persist", "softmax_strided"};
static const char *const kDebugEnv[SN_OPT_COUNT] = {"SNIPER_FULL_SORT", "SNIPER_NMS_FULL", "SNIPER_CONV_NO_PERSIST", "SNIPER_SOFTMAX_STRIDED"};
namespace {
struct DebugInit {
  DebugInit() {
    for (int i = 0; i < SN_OPT_COUNT; ++i) g_debug[i].store(getenv(kDebugEnv[i]) != nullptr ? 1 : 0, std::memory_order_relaxed);
  }
} g_debug_init;
}  // namespace

int sn_debug_get(SnDebugOption which) { return g_debug[which].load(std::memory_order_relaxed); }

__global__ __launch_bounds__(256) void partial_sum_kernel(const float *__restrict__ part, int nblk, long n, float *__restrict__ dst) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  // the blocks are added in block order (fixed bits), but their loads are independent: eight in flight instead of a chain
  // of nblk dependent L2 round trips (13.5 us for 96 blocks)
  float s = 0.f;
  int k = 0;
  for (; k + 8 <= nblk; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(k + u) * n + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < nblk; ++k) s += part[(size_t)k * n + e];
  dst[e] += s;
}

int sn_partial_sum(const float *part, int nblk, long n, float *dst, hipStream_t s) {
  hipLaunchKernelGGL(partial_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, nblk, n, dst);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_debug_option(const char *name, int value) {
  SN_REQUIRE(name, "sn_debug_option: null name");
  for (int i = 0; i < SN_OPT_COUNT; ++i)
    if (strcmp(name, kDebugNames[i]) == 0) {
      g_debug[i].store(value, std::memory_order_relaxed);
      return SN_OK;
    }
  SN_REQUIRE(false, "sn_debug_option: unknown option '%s'", name);
}
