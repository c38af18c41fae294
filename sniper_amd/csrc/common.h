// common.h -- shared helpers for the gfx950 kernel library (internal, not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sniper_hip.h"

#define SN_EXPORT extern "C" __attribute__((visibility("default")))

void sn_set_error(const char *fmt, ...);

#define SN_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      sn_set_error(__VA_ARGS__);   \
      return SN_ERR_ARG;           \
    }                              \
  } while (0)

// Launch-time errors only (no sync): a failed launch is reported, asynchronous faults surface at
// the caller's next synchronisation like any HIP error.
#define SN_CHECK_LAUNCH()                                                      \
  do {                                                                         \
    hipError_t e__ = hipGetLastError();                                        \
    if (e__ != hipSuccess) {                                                   \
      sn_set_error("%s:%d HIP launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e__)); \
      return SN_ERR_HIP;                                                       \
    }                                                                          \
  } while (0)

#define SN_HIP(call)                                                           \
  do {                                                                         \
    hipError_t e__ = (call);                                                   \
    if (e__ != hipSuccess) {                                                   \
      sn_set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
      return SN_ERR_HIP;                                                       \
    }                                                                          \
  } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device property of a kernel: applied once per (kernel, device),
// thread-safe (a mutex-guarded registry, no unsynchronised flag).
hipError_t sn_once_per_device_max_lds(const void *kernel, int bytes);
// Process-wide test / A-B switches (sn_debug_option in the header): relaxed atomics, initialised from the environment once at
// load time (SNIPER_FULL_SORT, SNIPER_NMS_FULL, SNIPER_CONV_NO_PERSIST, SNIPER_SOFTMAX_STRIDED), never a getenv inside a launch path.
enum SnDebugOption { SN_OPT_PROPOSAL_FULL_SORT = 0, SN_OPT_NMS_FULL_MASK = 1, SN_OPT_CONV_NO_PERSIST = 2, SN_OPT_SOFTMAX_STRIDED = 3, SN_OPT_COUNT };
int sn_debug_get(SnDebugOption which);

static inline hipStream_t sn_stream(sn_stream_t s) { return (hipStream_t)s; }
static inline int sn_div_up(int a, int b) { return (a + b - 1) / b; }
static inline size_t sn_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// integer environment switch read once at load time (static initialisers of the A/B and tuning overrides)
static inline int sn_env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}
// output extent of a convolution / pooling window along one axis
static inline int sn_conv_out(int in, int k, int stride, int pad, int dil) { return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1; }
// 1-D grid of a grid-stride kernel with 256-thread blocks: one thread per element up to `cap` blocks, never an empty grid
static inline int sn_blocks(long total, int cap) {
  const long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

constexpr int kWave = 64;  // CDNA wavefront width

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// order-preserving map float32 -> uint32 (any sign, no NaN): a < b <=> key(a) < key(b)
__device__ __forceinline__ unsigned sn_float_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// dst[e] += sum_k part[k * n + e], e < n: per-block partial sums added in block order (no atomics, the same bits every run) --
// the finish of the depthwise / grouped weight gradients and of the bias gradient (common.hip)
int sn_partial_sum(const float *part, int nblk, long n, float *dst, hipStream_t s);

// Division by a launch-invariant divisor as multiply-high + shift (n < 2^31, d >= 1): q = (umulhi(n, mul) + n) >> sh.  An integer
// division costs ~40 VALU instructions on gfx950 (64-bit: ~80); index decompositions of element-wise kernels use these instead.
struct SnDiv { unsigned mul, sh, d; };
static inline SnDiv sn_div_make(unsigned d) {
  SnDiv f;
  unsigned s = 0;
  while ((1ull << s) < d) ++s;
  f.mul = (unsigned)((((unsigned long long)1 << 32) * (((unsigned long long)1 << s) - d)) / d + 1);
  f.sh = s;
  f.d = d;
  return f;
}
__device__ __forceinline__ unsigned sn_div(unsigned n, const SnDiv f) { return (__umulhi(n, f.mul) + n) >> f.sh; }
// n -> (n / d, n % d)
__device__ __forceinline__ unsigned sn_divmod(unsigned n, const SnDiv f, unsigned &rem) {
  const unsigned q = sn_div(n, f);
  rem = n - q * f.d;
  return q;
}
