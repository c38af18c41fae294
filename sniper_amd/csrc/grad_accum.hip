// grad_accum.hip -- gradient accumulation: the fp32 gradient arena of one micro-batch is copied into (first) or added onto a second
// arena of the same size, so that the optimizer pass runs once per k micro-batches on their sum (include/sniper_hip.h; DESIGN.md
// section 33).  One launch per micro-step, beside the replayed forward/backward graph.
//
// The pass is a pure stream -- 8 bytes per element for the copy, 12 for the add -- in the form of the guard's partial pass
// (grad_guard.hip): 256-thread blocks, four 16-byte accesses per array in flight per lane per trip (16 KiB per array, block and trip), a
// grid-stride loop over at most 2048 blocks (eight per CU).  The split follows the WRITTEN array: d_acc is peeled to its 16-byte
// boundary, the body stores 16 bytes per lane, block 0 does the 0-3 head and 0-3 tail elements one at a time.  d_grad behind the head
// is read 16 bytes wide when it is 16-byte aligned there too (the engine's two arenas always are: same offset from two allocations of
// the runtime), else with four 4-byte loads per store.  No atomics, no LDS, no scratch; every element is read and written by
// exactly one thread, once, so the result does not depend on the grid.
#include "common.h"

namespace {

constexpr int kThreads = 256;                 // threads per block
constexpr int kVec = 4;                       // 16-byte stores per lane per trip
constexpr int kElems = 4 * kVec;              // floats per thread per trip
constexpr int kSpan = kThreads * kElems;      // floats per block per trip
constexpr int kDefaultBlocks = 2048;          // the library's grid cap (max_blocks = 0)
constexpr int kMaxBlocks = 65535;

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

inline int accum_blocks(long n, int max_blocks) {
  const long cap = max_blocks > 0 ? max_blocks : kDefaultBlocks;
  const long b = (n + kSpan - 1) / kSpan;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// four elements of the gradient behind the head: one 16-byte load, or four 4-byte loads where that address is not 16-byte aligned.
// Bit patterns, not floats: the copy must not touch a NaN payload.
template <bool kGradVec>
__device__ __forceinline__ uintx4 accum_load(const unsigned *__restrict__ g, long i) {
  if (kGradVec) return reinterpret_cast<const uintx4 *>(g)[i];
  uintx4 v;
  v.x = g[4 * i + 0];
  v.y = g[4 * i + 1];
  v.z = g[4 * i + 2];
  v.w = g[4 * i + 3];
  return v;
}

__device__ __forceinline__ unsigned accum_one(unsigned a, unsigned g) { return __float_as_uint(__uint_as_float(a) + __uint_as_float(g)); }

// acc[0, head): in front of the first 16-byte boundary of acc; body = n4 groups of four from there; tail = what is left (0-3)
template <bool kFirst, bool kGradVec>
__global__ __launch_bounds__(kThreads) void grad_accum_kernel(unsigned *__restrict__ acc, const unsigned *__restrict__ grad, long n,
                                                              long head, long n4) {
  uintx4 *__restrict__ abody = reinterpret_cast<uintx4 *>(acc + head);
  const unsigned *__restrict__ gbody = grad + head;
  const long stride = (long)gridDim.x * (kThreads * kVec);
  for (long base = (long)blockIdx.x * (kThreads * kVec) + threadIdx.x; base < n4; base += stride) {
    uintx4 g[kVec], a[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const long i = base + (long)j * kThreads;
      if (i < n4) {
        g[j] = accum_load<kGradVec>(gbody, i);
        if (!kFirst) a[j] = abody[i];
      }
    }
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const long i = base + (long)j * kThreads;
      if (i < n4) {
        uintx4 r = g[j];
        if (!kFirst) {
          r.x = accum_one(a[j].x, g[j].x);
          r.y = accum_one(a[j].y, g[j].y);
          r.z = accum_one(a[j].z, g[j].z);
          r.w = accum_one(a[j].w, g[j].w);
        }
        abody[i] = r;
      }
    }
  }
  if (blockIdx.x == 0) {
    const long done = head + 4 * n4;
    const long t = threadIdx.x;
    if (t < head) acc[t] = kFirst ? grad[t] : accum_one(acc[t], grad[t]);
    if (done + t < n) acc[done + t] = kFirst ? grad[done + t] : accum_one(acc[done + t], grad[done + t]);      // (n - done <= 3)
  }
}

}  // namespace

SN_EXPORT int sn_grad_accumulate_limits(int32_t *h_out3) {
  SN_REQUIRE(h_out3, "sn_grad_accumulate_limits: null pointer");
  h_out3[0] = kThreads;
  h_out3[1] = kElems;
  h_out3[2] = kDefaultBlocks;
  return SN_OK;
}

SN_EXPORT int sn_grad_accumulate(float *d_acc, const float *d_grad, long n, int first, int max_blocks, sn_stream_t stream) {
  SN_REQUIRE(n >= 0, "sn_grad_accumulate: n = %ld", n);
  SN_REQUIRE(max_blocks >= 0 && max_blocks <= kMaxBlocks, "sn_grad_accumulate: max_blocks = %d outside 0 .. %d", max_blocks, kMaxBlocks);
  SN_REQUIRE(((uintptr_t)d_acc & 3) == 0 && ((uintptr_t)d_grad & 3) == 0, "sn_grad_accumulate: d_acc and d_grad must be 4-byte aligned");
  if (n == 0) return SN_OK;
  SN_REQUIRE(d_acc && d_grad, "sn_grad_accumulate: null pointer");
  const uintptr_t a0 = (uintptr_t)d_acc, g0 = (uintptr_t)d_grad, bytes = (uintptr_t)n * 4;
  SN_REQUIRE(a0 + bytes <= g0 || g0 + bytes <= a0, "sn_grad_accumulate: [d_acc, d_acc + n) and [d_grad, d_grad + n) overlap");
  long head = (long)(((16 - (a0 & 15)) & 15) / 4);
  if (head > n) head = n;
  const long n4 = (n - head) / 4;
  const bool grad_vec = ((g0 + 4 * (uintptr_t)head) & 15) == 0;
  const dim3 grid(accum_blocks(n, max_blocks)), block(kThreads);
  unsigned *acc = reinterpret_cast<unsigned *>(d_acc);
  const unsigned *grad = reinterpret_cast<const unsigned *>(d_grad);
  hipStream_t s = sn_stream(stream);
  if (first) {
    if (grad_vec)
      hipLaunchKernelGGL((grad_accum_kernel<true, true>), grid, block, 0, s, acc, grad, n, head, n4);
    else
      hipLaunchKernelGGL((grad_accum_kernel<true, false>), grid, block, 0, s, acc, grad, n, head, n4);
  } else {
    if (grad_vec)
      hipLaunchKernelGGL((grad_accum_kernel<false, true>), grid, block, 0, s, acc, grad, n, head, n4);
    else
      hipLaunchKernelGGL((grad_accum_kernel<false, false>), grid, block, 0, s, acc, grad, n, head, n4);
  }
  SN_CHECK_LAUNCH();
  return SN_OK;
}
