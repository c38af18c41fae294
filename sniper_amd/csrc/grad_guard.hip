// grad_guard.hip -- the gradient guard of the optimizer pass: ONE read of the fp32 gradient arena gives the sum of squares of its finite
// elements and the number of non-finite ones; a single-block finalize turns them into the eight doubles of device state that
// sn_sgd_mom_update_guarded_dev (nn_ops.hip) consults: the norm, the global-norm clipping coefficient, the skip flag, the counters.
// Everything stays on the device and inside the replayed optimizer graph (include/sniper_hip.h: the state layout).
//
// The pass is a pure read stream: 256-thread blocks, four 16-byte loads in flight per lane per trip (16 KiB per block and trip),
// a grid-stride loop over at most 1024 blocks (four per CU: 64 KiB of loads in flight per CU).  Sums are fp64 -- the square of an
// fp32 value is exact in fp64 -- per thread, then per wave (shuffles), then per block (LDS), one partial per block; the finalize
// launch adds the partials in index order.  No atomics anywhere: for a given (n, max_blocks, alignment of d_grad) the same bits
// every run.  (A "last block finalizes" variant inside the first launch lost to this separate launch every time it was tried.)
#include <float.h>
#include <math.h>

#include "common.h"
#include "grad_guard.h"

namespace {

// non-finite <=> !(|g| <= FLT_MAX): counted and left out of the sum (adding 0.0 is exact)
__device__ __forceinline__ void guard_take(float g, double &s, unsigned &c) {
  const bool ok = fabsf(g) <= FLT_MAX;
  const double d = ok ? (double)g : 0.0;
  s += d * d;
  c += ok ? 0u : 1u;
}

// grad[0, head): the elements in front of the first 16-byte boundary; body = n4 float4 from there; tail = what is left (0-3)
__global__ __launch_bounds__(kThreads) void grad_guard_partial_kernel(const float *__restrict__ grad, long n, long head, long n4,
                                                                      double *__restrict__ psum,
                                                                      unsigned long long *__restrict__ pcnt) {
  const float4 *__restrict__ body = reinterpret_cast<const float4 *>(grad + head);
  double s = 0.0;
  unsigned c = 0;
  const long stride = (long)gridDim.x * (kThreads * kVec);
  for (long base = (long)blockIdx.x * (kThreads * kVec) + threadIdx.x; base < n4; base += stride) {
    float4 v[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const long i = base + (long)j * kThreads;
      v[j] = i < n4 ? body[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      guard_take(v[j].x, s, c);
      guard_take(v[j].y, s, c);
      guard_take(v[j].z, s, c);
      guard_take(v[j].w, s, c);
    }
  }
  if (blockIdx.x == 0) {
    const long done = head + 4 * n4;
    if ((long)threadIdx.x < head) guard_take(grad[threadIdx.x], s, c);
    if (done + (long)threadIdx.x < n) guard_take(grad[done + threadIdx.x], s, c);      // (n - done <= 3)
  }
  unsigned long long cc = c;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    s += __shfl_down(s, off, kWave);
    cc += __shfl_down(cc, off, kWave);
  }
  __shared__ double wave_s[kThreads / kWave];
  __shared__ unsigned long long wave_c[kThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    wave_s[threadIdx.x / kWave] = s;
    wave_c[threadIdx.x / kWave] = cc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double bs = wave_s[0];
    unsigned long long bc = wave_c[0];
#pragma unroll
    for (int w = 1; w < kThreads / kWave; ++w) {
      bs += wave_s[w];
      bc += wave_c[w];
    }
    psum[blockIdx.x] = bs;
    pcnt[blockIdx.x] = bc;
  }
}

__global__ __launch_bounds__(kThreads) void grad_guard_finalize_kernel(const double *__restrict__ psum,
                                                                       const unsigned long long *__restrict__ pcnt, int nblk,
                                                                       const float *__restrict__ hyper, float clip_global_norm,
                                                                       int skip_nonfinite, double *__restrict__ state) {
  double sumsq;
  unsigned long long bad;
  if (!guard_sum_partials(psum, pcnt, nblk, sumsq, bad)) return;
  const double norm = sqrt(sumsq) * fabs((double)hyper[3]);
  double coef = 1.0;
  if (clip_global_norm > 0.f) {
    coef = (double)clip_global_norm / (norm + 1e-6);
    if (!(coef < 1.0)) coef = 1.0;       // (also a NaN norm -- a non-finite rescale_grad -- clips nothing)
  }
  const double skip = (skip_nonfinite && bad > 0) ? 1.0 : 0.0;
  state[0] = norm;
  state[1] = coef;
  state[2] = skip;
  state[3] = (double)bad;
  state[4] += 1.0;
  state[5] += skip;
  state[6] = skip != 0.0 ? state[6] + 1.0 : 0.0;
  state[7] = sumsq;
}

}  // namespace

SN_EXPORT int sn_grad_guard_limits(int32_t *h_out4) {
  SN_REQUIRE(h_out4, "sn_grad_guard_limits: null pointer");
  h_out4[0] = kThreads;
  h_out4[1] = kElems;
  h_out4[2] = kDefaultBlocks;
  h_out4[3] = kStateDoubles;
  return SN_OK;
}

SN_EXPORT size_t sn_grad_guard_workspace_bytes(long n, int max_blocks) {
  if (n < 0 || max_blocks < 0 || max_blocks > kMaxBlocks) return 0;
  return sn_align((size_t)guard_blocks(n, max_blocks) * (sizeof(double) + sizeof(unsigned long long)));
}

// the argument checks and the partial pass of sn_grad_guard and sn_grad_guard_scaled (loss_scale.hip): the same kernel, grid, workspace
int sn_grad_guard_partials(const char *who, const float *d_grad, long n, const float *d_hyper, float clip_global_norm, int max_blocks,
                           void *d_ws, double *d_state, int *nblk_out, hipStream_t s) {
  SN_REQUIRE(d_grad && d_hyper && d_ws && d_state, "%s: null pointer", who);
  SN_REQUIRE(n >= 0, "%s: n = %ld", who, n);
  SN_REQUIRE(clip_global_norm >= 0.f, "%s: clip_global_norm must be >= 0 (0 = off) and not NaN", who);
  SN_REQUIRE(max_blocks >= 0 && max_blocks <= kMaxBlocks, "%s: max_blocks = %d outside 0 .. %d", who, max_blocks, kMaxBlocks);
  SN_REQUIRE(((uintptr_t)d_grad & 3) == 0 && ((uintptr_t)d_ws & 7) == 0 && ((uintptr_t)d_state & 7) == 0,
             "%s: d_grad must be 4-byte aligned, d_ws and d_state 8-byte aligned", who);
  const int nblk = guard_blocks(n, max_blocks);
  long head = (long)(((16 - ((uintptr_t)d_grad & 15)) & 15) / 4);
  if (head > n) head = n;
  const long n4 = (n - head) / 4;
  double *psum = (double *)d_ws;
  unsigned long long *pcnt = (unsigned long long *)(psum + nblk);
  hipLaunchKernelGGL(grad_guard_partial_kernel, dim3(nblk), dim3(kThreads), 0, s, d_grad, n, head, n4, psum, pcnt);
  SN_CHECK_LAUNCH();
  *nblk_out = nblk;
  return SN_OK;
}

SN_EXPORT int sn_grad_guard(const float *d_grad, long n, const float *d_hyper, float clip_global_norm, int skip_nonfinite,
                            int max_blocks, void *d_ws, double *d_state, sn_stream_t stream) {
  int nblk = 0;
  const int rc = sn_grad_guard_partials("sn_grad_guard", d_grad, n, d_hyper, clip_global_norm, max_blocks, d_ws, d_state, &nblk,
                                        sn_stream(stream));
  if (rc != SN_OK) return rc;
  double *psum = (double *)d_ws;
  unsigned long long *pcnt = (unsigned long long *)(psum + nblk);
  hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(kThreads), 0, sn_stream(stream), (const double *)psum,
                     (const unsigned long long *)pcnt, nblk, d_hyper, clip_global_norm, skip_nonfinite ? 1 : 0, d_state);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
