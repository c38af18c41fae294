// grad_guard.h -- what the gradient guard (grad_guard.hip) and the guard behind the dynamic loss scale (loss_scale.hip) share: the
// geometry of the partial pass, the pass itself behind one host function, and the finalize block's sum of the partials.
// Internal, not part of the C ABI.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;                 // threads per block
constexpr int kVec = 4;                       // 16-byte loads per lane per trip
constexpr int kElems = 4 * kVec;              // floats per thread per trip
constexpr int kSpan = kThreads * kElems;      // floats per block per trip
constexpr int kDefaultBlocks = 1024;          // the library's grid cap (max_blocks = 0)
constexpr int kMaxBlocks = 65535;
constexpr int kStateDoubles = 8;
constexpr int kChunk = 1024;                  // partials per round of the finalize block

inline int guard_blocks(long n, int max_blocks) {
  const long cap = max_blocks > 0 ? max_blocks : kDefaultBlocks;
  const long b = (n + kSpan - 1) / kSpan;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// The finalize block (kThreads threads, all of them call): the partials added in index order.  True for thread 0 alone, which holds
// both totals; the other threads are done.
__device__ __forceinline__ bool guard_sum_partials(const double *__restrict__ psum, const unsigned long long *__restrict__ pcnt, int nblk,
                                                   double &sumsq_out, unsigned long long &bad_out) {
  __shared__ double ls[kChunk];
  __shared__ unsigned long long lc[kChunk];
  __shared__ unsigned long long bad_total;
  double sumsq = 0.0;
  unsigned long long bad = 0;
  for (int b0 = 0; b0 < nblk; b0 += kChunk) {
    const int m = nblk - b0 < kChunk ? nblk - b0 : kChunk;
    for (int i = threadIdx.x; i < kChunk; i += kThreads) {      // (zeros behind the last partial: a round is whole groups of eight)
      ls[i] = i < m ? psum[b0 + i] : 0.0;
      lc[i] = i < m ? pcnt[b0 + i] : 0ull;
    }
    __syncthreads();
    // one lane adds the sums in index order, the first lane of the next wave the counts beside it; eight LDS reads are issued
    // before the eight dependent additions (one read, one wait, one addition at a time was most of this launch)
    if (threadIdx.x == 0) {
      for (int i = 0; i < m; i += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ls[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) sumsq += v[j];
      }
    } else if (threadIdx.x == kWave) {
      for (int i = 0; i < m; i += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = lc[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) bad += v[j];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == kWave) bad_total = bad;
  __syncthreads();
  if (threadIdx.x != 0) return false;
  sumsq_out = sumsq;
  bad_out = bad_total;
  return true;
}

}  // namespace

// grad_guard.hip: the argument checks of sn_grad_guard (messages under the caller's name `who`) and the partial pass -- one partial
// sum and one non-finite count per block into d_ws; *nblk_out = the grid, i.e. the number of partials.
int sn_grad_guard_partials(const char *who, const float *d_grad, long n, const float *d_hyper, float clip_global_norm, int max_blocks,
                           void *d_ws, double *d_state, int *nblk_out, hipStream_t s);
