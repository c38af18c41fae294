// eval_order.h -- what the box evaluators (coco_eval.hip, voc_eval.hip) share: the per-category ordering of detections by
// (descending score, position) and the wave scans of their curve kernels.  Internal, not part of the C ABI.  float64 compares and
// integer adds only: nothing here depends on the fp-contract setting of the including file.
#pragma once
#include "common.h"

constexpr int kEvalSortTile = 256;      // detections per workgroup of the ordering launch (= its block size)
constexpr int kEvalScanChunk = 256;     // detections per chunk of the scans (= the block size of the curve kernels)

// One workgroup of kEvalSortTile threads, tile blockIdx.x of a category whose N scores lie at score[c0 .. c0 + N): thread i counts
// the category's detections that precede its own by (descending score, position in the concatenation) -- the total order a stable
// mergesort of -score yields -- tile by tile through LDS, and writes base + its position at order[c0 + its rank].  A workgroup whose
// tile lies past N leaves whole, so no barrier is skipped by a part of it.  Call it from uniform control flow, as the last thing a
// kernel does.
__device__ __forceinline__ void sn_eval_order_tile(int c0, int N, const double *__restrict__ score, int32_t *__restrict__ order, int base,
                                                   double *s_tile /* kEvalSortTile doubles of LDS */) {
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kEvalSortTile + tid;
  if (blockIdx.x * kEvalSortTile >= N) return;
  const double si = i < N ? score[c0 + i] : 0.;
  int before = 0;
  for (int b = 0; b < N; b += kEvalSortTile) {
    __syncthreads();
    if (b + tid < N) s_tile[tid] = score[c0 + b + tid];
    __syncthreads();
    const int n = N - b < kEvalSortTile ? N - b : kEvalSortTile;
    for (int j = 0; j < n; ++j) {
      const double sj = s_tile[j];
      before += (sj > si) | ((sj == si) & (b + j < i));
    }
  }
  if (i < N) order[c0 + before] = base + i;
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int wave_scan_add(int v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}
// inclusive running max from the last lane of a wave down to this one
__device__ __forceinline__ double wave_scan_max_rev(double v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double o = __shfl_down(v, off, 64);
    if (lane + off < kWave) v = fmax(v, o);
  }
  return v;
}
