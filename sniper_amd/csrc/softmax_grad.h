// softmax_grad.h -- the SoftmaxOutput gradient, one copy for the kernels that take the multiplier as a launch argument (nn_ops.hip)
// and the ones that read the loss scale from device memory (loss_scale.hip): the per-element statements, the row-block geometry and
// the choice between the two paths.  Internal, not part of the C ABI.
#pragma once
#include <algorithm>

#include "common.h"

// ---- inner == 1 (the R-CNN classifier: 6000 rows of 81): a workgroup owns a block of R consecutive rows, i.e. one contiguous range
// of memory.  R is a multiple of 4 (every block starts 16-byte aligned) and at most 64 (6000 rows -> 94 workgroups).
constexpr int kSoftmaxRowsMax = 64, kSoftmaxLdsFloats = 16384;      // 64 KB of LDS at most
static inline int softmax_rows_per_block(int K) { return std::min(kSoftmaxRowsMax, kSoftmaxLdsFloats / (K | 1)) & ~3; }
// the row path: contiguous rows, a block of at least 16 of them in LDS (K <= 1023), 16-byte aligned tensors
static inline bool softmax_rows_ok(const void *a, const void *b, int K, long inner) {
  return inner == 1 && softmax_rows_per_block(K) >= 16 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0 &&
         sn_debug_get(SN_OPT_SOFTMAX_STRIDED) == 0;
}
static inline int softmax_strided_blocks(long total) { return sn_blocks(total, 8192); }

// valid-label counter of normalization='valid': memset of ws[0], then the counting launch (nn_ops.hip)
int sn_softmax_count_valid(const float *label, long n, float ignore_label, int use_ignore, int *ws, hipStream_t s);

// grad_scale, or grad_scale / max(valid, 1)
__device__ __forceinline__ float softmax_grad_mul(float grad_scale, int normalize_valid, const int *__restrict__ valid_count) {
  float mul = grad_scale;
  if (normalize_valid) {
    const int vc = *valid_count;
    mul = grad_scale / (float)(vc > 1 ? vc : 1);
  }
  return mul;
}

// one thread per (outer, inner) position, K strided writes
__device__ __forceinline__ void softmax_bwd_strided(const float *__restrict__ p, const float *__restrict__ label, float *__restrict__ g,
                                                    long outer, int K, long inner, float ignore, int use_ignore, float mul) {
  const long total = outer * inner;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long o = i / inner, s = i - o * inner;
    const float l = label[i];
    const bool ign = use_ignore && l == ignore;
    const int li = (int)l;
    for (int k = 0; k < K; ++k) {
      const long idx = o * K * inner + (long)k * inner + s;
      g[idx] = ign ? 0.f : mul * (p[idx] - (k == li ? 1.f : 0.f));
    }
  }
}

// the gradient is elementwise given p, the row's label and the count: row blocks of R rows, 16 bytes per lane, no LDS
__device__ __forceinline__ void softmax_bwd_rows(const float *__restrict__ p, const float *__restrict__ label, float *__restrict__ g,
                                                 long outer, int K, int R, SnDiv dK, float ignore, int use_ignore, float mul) {
  const long row0 = (long)blockIdx.x * R;
  const int nr = (int)(outer - row0 < R ? outer - row0 : R);
  const int n = nr * K, n4 = n >> 2;
  const float *pb = p + row0 * K, *lb = label + row0;
  float *gb = g + row0 * K;
  auto one = [&](float pv, unsigned r, unsigned k) {
    const float l = lb[r];
    const bool ign = use_ignore && l == ignore;
    const int li = (int)l;
    return ign ? 0.f : mul * (pv - ((int)k == li ? 1.f : 0.f));
  };
  for (int v = threadIdx.x; v < n4; v += 256) {
    const float4 f = reinterpret_cast<const float4 *>(pb)[v];
    float e[4] = {f.x, f.y, f.z, f.w};
    unsigned k, r = sn_divmod(4u * v, dK, k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j] = one(e[j], r, k);
      if (++k == (unsigned)K) { k = 0; ++r; }
    }
    reinterpret_cast<float4 *>(gb)[v] = make_float4(e[0], e[1], e[2], e[3]);
  }
  for (int i = 4 * n4 + threadIdx.x; i < n; i += 256) {
    unsigned k, r = sn_divmod((unsigned)i, dK, k);
    gb[i] = one(pb[i], r, k);
  }
}
