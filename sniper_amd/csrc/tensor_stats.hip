// tensor_stats.hip -- per-tensor statistics of a flat arena (gradients, masters, momentum, fp16 copies): ONE read of the arena gives,
// for every tensor of a segment table, the sum of squares and the sum of its finite elements, the number and the first index of its
// non-finite ones, the largest finite magnitude and the number of zeros (include/sniper_hip.h: the record layout).
//
// Balance: the tensors of a detector run from 4 elements to 14 M, so the work is the plan's items (tensor_stats_plan.cpp): chunks of
// kChunk elements of ONE tensor, a shorter tensor being one item.  The pass is a pure read stream shaped like the gradient guard's:
// 256-thread blocks, four 16-byte loads in flight per lane per trip; a block takes items blockIdx.x, + gridDim.x, ... and reduces each
// to one partial record in the workspace -- fp64 per thread, then wave shuffles, then LDS.  An item is reduced by one block in a fixed
// order, so the grid (max_blocks) changes which block computes a partial and never its bits.  The second launch gives every tensor one
// wave that adds the tensor's partials IN CHUNK ORDER (min / max / integer sums for the exact fields) and one more block that writes
// the header from a bit per tensor in LDS.  No floating-point atomics anywhere; "last block finalizes" was not retried (grad_guard.hip).
//
// only_if_skipped: every block of both launches reads the guard's skip flag before its first load and returns when it is 0; nothing
// is written then.  That is the form that rides in the captured optimizer graph on every step.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "tensor_stats.h"

using namespace tstats;

namespace {

struct Acc {
  double sumsq, sum;
  unsigned bad, zeros;
  unsigned maxbits;       // the bits of max |x|: non-negative floats order as their bits do
  int first;              // index inside the ITEM of the first non-finite element, kNone if none
};
constexpr int kNone = INT_MAX;

// finite <=> fabsf(x) <= FLT_MAX (the guard's rule) <=> the bits of |x| are at most those of FLT_MAX.  A non-finite element is counted
// and adds 0.0 (exact) to both sums.  All of it in vector integer arithmetic: 8 elements x 4 loads of compare masks did not fit the
// scalar registers.
__device__ __forceinline__ void take(float x, Acc &a) {
  const unsigned u = __float_as_uint(x);
  const unsigned bits = u & 0x7fffffffu;
  const unsigned nb = (0x7f7fffffu - bits) >> 31;       // 1 iff non-finite (bits <= 0x7fffffff: the difference is negative iff bits is larger)
  const unsigned mask = nb - 1u;                        // finite: all ones
  const double d = (double)__uint_as_float(u & mask);
  a.sumsq += d * d;
  a.sum += d;
  a.bad += nb;
  a.zeros += (bits - 1u) >> 31;                         // 1 iff bits == 0: +0.0 or -0.0
  const unsigned mb = bits & mask;
  a.maxbits = mb > a.maxbits ? mb : a.maxbits;
}

template <typename E> struct Vec;
template <> struct Vec<float> {
  typedef floatx4 type;
  static constexpr int N = 4;
};
template <> struct Vec<half_t> {
  typedef half8 type;
  static constexpr int N = 8;
};

// one 16-byte vector, vector `vi` of the item's body; fv: the first vector of this thread that counted a non-finite element
template <typename E>
__device__ __forceinline__ void take_vec(const typename Vec<E>::type v, unsigned vi, unsigned &fv, Acc &a) {
  const unsigned before = a.bad;
#pragma unroll
  for (int e = 0; e < Vec<E>::N; ++e) take((float)v[e], a);
  const unsigned cand = a.bad != before ? vi : 0xffffffffu;
  fv = cand < fv ? cand : fv;
}

template <typename E>
__device__ __forceinline__ void take_one(E x, int idx, Acc &a) {
  const unsigned before = a.bad;
  take((float)x, a);
  if (a.bad != before && idx < a.first) a.first = idx;
}

template <typename E>
__global__ __launch_bounds__(kThreads) void tensor_stats_pass_kernel(const E *__restrict__ x, const Item *__restrict__ items, int n_items,
                                                                     const double *__restrict__ guard_state, int only_if_skipped,
                                                                     double *__restrict__ ws) {
  typedef typename Vec<E>::type V;
  constexpr int VE = Vec<E>::N;
  if (only_if_skipped && guard_state[2] == 0.0) return;
  __shared__ double l_sumsq[kThreads / kWave], l_sum[kThreads / kWave];
  __shared__ unsigned l_bad[kThreads / kWave], l_zeros[kThreads / kWave], l_max[kThreads / kWave];
  __shared__ int l_first[kThreads / kWave];
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const Item it = items[item];
    const E *__restrict__ p = x + it.off;
    const int len = it.len;                            // (<= kChunk: indices inside an item are ints)
    // p[0, head): in front of the first 16-byte boundary; body = nv vectors from there; tail = what is left (< VE)
    int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(E));
    if (head > len) head = len;
    const int nv = (len - head) / VE;
    const int done = head + nv * VE;
    const V *__restrict__ body = reinterpret_cast<const V *>(p + head);
    Acc a = {0.0, 0.0, 0u, 0u, 0u, kNone};
    unsigned fv = 0xffffffffu;
    for (int t0 = 0; t0 < nv; t0 += kThreads * kVec) {
      if (t0 + kThreads * kVec <= nv) {
        V v[kVec];
#pragma unroll
        for (int j = 0; j < kVec; ++j) v[j] = body[t0 + j * kThreads + tid];
#pragma unroll
        for (int j = 0; j < kVec; ++j) take_vec<E>(v[j], (unsigned)(t0 + j * kThreads + tid), fv, a);
      } else {
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
          const int i = t0 + j * kThreads + tid;
          if (i < nv) take_vec<E>(body[i], (unsigned)i, fv, a);
        }
      }
    }
    if (fv != 0xffffffffu) {                           // rare: read that vector again and find the element
      const V v = body[fv];
      int e = VE;
#pragma unroll
      for (int k = VE - 1; k >= 0; --k) e = fabsf((float)v[k]) <= FLT_MAX ? e : k;
      a.first = head + (int)fv * VE + e;
    }
    if (tid < head) take_one<E>(p[tid], tid, a);
    if (done + tid < len) take_one<E>(p[done + tid], done + tid, a);       // (len - done < VE)
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      a.sumsq += __shfl_down(a.sumsq, off, kWave);
      a.sum += __shfl_down(a.sum, off, kWave);
      a.bad += __shfl_down(a.bad, off, kWave);
      a.zeros += __shfl_down(a.zeros, off, kWave);
      const unsigned mb = __shfl_down(a.maxbits, off, kWave);
      a.maxbits = mb > a.maxbits ? mb : a.maxbits;
      const int f = __shfl_down(a.first, off, kWave);
      a.first = f < a.first ? f : a.first;
    }
    if ((tid & (kWave - 1)) == 0) {
      const int w = tid / kWave;
      l_sumsq[w] = a.sumsq;
      l_sum[w] = a.sum;
      l_bad[w] = a.bad;
      l_zeros[w] = a.zeros;
      l_max[w] = a.maxbits;
      l_first[w] = a.first;
    }
    __syncthreads();
    if (tid == 0) {
      double s2 = l_sumsq[0], s1 = l_sum[0];
      unsigned long long bad = l_bad[0], zeros = l_zeros[0];
      unsigned mx = l_max[0];
      int first = l_first[0];
#pragma unroll
      for (int w = 1; w < kThreads / kWave; ++w) {
        s2 += l_sumsq[w];
        s1 += l_sum[w];
        bad += l_bad[w];
        zeros += l_zeros[w];
        mx = l_max[w] > mx ? l_max[w] : mx;
        first = l_first[w] < first ? l_first[w] : first;
      }
      double *out = ws + (long long)item * kRecord;
      out[P_SUMSQ] = s2;
      out[P_SUM] = s1;
      reinterpret_cast<unsigned long long *>(out)[P_BAD] = bad;
      reinterpret_cast<long long *>(out)[P_FIRST] = first == kNone ? kNoIndex : it.toff + first;
      out[P_MAXABS] = (double)__uint_as_float(mx);
      reinterpret_cast<unsigned long long *>(out)[P_ZEROS] = zeros;
    }
    __syncthreads();       // (the LDS words are the next item's)
  }
}

// blocks 0 .. gridDim.x - 2: one wave per tensor; the last block: the header
__global__ __launch_bounds__(kThreads) void tensor_stats_finalize_kernel(const Item *__restrict__ items, const Tensor *__restrict__ tensors,
                                                                         int n_items, int T, const double *__restrict__ guard_state,
                                                                         int only_if_skipped, const double *__restrict__ ws,
                                                                         double *__restrict__ out) {
  if (only_if_skipped && guard_state[2] == 0.0) return;
  const int tid = threadIdx.x;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ unsigned bits[kMaxTensors / 32];
    __shared__ int l_cnt[kThreads / kWave], l_min[kThreads / kWave];
    const int words = (T + 31) / 32;
    for (int i = tid; i < words; i += kThreads) bits[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n_items; i += kThreads)
      if (reinterpret_cast<const unsigned long long *>(ws)[(long long)i * kRecord + P_BAD] != 0ull) {
        const int t = items[i].tensor;
        atomicOr(&bits[t >> 5], 1u << (t & 31));        // (an integer OR: any order, the same word)
      }
    __syncthreads();
    int cnt = 0, first = INT_MAX;
    for (int i = tid; i < words; i += kThreads) {
      const unsigned b = bits[i];
      if (b != 0u) {
        cnt += __popc(b);
        const int f = i * 32 + (__ffs((int)b) - 1);
        first = f < first ? f : first;
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      cnt += __shfl_down(cnt, off, kWave);
      const int f = __shfl_down(first, off, kWave);
      first = f < first ? f : first;
    }
    if ((tid & (kWave - 1)) == 0) {
      l_cnt[tid / kWave] = cnt;
      l_min[tid / kWave] = first;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kThreads / kWave; ++w) {
        cnt += l_cnt[w];
        first = l_min[w] < first ? l_min[w] : first;
      }
      out[0] = 1.0;
      out[1] = guard_state ? guard_state[4] : 0.0;
      out[2] = (double)T;
      out[3] = (double)cnt;
      out[4] = cnt > 0 ? (double)first : -1.0;
      out[5] = out[6] = out[7] = 0.0;
    }
    return;
  }
  const int lane = tid & (kWave - 1);
  const int t = blockIdx.x * (kThreads / kWave) + tid / kWave;
  if (t >= T) return;
  const Tensor tn = tensors[t];
  double s2 = 0.0, s1 = 0.0, mx = 0.0;
  unsigned long long bad = 0ull, zeros = 0ull;
  long long first = kNoIndex;
  for (int r0 = 0; r0 < tn.count; r0 += kWave) {
    const int m = tn.count - r0 < kWave ? tn.count - r0 : kWave;
    double v2 = 0.0, v1 = 0.0;
    if (lane < m) {
      const double *rec = ws + (long long)(tn.first + r0 + lane) * kRecord;
      v2 = rec[P_SUMSQ];
      v1 = rec[P_SUM];
      bad += reinterpret_cast<const unsigned long long *>(rec)[P_BAD];
      zeros += reinterpret_cast<const unsigned long long *>(rec)[P_ZEROS];
      const long long f = reinterpret_cast<const long long *>(rec)[P_FIRST];
      first = f < first ? f : first;
      mx = fmax(mx, rec[P_MAXABS]);
    }
    for (int j = 0; j < m; ++j) {        // in chunk order, every lane the same sums
      s2 += __shfl(v2, j, kWave);
      s1 += __shfl(v1, j, kWave);
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    bad += __shfl_down(bad, off, kWave);
    zeros += __shfl_down(zeros, off, kWave);
    const long long f = __shfl_down(first, off, kWave);
    first = f < first ? f : first;
    mx = fmax(mx, __shfl_down(mx, off, kWave));
  }
  if (lane == 0) {
    double *rec = out + (long long)(1 + t) * kRecord;
    rec[0] = s2;
    rec[1] = s1;
    rec[2] = (double)bad;
    rec[3] = first == kNoIndex ? -1.0 : (double)first;
    rec[4] = mx;
    rec[5] = (double)zeros;
    rec[6] = (double)tn.n;
    rec[7] = 0.0;
  }
}

}  // namespace

SN_EXPORT int sn_tensor_stats(const void *d_x, int dtype, const void *d_plan, int n_items, int T, int max_blocks,
                              const double *d_guard_state, int only_if_skipped, void *d_ws, double *d_out, sn_stream_t stream) {
  SN_REQUIRE(d_x && d_plan && d_ws && d_out, "sn_tensor_stats: null pointer");
  SN_REQUIRE(dtype == 0 || dtype == 1, "sn_tensor_stats: dtype = %d (0 = fp16, 1 = fp32)", dtype);
  SN_REQUIRE(T >= 0 && T <= kMaxTensors, "sn_tensor_stats: T = %d outside 0 .. %d", T, kMaxTensors);
  SN_REQUIRE(n_items >= 0, "sn_tensor_stats: n_items = %d", n_items);
  SN_REQUIRE(max_blocks >= 0 && max_blocks <= kMaxBlocks, "sn_tensor_stats: max_blocks = %d outside 0 .. %d", max_blocks, kMaxBlocks);
  SN_REQUIRE(!only_if_skipped || d_guard_state, "sn_tensor_stats: only_if_skipped needs d_guard_state");
  SN_REQUIRE(((uintptr_t)d_x & (dtype == 1 ? 3 : 1)) == 0, "sn_tensor_stats: d_x must be aligned to its element size");
  SN_REQUIRE(((uintptr_t)d_plan & 7) == 0 && ((uintptr_t)d_ws & 7) == 0 && ((uintptr_t)d_out & 7) == 0 && ((uintptr_t)d_guard_state & 7) == 0,
             "sn_tensor_stats: d_plan, d_ws, d_out and d_guard_state must be 8-byte aligned");
  hipStream_t s = sn_stream(stream);
  const Item *items = (const Item *)d_plan;
  const Tensor *tensors = (const Tensor *)(items + n_items);
  const int skip_only = only_if_skipped ? 1 : 0;
  if (n_items > 0) {
    const int cap = max_blocks > 0 ? max_blocks : kDefaultBlocks;
    const int grid = n_items < cap ? n_items : cap;
    if (dtype == 1)
      hipLaunchKernelGGL(tensor_stats_pass_kernel<float>, dim3(grid), dim3(kThreads), 0, s, (const float *)d_x, items, n_items, d_guard_state,
                         skip_only, (double *)d_ws);
    else
      hipLaunchKernelGGL(tensor_stats_pass_kernel<half_t>, dim3(grid), dim3(kThreads), 0, s, (const half_t *)d_x, items, n_items,
                         d_guard_state, skip_only, (double *)d_ws);
    SN_CHECK_LAUNCH();
  }
  const int grid2 = (T + kThreads / kWave - 1) / (kThreads / kWave) + 1;
  hipLaunchKernelGGL(tensor_stats_finalize_kernel, dim3(grid2), dim3(kThreads), 0, s, items, tensors, n_items, T, d_guard_state, skip_only,
                     (const double *)d_ws, d_out);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
