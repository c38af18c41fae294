// mask_infer.hip -- the mask head's output stage at test time.  Every RoI has ONE class there, so of the
// 2K maps of mask_out only two are read: the class's negative map c and its positive map c + K.  The stock chain computes all 2K
// channels (1x1 convolution), rounds them to fp16, picks twice, concatenates and runs a 2-way softmax: five launches and an
// (N, HW, 2K) tensor nobody keeps.  Here one launch reads x once and writes the foreground probability:
//
//   neg = clip((int)cls[n], 0, 2K-1),  pos = clip((int)cls[n] + K, 0, 2K-1)          (sn_pick_fwd's clipping on 2K channels)
//   z_neg = sum_k x[n,p,k] * w[neg,k] + bias[neg],  z_pos likewise                   (fp16 operands, fp32 accumulation)
//   prob[n,p] = softmax(z_neg, z_pos)[1]                                             (sn_softmax_fwd's statements for a K = 2 row)
//
// The logits are NOT rounded to fp16 on the way: the one numerical difference from the stock chain.
#include "common.h"

// Shape of the work: per RoI a (HW x C) by (C x 2) product -- two columns, far too thin for the matrix cores; the kernel streams x
// (512 B per pixel at C = 256) and is bound by reading it.
//   * A lane owns 8 consecutive channels (one 16-byte load), the 32 lanes of a wave half own one 256-channel pass of a pixel, the two
//     halves two consecutive pixels: one load instruction of a wave covers 2 * 512 contiguous bytes at C = 256.  C > 256 is a loop
//     over passes, C < 256 leaves the upper lanes of a half without work (their operands read as zero).
//   * A wave owns a tile of kPairs pixel pairs = 16 consecutive pixels: kPairs independent loads in flight, then 8 mixed-precision
//     FMAs per loaded chunk and weight row (the product of two fp16 values is exact in fp32, the accumulation rounds once per FMA;
//     the packed fp16 dot-product instruction is not used: it flushes subnormals, and the head's ReLU output does hold them).
//   * The kPairs x 2 partial sums of a lane meet across the 32 lanes of the half in a reduce-scatter: at the xor-16 / 8 / 4 steps a
//     lane passes on the half of its values its partner keeps, so 7 exchanges instead of 8 x 3, then xor-2 / xor-1 on the one value
//     left.  Lane l ends up with pixel pair (l >> 2) & 7 of its half: 16 lanes store 16 consecutive floats, one 64-byte run per wave.
//   * The two weight rows of the RoI (8 channels each per lane and pass) stay in registers over the tile.
// No LDS, no atomics, no workspace; every sum has one fixed order, so the same bits every run.
constexpr int kMaskPairs = 8;                     // pixel pairs per wave tile
constexpr int kMaskTile = 2 * kMaskPairs;         // pixels per wave
constexpr int kMaskBlockPix = 4 * kMaskTile;      // pixels per 256-thread workgroup
constexpr int kMaskPass = 32 * 8;                 // channels per pass

// one reduce-scatter step: NV values per lane -> NV / 2, each now the sum over the lane pair (l, l ^ OFF)
template <int OFF, int NV>
__device__ __forceinline__ void mask_scatter_step(float (&v)[kMaskPairs], bool hi) {
#pragma unroll
  for (int j = 0; j < NV / 2; ++j) {
    const float keep = hi ? v[j + NV / 2] : v[j];
    const float send = hi ? v[j] : v[j + NV / 2];
    v[j] = keep + __shfl_xor(send, OFF, 64);
  }
}

// v[j] of the 32 lanes of a wave half -> the full sum of pixel pair (lane >> 2) & 7, in every lane of that quad
__device__ __forceinline__ float mask_reduce_pairs(float (&v)[kMaskPairs], int lane) {
  static_assert(kMaskPairs == 8, "the reduce-scatter below is written for 8 values per lane");
  mask_scatter_step<16, 8>(v, (lane & 16) != 0);
  mask_scatter_step<8, 4>(v, (lane & 8) != 0);
  mask_scatter_step<4, 2>(v, (lane & 4) != 0);
  float s = v[0];
  s = s + __shfl_xor(s, 2, 64);
  s = s + __shfl_xor(s, 1, 64);
  return s;
}

__global__ __launch_bounds__(256) void mask_class_prob_kernel(const half_t *__restrict__ x, const half_t *__restrict__ w,
                                                              const float *__restrict__ bias, const float *__restrict__ cls,
                                                              float *__restrict__ prob, int HW, int C, int K, SnDiv blocks_per_roi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & 31, half = lane >> 5;
  unsigned blk;
  const unsigned n = sn_divmod(blockIdx.x, blocks_per_roi, blk);
  const int pix0 = (int)blk * kMaskBlockPix + wave * kMaskTile;       // first pixel of this wave's tile
  if (pix0 >= HW) return;                                              // (no barrier below: a whole wave may leave)
  const int c = (int)cls[n], top = 2 * K - 1;
  const int neg = c < 0 ? 0 : (c > top ? top : c);
  const int pos = c > top ? top : (c + K < 0 ? 0 : (c + K > top ? top : c + K));      // (c + K only where it cannot overflow)
  const half_t *wn = w + (size_t)neg * C, *wp = w + (size_t)pos * C;
  const half_t *xr = x + (size_t)n * HW * C;
  const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  float an[kMaskPairs], ap[kMaskPairs];
#pragma unroll
  for (int j = 0; j < kMaskPairs; ++j) an[j] = ap[j] = 0.f;
  for (int c0 = 0; c0 < C; c0 += kMaskPass) {
    // a lane past the last channel loads from channel 0 (a valid address) and takes zeros: the select is on the VALUE, the loads
    // themselves stay unconditional and all in flight together
    const int ch = c0 + sub * 8;
    const bool live = ch < C;
    const int cc = live ? ch : 0;
    half8 xv[kMaskPairs];
#pragma unroll
    for (int j = 0; j < kMaskPairs; ++j) {
      int p = pix0 + 2 * j + half;
      p = p < HW ? p : HW - 1;                                         // tail pixels re-read the last one; their result is not stored
      xv[j] = *reinterpret_cast<const half8 *>(xr + (size_t)p * C + cc);
    }
    half8 a = *reinterpret_cast<const half8 *>(wn + cc), b = *reinterpret_cast<const half8 *>(wp + cc);
    a = live ? a : zero8;
    b = live ? b : zero8;
#pragma unroll
    for (int j = 0; j < kMaskPairs; ++j) {
      const half8 v = live ? xv[j] : zero8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        an[j] = __builtin_fmaf((float)v[e], (float)a[e], an[j]);
        ap[j] = __builtin_fmaf((float)v[e], (float)b[e], ap[j]);
      }
    }
  }
  float zn = mask_reduce_pairs(an, lane), zp = mask_reduce_pairs(ap, lane);
  if (bias) {
    zn = zn + bias[neg];
    zp = zp + bias[pos];
  }
  // softmax_fwd_kernel's statements (nn_ops.hip) for the row (zn, zp), channel 1
  const float m = fmaxf(zn, zp);
  float z = 0.f;
  z += expf(zn - m);
  z += expf(zp - m);
  const float iz = 1.f / z;
  const float p1 = expf(zp - m) * iz;
  const int pix = pix0 + 2 * ((lane >> 2) & 7) + half;
  if ((lane & 3) == 0 && pix < HW) prob[(size_t)n * HW + pix] = p1;
}

SN_EXPORT int sn_mask_class_prob(const void *x, const void *w16, const float *bias, const float *cls, float *prob, int N, int HW, int C,
                                 int K, sn_stream_t stream) {
  SN_REQUIRE(x && w16 && cls && prob, "sn_mask_class_prob: null pointer (x, w16, cls and prob are required)");
  SN_REQUIRE(N >= 1 && HW >= 1 && C >= 1 && K >= 1, "sn_mask_class_prob: N, HW, C and K must be at least 1 (got %d, %d, %d, %d)", N, HW,
             C, K);
  SN_REQUIRE(C % 8 == 0, "sn_mask_class_prob: C = %d is not a multiple of 8 (16-byte channel runs)", C);
  SN_REQUIRE((long)N * HW * C < (1l << 31), "sn_mask_class_prob: N * HW * C = %ld is past 32-bit indexing", (long)N * HW * C);
  SN_REQUIRE(K < (1 << 29), "sn_mask_class_prob: K = %d is too large", K);
  SN_REQUIRE((((uintptr_t)x | (uintptr_t)w16) & 15) == 0, "sn_mask_class_prob: x and w16 must be 16-byte aligned");
  const int bpr = sn_div_up(HW, kMaskBlockPix);
  hipLaunchKernelGGL(mask_class_prob_kernel, dim3((unsigned)N * (unsigned)bpr), dim3(256), 0, sn_stream(stream), (const half_t *)x,
                     (const half_t *)w16, bias, cls, prob, HW, C, K, sn_div_make((unsigned)bpr));
  SN_CHECK_LAUNCH();
  return SN_OK;
}
