// gconv.hip -- grouped convolution (Convolution with 1 < num_group < channels: the ResNeXt 3x3, num_group = 64), channels-last
// fp16 with a pixel pitch, fp32 accumulation.  Weights stay in the compact [O][KH*KW][Cg] fp16 layout (Cg = C / groups) for the
// forward pass AND the data gradient: no derived buffer, no transposed copy.
//
// Fast path (Cg == Og in {4, 8, 16, 32}, C % 32 == 0, 1x1 or 3x3): v_mfma_f32_16x16x32_f16 over 32-channel SLABS.  A slab is
// 32 / Cg neighbouring groups: 32 input channels -> the same 32 output channels, block diagonal.  A wave owns one slab for its whole
// life and keeps the slab's weights as MFMA A-operand fragments in registers (KH*KW taps x two 16-row blocks, off-diagonal zeros
// built in registers from the compact weights); the activations are the B operand, loaded straight from global memory: lane
// (pixel = lane & 15, quarter = lane >> 4) reads channels 8 * quarter .. + 7 of its pixel's tap -- one 16-byte load, no LDS, halos
// from L1 / L2.  The rows of the two blocks are interleaved (row r of block b = channel 8 * (r >> 2) + 4 * b + (r & 3)), so the
// accumulators of a lane are 8 CONSECUTIVE output channels of one pixel: one 16-byte store.  The data gradient is the same kernel
// with the slab's weights transposed in registers and the taps gathered per dx pixel on the stride lattice.
// The weight gradient contracts over pixels: dy and the tap-shifted x of 32 pixels go through a wave-private LDS image as they lie
// ([pixel][channel], 16-byte writes), are read back transposed (ds_read_b64_tr_b16), and every workgroup writes ONE partial per weight to its slab of the
// workspace; sn_partial_sum (common.hip) adds the slabs to dw in block order (no atomics: the same bits every run).
// Everything else (Cg != Og, other widths, other kernel sizes, fp32 output) takes the plain kernels at the end of the file.
#include "conv_common.h"
#include "gconv_slab.h"

struct GconvParams {
  int N, H, W, Ho, Wo;        // input and output extents of the CONVOLUTION (the data gradient reads Ho x Wo, writes H x W)
  int C, O, Cg, Og, groups;
  int KH, KW, stride, pad, dil;
  int cg_shift, s_shift;      // fast path: Cg and stride are powers of two
  int src_ps, dst_ps, acc_ps;
  int relu;
  long M;                     // pixels written: N * Ho * Wo (forward), N * H * W (data gradient)
  int ntiles;                 // 16-pixel tiles
};

// ---------------------------------------------------------------------------------------------------------------------------------
// forward / data gradient on the matrix cores
// ---------------------------------------------------------------------------------------------------------------------------------
template <int T, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_mfma_kernel(const half_t *__restrict__ src, const half_t *__restrict__ w,
                                                         const float *__restrict__ bias, const half_t *accp, half_t *dst,
                                                         const GconvParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int slab = blockIdx.y * (blockDim.x >> 6) + wave;
  const int ch0 = slab * 32;
  // the slab's weights as A-operand fragments: row -> written channel, k = 8q + j -> contracted channel
  half8 wa[T][2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int row_ch = 8 * (r >> 2) + 4 * b + (r & 3);
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k_ch = 8 * q + j;
        const int o = DGRAD ? k_ch : row_ch, ci = DGRAD ? row_ch : k_ch;
        half_t v = (half_t)0.f;
        if ((o >> p.cg_shift) == (ci >> p.cg_shift)) v = w[((size_t)(ch0 + o) * T + t) * p.Cg + (ci & (p.Cg - 1))];
        wa[t][b][j] = v;
      }
    }
  }
  const int PH = DGRAD ? p.H : p.Ho, PW = DGRAD ? p.W : p.Wo;      // extents of the written tensor
  const int SH = DGRAD ? p.Ho : p.H, SW = DGRAD ? p.Wo : p.W;      // extents of the read tensor
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int m = tile * 16 + r;                 // (M < 2^31: checked by the host)
    const bool live = m < (int)p.M;
    const int px = m % PW, t2 = m / PW;
    const int py = t2 % PH, n = t2 / PH;
    half8 xb[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      constexpr int KW = T == 9 ? 3 : 1;
      const int kh = t / KW, kw = t - kh * KW;
      int sy, sx;
      bool ok = live;
      if (DGRAD) {
        const int ty = py + p.pad - kh * p.dil, tx = px + p.pad - kw * p.dil;
        ok = ok && ty >= 0 && tx >= 0 && ((ty | tx) & (p.stride - 1)) == 0;      // on the stride lattice
        sy = ty >> p.s_shift;
        sx = tx >> p.s_shift;
        ok = ok && sy < SH && sx < SW;
      } else {
        sy = py * p.stride - p.pad + kh * p.dil;
        sx = px * p.stride - p.pad + kw * p.dil;
        ok = ok && (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW;
      }
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ok) v = *reinterpret_cast<const half8 *>(src + (((size_t)n * SH + sy) * SW + sx) * p.src_ps + ch0 + 8 * q);
      xb[t] = v;
    }
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], xb[t], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], xb[t], acc1, 0, 0, 0);
    }
    // lane: pixel r, channels ch0 + 8q + {0..3} (block 0) and + {4..7} (block 1)
    if (live) {
      float o[8] = {acc0[0], acc0[1], acc0[2], acc0[3], acc1[0], acc1[1], acc1[2], acc1[3]};
      if (!DGRAD && bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += bias[ch0 + 8 * q + j];
      }
      if (DGRAD && accp) {
        const half8 a = *reinterpret_cast<const half8 *>(accp + (size_t)m * p.acc_ps + ch0 + 8 * q);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += (float)a[j];
      }
      half8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = (half_t)((!DGRAD && p.relu) ? fmaxf(o[j], 0.f) : o[j]);
      *reinterpret_cast<half8 *>(dst + (size_t)m * p.dst_ps + ch0 + 8 * q) = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradient on the matrix cores: D[o][ci] += sum over 32 pixels dyT[o][pix] * xT[ci][pix] per tap
// ---------------------------------------------------------------------------------------------------------------------------------
// NB = 1: Cg <= 16, only the two diagonal 16 x 16 blocks of a slab hold weights;  NB = 2: Cg == 32, all four
template <int T, int NB>
__global__ __launch_bounds__(256) void gconv_wgrad_mfma_kernel(const half_t *__restrict__ dy, const half_t *__restrict__ x,
                                                               float *__restrict__ part, const GconvParams p, int chunks_per_block) {
  __shared__ __attribute__((aligned(16))) half_t lds[4][3][32 * kTP];      // per wave: dyT and two xT buffers
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int slab = blockIdx.y * (blockDim.x >> 6) + wave;
  const int ch0 = slab * 32;
  half_t *dyT = lds[wave][0];
  const int tr_off = (8 * q + (r >> 2)) * kTP + 4 * (r & 3);      // tr_frag: this lane's address of pixel row 8q + (r >> 2)
  floatx4 acc[T][2][NB];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int bo = 0; bo < 2; ++bo)
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[t][bo][i] = floatx4{0.f, 0.f, 0.f, 0.f};
  const long M = (long)p.N * p.Ho * p.Wo;
  const long c0 = (long)blockIdx.x * chunks_per_block;
  // loads: piece i of a lane = (pixel (lane >> 2) + 16 i of the chunk, channels 8 (lane & 3) .. + 7)
  const int lp = lane >> 2, lc = (lane & 3) * 8;
  for (int c = 0; c < chunks_per_block; ++c) {
    const long mbase = (c0 + c) * 32;            // (uniform over the block: every wave passes every barrier)
    int mm[2], oy[2], ox[2], nn[2];             // (M < 2^31 / 16: checked by the host; a chunk past the end loads nothing)
    bool live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long m = mbase + lp + 16 * i;
      live[i] = m < M;
      mm[i] = live[i] ? (int)m : 0;
      ox[i] = mm[i] % p.Wo;
      const int t2 = mm[i] / p.Wo;
      oy[i] = t2 % p.Ho;
      nn[i] = t2 / p.Ho;
    }
    // every global load of the chunk is issued before the first LDS write: one memory latency per chunk, not one per tap
    half8 gv[2], xv[T][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      gv[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live[i]) gv[i] = *reinterpret_cast<const half8 *>(dy + (size_t)mm[i] * p.src_ps + ch0 + lc);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      constexpr int KW = T == 9 ? 3 : 1;
      const int kh = t / KW, kw = t - kh * KW;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int sy = oy[i] * p.stride - p.pad + kh * p.dil, sx = ox[i] * p.stride - p.pad + kw * p.dil;
        xv[t][i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live[i] && (unsigned)sy < (unsigned)p.H && (unsigned)sx < (unsigned)p.W)
          xv[t][i] = *reinterpret_cast<const half8 *>(x + (((size_t)nn[i] * p.H + sy) * p.W + sx) * p.dst_ps + ch0 + lc);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<half8 *>(dyT + (lp + 16 * i) * kTP + lc) = gv[i];
    half8 fa[2];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      half_t *xT = lds[wave][1 + (t & 1)];
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<half8 *>(xT + (lp + 16 * i) * kTP + lc) = xv[t][i];
      __syncthreads();
      if (t == 0) {
#pragma unroll
        for (int bo = 0; bo < 2; ++bo) fa[bo] = tr_frag(dyT, tr_off + bo * 16, kTrSecond);
      }
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        const half8 fb = tr_frag(xT, tr_off + bi * 16, kTrSecond);
        if (NB == 2) {
#pragma unroll
          for (int bo = 0; bo < 2; ++bo) acc[t][bo][bi % NB] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[bo], fb, acc[t][bo][bi % NB], 0, 0, 0);
        } else {
          acc[t][bi][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[bi], fb, acc[t][bi][0], 0, 0, 0);
        }
      }
    }
    __syncthreads();          // the next chunk rewrites dyT and the first xT buffer
  }
  // lane holds D[row o = 4q + reg][col ci = r] of every block: one partial per weight of the slab, [block][O][T][Cg]
  float *po = part + (size_t)blockIdx.x * p.O * T * p.Cg;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int bo = 0; bo < 2; ++bo)
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int bi = NB == 2 ? i : bo;
        const int ci = bi * 16 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = bo * 16 + 4 * q + e;
          if (o / p.Cg == ci / p.Cg) po[((size_t)(ch0 + o) * T + t) * p.Cg + ci % p.Cg] = acc[t][bo][i][e];
        }
      }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plain kernels: any C % groups == 0, O % groups == 0, any kernel size.  One thread per written element.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gconv_plain_fwd_kernel(const half_t *__restrict__ x, const half_t *__restrict__ w,
                                                              const float *__restrict__ bias, void *__restrict__ y,
                                                              const GconvParams p, int out_f32) {
  const long total = p.M * p.O;
  const int T = p.KH * p.KW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int o = (int)(i % p.O);
    const long m = i / p.O;
    const int ox = (int)(m % p.Wo);
    const long t2 = m / p.Wo;
    const int oy = (int)(t2 % p.Ho), n = (int)(t2 / p.Ho);
    const int c0 = (o / p.Og) * p.Cg;
    float acc = bias ? bias[o] : 0.f;
    for (int kh = 0; kh < p.KH; ++kh) {
      const int sy = oy * p.stride - p.pad + kh * p.dil;
      if ((unsigned)sy >= (unsigned)p.H) continue;
      for (int kw = 0; kw < p.KW; ++kw) {
        const int sx = ox * p.stride - p.pad + kw * p.dil;
        if ((unsigned)sx >= (unsigned)p.W) continue;
        const half_t *xp = x + (((size_t)n * p.H + sy) * p.W + sx) * p.src_ps + c0;
        const half_t *wp = w + ((size_t)o * T + kh * p.KW + kw) * p.Cg;
        for (int c = 0; c < p.Cg; ++c) acc += (float)xp[c] * (float)wp[c];
      }
    }
    if (p.relu) acc = fmaxf(acc, 0.f);
    if (out_f32)
      ((float *)y)[(size_t)m * p.dst_ps + o] = acc;
    else
      ((half_t *)y)[(size_t)m * p.dst_ps + o] = (half_t)acc;
  }
}

__global__ __launch_bounds__(256) void gconv_plain_dgrad_kernel(const half_t *__restrict__ dy, const half_t *__restrict__ w,
                                                                const half_t *accp, half_t *dx, const GconvParams p) {
  const long total = p.M * p.C;
  const int T = p.KH * p.KW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % p.C);
    const long m = i / p.C;
    const int xx = (int)(m % p.W);
    const long t2 = m / p.W;
    const int yy = (int)(t2 % p.H), n = (int)(t2 / p.H);
    const int g = ci / p.Cg, cl = ci - g * p.Cg, o0 = g * p.Og;
    float acc = accp ? (float)accp[(size_t)m * p.acc_ps + ci] : 0.f;
    for (int kh = 0; kh < p.KH; ++kh) {
      const int ty = yy + p.pad - kh * p.dil;
      if (ty < 0 || ty % p.stride != 0 || ty / p.stride >= p.Ho) continue;
      for (int kw = 0; kw < p.KW; ++kw) {
        const int tx = xx + p.pad - kw * p.dil;
        if (tx < 0 || tx % p.stride != 0 || tx / p.stride >= p.Wo) continue;
        const half_t *gp = dy + (((size_t)n * p.Ho + ty / p.stride) * p.Wo + tx / p.stride) * p.src_ps + o0;
        const half_t *wp = w + ((size_t)o0 * T + kh * p.KW + kw) * p.Cg + cl;
        for (int o = 0; o < p.Og; ++o) acc += (float)gp[o] * (float)wp[(size_t)o * T * p.Cg];
      }
    }
    dx[(size_t)m * p.dst_ps + ci] = (half_t)acc;
  }
}

// one thread per (pixel block, weight element): a partial over the block's pixels in pixel order
__global__ __launch_bounds__(256) void gconv_plain_wgrad_kernel(const half_t *__restrict__ dy, const half_t *__restrict__ x,
                                                                float *__restrict__ part, const GconvParams p, int pix_per_block) {
  const int T = p.KH * p.KW;
  const long nw = (long)p.O * T * p.Cg;
  const long e = (long)blockIdx.y * 256 + threadIdx.x;
  if (e >= nw) return;
  const int cl = (int)(e % p.Cg);
  const long t1 = e / p.Cg;
  const int t = (int)(t1 % T), o = (int)(t1 / T);
  const int kh = t / p.KW, kw = t - kh * p.KW;
  const int ci = (o / p.Og) * p.Cg + cl;
  const long M = (long)p.N * p.Ho * p.Wo;
  const long m0 = (long)blockIdx.x * pix_per_block, m1 = m0 + pix_per_block < M ? m0 + pix_per_block : M;
  float acc = 0.f;
  for (long m = m0; m < m1; ++m) {
    const int ox = (int)(m % p.Wo);
    const long t2 = m / p.Wo;
    const int oy = (int)(t2 % p.Ho), n = (int)(t2 / p.Ho);
    const int sy = oy * p.stride - p.pad + kh * p.dil, sx = ox * p.stride - p.pad + kw * p.dil;
    if ((unsigned)sy >= (unsigned)p.H || (unsigned)sx >= (unsigned)p.W) continue;
    acc += (float)dy[(size_t)m * p.src_ps + o] * (float)x[(((size_t)n * p.H + sy) * p.W + sx) * p.dst_ps + ci];
  }
  part[(size_t)blockIdx.x * nw + e] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
// the geometry of a problem whose arguments are in range; false = empty output
static bool gc_geometry(GconvParams *p, int N, int H, int W, int C, int O, int groups, int KH, int KW, int stride, int pad, int dil) {
  p->N = N; p->H = H; p->W = W; p->C = C; p->O = O; p->groups = groups;
  p->Cg = C / groups; p->Og = O / groups;
  p->KH = KH; p->KW = KW; p->stride = stride; p->pad = pad; p->dil = dil;
  p->Ho = sn_conv_out(H, KH, stride, pad, dil);
  p->Wo = sn_conv_out(W, KW, stride, pad, dil);
  p->relu = 0; p->acc_ps = 0; p->cg_shift = p->s_shift = 0;
  while ((1 << p->cg_shift) < p->Cg) ++p->cg_shift;
  while ((1 << p->s_shift) < stride) ++p->s_shift;
  return p->Ho > 0 && p->Wo > 0;
}
static int gc_check(const void *a, const void *b, const void *c, int N, int H, int W, int C, int O, int groups, int KH, int KW,
                    int stride, int pad, int dil, GconvParams *p, const char *who) {
  SN_REQUIRE(a && b && c, "%s: null pointer", who);
  SN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && O > 0 && KH > 0 && KW > 0 && stride > 0 && dil > 0 && pad >= 0, "%s: bad geometry", who);
  SN_REQUIRE(groups > 1, "%s: groups == %d is a dense convolution (sn_conv_fwd / _dgrad / _wgrad)", who, groups);
  SN_REQUIRE(C % groups == 0 && O % groups == 0, "%s: C = %d and O = %d must be multiples of groups = %d", who, C, O, groups);
  SN_REQUIRE(!(groups == C && groups == O), "%s: groups == C == O is the depthwise convolution (sn_dwconv_*)", who);
  SN_REQUIRE(gc_geometry(p, N, H, W, C, O, groups, KH, KW, stride, pad, dil), "%s: empty output", who);
  SN_REQUIRE((long)N * H * W < (1l << 31) / 16 && (long)N * p->Ho * p->Wo < (1l << 31) / 16, "%s: too many pixels", who);
  return SN_OK;
}

static bool gc_fast(const GconvParams &p) {
  const int T = p.KH * p.KW;
  return p.Cg == p.Og && (p.Cg == 4 || p.Cg == 8 || p.Cg == 16 || p.Cg == 32) && p.C % 32 == 0 && p.KH == p.KW && (T == 1 || T == 9) &&
         (p.stride == 1 || p.stride == 2);
}
static int gc_blocks(long total) { return sn_blocks(total, 16384); }

template <bool DGRAD>
static void gc_launch_mfma(const void *src, const void *w, const float *bias, const void *acc, void *dst, GconvParams &p, hipStream_t s) {
  const int nslab = p.C / 32, wpb = gc_waves(nslab), gy = nslab / wpb;
  p.ntiles = (int)((p.M + 15) / 16);
  int gx = sn_div_up(256 * 3, gy);                  // three workgroups per CU (all resident), each wave loops over the tiles
  if (gx > p.ntiles) gx = p.ntiles;
  if (p.KH * p.KW == 9)
    hipLaunchKernelGGL((gconv_mfma_kernel<9, DGRAD>), dim3(gx, gy), dim3(64 * wpb), 0, s, (const half_t *)src, (const half_t *)w, bias,
                       (const half_t *)acc, (half_t *)dst, p);
  else
    hipLaunchKernelGGL((gconv_mfma_kernel<1, DGRAD>), dim3(gx, gy), dim3(64 * wpb), 0, s, (const half_t *)src, (const half_t *)w, bias,
                       (const half_t *)acc, (half_t *)dst, p);
}

SN_EXPORT int sn_gconv_fwd(const void *x, const void *w, const float *bias, void *y, int N, int H, int W, int C, int in_pix_stride,
                           int O, int out_pix_stride, int groups, int KH, int KW, int stride, int pad, int dil, int relu, int out_f32,
                           sn_stream_t stream) {
  GconvParams p;
  if (int rc = gc_check(x, w, y, N, H, W, C, O, groups, KH, KW, stride, pad, dil, &p, "sn_gconv_fwd")) return rc;
  SN_REQUIRE(in_pix_stride % 8 == 0 && out_pix_stride % 8 == 0 && in_pix_stride >= C && out_pix_stride >= O,
             "sn_gconv_fwd: pixel pitches must be a multiple of 8 and cover the channels");
  p.src_ps = in_pix_stride; p.dst_ps = out_pix_stride; p.relu = relu;
  p.M = (long)N * p.Ho * p.Wo;
  hipStream_t s = sn_stream(stream);
  if (gc_fast(p) && !out_f32)
    gc_launch_mfma<false>(x, w, bias, nullptr, y, p, s);
  else
    hipLaunchKernelGGL(gconv_plain_fwd_kernel, dim3(gc_blocks(p.M * O)), dim3(256), 0, s, (const half_t *)x, (const half_t *)w, bias, y, p,
                       out_f32);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_gconv_dgrad(const void *dy, const void *w, const void *accumulate, void *dx, int N, int H, int W, int C, int O,
                             int dy_pix_stride, int acc_pix_stride, int dx_pix_stride, int groups, int KH, int KW, int stride, int pad,
                             int dil, sn_stream_t stream) {
  GconvParams p;
  if (int rc = gc_check(dy, w, dx, N, H, W, C, O, groups, KH, KW, stride, pad, dil, &p, "sn_gconv_dgrad")) return rc;
  SN_REQUIRE(dy_pix_stride % 8 == 0 && dx_pix_stride % 8 == 0 && (!accumulate || acc_pix_stride % 8 == 0) && dy_pix_stride >= O &&
                 dx_pix_stride >= C && (!accumulate || acc_pix_stride >= C),
             "sn_gconv_dgrad: pixel pitches must be a multiple of 8 and cover the channels");
  p.src_ps = dy_pix_stride; p.dst_ps = dx_pix_stride; p.acc_ps = acc_pix_stride;
  p.M = (long)N * H * W;
  hipStream_t s = sn_stream(stream);
  if (gc_fast(p))
    gc_launch_mfma<true>(dy, w, nullptr, accumulate, dx, p, s);
  else
    hipLaunchKernelGGL(gconv_plain_dgrad_kernel, dim3(gc_blocks(p.M * C)), dim3(256), 0, s, (const half_t *)dy, (const half_t *)w,
                       (const half_t *)accumulate, (half_t *)dx, p);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

// -> pixel blocks (= partial slabs in the workspace); fast path: 32-pixel chunks per block, plain path: pixels per block
static int gc_wgrad_blocks(const GconvParams &p, int *per_block) {
  const long M = (long)p.N * p.Ho * p.Wo;
  if (gc_fast(p)) {
    return gc_chunk_blocks(M, p.C / 32, per_block);
  }
  long blocks = (M + 63) / 64;
  if (blocks > 128) blocks = 128;
  *per_block = (int)((M + blocks - 1) / blocks);
  return (int)((M + *per_block - 1) / *per_block);
}

SN_EXPORT size_t sn_gconv_wgrad_workspace_bytes(int N, int H, int W, int C, int O, int groups, int KH, int KW, int stride, int pad,
                                                int dil) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || O <= 0 || groups <= 1 || C % groups || O % groups || KH <= 0 || KW <= 0 || stride <= 0 ||
      dil <= 0 || pad < 0)
    return 0;
  GconvParams p;
  if (!gc_geometry(&p, N, H, W, C, O, groups, KH, KW, stride, pad, dil)) return 0;
  int per;
  return sn_align(sizeof(float) * (size_t)gc_wgrad_blocks(p, &per) * O * KH * KW * p.Cg);
}

SN_EXPORT int sn_gconv_wgrad(const void *dy, const void *x, float *dw, int N, int H, int W, int C, int O, int dy_pix_stride,
                             int x_pix_stride, int groups, int KH, int KW, int stride, int pad, int dil, void *ws, size_t ws_bytes,
                             sn_stream_t stream) {
  GconvParams p;
  if (int rc = gc_check(dy, x, dw, N, H, W, C, O, groups, KH, KW, stride, pad, dil, &p, "sn_gconv_wgrad")) return rc;
  SN_REQUIRE(dy_pix_stride % 8 == 0 && x_pix_stride % 8 == 0 && dy_pix_stride >= O && x_pix_stride >= C,
             "sn_gconv_wgrad: pixel pitches must be a multiple of 8 and cover the channels");
  p.src_ps = dy_pix_stride; p.dst_ps = x_pix_stride;        // (the weight gradient reads both: src = dy, dst = x)
  p.M = (long)N * p.Ho * p.Wo;
  int per;
  const int blocks = gc_wgrad_blocks(p, &per);
  const long nw = (long)O * KH * KW * p.Cg;
  SN_REQUIRE(ws && ws_bytes >= sizeof(float) * (size_t)blocks * nw,
             "sn_gconv_wgrad: needs sn_gconv_wgrad_workspace_bytes(...) of scratch (per-block partials, summed in order)");
  hipStream_t s = sn_stream(stream);
  if (gc_fast(p)) {
    const int nslab = C / 32, wpb = gc_waves(nslab);
    const dim3 grid((unsigned)blocks, nslab / wpb), block(64 * wpb);
    const int T = KH * KW;
    if (T == 9 && p.Cg == 32)
      hipLaunchKernelGGL((gconv_wgrad_mfma_kernel<9, 2>), grid, block, 0, s, (const half_t *)dy, (const half_t *)x, (float *)ws, p, per);
    else if (T == 9)
      hipLaunchKernelGGL((gconv_wgrad_mfma_kernel<9, 1>), grid, block, 0, s, (const half_t *)dy, (const half_t *)x, (float *)ws, p, per);
    else if (p.Cg == 32)
      hipLaunchKernelGGL((gconv_wgrad_mfma_kernel<1, 2>), grid, block, 0, s, (const half_t *)dy, (const half_t *)x, (float *)ws, p, per);
    else
      hipLaunchKernelGGL((gconv_wgrad_mfma_kernel<1, 1>), grid, block, 0, s, (const half_t *)dy, (const half_t *)x, (float *)ws, p, per);
  } else {
    hipLaunchKernelGGL(gconv_plain_wgrad_kernel, dim3((unsigned)blocks, (unsigned)((nw + 255) / 256)), dim3(256), 0, s,
                       (const half_t *)dy, (const half_t *)x, (float *)ws, p, per);
  }
  SN_CHECK_LAUNCH();
  return sn_partial_sum((const float *)ws, blocks, nw, dw, s);
}
