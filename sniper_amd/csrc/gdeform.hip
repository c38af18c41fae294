// gdeform.hip -- grouped deformable convolution (DeformableConvolution with num_group > 1: the ResNeXt stage-4 3x3 with
// num_group = 64, num_deformable_group = 4), channels-last fp16 with pixel pitches, fp32 accumulation, compact [O][9][Cg] weights.
// There is no column buffer in the forward pass or the weight gradient: the DCN v1 bilinear sample (deform_sample.h) is taken in
// registers and fed to the 32-channel-slab MFMAs of gconv.hip, whose structure these kernels keep --
//   forward          a wave owns a slab and its 9 x 2 weight fragments; lane (pixel = lane & 15, quarter = lane >> 4) gathers the four
//                    corners of its pixel's tap for channels 8 * quarter .. + 7 (four 16-byte loads, issued one tap ahead of the
//                    blend), blends in fp32, rounds once to fp16 and feeds the same 18 MFMAs in the same order;
//   weight gradient  32-pixel chunks through wave-private LDS images read back transposed; the tap-shifted x tile is the sampled tile;
//                    one partial per weight into the caller's workspace, summed in block order by sn_partial_sum (no atomics);
//   column gradient  dcol[m][t][ci] = sum_o dy[m][o] * w[o][t][ci]: the slab kernel with the weights transposed in registers, one
//                    16-byte store per tap, no image read.  sn_deform_col2im (roi_deform.hip) turns it into d_data and d_offset.
// This is the only path: Cg == Og in {4, 8, 16, 32}, C % 32 == 0, (C / deformable groups) % 32 == 0 (a slab lies inside one
// deformable group), 3x3.  Everything else is an argument error.
#include "conv_common.h"
#include "deform_sample.h"
#include "gconv_slab.h"

struct GdeformParams {
  int N, H, W, Ho, Wo;
  int C, Cg, cg_shift;
  int stride, pad, dil;
  int dg_ch;                  // channels per deformable group
  int off_ps;                 // offset pixel pitch (elements)
  int x_ps, y_ps;             // pixel pitches of x and of y / dy
  int relu;
  long M;                     // output pixels N * Ho * Wo
  int ntiles;                 // 16-pixel tiles
};

constexpr int kT = 9;

// the slab's weights as A-operand fragments (gconv_mfma_kernel): row -> written channel, k = 8q + j -> contracted channel;
// TRANSPOSED: rows are input channels and k runs over output channels (the column gradient)
template <bool TRANSPOSED>
__device__ __forceinline__ void gd_weight_frags(const half_t *__restrict__ w, int ch0, int Cg, int cg_shift, int r, int q,
                                                half8 (&wa)[kT][2]) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int row_ch = 8 * (r >> 2) + 4 * b + (r & 3);
#pragma unroll
    for (int t = 0; t < kT; ++t) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k_ch = 8 * q + j;
        const int o = TRANSPOSED ? k_ch : row_ch, ci = TRANSPOSED ? row_ch : k_ch;
        half_t v = (half_t)0.f;
        if ((o >> cg_shift) == (ci >> cg_shift)) v = w[((size_t)(ch0 + o) * kT + t) * Cg + (ci & (Cg - 1))];
        wa[t][b][j] = v;
      }
    }
  }
}

// the four corners of one sampling point for 8 channels; zero when the point samples nothing
struct GdCorners {
  half8 v1, v2, v3, v4;
};

// img: the pixel's image at the lane's first channel; (ly, lx) + (dy, dx): the tap's lattice point and offset.  Loads are issued
// only under s.ok, where deform_sample has put every index inside the map: a NaN, infinite or huge offset loads nothing.
__device__ __forceinline__ GdCorners gd_gather(const half_t *__restrict__ img, bool live, int ly, int lx, float dy, float dx, int H,
                                               int W, int ps) {
  GdCorners c;
  c.v1 = c.v2 = c.v3 = c.v4 = half8{0, 0, 0, 0, 0, 0, 0, 0};
  const DeformSample s = deform_sample((float)ly + dy, (float)lx + dx, H, W);
  if (live && s.ok) {
    c.v1 = *reinterpret_cast<const half8 *>(img + ((size_t)s.y0 * W + s.x0) * ps);
    c.v2 = *reinterpret_cast<const half8 *>(img + ((size_t)s.y0 * W + s.x1) * ps);
    c.v3 = *reinterpret_cast<const half8 *>(img + ((size_t)s.y1 * W + s.x0) * ps);
    c.v4 = *reinterpret_cast<const half8 *>(img + ((size_t)s.y1 * W + s.x1) * ps);
  }
  return c;
}

// w1 v1 + w2 v2 + w3 v3 + w4 v4 in fp32, rounded once to fp16 (deform_im2col_kernel's expression).  The weights are derived again
// from the same position here, not carried from the gather: the corners of the next tap are in flight meanwhile, and eight more
// live registers per point cost the weight gradient a wave per SIMD.
__device__ __forceinline__ half8 gd_blend(const GdCorners &c, bool live, int ly, int lx, float dy, float dx, int H, int W) {
  const DeformSample s = deform_sample((float)ly + dy, (float)lx + dx, H, W);
  half8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live && s.ok) {
    const float w1 = (1.f - s.ly) * (1.f - s.lx), w2 = (1.f - s.ly) * s.lx, w3 = s.ly * (1.f - s.lx), w4 = s.ly * s.lx;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)(w1 * (float)c.v1[j] + w2 * (float)c.v2[j] + w3 * (float)c.v3[j] + w4 * (float)c.v4[j]);
  }
  return o;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256, 3) void gdeform_fwd_kernel(const half_t *__restrict__ x, const TO *__restrict__ offset,
                                                          const half_t *__restrict__ w, const float *__restrict__ bias,
                                                          half_t *__restrict__ y, const GdeformParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int slab = blockIdx.y * (blockDim.x >> 6) + wave;
  const int ch0 = slab * 32;
  half8 wa[kT][2];
  gd_weight_frags<false>(w, ch0, p.Cg, p.cg_shift, r, q, wa);
  const int og = (ch0 / p.dg_ch) * 2 * kT;       // the slab's deformable group: first offset channel
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int m = tile * 16 + r;                 // (M < 2^31 / 16: checked by the host)
    const bool live = m < (int)p.M;
    const int ox = m % p.Wo, t2 = m / p.Wo;
    const int oy = t2 % p.Ho, n = t2 / p.Ho;
    float ov[2 * kT];
#pragma unroll
    for (int i = 0; i < 2 * kT; ++i) ov[i] = live ? (float)offset[(size_t)m * p.off_ps + og + i] : 0.f;
    const half_t *img = x + (size_t)(live ? n : 0) * p.H * p.W * p.x_ps + ch0 + 8 * q;
    const int y0 = oy * p.stride - p.pad, x0 = ox * p.stride - p.pad;
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    GdCorners cur = gd_gather(img, live, y0, x0, ov[0], ov[1], p.H, p.W, p.x_ps);
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      GdCorners nxt = cur;
      if (t + 1 < kT) {
        const int nh = (t + 1) / 3, nw = (t + 1) - nh * 3;
        nxt = gd_gather(img, live, y0 + nh * p.dil, x0 + nw * p.dil, ov[2 * t + 2], ov[2 * t + 3], p.H, p.W, p.x_ps);
      }
      const int kh = t / 3, kw = t - kh * 3;
      const half8 xb = gd_blend(cur, live, y0 + kh * p.dil, x0 + kw * p.dil, ov[2 * t], ov[2 * t + 1], p.H, p.W);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], xb, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], xb, acc1, 0, 0, 0);
      cur = nxt;
    }
    // lane: pixel r, channels ch0 + 8q + {0..3} (block 0) and + {4..7} (block 1)
    if (live) {
      float o[8] = {acc0[0], acc0[1], acc0[2], acc0[3], acc1[0], acc1[1], acc1[2], acc1[3]};
      if (bias) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += bias[ch0 + 8 * q + j];
      }
      half8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = (half_t)(p.relu ? fmaxf(o[j], 0.f) : o[j]);
      *reinterpret_cast<half8 *>(y + (size_t)m * p.y_ps + ch0 + 8 * q) = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// column gradient: dcol (M, 9, C) fp16
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gdeform_dcol_kernel(const half_t *__restrict__ dy, const half_t *__restrict__ w,
                                                           half_t *__restrict__ dcol, const GdeformParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int slab = blockIdx.y * (blockDim.x >> 6) + wave;
  const int ch0 = slab * 32;
  half8 wa[kT][2];
  gd_weight_frags<true>(w, ch0, p.Cg, p.cg_shift, r, q, wa);
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int m = tile * 16 + r;
    const bool live = m < (int)p.M;
    half8 g = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) g = *reinterpret_cast<const half8 *>(dy + (size_t)m * p.y_ps + ch0 + 8 * q);
    half_t *dst = dcol + ((size_t)(live ? m : 0) * kT) * p.C + ch0 + 8 * q;
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      const floatx4 z = {0.f, 0.f, 0.f, 0.f};
      const floatx4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][0], g, z, 0, 0, 0);
      const floatx4 a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[t][1], g, z, 0, 0, 0);
      const half8 out = {(half_t)a0[0], (half_t)a0[1], (half_t)a0[2], (half_t)a0[3],
                         (half_t)a1[0], (half_t)a1[1], (half_t)a1[2], (half_t)a1[3]};
      if (live) *reinterpret_cast<half8 *>(dst + (size_t)t * p.C) = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradient: D[o][ci] += sum over 32 pixels dyT[o][pix] * sampledT[ci][pix] per tap (gconv_wgrad_mfma_kernel)
// ---------------------------------------------------------------------------------------------------------------------------------
// NB = 1: Cg <= 16, only the two diagonal 16 x 16 blocks of a slab hold weights;  NB = 2: Cg == 32, all four.  Two waves per SIMD
// for NB = 1; the 144 accumulator registers of NB = 2 leave room for the corners in flight of one wave only (asked for two, the
// compiler spills ~90 registers), so that one runs a workgroup per CU and the launch's two per CU take turns.
template <typename TO, int NB>
__global__ __launch_bounds__(256, NB == 2 ? 1 : 2) void gdeform_wgrad_kernel(const half_t *__restrict__ dy, const half_t *__restrict__ x,
                                                            const TO *__restrict__ offset, float *__restrict__ part,
                                                            const GdeformParams p, int O, int chunks_per_block) {
  __shared__ __attribute__((aligned(16))) half_t lds[4][3][32 * kTP];      // per wave: dyT and two sampled-tile buffers
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int slab = blockIdx.y * (blockDim.x >> 6) + wave;
  const int ch0 = slab * 32;
  const int og = (ch0 / p.dg_ch) * 2 * kT;
  half_t *dyT = lds[wave][0];
  const int tr_off = (8 * q + (r >> 2)) * kTP + 4 * (r & 3);      // tr_frag: this lane's address of pixel row 8q + (r >> 2)
  floatx4 acc[kT][2][NB];
#pragma unroll
  for (int t = 0; t < kT; ++t)
#pragma unroll
    for (int bo = 0; bo < 2; ++bo)
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[t][bo][i] = floatx4{0.f, 0.f, 0.f, 0.f};
  const long c0 = (long)blockIdx.x * chunks_per_block;
  // loads: piece i of a lane = (pixel (lane >> 2) + 16 i of the chunk, channels 8 (lane & 3) .. + 7)
  const int lp = lane >> 2, lc = (lane & 3) * 8;
  for (int c = 0; c < chunks_per_block; ++c) {
    const long mbase = (c0 + c) * 32;            // (uniform over the block: every wave passes every barrier)
    int y0[2], x0[2];
    bool live[2];
    const half_t *img[2];
    const TO *op[2];
    half8 gv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long m = mbase + lp + 16 * i;       // (M < 2^31 / 16: checked by the host; a chunk past the end loads nothing)
      live[i] = m < p.M;
      const int mm = live[i] ? (int)m : 0;
      const int ox = mm % p.Wo, t2 = mm / p.Wo;
      const int oy = t2 % p.Ho, n = t2 / p.Ho;
      y0[i] = oy * p.stride - p.pad;
      x0[i] = ox * p.stride - p.pad;
      img[i] = x + (size_t)n * p.H * p.W * p.x_ps + ch0 + lc;
      op[i] = offset + (size_t)mm * p.off_ps + og;
      gv[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live[i]) gv[i] = *reinterpret_cast<const half8 *>(dy + (size_t)mm * p.y_ps + ch0 + lc);
    }
    // a tap's offsets are read two taps ahead of its blend, its corners one tap ahead: a gather waits for nothing but itself
    TO ov[2][2 * kT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) ov[i][k] = op[i][k];      // (pixel 0's offsets for a dead piece: read, never used)
    GdCorners cur[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) cur[i] = gd_gather(img[i], live[i], y0[i], x0[i], (float)ov[i][0], (float)ov[i][1], p.H, p.W, p.x_ps);
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<half8 *>(dyT + (lp + 16 * i) * kTP + lc) = gv[i];
    half8 fa[2];
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      half_t *xT = lds[wave][1 + (t & 1)];
      GdCorners nxt[2] = {cur[0], cur[1]};
      if (t + 2 < kT) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          ov[i][2 * t + 4] = op[i][2 * t + 4];
          ov[i][2 * t + 5] = op[i][2 * t + 5];
        }
      }
      if (t + 1 < kT) {
        const int nh = (t + 1) / 3, nw = (t + 1) - nh * 3;
#pragma unroll
        for (int i = 0; i < 2; ++i)
          nxt[i] = gd_gather(img[i], live[i], y0[i] + nh * p.dil, x0[i] + nw * p.dil, (float)ov[i][2 * t + 2], (float)ov[i][2 * t + 3],
                             p.H, p.W, p.x_ps);
      }
      const int kh = t / 3, kw = t - kh * 3;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        *reinterpret_cast<half8 *>(xT + (lp + 16 * i) * kTP + lc) =
            gd_blend(cur[i], live[i], y0[i] + kh * p.dil, x0[i] + kw * p.dil, (float)ov[i][2 * t], (float)ov[i][2 * t + 1], p.H, p.W);
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
      cur[0] = nxt[0];
      cur[1] = nxt[1];
    }
    __syncthreads();          // the next chunk rewrites dyT and the first sampled-tile buffer
  }
  // lane holds D[row o = 4q + reg][col ci = r] of every block: one partial per weight of the slab, [block][O][9][Cg]
  float *po = part + (size_t)blockIdx.x * O * kT * p.Cg;
#pragma unroll
  for (int t = 0; t < kT; ++t)
#pragma unroll
    for (int bo = 0; bo < 2; ++bo)
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int bi = NB == 2 ? i : bo;
        const int ci = bi * 16 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = bo * 16 + 4 * q + e;
          if (o / p.Cg == ci / p.Cg) po[((size_t)(ch0 + o) * kT + t) * p.Cg + ci % p.Cg] = acc[t][bo][i][e];
        }
      }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
// every condition of the one path, each named; DG < 0: the entry point takes no deformable groups (the column gradient)
static int gd_check(const char *who, bool pointers, int N, int H, int W, int C, int O, int groups, int DG, int KH, int KW, int stride,
                    int pad, int dil, GdeformParams *p) {
  SN_REQUIRE(pointers, "%s: null pointer", who);
  SN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && O > 0 && KH > 0 && KW > 0 && stride > 0 && dil > 0 && pad >= 0 && groups > 0 && DG != 0,
             "%s: bad geometry", who);
  SN_REQUIRE(groups > 1, "%s: groups == %d is the dense deformable convolution (sn_deform_im2col + sn_conv_fwd)", who, groups);
  SN_REQUIRE(C % groups == 0 && O % groups == 0 && C / groups == O / groups,
             "%s: Cg != Og (C = %d, O = %d, groups = %d): only square groups are built", who, C, O, groups);
  const int Cg = C / groups;
  SN_REQUIRE((Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32) && C % 32 == 0,
             "%s: off the slab grid: C / groups = %d must be 4, 8, 16 or 32 and C = %d a multiple of 32", who, Cg, C);
  SN_REQUIRE(KH == 3 && KW == 3, "%s: %dx%d kernel: only 3x3 is built", who, KH, KW);
  SN_REQUIRE(DG < 0 || (C % DG == 0 && (C / DG) % 32 == 0),
             "%s: a deformable group splits a slab: C / deformable_groups = %d / %d must be a multiple of 32", who, C, DG);
  p->N = N; p->H = H; p->W = W; p->C = C; p->Cg = Cg;
  p->stride = stride; p->pad = pad; p->dil = dil;
  p->Ho = sn_conv_out(H, KH, stride, pad, dil);
  p->Wo = sn_conv_out(W, KW, stride, pad, dil);
  SN_REQUIRE(p->Ho > 0 && p->Wo > 0, "%s: empty output", who);
  p->cg_shift = 0;
  while ((1 << p->cg_shift) < Cg) ++p->cg_shift;
  p->dg_ch = DG > 0 ? C / DG : C;
  p->M = (long)N * p->Ho * p->Wo;
  SN_REQUIRE((long)N * H * W < (1l << 31) / 16 && p->M < (1l << 31) / 16, "%s: too many pixels for 32-bit indexing", who);
  p->ntiles = (int)((p->M + 15) / 16);
  p->off_ps = p->x_ps = p->y_ps = p->relu = 0;
  return SN_OK;
}

static int gd_check_offset(const char *who, int DG, int off_ps, int offset_dtype, GdeformParams *p) {
  SN_REQUIRE(offset_dtype == 0 || offset_dtype == 1, "%s: offset_dtype must be 0 (fp16) or 1 (fp32)", who);
  SN_REQUIRE(off_ps >= 2 * kT * DG, "%s: offset_pix_stride = %d does not cover 2 * 9 * deformable_groups = %d channels", who, off_ps,
             2 * kT * DG);
  p->off_ps = off_ps;
  return SN_OK;
}

// grid of the tile-looping kernels: slabs / waves rows, `per_cu` workgroups per CU over them
static dim3 gd_tile_grid(const GdeformParams &p, int per_cu, int *wpb) {
  const int nslab = p.C / 32;
  *wpb = gc_waves(nslab);
  const int gy = nslab / *wpb;
  int gx = sn_div_up(256 * per_cu, gy);
  if (gx > p.ntiles) gx = p.ntiles;
  return dim3(gx, gy);
}

SN_EXPORT int sn_gdeform_fwd(const void *x, const void *offset, const void *w, const float *bias, void *y, int N, int H, int W, int C,
                             int in_pix_stride, int O, int out_pix_stride, int groups, int deformable_groups, int KH, int KW,
                             int stride, int pad, int dil, int offset_pix_stride, int offset_dtype, int relu, sn_stream_t stream) {
  GdeformParams p;
  if (int rc = gd_check("sn_gdeform_fwd", x && offset && w && y, N, H, W, C, O, groups, deformable_groups > 0 ? deformable_groups : 0,
                        KH, KW, stride, pad, dil, &p))
    return rc;
  if (int rc = gd_check_offset("sn_gdeform_fwd", deformable_groups, offset_pix_stride, offset_dtype, &p)) return rc;
  SN_REQUIRE(in_pix_stride % 8 == 0 && out_pix_stride % 8 == 0 && in_pix_stride >= C && out_pix_stride >= O,
             "sn_gdeform_fwd: pixel pitches must be a multiple of 8 and cover the channels");
  p.x_ps = in_pix_stride; p.y_ps = out_pix_stride; p.relu = relu;
  int wpb;
  const dim3 grid = gd_tile_grid(p, 3, &wpb);       // three workgroups per CU (all resident), each wave loops over the tiles
  hipStream_t s = sn_stream(stream);
  if (offset_dtype == 0)
    hipLaunchKernelGGL((gdeform_fwd_kernel<half_t>), grid, dim3(64 * wpb), 0, s, (const half_t *)x, (const half_t *)offset,
                       (const half_t *)w, bias, (half_t *)y, p);
  else
    hipLaunchKernelGGL((gdeform_fwd_kernel<float>), grid, dim3(64 * wpb), 0, s, (const half_t *)x, (const float *)offset,
                       (const half_t *)w, bias, (half_t *)y, p);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_gdeform_dcol(const void *dy, const void *w, void *dcol, int N, int H, int W, int C, int O, int dy_pix_stride,
                              int groups, int KH, int KW, int stride, int pad, int dil, sn_stream_t stream) {
  GdeformParams p;
  if (int rc = gd_check("sn_gdeform_dcol", dy && w && dcol, N, H, W, C, O, groups, -1, KH, KW, stride, pad, dil, &p)) return rc;
  SN_REQUIRE(dy_pix_stride % 8 == 0 && dy_pix_stride >= O, "sn_gdeform_dcol: pixel pitches must be a multiple of 8 and cover the channels");
  SN_REQUIRE(p.M * kT * C < 2147483647L, "sn_gdeform_dcol: too many column elements for 32-bit indexing (sn_deform_col2im reads them)");
  p.y_ps = dy_pix_stride;
  int wpb;
  const dim3 grid = gd_tile_grid(p, 3, &wpb);
  hipLaunchKernelGGL(gdeform_dcol_kernel, grid, dim3(64 * wpb), 0, sn_stream(stream), (const half_t *)dy, (const half_t *)w,
                     (half_t *)dcol, p);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT size_t sn_gdeform_wgrad_workspace_bytes(int N, int H, int W, int C, int O, int groups, int KH, int KW, int stride, int pad,
                                                  int dil) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || O <= 0 || groups <= 1 || C % groups || O % groups || C % 32 || KH != 3 || KW != 3 ||
      stride <= 0 || dil <= 0 || pad < 0)
    return 0;
  const int Ho = sn_conv_out(H, KH, stride, pad, dil), Wo = sn_conv_out(W, KW, stride, pad, dil);
  if (Ho <= 0 || Wo <= 0) return 0;
  int per;
  return sn_align(sizeof(float) * (size_t)gc_chunk_blocks((long)N * Ho * Wo, C / 32, &per) * O * kT * (C / groups));
}

SN_EXPORT int sn_gdeform_wgrad(const void *dy, const void *x, const void *offset, float *dw, int N, int H, int W, int C, int O,
                               int dy_pix_stride, int x_pix_stride, int groups, int deformable_groups, int KH, int KW, int stride,
                               int pad, int dil, int offset_pix_stride, int offset_dtype, void *ws, size_t ws_bytes,
                               sn_stream_t stream) {
  GdeformParams p;
  if (int rc = gd_check("sn_gdeform_wgrad", dy && x && offset && dw, N, H, W, C, O, groups, deformable_groups > 0 ? deformable_groups : 0,
                        KH, KW, stride, pad, dil, &p))
    return rc;
  if (int rc = gd_check_offset("sn_gdeform_wgrad", deformable_groups, offset_pix_stride, offset_dtype, &p)) return rc;
  SN_REQUIRE(dy_pix_stride % 8 == 0 && x_pix_stride % 8 == 0 && dy_pix_stride >= O && x_pix_stride >= C,
             "sn_gdeform_wgrad: pixel pitches must be a multiple of 8 and cover the channels");
  p.y_ps = dy_pix_stride; p.x_ps = x_pix_stride;
  int per;
  const int nslab = C / 32, wpb = gc_waves(nslab);
  const int blocks = gc_chunk_blocks(p.M, nslab, &per);
  const long nw = (long)O * kT * p.Cg;
  SN_REQUIRE(ws && ws_bytes >= sizeof(float) * (size_t)blocks * nw,
             "sn_gdeform_wgrad: short workspace: needs sn_gdeform_wgrad_workspace_bytes(...) of scratch (per-block partials, summed in order)");
  hipStream_t s = sn_stream(stream);
  const dim3 grid((unsigned)blocks, nslab / wpb), block(64 * wpb);
  const half_t *gy = (const half_t *)dy, *gx = (const half_t *)x;
  if (offset_dtype == 0 && p.Cg == 32)
    hipLaunchKernelGGL((gdeform_wgrad_kernel<half_t, 2>), grid, block, 0, s, gy, gx, (const half_t *)offset, (float *)ws, p, O, per);
  else if (offset_dtype == 0)
    hipLaunchKernelGGL((gdeform_wgrad_kernel<half_t, 1>), grid, block, 0, s, gy, gx, (const half_t *)offset, (float *)ws, p, O, per);
  else if (p.Cg == 32)
    hipLaunchKernelGGL((gdeform_wgrad_kernel<float, 2>), grid, block, 0, s, gy, gx, (const float *)offset, (float *)ws, p, O, per);
  else
    hipLaunchKernelGGL((gdeform_wgrad_kernel<float, 1>), grid, block, 0, s, gy, gx, (const float *)offset, (float *)ws, p, O, per);
  SN_CHECK_LAUNCH();
  return sn_partial_sum((const float *)ws, blocks, nw, dw, s);
}
