// jpeg_decode.hip -- baseline JPEG decoding on gfx950 (the C ABI is in include/sniper_hip.h).
//   jpeg_entropy_kernel   one workgroup per segment (a restart interval, or the whole scan).  The segment is cut into subsequences of
//                         `sub` bytes and decoded by the self-synchronising scheme: every lane decodes its subsequences from the guess
//                         "a block starts here"; in each later round a lane takes the exit state of the subsequence before as its
//                         entry and decodes again only where that entry changed.  After round t the first t subsequences are exact,
//                         so the loop ends after at most as many rounds as there are subsequences, whatever the data; it ends earlier
//                         when a round changes nothing.  Then an exclusive scan of the completed-block counts, and a second pass
//                         that decodes once more from the exact entries and writes the coefficients (int16, natural order, DC as
//                         differences) into the zeroed buffer.  The four Huffman tables of the image are built into LDS.
//   jpeg_dc_kernel        one wave per (segment, component): the running sum of the DC differences in block order.
//   jpeg_idct_kernel      one lane per 8 x 8 block: dequantise, slow-integer IDCT (columns, then rows), the samples into component
//                         planes in HBM (MCU padding included: the planes are the caller's scratch).
//   jpeg_colour_kernel    four output pixels per lane: fancy upsampling of the chroma planes, YCbCr -> BGR, three dword stores.
// The decoding itself (tables, bit reader, spans) is csrc/jpeg_entropy.h, which is also a host program with the sanitizers on: its
// bounds are proven there.  Plain vector stores; the only atomic is the OR of a non-zero status into the image's word.
#include "common.h"
#include "jpeg_entropy.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxImages = 65535;
constexpr int kMinSub = 16;          // a symbol is at most 27 bits, 8 bytes with stuffing: an entry never skips a whole subsequence
constexpr int kMaxSub = 4096;
constexpr int kDeviceMaxBpm = 6;
constexpr int kMaxSegmentSubs = 16384;      // a segment is one workgroup's: its rounds, at the worst one per subsequence, stay a fraction of a second
constexpr int kImgFields = 16;
constexpr int kSegFields = 8;
// img: W, H, ncomp, hs, vs, mcux, mcuy, bpm, seg0, nseg, blk0, plane0, stream0, stream_len, sel, ri
enum { IW = 0, IH, INC, IHS, IVS, IMX, IMY, IBPM, ISEG0, INSEG, IBLK0, IPLANE0, ISTREAM0, ILEN, ISEL, IRI };
// seg: image, first byte, end byte (inside the image's stream), first subsequence, subsequences
enum { SIMG = 0, SFIRST, SEND, SSUB0, SNSUB };

const int kDefaultSub = [] {
  const int v = sn_env_int("SNIPER_JPEG_SUB", 128);
  return v < kMinSub ? kMinSub : (v > kMaxSub ? kMaxSub : v);
}();

__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(const uint8_t *__restrict__ data, const int32_t *__restrict__ img,
                                                                const int32_t *__restrict__ seg, const uint8_t *__restrict__ dht, int sub,
                                                                long n_sub, uint32_t *state, int32_t *counts, int16_t *coef,
                                                                int32_t *rounds, int32_t *status, int phases) {
  __shared__ SnJpegHuff huff[4];
  __shared__ int sc[kThreads];
  const int tid = threadIdx.x;
  const int32_t *sg = seg + (long)blockIdx.x * kSegFields;
  const int im = sg[SIMG];
  const int32_t *ig = img + (long)im * kImgFields;
  if (tid < 4) sn_jpeg_build_table(dht + ((long)im * 4 + tid) * kJpegDhtBytes, &huff[tid]);
  __syncthreads();
  const uint32_t len = (uint32_t)ig[ILEN];
  uint32_t end = (uint32_t)sg[SEND], first = (uint32_t)sg[SFIRST];
  end = end < len ? end : len;
  first = first < end ? first : end;
  const uint32_t nsub = (uint32_t)sg[SNSUB];
  const long sub0 = sg[SSUB0];
  SnJpegCtx c;
  c.data = data + ig[ISTREAM0];
  c.end = end;
  c.huff = huff;
  c.bpm = (uint32_t)ig[IBPM];
  c.nluma = (uint32_t)(ig[IHS] * ig[IVS]);
  c.sel = (uint32_t)ig[ISEL];
  uint2 *entry = (uint2 *)state + sub0;
  uint2 *exits = (uint2 *)state + n_sub + sub0;          // two buffers of exit states, n_sub apart: a round reads one and writes the other
  int32_t *cnt = counts + sub0, *base = counts + n_sub + sub0;

  if (phases & 1) {
    int dummy = 0;
    for (uint32_t i = tid; i < nsub; i += kThreads) {
      const uint32_t lo = first + i * sub, hi = i + 1 == nsub ? end : first + (i + 1) * sub;
      SnJpegState in, out;
      if (i == 0) {
        in.p = first * 8u;
        in.bk = 0;
      } else {
        in = sn_jpeg_guess(c.data, first, lo, end);
      }
      const int n = sn_jpeg_decode_span(c, in, lo, hi, nullptr, 0, kJpegNoLimit, &out, &dummy);
      entry[i] = make_uint2(in.p, in.bk);
      exits[i] = make_uint2(out.p, out.bk);
      cnt[i] = n;
    }
    __syncthreads();
    int cur = 0, nrounds = 1;
    for (uint32_t t = 1; t < nsub; ++t) {
      const uint2 *prev = exits + (long)cur * n_sub;
      uint2 *next = exits + (long)(cur ^ 1) * n_sub;
      int changed = 0;
      for (uint32_t i = tid; i < nsub; i += kThreads) {
        if (i == 0) {
          next[0] = prev[0];
          continue;
        }
        const uint2 e = prev[i - 1], mine = entry[i];
        if (e.x != mine.x || e.y != mine.y) {
          const uint32_t lo = first + i * sub, hi = i + 1 == nsub ? end : first + (i + 1) * sub;
          SnJpegState in = {e.x, e.y}, out;
          const int n = sn_jpeg_decode_span(c, in, lo, hi, nullptr, 0, kJpegNoLimit, &out, &dummy);
          entry[i] = e;
          next[i] = make_uint2(out.p, out.bk);
          cnt[i] = n;
          changed = 1;
        } else {
          next[i] = prev[i];
        }
      }
      cur ^= 1;
      if (!__syncthreads_or(changed)) break;
      ++nrounds;
    }
    // exclusive scan of the block counts, 256 subsequences at a time
    int carry = 0;
    for (uint32_t b0 = 0; b0 < nsub; b0 += kThreads) {
      const uint32_t i = b0 + tid;
      const int v = i < nsub ? cnt[i] : 0;
      sc[tid] = v;
      __syncthreads();
      for (int d = 1; d < kThreads; d <<= 1) {
        const int add = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += add;
        __syncthreads();
      }
      if (i < nsub) base[i] = carry + sc[tid] - v;
      carry += sc[kThreads - 1];
      __syncthreads();
    }
    if (tid == 0) rounds[blockIdx.x] = nrounds;
    __syncthreads();
  }

  if (phases & 2) {
    int st = 0, finished = 0;
    const int ls = (int)blockIdx.x - ig[ISEG0];
    const int ri = ig[IRI], n_mcu = ig[IMX] * ig[IMY];
    const int mcus = ri ? (n_mcu - ls * ri < ri ? n_mcu - ls * ri : ri) : n_mcu;
    const int expect = mcus * (int)c.bpm;
    int16_t *out_blocks = coef + ((long)ig[IBLK0] + (long)ls * ri * (long)c.bpm) * 64;
    for (uint32_t i = tid; i < nsub; i += kThreads) {
      const uint32_t lo = first + i * sub, hi = i + 1 == nsub ? end : first + (i + 1) * sub;
      const uint2 e = entry[i];
      SnJpegState in = {e.x, e.y}, out;
      const int b = base[i];
      const int n = sn_jpeg_decode_span(c, in, lo, hi, out_blocks, b, expect, &out, &st);
      // the lane whose span completes the segment's last block stops there; what the rounds counted after it was padding
      if (b < expect && b + n == expect && out.p != kJpegNoState && out.bk == 0) finished = 1;
    }
    if (!__syncthreads_or(finished) && tid == 0) st |= SNJ_BLOCKS;
    if (tid == 0 && ls + 1 < ig[INSEG]) {
      // the restart marker that is due after this segment
      const uint32_t at = (uint32_t)sg[SEND];
      if (at + 1 >= (uint32_t)ig[ILEN] || c.data[at] != 0xff || c.data[at + 1] != (uint8_t)(0xd0 + (ls & 7))) st |= SNJ_BAD_MARKER;
    }
    if (st) atomicOr(&status[im], st);
  }
}

__global__ __launch_bounds__(kWave) void jpeg_dc_kernel(const int32_t *__restrict__ img, const int32_t *__restrict__ seg, int16_t *coef,
                                                        int32_t *status) {
  const int32_t *sg = seg + (long)blockIdx.x * kSegFields;
  const int im = sg[SIMG];
  const int32_t *ig = img + (long)im * kImgFields;
  const int comp = blockIdx.y;
  if (comp >= ig[INC]) return;
  const int bpm = ig[IBPM], nluma = ig[IHS] * ig[IVS];
  const int ls = (int)blockIdx.x - ig[ISEG0];
  const int ri = ig[IRI], n_mcu = ig[IMX] * ig[IMY];
  const int mcus = ri ? (n_mcu - ls * ri < ri ? n_mcu - ls * ri : ri) : n_mcu;
  const int nl = comp == 0 ? nluma : 1, j0 = comp == 0 ? 0 : nluma + comp - 1;
  const int count = mcus * nl;
  int16_t *blocks = coef + ((long)ig[IBLK0] + (long)ls * ri * bpm) * 64;
  const int lane = threadIdx.x;
  int carry = 0, bad = 0;
  for (int q0 = 0; q0 < count; q0 += kWave) {
    const int q = q0 + lane;
    long at = 0;
    int v = 0;
    if (q < count) {
      const int mcu = q / nl, j = q - mcu * nl;
      at = ((long)mcu * bpm + j0 + j) * 64;
      v = blocks[at];
    }
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(v, d, kWave);
      if (lane >= d) v += up;
    }
    v += carry;
    if (q < count) {
      if (v < -32768 || v > 32767) bad = 1;
      blocks[at] = (int16_t)v;
    }
    carry = __shfl(v, kWave - 1, kWave);
  }
  if (bad) atomicOr(&status[im], SNJ_BAD_DC);
}

// the 1-D pass of the slow-integer IDCT on i[0 .. 7], each output (x + 2^(n-1)) >> n
template <int N>
__device__ __forceinline__ void idct_pass(int &i0, int &i1, int &i2, int &i3, int &i4, int &i5, int &i6, int &i7) {
  int z1 = (i2 + i6) * 4433;
  const int t2 = z1 - i6 * 15137, t3 = z1 + i2 * 6270;
  const int t0 = (i0 + i4) * 8192, t1 = (i0 - i4) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446;
  a1 *= 16819;
  a2 *= 25172;
  a3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  constexpr int R = 1 << (N - 1);
  i0 = (t10 + a3 + R) >> N;
  i7 = (t10 - a3 + R) >> N;
  i1 = (t11 + a2 + R) >> N;
  i6 = (t11 - a2 + R) >> N;
  i2 = (t12 + a1 + R) >> N;
  i5 = (t12 - a1 + R) >> N;
  i3 = (t13 + a0 + R) >> N;
  i4 = (t13 - a0 + R) >> N;
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const int32_t *__restrict__ img, const uint16_t *__restrict__ qtab,
                                                             const int16_t *__restrict__ coef, uint8_t *__restrict__ planes,
                                                             int32_t *status) {
  __shared__ int q[3 * 64];
  const int im = blockIdx.y;
  const int32_t *ig = img + (long)im * kImgFields;
  if (threadIdx.x < 192) q[threadIdx.x] = qtab[(long)im * 192 + threadIdx.x];
  __syncthreads();
  const int bpm = ig[IBPM], hs = ig[IHS], vs = ig[IVS], mcux = ig[IMX], mcuy = ig[IMY];
  const int nblk = mcux * mcuy * bpm;
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= nblk) return;
  const int mcu = b / bpm, j = b - mcu * bpm;
  const int my = mcu / mcux, mx = mcu - my * mcux;
  const int nluma = hs * vs;
  int comp, row0, col0, width;
  long plane = ig[IPLANE0];
  if (j < nluma) {
    comp = 0;
    const int by = j / hs, bx = j - by * hs;
    width = mcux * hs * 8;
    row0 = (my * vs + by) * 8;
    col0 = (mx * hs + bx) * 8;
  } else {
    comp = 1 + j - nluma;
    width = mcux * 8;
    row0 = my * 8;
    col0 = mx * 8;
    plane += (long)mcux * mcuy * nluma * 64 + (long)(comp - 1) * mcux * mcuy * 64;
  }
  const int *qc = q + comp * 64;
  int x[64];
  const int4 *src = (const int4 *)(coef + ((long)ig[IBLK0] + b) * 64);
  int bad = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int4 w = src[k];
    const int ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int lo = (int)(short)(ws[m] & 0xffff) * qc[k * 8 + 2 * m], hi = (ws[m] >> 16) * qc[k * 8 + 2 * m + 1];
      bad |= (unsigned)(lo + 32768) > 65535u;
      bad |= (unsigned)(hi + 32768) > 65535u;
      x[k * 8 + 2 * m] = lo;
      x[k * 8 + 2 * m + 1] = hi;
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    idct_pass<11>(x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col], x[48 + col], x[56 + col]);
#pragma unroll
    for (int r = 0; r < 8; ++r) bad |= (unsigned)(x[r * 8 + col] + 32768) > 65535u;
  }
  uint8_t *dst = planes + plane + (long)row0 * width + col0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    idct_pass<18>(x[r * 8], x[r * 8 + 1], x[r * 8 + 2], x[r * 8 + 3], x[r * 8 + 4], x[r * 8 + 5], x[r * 8 + 6], x[r * 8 + 7]);
    unsigned pk[2] = {0, 0};
#pragma unroll
    for (int col = 0; col < 8; ++col) {
      int v = x[r * 8 + col];
      bad |= (unsigned)(v + 512) > 1023u;          // outside -512 .. 511 the C and the SIMD forms of libjpeg part ways
      v = ((v + 512) & 1023) - 512 + 128;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      pk[col >> 2] |= (unsigned)v << (8 * (col & 3));
    }
    *(uint2 *)(dst + (long)r * width) = make_uint2(pk[0], pk[1]);
  }
  if (bad) atomicOr(&status[im], SNJ_RANGE);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one chroma sample at output pixel (y, x): the triangle filters of libjpeg's fancy upsampling; planes up to 2 samples wide are
// replicated, as libjpeg does
__device__ __forceinline__ int chroma_at(const uint8_t *__restrict__ p, int width, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(long)y * width + x];
  if (cw <= 2) return p[(long)(y >> (vs - 1)) * width + (x >> 1)];
  const int c = x >> 1, odd = x & 1;
  const int nb = odd ? (c + 1 < cw ? c + 1 : cw - 1) : (c > 0 ? c - 1 : 0);
  if (vs == 1) {
    const uint8_t *row = p + (long)y * width;
    return (3 * row[c] + row[nb] + (odd ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  const int nr = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
  const uint8_t *row = p + (long)r * width, *other = p + (long)nr * width;
  const int tc = 3 * row[c] + other[c], tn = 3 * row[nb] + other[nb];
  return (3 * tc + tn + (odd ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(const int32_t *__restrict__ img, const uint8_t *__restrict__ planes,
                                                               const uint64_t *__restrict__ out_ptrs) {
  const int im = blockIdx.y;
  const int32_t *ig = img + (long)im * kImgFields;
  const int W = ig[IW], H = ig[IH], nc = ig[INC], hs = ig[IHS], vs = ig[IVS], mcux = ig[IMX], mcuy = ig[IMY];
  const long npix = (long)W * H;
  const long p0 = ((long)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (p0 >= npix) return;
  const uint8_t *yp = planes + ig[IPLANE0];
  const int yw = mcux * hs * 8, cwid8 = mcux * 8;
  const uint8_t *cbp = yp + (long)yw * mcuy * vs * 8, *crp = cbp + (long)cwid8 * mcuy * 8;
  const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
  uint8_t *out = (uint8_t *)out_ptrs[im];
  uint8_t px[12];
  int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
  const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int B = 0, G = 0, R = 0;
    if (k < n) {
      const int Y = yp[(long)y * yw + x];
      if (nc == 1) {
        B = G = R = Y;
      } else {
        const int cb = chroma_at(cbp, cwid8, cw, ch, hs, vs, y, x) - 128, cr = chroma_at(crp, cwid8, cw, ch, hs, vs, y, x) - 128;
        R = clamp255(Y + ((91881 * cr + 32768) >> 16));
        B = clamp255(Y + ((116130 * cb + 32768) >> 16));
        G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      }
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
    px[3 * k] = (uint8_t)B;
    px[3 * k + 1] = (uint8_t)G;
    px[3 * k + 2] = (uint8_t)R;
  }
  if (n == 4) {
    unsigned w[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) w[m] = px[4 * m] | (px[4 * m + 1] << 8) | (px[4 * m + 2] << 16) | ((unsigned)px[4 * m + 3] << 24);
    unsigned *o = (unsigned *)(out + p0 * 3);          // p0 is a multiple of 4 and the tensor's storage is aligned: 12-byte steps
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
  } else {
#pragma unroll
    for (int m = 0; m < 12; ++m)
      if (m < 3 * n) out[p0 * 3 + m] = px[m];
  }
}

// the images' table as the host holds it: everything the kernels index with is checked here, before any launch (plane_bytes or
// total_bytes < 0: the call does not touch the planes / the streams)
int check_images(const char *fn, const int32_t *h_img, int I, long n_blocks, long plane_bytes, long total_bytes, int S, long *max_blocks,
                 long *max_pixels) {
  SN_REQUIRE(I >= 1 && I <= kMaxImages, "%s: 1 <= I <= %d required (I = %d)", fn, kMaxImages, I);
  long blk = 0, seg = 0;
  *max_blocks = 0;
  *max_pixels = 0;
  for (int i = 0; i < I; ++i) {
    const int32_t *g = h_img + (long)i * kImgFields;
    const long W = g[IW], H = g[IH], nc = g[INC], hs = g[IHS], vs = g[IVS], mx = g[IMX], my = g[IMY], bpm = g[IBPM];
    SN_REQUIRE(W >= 1 && H >= 1 && W <= 65535 && H <= 65535, "%s: image %d is %ld x %ld: 1 .. 65535 required", fn, i, H, W);
    SN_REQUIRE((nc == 1 && hs == 1 && vs == 1) || (nc == 3 && hs >= 1 && hs <= 2 && vs >= 1 && vs <= hs),
               "%s: image %d: %ld components with luma sampling %ld x %ld: 1 component, or 3 with 1x1, 2x1 or 2x2 required", fn, i, nc, hs, vs);
    SN_REQUIRE(!(hs == 2 && W <= 2), "%s: image %d: a subsampled chroma plane one sample wide (W = %ld) is not decoded here", fn, i, W);
    SN_REQUIRE(mx == (W + 8 * hs - 1) / (8 * hs) && my == (H + 8 * vs - 1) / (8 * vs) && bpm == hs * vs + nc - 1 && bpm <= kDeviceMaxBpm,
               "%s: image %d: the MCU grid %ld x %ld of %ld blocks does not follow from its size and sampling", fn, i, my, mx, bpm);
    const long nb = mx * my * bpm, ri = g[IRI];
    SN_REQUIRE(ri >= 0 && g[INSEG] == (ri ? (mx * my + ri - 1) / ri : 1), "%s: image %d: %d segments for %ld MCUs at a restart interval of %ld",
               fn, i, g[INSEG], mx * my, ri);
    SN_REQUIRE(g[ISEG0] == seg && g[IBLK0] == blk, "%s: image %d: seg0 = %d, blk0 = %d, the images before give %ld and %ld", fn, i, g[ISEG0],
               g[IBLK0], seg, blk);
    SN_REQUIRE(plane_bytes < 0 || (g[IPLANE0] >= 0 && (g[IPLANE0] & 15) == 0 && g[IPLANE0] + nb * 64 <= plane_bytes),
               "%s: image %d: its planes (%ld bytes at %d, 16-byte aligned) do not fit plane_bytes = %ld", fn, i, nb * 64, g[IPLANE0], plane_bytes);
    SN_REQUIRE(total_bytes < 0 || (g[ISTREAM0] >= 0 && g[ILEN] >= 0 && (long)g[ISTREAM0] + g[ILEN] <= total_bytes),
               "%s: image %d: its stream (%d bytes at %d) does not fit total_bytes = %ld", fn, i, g[ILEN], g[ISTREAM0], total_bytes);
    SN_REQUIRE(g[ISEL] >= 0 && g[ISEL] < 64, "%s: image %d: sel = %d, six table bits required", fn, i, g[ISEL]);
    blk += nb;
    seg += g[INSEG];
    if (nb > *max_blocks) *max_blocks = nb;
    if (W * H > *max_pixels) *max_pixels = W * H;
  }
  SN_REQUIRE(blk == n_blocks, "%s: n_blocks = %ld, the images give %ld", fn, n_blocks, blk);
  SN_REQUIRE(seg == S, "%s: S = %d, the images give %ld segments", fn, S, seg);
  SN_REQUIRE(n_blocks < (1L << 25) && plane_bytes < (1L << 31) && total_bytes < (1L << 31),
             "%s: n_blocks < 2^25, plane_bytes < 2^31 and total_bytes < 2^31 required (%ld, %ld, %ld)", fn, n_blocks, plane_bytes, total_bytes);
  return SN_OK;
}

int check_segments(const char *fn, const int32_t *h_img, int I, const int32_t *h_seg, int S, int sub, long n_sub) {
  long at = 0;
  for (int s = 0; s < S; ++s) {
    const int32_t *g = h_seg + (long)s * kSegFields;
    SN_REQUIRE(g[SIMG] >= 0 && g[SIMG] < I, "%s: segment %d names image %d of %d", fn, s, g[SIMG], I);
    const int32_t *ig = h_img + (long)g[SIMG] * kImgFields;
    SN_REQUIRE(s >= ig[ISEG0] && s < ig[ISEG0] + ig[INSEG], "%s: segment %d is not one of image %d's", fn, s, g[SIMG]);
    SN_REQUIRE(g[SFIRST] >= 0 && g[SFIRST] <= g[SEND] && g[SEND] <= ig[ILEN], "%s: segment %d: bytes %d .. %d of a stream of %d", fn, s,
               g[SFIRST], g[SEND], ig[ILEN]);
    const long bytes = g[SEND] - g[SFIRST], want = bytes > sub ? (bytes + sub - 1) / sub : 1;
    SN_REQUIRE(want <= kMaxSegmentSubs, "%s: segment %d has %ld subsequences of %d bytes, %d at the most (longer scans are the host's)", fn, s, want,
               sub, kMaxSegmentSubs);
    SN_REQUIRE(g[SNSUB] == want && g[SSUB0] == at, "%s: segment %d: %d subsequences from %d on, its %ld bytes give %ld from %ld on", fn, s,
               g[SNSUB], g[SSUB0], bytes, want, at);
    at += want;
  }
  SN_REQUIRE(at == n_sub, "%s: n_sub = %ld, the segments give %ld", fn, n_sub, at);
  return SN_OK;
}

}  // namespace

SN_EXPORT int sn_jpeg_limits(int32_t *h_out8) {
  SN_REQUIRE(h_out8, "sn_jpeg_limits: null pointer");
  h_out8[0] = kDefaultSub;
  h_out8[1] = kThreads;
  h_out8[2] = kMaxImages;
  h_out8[3] = kDeviceMaxBpm;
  h_out8[4] = (int32_t)(4 * sizeof(SnJpegHuff));
  h_out8[5] = kImgFields;
  h_out8[6] = kSegFields;
  h_out8[7] = kMinSub;
  return SN_OK;
}

SN_EXPORT int sn_jpeg_entropy(const uint8_t *data, long total_bytes, const int32_t *img, const int32_t *h_img, int I, const int32_t *seg,
                              const int32_t *h_seg, int S, const uint8_t *dht, int sub_bytes, long n_sub, long n_blocks, uint32_t *state,
                              int32_t *counts, int16_t *coef, int32_t *rounds, int32_t *status, int phases, sn_stream_t stream) {
  SN_REQUIRE(data && img && h_img && seg && h_seg && dht && state && counts && coef && rounds && status, "sn_jpeg_entropy: null pointer");
  SN_REQUIRE(sub_bytes >= kMinSub && sub_bytes <= kMaxSub, "sn_jpeg_entropy: %d <= sub_bytes <= %d required (sub_bytes = %d)", kMinSub, kMaxSub,
             sub_bytes);
  SN_REQUIRE(phases >= 1 && phases <= 3, "sn_jpeg_entropy: phases = %d: 1 (rounds), 2 (write) or 3 (both) required", phases);
  SN_REQUIRE(S >= 1, "sn_jpeg_entropy: S >= 1 required (S = %d)", S);
  SN_REQUIRE(total_bytes >= 0, "sn_jpeg_entropy: total_bytes >= 0 required (total_bytes = %ld)", total_bytes);
  long mb, mp;
  int rc = check_images("sn_jpeg_entropy", h_img, I, n_blocks, -1, total_bytes, S, &mb, &mp);
  if (rc) return rc;
  rc = check_segments("sn_jpeg_entropy", h_img, I, h_seg, S, sub_bytes, n_sub);
  if (rc) return rc;
  jpeg_entropy_kernel<<<dim3((unsigned)S), dim3(kThreads), 0, sn_stream(stream)>>>(data, img, seg, dht, sub_bytes, n_sub, state, counts, coef, rounds,
                                                                                  status, phases);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_jpeg_dc(const int32_t *img, const int32_t *h_img, int I, const int32_t *seg, const int32_t *h_seg, int S, long n_blocks,
                         int16_t *coef, int32_t *status, sn_stream_t stream) {
  SN_REQUIRE(img && h_img && seg && h_seg && coef && status, "sn_jpeg_dc: null pointer");
  SN_REQUIRE(S >= 1, "sn_jpeg_dc: S >= 1 required (S = %d)", S);
  long mb, mp;
  int rc = check_images("sn_jpeg_dc", h_img, I, n_blocks, -1, -1, S, &mb, &mp);
  if (rc) return rc;
  for (int s = 0; s < S; ++s) {
    const int32_t *g = h_seg + (long)s * kSegFields;
    SN_REQUIRE(g[SIMG] >= 0 && g[SIMG] < I && s >= h_img[(long)g[SIMG] * kImgFields + ISEG0] &&
                   s < h_img[(long)g[SIMG] * kImgFields + ISEG0] + h_img[(long)g[SIMG] * kImgFields + INSEG],
               "sn_jpeg_dc: segment %d is not one of image %d's", s, g[SIMG]);
  }
  jpeg_dc_kernel<<<dim3((unsigned)S, 3), dim3(kWave), 0, sn_stream(stream)>>>(img, seg, coef, status);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_jpeg_pixels(const int32_t *img, const int32_t *h_img, int I, const uint16_t *qtab, const int16_t *coef, long n_blocks,
                             uint8_t *planes, long plane_bytes, const uint64_t *out_ptrs, int32_t *status, sn_stream_t stream) {
  SN_REQUIRE(img && h_img && qtab && coef && planes && out_ptrs && status, "sn_jpeg_pixels: null pointer");
  SN_REQUIRE(plane_bytes >= 0, "sn_jpeg_pixels: plane_bytes >= 0 required (plane_bytes = %ld)", plane_bytes);
  long mb, mp, segs = 0;
  for (int i = 0; i < (I >= 1 && I <= kMaxImages ? I : 0); ++i) segs += h_img[(long)i * kImgFields + INSEG];
  int rc = check_images("sn_jpeg_pixels", h_img, I, n_blocks, plane_bytes, -1, (int)segs, &mb, &mp);
  if (rc) return rc;
  jpeg_idct_kernel<<<dim3((unsigned)((mb + kThreads - 1) / kThreads), (unsigned)I), dim3(kThreads), 0, sn_stream(stream)>>>(img, qtab, coef, planes,
                                                                                                                          status);
  SN_CHECK_LAUNCH();
  const long quads = (mp + 3) / 4;
  jpeg_colour_kernel<<<dim3((unsigned)((quads + kThreads - 1) / kThreads), (unsigned)I), dim3(kThreads), 0, sn_stream(stream)>>>(img, planes, out_ptrs);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
