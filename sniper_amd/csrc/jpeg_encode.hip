// jpeg_encode.hip -- baseline JPEG encoding of a batch of pictures on the device: what turns a rendered batch
// (render.hip) into the entropy-coded scans of .jpg files, byte for byte the scans libjpeg writes (quality scaling of the Annex K
// tables, 4:2:0 / 4:2:2 / 4:4:4 or grey, slow-integer DCT, the Annex K Huffman tables, no restart markers).  Integer arithmetic only,
// the same bytes every run; the per-block code is csrc/jpeg_enc_code.h, shared with a stand-alone host program.
//
//   jpeg_enc_blocks_kernel   one lane per 8 x 8 block in scan order, its 64 values in registers: colour conversion, libjpeg's edge rule,
//                            chroma downsampling, forward DCT, quantisation by exact reciprocals held in LDS; the block is stored as
//                            int16 in zig-zag order.  A dummy block of an edge MCU takes the DC of the last real luma block before it.
//   jpeg_enc_size_kernel     one lane per block: the bits of its code (the DC against the same component's previous block).
//   jpeg_enc_write_kernel    one lane per block at the bit offset the caller's scan of the sizes gives: the code OR-ed into the
//                            zeroed raw stream of its picture; the last block adds the ones that fill the last byte.
//   jpeg_enc_stuff_kernel    one lane per 64-byte chunk of a raw stream: phase 1 counts the chunk's bytes after FF 00 stuffing, phase 2
//                            writes them at the byte offset the caller's scan of the counts gives.
// The raw stream of picture i starts at chunk chunk_off[i] (64-byte chunks, so that a chunk belongs to one picture).  The only
// atomics are the 32-bit ORs into zeroed words (order-independent).  No scratch; plain vector stores.
#include "common.h"
#include "jpeg_enc_code.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPictures = 65535;
constexpr long kMaxBlocks = 1L << 22;      // per call: the raw and the stuffed capacity (3 x 208 bytes a block) stay below 2^32
constexpr int kChunk = 64;                 // bytes of raw stream per lane of the stuffing kernel
constexpr int kChunkWords = kChunk / 4;

struct Geo {
  int hs, vs, nluma, bpm;
};

__host__ __device__ inline Geo geo_of(int ncomp, int sampling) {
  Geo g;
  g.hs = (ncomp == 3 && sampling >= 1) ? 2 : 1;
  g.vs = (ncomp == 3 && sampling == 2) ? 2 : 1;
  g.nluma = g.hs * g.vs;
  g.bpm = g.nluma + (ncomp == 3 ? 2 : 0);
  return g;
}

__host__ __device__ inline long blocks_of(long h, long w, const Geo g) {
  return ((w + 8 * g.hs - 1) / (8 * g.hs)) * ((h + 8 * g.vs - 1) / (8 * g.vs)) * g.bpm;
}

// the last s in [0, S) with off[s] <= v (17 steps for S <= 65535)
__device__ __forceinline__ int locate(const int64_t *__restrict__ off, int S, long long v) {
  int lo = 0, hi = S - 1;
  for (int it = 0; it < 17; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (lo < hi) {
      if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
  }
  return lo;
}

// where block b lies: everything clamped into what the sizes give
struct BlockAt {
  int img, h, w, mcux, k, mx, my;
  long long j, nblk;
  bool ok;
};

__device__ __forceinline__ BlockAt block_at(const int32_t *__restrict__ hw, const int64_t *__restrict__ blk_off, int I, long long b, const Geo g) {
  BlockAt a;
  a.img = locate(blk_off, I, b);
  a.h = min(max(hw[2 * a.img], 1), 65535);
  a.w = min(max(hw[2 * a.img + 1], 1), 65535);
  a.mcux = (a.w + 8 * g.hs - 1) / (8 * g.hs);
  a.nblk = blocks_of(a.h, a.w, g);
  a.j = b - blk_off[a.img];
  a.ok = a.j >= 0 && a.j < a.nblk && blk_off[a.img + 1] - blk_off[a.img] == a.nblk;
  const long long j = a.ok ? a.j : 0;
  const int mcu = (int)(j / g.bpm);
  a.k = (int)(j - (long long)mcu * g.bpm);
  a.my = mcu / a.mcux;
  a.mx = mcu - a.my * a.mcux;
  return a;
}

// the block of the same component before block b in scan order, or -1
__device__ __forceinline__ long long pred_block(long long b, const BlockAt &a, const Geo g) {
  const bool first_mcu = a.j < g.bpm;
  if (a.k < g.nluma) return a.k > 0 ? b - 1 : (first_mcu ? -1 : b - g.bpm + g.nluma - 1);
  return first_mcu ? -1 : b - g.bpm;
}

struct QuantLds {
  uint32_t recip[2][64];
  uint32_t d[2][64];
};

__device__ __forceinline__ int luma_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int cb_of(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int cr_of(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// component `comp` of the pixel (x, y) of an (h, w, ncomp) picture; x and y inside the picture
__device__ __forceinline__ int comp_at(const uint8_t *__restrict__ p, int w, int ncomp, int comp, int x, int y) {
  const long long at = (long long)y * w + x;
  if (ncomp == 1) return p[at];
  const int r = p[3 * at], g = p[3 * at + 1], b = p[3 * at + 2];
  return comp == 0 ? luma_of(r, g, b) : (comp == 1 ? cb_of(r, g, b) : cr_of(r, g, b));
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_blocks_kernel(const uint8_t *__restrict__ pix, long long total_pixels,
                                                                   const int32_t *__restrict__ hw, const int64_t *__restrict__ pix_off,
                                                                   const int64_t *__restrict__ blk_off, int I, long long n_blocks, int ncomp,
                                                                   int sampling, int quality, int16_t *__restrict__ coef) {
  __shared__ QuantLds Q;
  if (threadIdx.x < 128) {
    const int t = threadIdx.x >> 6, zz = threadIdx.x & 63;
    const uint32_t d = 8u * (uint32_t)sn_jpeg_enc_quant_entry(t, zz, quality);
    Q.d[t][zz] = d;
    Q.recip[t][zz] = sn_jpeg_enc_recip(d);
  }
  __syncthreads();
  const long long b = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (b >= n_blocks) return;
  const Geo g = geo_of(ncomp, sampling);
  const BlockAt a = block_at(hw, blk_off, I, b, g);
  const int h = a.h, w = a.w;
  const long long p0 = pix_off[a.img];
  uint4 *dst = reinterpret_cast<uint4 *>(coef + b * 64);
  if (!a.ok || p0 < 0 || p0 + (long long)h * w > total_pixels) {
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint8_t *p = pix + (long long)ncomp * p0;
  const int comp = a.k < g.nluma ? 0 : a.k - g.nluma + 1;
  int d[64];
  bool dummy = false;
  // the block's first sample in its component, and how a sample is made: of one pixel, of a pair (h2v1: the row extended by its last
  // sample, bias 0, 1, 0, 1, ..) or of 2 x 2 (h2v2: the rows extended to an even count, bias 1, 2, 1, 2, ..; below the last
  // DOWNSAMPLED row, that row again).  mul brings all three to a sum of four: (4 v) >> 2 = v, (2 (a + b + bias)) >> 2 = (a + b + bias) >> 1.
  int bx = a.mx, by = a.my;
  const bool two_x = comp != 0 && g.hs == 2, two_y = comp != 0 && g.vs == 2;
  if (comp == 0) {
    const int wb = (w + 7) >> 3, hb = (h + 7) >> 3;
    bx = a.mx * g.hs + (a.k & (g.hs - 1));
    by = a.my * g.vs + a.k / g.hs;
    if (bx >= wb || by >= hb) {
      // a dummy block: the DC of the block before it in the MCU, which is the last real one before it (block 0 is always real)
      dummy = true;
      int src = 0;
      for (int kk = a.k - 1; kk > 0; --kk) {
        const int x2 = a.mx * g.hs + (kk & (g.hs - 1)), y2 = a.my * g.vs + kk / g.hs;
        if (x2 < wb && y2 < hb) {
          src = kk;
          break;
        }
      }
      bx = a.mx * g.hs + (src & (g.hs - 1));
      by = a.my * g.vs + src / g.hs;
    }
  }
  const int mul = two_y ? 1 : (two_x ? 2 : 4);
  const int bias_even = two_y ? 1 : 0, bias_odd = two_y ? 2 : (two_x ? 2 : 0);
  const int last_row = two_y ? ((h + 1) >> 1) - 1 : h - 1;          // of the component
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int cy = min(8 * by + r, last_row);
    const int y0 = two_y ? min(2 * cy, h - 1) : cy, y1 = min(2 * cy + 1, h - 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int cx = 8 * bx + i;
      const int x0 = min(two_x ? 2 * cx : cx, w - 1), x1 = min(2 * cx + 1, w - 1);
      int s = comp_at(p, w, ncomp, comp, x0, y0);
      if (two_x) s += comp_at(p, w, ncomp, comp, x1, y0);
      if (two_y) s += comp_at(p, w, ncomp, comp, x0, y1) + comp_at(p, w, ncomp, comp, x1, y1);
      d[8 * r + i] = ((s * mul + ((i & 1) ? bias_odd : bias_even)) >> 2) - 128;
    }
  }
  sn_jpeg_enc_fdct(d);
  constexpr int nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  const int t = comp ? 1 : 0;
  uint32_t out[32];
#pragma unroll
  for (int zz = 0; zz < 64; zz += 2) {
    const int q0 = sn_jpeg_enc_quantise(d[nat[zz]], Q.d[t][zz], Q.recip[t][zz]);
    const int q1 = sn_jpeg_enc_quantise(d[nat[zz + 1]], Q.d[t][zz + 1], Q.recip[t][zz + 1]);
    out[zz >> 1] = ((uint32_t)q0 & 0xffffu) | ((uint32_t)q1 << 16);
  }
  if (dummy) {
    out[0] &= 0xffffu;
#pragma unroll
    for (int i = 1; i < 32; ++i) out[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_size_kernel(const int16_t *__restrict__ coef, const int32_t *__restrict__ hw,
                                                                 const int64_t *__restrict__ blk_off, int I, long long n_blocks, int ncomp,
                                                                 int sampling, int32_t *__restrict__ bits, int32_t *__restrict__ status) {
  __shared__ SnJpegEncTables T;
  if (threadIdx.x < 4) sn_jpeg_enc_build_table(&T, threadIdx.x);
  __syncthreads();
  const long long b = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (b >= n_blocks) return;
  const Geo g = geo_of(ncomp, sampling);
  const BlockAt a = block_at(hw, blk_off, I, b, g);
  if (!a.ok) {
    bits[b] = 0;
    return;
  }
  const long long pb = pred_block(b, a, g);
  const int pred = pb >= 0 ? (int)coef[pb * 64] : 0;
  SnJpegEncCount c;
  sn_jpeg_enc_block(coef + b * 64, pred, a.k >= g.nluma, T, c);
  bits[b] = (int32_t)c.bits;
  if (c.err) atomicOr(status, c.err);
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_write_kernel(const int16_t *__restrict__ coef, const int32_t *__restrict__ hw,
                                                                  const int64_t *__restrict__ blk_off, int I, long long n_blocks, int ncomp,
                                                                  int sampling, const int64_t *__restrict__ bit_excl,
                                                                  const int64_t *__restrict__ pic_first_bit, const int64_t *__restrict__ chunk_off,
                                                                  uint32_t *__restrict__ raw, long long cap_words, int32_t *__restrict__ status) {
  __shared__ SnJpegEncTables T;
  if (threadIdx.x < 4) sn_jpeg_enc_build_table(&T, threadIdx.x);
  __syncthreads();
  const long long b = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (b >= n_blocks) return;
  const Geo g = geo_of(ncomp, sampling);
  const BlockAt a = block_at(hw, blk_off, I, b, g);
  if (!a.ok) return;
  const long long pos = bit_excl[b] - pic_first_bit[a.img] + 8ll * kChunk * chunk_off[a.img];
  // the picture's raw stream ends before the next picture's first chunk
  const long long end_words = min(cap_words, (long long)kChunkWords * chunk_off[a.img + 1]);
  if (pos < 0 || pos >= 32 * end_words) {
    atomicOr(status, (int)SNE_NO_ROOM);
    return;
  }
  const long long pb = pred_block(b, a, g);
  const int pred = pb >= 0 ? (int)coef[pb * 64] : 0;
  SnJpegEncWriter wr(raw, (long)end_words, (long)pos);
  sn_jpeg_enc_block(coef + b * 64, pred, a.k >= g.nluma, T, wr);
  if (a.j == a.nblk - 1) sn_jpeg_enc_fill(wr.bitpos(), wr);
  wr.finish();
  if (wr.err) atomicOr(status, wr.err);
}

template <int kPhase>
__global__ __launch_bounds__(kThreads) void jpeg_enc_stuff_kernel(const uint32_t *__restrict__ raw, long long cap_words,
                                                                  const int64_t *__restrict__ chunk_off, const int64_t *__restrict__ raw_len, int I,
                                                                  long long n_chunks, int32_t *__restrict__ cnt, const int64_t *__restrict__ out_pos,
                                                                  uint8_t *__restrict__ out, long long capacity) {
  const long long c = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_chunks) return;
  int valid = 0;
  if (c < chunk_off[I] && (c + 1) * kChunkWords <= cap_words) {
    const int img = locate(chunk_off, I, c);
    const long long left = raw_len[img] - (long long)kChunk * (c - chunk_off[img]);
    valid = (int)min(max(left, 0ll), (long long)kChunk);
  }
  if (valid == 0) {
    if (kPhase == 1) cnt[c] = 0;
    return;
  }
  const uint4 *src = reinterpret_cast<const uint4 *>(raw + c * kChunkWords);
  uint32_t wd[kChunkWords];
#pragma unroll
  for (int i = 0; i < kChunkWords / 4; ++i) {
    const uint4 v = src[i];
    wd[4 * i] = v.x;
    wd[4 * i + 1] = v.y;
    wd[4 * i + 2] = v.z;
    wd[4 * i + 3] = v.w;
  }
  if (kPhase == 1) {
    int ff = 0;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) ff += (i < valid && ((wd[i >> 2] >> (8 * (i & 3))) & 0xffu) == 0xffu) ? 1 : 0;
    cnt[c] = valid + ff;
  } else {
    long long o = out_pos[c];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const uint32_t v = (wd[i >> 2] >> (8 * (i & 3))) & 0xffu;
      if (i < valid) {
        if (o >= 0 && o < capacity) out[o] = (uint8_t)v;
        ++o;
        if (v == 0xffu) {
          if (o >= 0 && o < capacity) out[o] = 0;
          ++o;
        }
      }
    }
  }
}

// the sizes (HOST) against the offsets (HOST); -> the message of what is wrong, or nullptr
const char *bad_pictures(const int32_t *h_hw, const int64_t *h_pix_off, const int64_t *h_blk_off, int I, const Geo g, int *which) {
  long pixels = 0, blocks = 0;
  for (int i = 0; i < I; ++i) {
    *which = i;
    const long h = h_hw[2 * i], w = h_hw[2 * i + 1];
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return "is outside 1 <= h, w <= 65535";
    if (h_pix_off && h_pix_off[i] != pixels) return "does not start at the pixel offset its predecessors' sizes give (pix_off)";
    if (h_blk_off[i] != blocks) return "does not start at the block offset its predecessors' sizes give (blk_off)";
    pixels += h * w;
    blocks += blocks_of(h, w, g);
  }
  *which = I;
  if (h_pix_off && h_pix_off[I] != pixels) return "(the end): pix_off does not end at the pixels the sizes give";
  if (h_blk_off[I] != blocks) return "(the end): blk_off does not end at the blocks the sizes give";
  return nullptr;
}

long raw_bound(const int32_t *h_hw, int I, const Geo g) {
  long bytes = 0;
  for (int i = 0; i < I; ++i) bytes += (blocks_of(h_hw[2 * i], h_hw[2 * i + 1], g) * kJpegEncRawBytesPerBlock + 1 + kChunk - 1) / kChunk * kChunk;
  return bytes;
}

unsigned grid_of(long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

#define SN_JPEG_ENC_COMMON(fn, h_hw, h_pix_off, h_blk_off, I, n_blocks, ncomp, sampling)                                                  \
  SN_REQUIRE(I >= 1 && I <= kMaxPictures, fn ": 1 <= I <= %d required (I = %d)", kMaxPictures, I);                                        \
  SN_REQUIRE(ncomp == 1 || ncomp == 3, fn ": ncomp = %d: 1 (grey) or 3 (RGB)", ncomp);                                                    \
  SN_REQUIRE(sampling >= 0 && sampling <= 2, fn ": sampling = %d: 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)", sampling);                          \
  do {                                                                                                                                    \
    int which__ = 0;                                                                                                                      \
    const char *why__ = bad_pictures(h_hw, h_pix_off, h_blk_off, I, geo_of(ncomp, sampling), &which__);                                   \
    SN_REQUIRE(!why__, fn ": picture %d %s", which__, why__);                                                                             \
  } while (0);                                                                                                                            \
  SN_REQUIRE(n_blocks == (long)h_blk_off[I], fn ": n_blocks = %ld, the sizes give %ld", (long)(n_blocks), (long)h_blk_off[I]);            \
  SN_REQUIRE(n_blocks <= kMaxBlocks, fn ": n_blocks = %ld: at most %ld blocks per call", (long)(n_blocks), kMaxBlocks)

SN_EXPORT int sn_jpeg_enc_limits(int32_t *h_out8) {
  SN_REQUIRE(h_out8, "sn_jpeg_enc_limits: null pointer");
  h_out8[0] = kThreads;
  h_out8[1] = kMaxPictures;
  h_out8[2] = (int32_t)kMaxBlocks;
  h_out8[3] = kJpegEncRawBytesPerBlock;
  h_out8[4] = kChunk;
  h_out8[5] = (int32_t)sizeof(QuantLds);
  h_out8[6] = (int32_t)sizeof(SnJpegEncTables);
  h_out8[7] = 2;      // bytes of stuffed capacity per byte of raw stream
  return SN_OK;
}

SN_EXPORT int sn_jpeg_enc_blocks(const uint8_t *pix, long total_pixels, const int32_t *hw, const int32_t *h_hw, const int64_t *pix_off,
                                 const int64_t *h_pix_off, const int64_t *blk_off, const int64_t *h_blk_off, int I, long n_blocks, int ncomp,
                                 int sampling, int quality, int16_t *coef, sn_stream_t stream) {
  SN_REQUIRE(pix && hw && h_hw && pix_off && h_pix_off && blk_off && h_blk_off && coef, "sn_jpeg_enc_blocks: null pointer");
  SN_REQUIRE(quality >= 1 && quality <= 100, "sn_jpeg_enc_blocks: quality = %d: 1 .. 100", quality);
  SN_JPEG_ENC_COMMON("sn_jpeg_enc_blocks", h_hw, h_pix_off, h_blk_off, I, n_blocks, ncomp, sampling);
  SN_REQUIRE(total_pixels == (long)h_pix_off[I], "sn_jpeg_enc_blocks: total_pixels = %ld, the sizes give %ld", total_pixels, (long)h_pix_off[I]);
  hipLaunchKernelGGL(jpeg_enc_blocks_kernel, dim3(grid_of(n_blocks)), dim3(kThreads), 0, sn_stream(stream), pix, (long long)total_pixels, hw,
                     pix_off, blk_off, I, (long long)n_blocks, ncomp, sampling, quality, coef);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_jpeg_enc_size(const int16_t *coef, const int32_t *hw, const int32_t *h_hw, const int64_t *blk_off, const int64_t *h_blk_off,
                               int I, long n_blocks, int ncomp, int sampling, int32_t *bits, int32_t *status, sn_stream_t stream) {
  SN_REQUIRE(coef && hw && h_hw && blk_off && h_blk_off && bits && status, "sn_jpeg_enc_size: null pointer");
  SN_JPEG_ENC_COMMON("sn_jpeg_enc_size", h_hw, (const int64_t *)nullptr, h_blk_off, I, n_blocks, ncomp, sampling);
  hipLaunchKernelGGL(jpeg_enc_size_kernel, dim3(grid_of(n_blocks)), dim3(kThreads), 0, sn_stream(stream), coef, hw, blk_off, I,
                     (long long)n_blocks, ncomp, sampling, bits, status);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_jpeg_enc_write(const int16_t *coef, const int32_t *hw, const int32_t *h_hw, const int64_t *blk_off, const int64_t *h_blk_off,
                                int I, long n_blocks, int ncomp, int sampling, const int64_t *bit_excl, const int64_t *pic_first_bit,
                                const int64_t *chunk_off, uint32_t *raw, long raw_capacity, int32_t *status, sn_stream_t stream) {
  SN_REQUIRE(coef && hw && h_hw && blk_off && h_blk_off && bit_excl && pic_first_bit && chunk_off && raw && status,
             "sn_jpeg_enc_write: null pointer");
  SN_JPEG_ENC_COMMON("sn_jpeg_enc_write", h_hw, (const int64_t *)nullptr, h_blk_off, I, n_blocks, ncomp, sampling);
  const long bound = raw_bound(h_hw, I, geo_of(ncomp, sampling));
  SN_REQUIRE(raw_capacity >= bound && raw_capacity % kChunk == 0,
             "sn_jpeg_enc_write: raw_capacity = %ld: a multiple of %d, at least the bound %ld (%d bytes per block and one, rounded up to %d, per picture)",
             raw_capacity, kChunk, bound, kJpegEncRawBytesPerBlock, kChunk);
  hipLaunchKernelGGL(jpeg_enc_write_kernel, dim3(grid_of(n_blocks)), dim3(kThreads), 0, sn_stream(stream), coef, hw, blk_off, I,
                     (long long)n_blocks, ncomp, sampling, bit_excl, pic_first_bit, chunk_off, raw, (long long)(raw_capacity / 4), status);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_jpeg_enc_stuff(const uint32_t *raw, long raw_capacity, const int64_t *chunk_off, const int64_t *raw_len, int I, long n_chunks,
                                int phase, int32_t *cnt, const int64_t *out_pos, uint8_t *out, long capacity, sn_stream_t stream) {
  SN_REQUIRE(raw && chunk_off && raw_len, "sn_jpeg_enc_stuff: null pointer");
  SN_REQUIRE(phase == 1 || phase == 2, "sn_jpeg_enc_stuff: phase = %d: 1 (count) or 2 (write)", phase);
  SN_REQUIRE(phase == 1 ? cnt != nullptr : (out_pos && out), "sn_jpeg_enc_stuff: null pointer (phase 1 needs cnt, phase 2 out_pos and out)");
  SN_REQUIRE(I >= 1 && I <= kMaxPictures, "sn_jpeg_enc_stuff: 1 <= I <= %d required (I = %d)", kMaxPictures, I);
  SN_REQUIRE(n_chunks >= 1 && n_chunks <= 4 * kMaxBlocks + kMaxPictures, "sn_jpeg_enc_stuff: n_chunks = %ld: 1 .. %ld", n_chunks,
             4 * kMaxBlocks + kMaxPictures);
  SN_REQUIRE(raw_capacity >= n_chunks * kChunk, "sn_jpeg_enc_stuff: raw_capacity = %ld is below n_chunks * %d = %ld", raw_capacity, kChunk,
             n_chunks * kChunk);
  SN_REQUIRE(phase == 1 || capacity >= 2 * n_chunks * kChunk, "sn_jpeg_enc_stuff: capacity = %ld is below the bound %ld (two bytes per raw byte)",
             capacity, 2 * n_chunks * kChunk);
  if (phase == 1)
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel<1>, dim3(grid_of(n_chunks)), dim3(kThreads), 0, sn_stream(stream), raw, (long long)(raw_capacity / 4),
                       chunk_off, raw_len, I, (long long)n_chunks, cnt, out_pos, out, (long long)capacity);
  else
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel<2>, dim3(grid_of(n_chunks)), dim3(kThreads), 0, sn_stream(stream), raw, (long long)(raw_capacity / 4),
                       chunk_off, raw_len, I, (long long)n_chunks, cnt, out_pos, out, (long long)capacity);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
