// png_decode.hip -- zlib streams inflated on the device, and PNG files on top of that: the counterpart of
// png_encode.hip.  Integer arithmetic, exact bytes, the same every run; no global atomics, plain vector stores.
//
//   inflate_kernel        one wave (a workgroup of 64 lanes) per stream.  Every lane runs the decoder of inflate_code.h with the same
//                         values -- Huffman decoding is serial inside a stream -- and the wave as a whole does the copies: the last
//                         32 KiB of the output are a ring in LDS, a match reads the ring and writes the ring (up to 5 bytes per lane,
//                         all reads before all writes: a distance near 32768 makes source and destination share ring slots), and the
//                         ring is stored to HBM 16 KiB at a time, four bytes per lane, with the Adler-32 of those bytes summed on the
//                         way.  A copy therefore never reads global memory that another lane stored: LDS operations of one wave
//                         are executed in order, and the workgroup barrier (one wave: no s_barrier, only the ordering) keeps the
//                         compiler from moving them.
//   png_unfilter_kernel   one wave per image, in place in the inflated bytes: a diagonal front over a band of 64 rows -- lane k works
//                         on row r0 + k and is one pixel behind lane k - 1, so the pixel above comes from the neighbour lane by a
//                         shuffle and the pixel to the left is the lane's own last result; lane 0 reads the last row of the band
//                         before from memory (stored by lane 63, made visible by the barrier between two bands).
//   png_expand_kernel     one thread per output pixel: BGR pixels as PIL's convert('RGB') gives them, or palette / grey indices.
#include "common.h"
#include "inflate_code.h"

namespace {

constexpr int kMaxStreams = 65535;
constexpr int kMaxStreamBytes = 1 << 30;        // of a stream and of its output: positions are 32-bit
constexpr int kRing = kInflateWindow;           // 32768
constexpr int kRingMask = kRing - 1;
constexpr int kFlush = 16384;                   // the ring is stored once this many bytes wait
constexpr int kTabFields = 4;                   // in_off, in_len, out_off, out_cap (int64)
constexpr int kImgFields = 8;                   // w, h, depth, colour type, row bytes, bpp, palette entries, 0
constexpr int kMaxImages = 65535;
constexpr int kMaxSide = 1 << 20;
// status bits beyond those of inflate_code.h
constexpr int kStatusFilter = 1024;             // a filter type above 4
constexpr int kStatusLength = 2048;             // the stream inflated to another length than h * (row bytes + 1)
static_assert(kFlush + kInflateMaxMatch + kInflateRawPiece <= kRing, "bytes that wait for their store are never overwritten");
static_assert((kInflateMaxMatch + kWave - 1) / kWave == 5, "a match is at most 5 bytes per lane");

struct InflateLds {
  alignas(16) uint8_t ring[kRing];
  SnInflateTables T;
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
  return v;
}

// the sink of inflate_code.h for a wave: pos / flushed / the sums are the same in every lane
struct WaveSink {
  uint8_t *ring;       // LDS
  uint8_t *out;        // global, `cap` bytes
  int cap, n, flushed, lane;
  uint32_t a, b;

  __device__ __forceinline__ int pos() const { return n; }

  // ring bytes [flushed, n) -> out, and into the Adler-32; at most kFlush + 258 + 256 of them
  __device__ __forceinline__ void flush() {
    __syncthreads();
    const int f = flushed, e = n;
    uint32_t la = 0, lb = 0;
    for (int base = (f & ~3) + 4 * lane; base < e; base += 4 * kWave) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(ring + (base & kRingMask));
      const bool whole = base >= f && base + 4 <= e;
      if (whole && ((reinterpret_cast<uintptr_t>(out + base) & 3) == 0)) {
        *reinterpret_cast<uint32_t *>(out + base) = w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (base + j >= f && base + j < e) out[base + j] = (uint8_t)(w >> (8 * j));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (base + j >= f && base + j < e) {
          const uint32_t v = (w >> (8 * j)) & 255u;
          la += v;
          lb += v * (uint32_t)(e - (base + j));
        }
      }
    }
    // per lane: <= 268 bytes of weight <= 16898 -> lb < 2^31
    const uint32_t sa = wave_sum(la), sb = wave_sum(lb % kAdlerBase);
    b = (uint32_t)((b + (uint64_t)(uint32_t)(e - f) * a + sb) % kAdlerBase);
    a = (a + sa) % kAdlerBase;
    flushed = e;
    __syncthreads();          // the ring slots just read may be written again
  }

  __device__ __forceinline__ bool literal(int v) {
    if (n >= cap) return false;
    if (lane == 0) ring[n & kRingMask] = (uint8_t)v;
    n += 1;
    if (n - flushed >= kFlush) flush();
    return true;
  }

  __device__ __forceinline__ bool match(int len, int dist) {
    if (len > cap - n) return false;
    __syncthreads();          // the bytes other lanes stored
    uint8_t t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = lane + kWave * k;
      t[k] = 0;
      if (i < len) t[k] = ring[(n - dist + (dist < len ? i % dist : i)) & kRingMask];
    }
    __syncthreads();          // all reads before any write: at a distance near the ring's size they share slots
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = lane + kWave * k;
      if (i < len) ring[(n + i) & kRingMask] = t[k];
    }
    n += len;
    if (n - flushed >= kFlush) flush();
    return true;
  }

  __device__ __forceinline__ bool raw(const uint8_t *src, int k) {
    if (k > cap - n) return false;
    for (int i = lane; i < k; i += kWave) ring[(n + i) & kRingMask] = src[i];
    n += k;
    if (n - flushed >= kFlush) flush();
    return true;
  }

  __device__ __forceinline__ uint32_t adler() {
    flush();
    return (b << 16) | a;
  }
};

__global__ __launch_bounds__(kWave) void inflate_kernel(const uint8_t *__restrict__ data, long long total_in,
                                                        const int64_t *__restrict__ tab, int S, uint8_t *__restrict__ out,
                                                        long long out_total, int32_t *__restrict__ meta) {
  __shared__ InflateLds L;
  const int s = blockIdx.x;
  if (s >= S) return;
  long long in_off = tab[kTabFields * s + 0], in_len = tab[kTabFields * s + 1];
  long long out_off = tab[kTabFields * s + 2], out_cap = tab[kTabFields * s + 3];
  // whatever the table holds, the stream and its output stay inside the two buffers
  in_off = in_off < 0 ? 0 : (in_off > total_in ? total_in : in_off);
  in_len = in_len < 0 ? 0 : (in_len > total_in - in_off ? total_in - in_off : in_len);
  out_off = out_off < 0 ? 0 : (out_off > out_total ? out_total : out_off);
  out_cap = out_cap < 0 ? 0 : (out_cap > out_total - out_off ? out_total - out_off : out_cap);
  if (in_len > kMaxStreamBytes) in_len = kMaxStreamBytes;
  if (out_cap > kMaxStreamBytes) out_cap = kMaxStreamBytes;
  WaveSink sink;
  sink.ring = L.ring;
  sink.out = out + out_off;
  sink.cap = (int)out_cap;
  sink.n = 0;
  sink.flushed = 0;
  sink.lane = threadIdx.x;
  sink.a = 1;
  sink.b = 0;
  const int status = sn_inflate_zlib(data + in_off, (int)in_len, sink, L.T);
  if (status && sink.flushed < sink.n) sink.flush();          // what a damaged stream gave before its damage
  if (threadIdx.x == 0) {
    meta[2 * s + 0] = sink.n;
    meta[2 * s + 1] = status;
  }
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the rows of one image, in place; returns 1 where a row has a filter type above 4 (taken as 0)
template <int BPP>
__device__ int unfilter_image(uint8_t *__restrict__ raw, int h, int rowbytes, int lane) {
  constexpr int W = (BPP + 3) / 4;
  const int wpx = rowbytes / BPP;
  const long long pitch = (long long)rowbytes + 1;
  int bad = 0;
  for (int r0 = 0; r0 < h; r0 += kWave) {
    __syncthreads();          // the band before is stored: lane 0 reads its last row
    const int r = r0 + lane;
    const bool live = r < h;
    uint8_t *row = raw + (long long)(live ? r : 0) * pitch;
    int ft = live ? row[0] : 0;
    if (ft > 4) {
      bad = 1;
      ft = 0;
    }
    const uint8_t *above = raw + (long long)(r0 > 0 ? r0 - 1 : 0) * pitch + 1;
    const int rows = h - r0 < kWave ? h - r0 : kWave;
    uint32_t a[W], c[W];
#pragma unroll
    for (int k = 0; k < W; ++k) a[k] = c[k] = 0;
    for (int t = 0; t < wpx + rows - 1; ++t) {
      const int x = t - lane;
      const bool on = live && x >= 0 && x < wpx;
      uint32_t b[W];
#pragma unroll
      for (int k = 0; k < W; ++k) b[k] = (uint32_t)__shfl_up((int)a[k], 1, kWave);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) b[k] = 0;
        if (on && r0 > 0) {
#pragma unroll
          for (int j = 0; j < BPP; ++j) b[j >> 2] |= (uint32_t)above[(long long)x * BPP + j] << (8 * (j & 3));
        }
      }
      if (on) {
        uint32_t o[W];
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] = 0;
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int sh = 8 * (j & 3);
          const int v = row[1 + (long long)x * BPP + j];
          const int pa = (a[j >> 2] >> sh) & 255, pb = (b[j >> 2] >> sh) & 255, pc = (c[j >> 2] >> sh) & 255;
          const int pred = ft == 0 ? 0 : ft == 1 ? pa : ft == 2 ? pb : ft == 3 ? ((pa + pb) >> 1) : paeth(pa, pb, pc);
          const int res = (v + pred) & 255;
          row[1 + (long long)x * BPP + j] = (uint8_t)res;
          o[j >> 2] |= (uint32_t)res << sh;
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
          a[k] = o[k];
          c[k] = b[k];
        }
      }
    }
  }
  return bad;
}

__global__ __launch_bounds__(kWave) void png_unfilter_kernel(uint8_t *__restrict__ raw, long long raw_total, const int32_t *__restrict__ img,
                                                             const int64_t *__restrict__ raw_off, int I, int32_t *__restrict__ meta) {
  const int i = blockIdx.x;
  if (i >= I) return;
  const int h = img[kImgFields * i + 1], rowbytes = img[kImgFields * i + 4], bpp = img[kImgFields * i + 5];
  const long long off = raw_off[i], need = (long long)h * ((long long)rowbytes + 1);
  int status = meta[2 * i + 1];
  const int got = meta[2 * i + 0];
  __syncthreads();          // every lane has read the status before lane 0 writes it
  if (status == 0 && (long long)got != need) status = kStatusLength;
  if (status == 0 && (h < 1 || rowbytes < 1 || off < 0 || off + need > raw_total || rowbytes % bpp)) status = kStatusLength;
  if (status == 0) {
    uint8_t *p = raw + off;
    const int lane = threadIdx.x;
    int bad = 0;
    switch (bpp) {
      case 1: bad = unfilter_image<1>(p, h, rowbytes, lane); break;
      case 2: bad = unfilter_image<2>(p, h, rowbytes, lane); break;
      case 3: bad = unfilter_image<3>(p, h, rowbytes, lane); break;
      case 4: bad = unfilter_image<4>(p, h, rowbytes, lane); break;
      case 6: bad = unfilter_image<6>(p, h, rowbytes, lane); break;
      case 8: bad = unfilter_image<8>(p, h, rowbytes, lane); break;
      default: bad = 1; break;
    }
    if (__any(bad)) status = kStatusFilter;
  }
  if (threadIdx.x == 0) meta[2 * i + 1] = status;
}

// mode 0: (h, w, 3) BGR; mode 1: (h, w) indices (palette: the index; grey: the sample scaled to 8 bits)
__global__ __launch_bounds__(256) void png_expand_kernel(const uint8_t *__restrict__ raw, const int32_t *__restrict__ img,
                                                         const int64_t *__restrict__ raw_off, const uint8_t *__restrict__ pal,
                                                         const uint64_t *__restrict__ out_ptrs, const int32_t *__restrict__ meta, int mode) {
  const int i = blockIdx.y;
  if (meta[2 * i + 1] != 0) return;
  const int w = img[kImgFields * i + 0], h = img[kImgFields * i + 1], depth = img[kImgFields * i + 2], ctype = img[kImgFields * i + 3];
  const int rowbytes = img[kImgFields * i + 4], plen = img[kImgFields * i + 6];
  const long long pixels = (long long)w * h;
  const uint8_t *src = raw + raw_off[i];
  uint8_t *dst = reinterpret_cast<uint8_t *>(out_ptrs[i]);
  const int channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    const uint8_t *row = src + (long long)y * (rowbytes + 1) + 1;
    int r, g = 0, b = 0;
    if (depth < 8) {          // grey or palette, samples packed high bits first
      const int bit = x * depth;
      const int v = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
      r = v;
    } else {
      const int step = depth >> 3;          // the high byte of a 16-bit sample comes first
      const uint8_t *q = row + (long long)x * channels * step;
      r = q[0];
      g = channels >= 3 ? q[step] : r;
      b = channels >= 3 ? q[2 * step] : r;
    }
    if (ctype == 3) {
      if (mode == 1) {
        dst[p] = (uint8_t)r;
        continue;
      }
      const int idx = r;
      r = idx < plen ? pal[768 * i + 3 * idx + 0] : 0;
      g = idx < plen ? pal[768 * i + 3 * idx + 1] : 0;
      b = idx < plen ? pal[768 * i + 3 * idx + 2] : 0;
    } else if (ctype == 0 || ctype == 4) {
      if (depth < 8) r *= depth == 1 ? 255 : depth == 2 ? 85 : 17;
      g = b = r;
      if (mode == 1) {
        dst[p] = (uint8_t)r;
        continue;
      }
    }
    dst[3 * p + 0] = (uint8_t)b;
    dst[3 * p + 1] = (uint8_t)g;
    dst[3 * p + 2] = (uint8_t)r;
  }
}

// the channels of a colour type, or 0
int channels_of(int ctype) { return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0; }

// h_img (HOST, I x 8) and h_raw_off (HOST, I): what is wrong with image i, or nullptr
const char *bad_image(const int32_t *f, long long off, long long raw_total, long long prev_end, int mode) {
  const long long w = f[0], h = f[1];
  const int depth = f[2], ctype = f[3], ch = channels_of(ctype);
  if (w < 1 || h < 1 || w > kMaxSide || h > kMaxSide || w * h >= (1LL << 29)) return "1 <= w, h <= 2^20 and w * h < 2^29 required";
  if (!ch) return "the colour type is none of 0, 2, 3, 4, 6";
  const bool ok = ctype == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                  : ctype == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                  : ctype == 4 ? depth == 8
                               : (depth == 8 || depth == 16);
  if (!ok) return "the bit depth is not one the colour type is decoded at";
  if (mode == 1 && ctype != 0 && ctype != 3) return "index mode takes grey and palette images";
  const long long rowbytes = (w * ch * depth + 7) / 8;
  if (f[4] != rowbytes) return "row bytes are not ceil(w * channels * depth / 8)";
  const int bpp = ch * depth / 8 < 1 ? 1 : ch * depth / 8;
  if (f[5] != bpp) return "bpp is not max(1, channels * depth / 8)";
  if (f[6] < 0 || f[6] > 256) return "0 <= palette entries <= 256 required";
  const long long need = h * (rowbytes + 1);
  if (need > kMaxStreamBytes) return "h * (row bytes + 1) is above the largest stream";
  if (off < prev_end || off + need > raw_total) return "the raw offsets overlap or pass raw_total";
  return nullptr;
}

}  // namespace

SN_EXPORT int sn_inflate_limits(int32_t *h_out6) {
  SN_REQUIRE(h_out6, "sn_inflate_limits: null pointer");
  h_out6[0] = kMaxStreams;
  h_out6[1] = kMaxStreamBytes;
  h_out6[2] = (int32_t)sizeof(InflateLds);
  h_out6[3] = kRing;
  h_out6[4] = kWave;
  h_out6[5] = kFlush;
  return SN_OK;
}

SN_EXPORT int sn_inflate(const uint8_t *data, long total_in, const int64_t *tab, const int64_t *h_tab, long S, uint8_t *out, long out_total,
                         int32_t *meta, sn_stream_t stream) {
  SN_REQUIRE(tab && h_tab && meta && (data || total_in == 0) && (out || out_total == 0), "sn_inflate: null pointer");
  SN_REQUIRE(S >= 1 && S <= kMaxStreams, "sn_inflate: 1 <= S <= %d required (S = %ld)", kMaxStreams, S);
  SN_REQUIRE(total_in >= 0 && total_in < (1L << 40), "sn_inflate: 0 <= total_in < 2^40 required (total_in = %ld)", total_in);
  SN_REQUIRE(out_total >= 0 && out_total < (1L << 40), "sn_inflate: 0 <= out_total < 2^40 required (out_total = %ld)", out_total);
  long prev_end = 0;
  for (long s = 0; s < S; ++s) {
    const long in_off = (long)h_tab[kTabFields * s + 0], in_len = (long)h_tab[kTabFields * s + 1];
    const long out_off = (long)h_tab[kTabFields * s + 2], out_cap = (long)h_tab[kTabFields * s + 3];
    SN_REQUIRE(in_off >= 0 && in_len >= 0 && in_len <= kMaxStreamBytes && in_off + in_len <= total_in,
               "sn_inflate: stream %ld lies at %ld + %ld: inside total_in = %ld and at most %d bytes required", s, in_off, in_len, total_in,
               kMaxStreamBytes);
    SN_REQUIRE(out_cap >= 0 && out_cap <= kMaxStreamBytes && out_off >= prev_end && out_off + out_cap <= out_total,
               "sn_inflate: the output of stream %ld lies at %ld + %ld: behind the output before it, inside out_total = %ld and at most %d "
               "bytes required",
               s, out_off, out_cap, out_total, kMaxStreamBytes);
    prev_end = out_off + out_cap;
  }
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)S), dim3(kWave), 0, sn_stream(stream), data, (long long)total_in, tab, (int)S, out,
                     (long long)out_total, meta);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

#define SN_PNG_IMAGES(fn, mode)                                                                                                      \
  SN_REQUIRE(I >= 1 && I <= kMaxImages, fn ": 1 <= I <= %d required (I = %d)", kMaxImages, I);                                       \
  SN_REQUIRE(raw_total >= 0 && raw_total < (1L << 40), fn ": 0 <= raw_total < 2^40 required (raw_total = %ld)", raw_total);          \
  do {                                                                                                                               \
    long long end__ = 0;                                                                                                             \
    for (int i = 0; i < I; ++i) {                                                                                                    \
      const char *why__ = bad_image(h_img + kImgFields * i, h_raw_off[i], raw_total, end__, mode);                                   \
      SN_REQUIRE(!why__, fn ": image %d: %s", i, why__);                                                                             \
      end__ = h_raw_off[i] + (long long)h_img[kImgFields * i + 1] * ((long long)h_img[kImgFields * i + 4] + 1);                      \
    }                                                                                                                                \
  } while (0)

SN_EXPORT int sn_png_unfilter(uint8_t *raw, long raw_total, const int32_t *img, const int32_t *h_img, const int64_t *raw_off,
                              const int64_t *h_raw_off, int I, int32_t *meta, sn_stream_t stream) {
  SN_REQUIRE(raw && img && h_img && raw_off && h_raw_off && meta, "sn_png_unfilter: null pointer");
  SN_PNG_IMAGES("sn_png_unfilter", 0);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)I), dim3(kWave), 0, sn_stream(stream), raw, (long long)raw_total, img, raw_off, I,
                     meta);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_png_expand(const uint8_t *raw, long raw_total, const int32_t *img, const int32_t *h_img, const int64_t *raw_off,
                            const int64_t *h_raw_off, int I, const uint8_t *pal, const uint64_t *out_ptrs, const int32_t *meta, int mode,
                            sn_stream_t stream) {
  SN_REQUIRE(raw && img && h_img && raw_off && h_raw_off && pal && out_ptrs && meta, "sn_png_expand: null pointer");
  SN_REQUIRE(mode == 0 || mode == 1, "sn_png_expand: mode 0 (BGR) or 1 (indices) required (mode = %d)", mode);
  SN_PNG_IMAGES("sn_png_expand", mode);
  long long most = 1;
  for (int i = 0; i < I; ++i) {
    const long long px = (long long)h_img[kImgFields * i] * h_img[kImgFields * i + 1];
    if (px > most) most = px;
  }
  hipLaunchKernelGGL(png_expand_kernel, dim3((unsigned)sn_blocks((long)most, 4096), (unsigned)I), dim3(256), 0, sn_stream(stream), raw, img,
                     raw_off, pal, out_ptrs, meta, mode);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
