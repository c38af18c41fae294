// png_encode.hip -- PNG row filters and a run-match deflate coder on the device: what turns a rendered batch
// (render.hip) into the bytes of PNG files without the raw pictures leaving HBM.  Integer arithmetic, exact bytes, the same every run.
//
//   png_filter_kernel     one wave per picture row: the five PNG filters (bpp = 3), the sum of min(v, 256 - v) of each over the row
//                         by wave reductions, the smallest sum wins (ties: the lowest type); the row is written as type byte + bytes.
//   deflate_plan_kernel   blk_first (S+1): the running count of kBlock-byte blocks over the streams (an empty stream has one block).
//   deflate_code_kernel   one workgroup per block: bytes into LDS, run boundaries as a bit per byte, tokens (below) counted into an LDS
//                         histogram, Adler-32 partial sums; then the code: a rank sort of the 286 frequencies by the workgroup, and ONE
//                         lane builds the length-limited code (huff_code.h), the code-length code and the block header.  The block's
//                         coded size decides dynamic (BTYPE 2) or stored (BTYPE 0).
//   deflate_write_kernel  one workgroup per block at the byte offset the caller's scan of the sizes gives: the tokens again, their bit
//                         lengths scanned over the workgroup, bits OR-ed into an LDS image of the block, the image stored as bytes.
//                         The first block of a stream writes the zlib header, the last one combines the stream's Adler-32.
// Tokens: inside a block the maximal runs of equal bytes are independent.  A run [s, e) gives a literal at s; the remaining
// Q = e - s - 1 bytes are cut into pieces of 258 from the left; a piece of 3 or more bytes is one match (its length, distance 1), a
// piece of 1 or 2 bytes is that many literals.  This IS the greedy left-to-right scan of DESIGN.md section 29 (at p, L = bytes from p equal to
// byte p - 1, capped at 258 and the block end; L >= 3 -> match), stated per byte so that every lane decides for its own bytes.
// No global atomics, no scratch; plain vector stores.
#include "common.h"
#include "eval_order.h"
#include "huff_code.h"

namespace {

constexpr int kBlock = 32768;              // bytes of input per deflate block
constexpr int kThreads = 512;
constexpr int kChunk = kBlock / kThreads;  // 64 contiguous bytes per thread: one 64-bit word of run-start flags
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxStreams = 65535;
constexpr int kLitSyms = kDeflateLitSyms;
constexpr int kHdrWords = kDeflateHdrWords;
// a block's record in blk_code (uint32 words)
constexpr int kRecCodes = 0;               // 286 x (reversed code | length << 16)
constexpr int kRecHdr = 288;               // kHdrWords of header bits
constexpr int kRecHdrBits = 360;
constexpr int kRecMode = 361;              // 0 stored, 1 dynamic
constexpr int kRecAdlerA = 362;            // sum of the bytes, modulo 65521
constexpr int kRecAdlerB = 363;            // sum of (len - p) * byte p, modulo 65521
constexpr int kRecSize = 364;              // the block's bytes in the stream (without zlib header and Adler-32)
constexpr int kRecWords = 368;
constexpr unsigned kAdler = 65521u;
constexpr int kFilterWaves = 4;            // rows per workgroup of the filter kernel
static_assert(kChunk == 64 && kBlock >= 8192 && kBlock <= 65535, "one flag word per thread; a stored block holds at most 65535 bytes");

struct BlockAt {
  int stream, first, last, len;
  long long start;
};

// which stream block b belongs to: the last s with blk_first[s] <= b (17 steps for S <= 65535); everything clamped into the buffers
__device__ __forceinline__ BlockAt locate(const int64_t *__restrict__ offsets, const int32_t *__restrict__ blk_first, int S, int b) {
  int lo = 0, hi = S - 1;
  for (int it = 0; it < 17; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (lo < hi) {
      if (blk_first[mid] <= b) lo = mid; else hi = mid - 1;
    }
  }
  BlockAt a;
  a.stream = lo;
  const int j = max(b - blk_first[lo], 0);
  const long long o0 = offsets[lo], o1 = max((long long)offsets[lo + 1], o0);
  a.start = min(o0 + (long long)j * kBlock, o1);
  a.len = (int)min((long long)kBlock, o1 - a.start);
  a.first = j == 0;
  a.last = b + 1 >= blk_first[lo + 1];
  return a;
}

// the block's bytes into LDS words (zero past len): aligned dword loads, shifted where the block starts off a dword.  A dword is
// read only when it holds at least one byte of the block.
__device__ __forceinline__ void load_block(const uint8_t *__restrict__ g, int len, uint32_t *__restrict__ words) {
  const int mis = (int)((uintptr_t)g & 3);
  const uint32_t *G = reinterpret_cast<const uint32_t *>(g - mis);
  for (int w = threadIdx.x; w < kBlock / 4 + 1; w += kThreads) {
    uint32_t v = 0;
    if (4 * w < len) {
      const uint32_t lo = G[w];
      v = lo;
      if (mis) {
        const uint32_t hi = 4 * w + 4 - mis < len ? G[w + 1] : 0u;
        v = (lo >> (8 * mis)) | (hi << (32 - 8 * mis));
      }
      const int left = len - 4 * w;
      if (left < 4) v &= (1u << (8 * left)) - 1u;
    }
    words[w] = v;
  }
}

struct Runs {
  unsigned long long m;      // bit i: byte c0 + i starts a run
  int s_before, e_after;     // the last run start before this chunk; the first run start after it, or len
};

// run-start flags of the block (byte 0, and every byte that differs from the one before it), then the two scans over the chunks
__device__ __forceinline__ Runs find_runs(const uint32_t *__restrict__ words, int len, uint32_t *__restrict__ flags /* 2 * kThreads */,
                                          int *__restrict__ wave_a, int *__restrict__ wave_b) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
  for (int i = tid; i < 2 * kThreads; i += kThreads) flags[i] = 0;
  __syncthreads();
  for (int w = tid; w < kBlock / 4; w += kThreads) {
    if (4 * w >= len) break;
    const uint32_t v = words[w];
    const uint32_t prev = w ? (uint32_t)bytes[4 * w - 1] : (~v & 0xffu);
    const uint32_t shifted = (v << 8) | prev;
    const uint32_t x = v ^ shifted;
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (((x >> (8 * k)) & 0xffu) && 4 * w + k < len) f |= 1u << k;
    if (f) atomicOr(&flags[w >> 3], f << (4 * (w & 7)));
  }
  __syncthreads();
  Runs r;
  r.m = (unsigned long long)flags[2 * tid] | ((unsigned long long)flags[2 * tid + 1] << 32);
  const int c0 = tid * kChunk;
  const int lastS = r.m ? c0 + 63 - __clzll((long long)r.m) : -1;
  const int firstS = r.m ? c0 + __ffsll((long long)r.m) - 1 : len;
  int a = lastS, b = firstS;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int oa = __shfl_up(a, off, 64), ob = __shfl_down(b, off, 64);
    if (lane >= off) a = max(a, oa);
    if (lane + off < kWave) b = min(b, ob);
  }
  if (lane == kWave - 1) wave_a[wave] = a;
  if (lane == 0) wave_b[wave] = b;
  int ea = __shfl_up(a, 1, 64), eb = __shfl_down(b, 1, 64);
  if (lane == 0) ea = -1;
  if (lane == kWave - 1) eb = len;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) ea = max(ea, wave_a[w]);
    if (w > wave) eb = min(eb, wave_b[w]);
  }
  r.s_before = ea;
  r.e_after = eb;
  return r;
}

// the length symbol (257 + code) of a match length 3 .. 258, its extra bits and their count
__device__ __forceinline__ int length_symbol(int L, int &extra, int &nextra) {
  if (L == 258) {
    extra = nextra = 0;
    return 285;
  }
  const int l = L - 3;
  if (l < 8) {
    extra = nextra = 0;
    return 257 + l;
  }
  nextra = 29 - __clz(l);                     // floor(log2 l) - 2
  extra = l & ((1 << nextra) - 1);
  return 257 + 4 * nextra + 4 + ((l >> nextra) & 3);
}

// the tokens that start in this thread's chunk, in order: f(byte, 0) for a literal, f(0, L) for a match
template <class F>
__device__ __forceinline__ void for_tokens(const uint8_t *__restrict__ bytes, int len, const Runs r, F f) {
  const int c0 = threadIdx.x * kChunk;
  const int hi = min(c0 + kChunk, len);
  for (int p = c0; p < hi; ++p) {
    const int i = p - c0;
    if ((r.m >> i) & 1ull) {
      f((int)bytes[p], 0);
      continue;
    }
    const unsigned long long below = r.m & ((1ull << i) - 1ull);
    const unsigned long long above = i < 63 ? (r.m >> (i + 1)) : 0ull;
    const int s = below ? c0 + 63 - __clzll((long long)below) : r.s_before;
    const int e = above ? p + __ffsll((long long)above) : r.e_after;
    const int k = p - s - 1, Q = e - s - 1;
    const int rr = k % 258;
    const int piece = min(258, Q - (k - rr));
    if (piece < 3)
      f((int)bytes[p], 0);
    else if (rr == 0)
      f(0, piece);
  }
}

struct CodeLds {
  uint32_t words[kBlock / 4 + 1];
  uint32_t flags[2 * kThreads];
  SnBlockCode code;
  uint32_t red[2 * kWaves];
  int wave_a[kWaves], wave_b[kWaves];
};

__global__ __launch_bounds__(kThreads) void deflate_plan_kernel(const int64_t *__restrict__ offsets, int S, int32_t *__restrict__ blk_first) {
  const int lane = threadIdx.x;
  int carry = 0;
  if (lane == 0) blk_first[0] = 0;
  for (int base = 0; base < S; base += kWave) {
    const int s = base + lane;
    int nb = 0;
    if (s < S) {
      const long long n = max((long long)(offsets[s + 1] - offsets[s]), 0ll);
      nb = n ? (int)((n + kBlock - 1) / kBlock) : 1;
    }
    const int inc = wave_scan_add(nb, lane);
    if (s < S) blk_first[s + 1] = carry + inc;
    carry += __shfl(inc, kWave - 1, 64);
  }
}

__global__ __launch_bounds__(kThreads) void deflate_code_kernel(const uint8_t *__restrict__ data, const int64_t *__restrict__ offsets,
                                                                const int32_t *__restrict__ blk_first, int S,
                                                                uint32_t *__restrict__ blk_code, int64_t *__restrict__ blk_size) {
  __shared__ CodeLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const BlockAt at = locate(offsets, blk_first, S, b);
  const int len = at.len;
  uint32_t *rec = blk_code + (size_t)b * kRecWords;
  load_block(data + at.start, len, L.words);
  SnBlockCode &C = L.code;
  for (int i = tid; i < kHuffMaxSyms; i += kThreads) {
    C.hist[i] = 0;
    C.lens[i] = 0;
  }
  if (tid < 32) C.chist[tid] = 0;
  if (tid < kHdrWords) C.hdr[tid] = 0;
  if (tid == 0) C.n_used = 0;
  __syncthreads();
  const Runs r = find_runs(L.words, len, L.flags, L.wave_a, L.wave_b);
  const uint8_t *bytes = reinterpret_cast<const uint8_t *>(L.words);
  for_tokens(bytes, len, r, [&](int lit, int mlen) {
    int extra, nextra;
    atomicAdd(&C.hist[mlen ? length_symbol(mlen, extra, nextra) : lit], 1u);
  });
  if (tid == 0) atomicAdd(&C.hist[256], 1u);
  // Adler-32 partial sums, exact: each lane's terms fit 64 bits, the lanes' residues fit 32
  unsigned long long sa = 0, sb = 0;
  for (int w = tid; w < kBlock / 4; w += kThreads) {
    if (4 * w >= len) break;
    const uint32_t v = L.words[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned d = (v >> (8 * k)) & 0xffu;
      sa += d;
      sb += (unsigned long long)d * (unsigned)max(len - (4 * w + k), 0);
    }
  }
  unsigned ra = (unsigned)(sa % kAdler), rb = (unsigned)(sb % kAdler);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ra += __shfl_xor(ra, off, 64);
    rb += __shfl_xor(rb, off, 64);
  }
  if (lane == 0) {
    L.red[2 * wave] = ra % kAdler;
    L.red[2 * wave + 1] = rb % kAdler;
  }
  __syncthreads();
  // rank of every symbol that occurs, by (frequency, symbol): the order the code construction is stated in
  if (tid < kLitSyms && C.hist[tid]) {
    const uint32_t h = C.hist[tid];
    int rank = 0;
    for (int j = 0; j < kLitSyms; ++j) {
      const uint32_t hj = C.hist[j];
      rank += (hj != 0) & ((hj < h) | ((hj == h) & (j < tid)));
    }
    C.fs[rank] = h;
    C.order[rank] = (uint16_t)tid;
    atomicAdd(&C.n_used, 1);
  }
  __syncthreads();
  if (tid == 0) {
    int hb = 0;
    const unsigned long long bits = sn_deflate_block_code(C, at.last, hb);
    // a block that is not the last of its stream ends with an empty stored block, which brings the stream to a byte boundary
    const long long dyn = at.last ? (long long)((bits + 7) >> 3) : (long long)((bits + 3 + 7) >> 3) + 4;
    const int mode = (len > 0 && dyn <= (long long)len + 5) ? 1 : 0;
    const long long size = mode ? dyn : (long long)len + 5;
    unsigned a = 0, bsum = 0;
    for (int w = 0; w < kWaves; ++w) {
      a += L.red[2 * w];
      bsum += L.red[2 * w + 1];
    }
    rec[kRecHdrBits] = (uint32_t)hb;
    rec[kRecMode] = (uint32_t)mode;
    rec[kRecAdlerA] = a % kAdler;
    rec[kRecAdlerB] = bsum % kAdler;
    rec[kRecSize] = (uint32_t)size;
    blk_size[b] = size + (at.first ? 2 : 0) + (at.last ? 4 : 0);
  }
  __syncthreads();
  for (int i = tid; i < kLitSyms; i += kThreads) rec[kRecCodes + i] = (uint32_t)C.codes[i] | ((uint32_t)C.lens[i] << 16);
  if (tid < kHdrWords) rec[kRecHdr + tid] = C.hdr[tid];
}

// dynamic LDS of the write kernel
struct WriteLds {
  uint32_t words[kBlock / 4 + 1];
  uint32_t image[kBlock / 4 + 4];
  uint32_t flags[2 * kThreads];
  uint32_t codes[kHuffMaxSyms];
  int wave_a[kWaves], wave_b[kWaves];
  int wave_bits[kWaves];
};

__device__ __forceinline__ void or_bits(uint32_t *__restrict__ image, int &at, uint32_t v, int n) {
  const int w = at >> 5, sh = at & 31;
  atomicOr(&image[w], v << sh);
  if (sh + n > 32) atomicOr(&image[w + 1], v >> (32 - sh));
  at += n;
}

__global__ __launch_bounds__(kThreads) void deflate_write_kernel(const uint8_t *__restrict__ data, const int64_t *__restrict__ offsets,
                                                                 const int32_t *__restrict__ blk_first, int S,
                                                                 const uint32_t *__restrict__ blk_code, const int64_t *__restrict__ blk_pos,
                                                                 uint8_t *__restrict__ out, long long capacity) {
  extern __shared__ __align__(16) unsigned char smem[];
  WriteLds &L = *reinterpret_cast<WriteLds *>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const BlockAt at = locate(offsets, blk_first, S, b);
  const int len = at.len;
  const uint32_t *rec = blk_code + (size_t)b * kRecWords;
  const int mode = (int)rec[kRecMode];
  const long long size = min((long long)rec[kRecSize], (long long)len + 5);
  long long o = blk_pos[b];
  auto store = [&](long long pos, unsigned v) {
    if (pos >= 0 && pos < capacity) out[pos] = (uint8_t)v;
  };
  if (at.first) {
    if (tid == 0) {
      store(o, 0x78);
      store(o + 1, 0x01);
    }
    o += 2;
  }
  if (!mode) {
    const uint8_t *g = data + at.start;
    if (tid == 0) {
      store(o, at.last ? 1u : 0u);
      store(o + 1, (unsigned)len & 0xffu);
      store(o + 2, (unsigned)len >> 8);
      store(o + 3, ~(unsigned)len & 0xffu);
      store(o + 4, (~(unsigned)len >> 8) & 0xffu);
    }
    for (int i = tid; i < len; i += kThreads) store(o + 5 + i, g[i]);
  } else {
    load_block(data + at.start, len, L.words);
    for (int i = tid; i < kBlock / 4 + 4; i += kThreads) L.image[i] = i < kHdrWords ? rec[kRecHdr + i] : 0u;
    for (int i = tid; i < kLitSyms; i += kThreads) L.codes[i] = rec[kRecCodes + i];
    __syncthreads();
    const Runs r = find_runs(L.words, len, L.flags, L.wave_a, L.wave_b);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(L.words);
    int nbits = 0;
    for_tokens(bytes, len, r, [&](int lit, int mlen) {
      int extra = 0, nextra = 0;
      const int sym = mlen ? length_symbol(mlen, extra, nextra) : lit;
      nbits += (int)(L.codes[sym] >> 16) + (mlen ? nextra + 1 : 0);
    });
    const int inc = wave_scan_add(nbits, lane);
    if (lane == kWave - 1) L.wave_bits[wave] = inc;
    __syncthreads();
    int bitpos = (int)rec[kRecHdrBits] + inc - nbits;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
      if (w < wave) bitpos += L.wave_bits[w];
    const int limit = 8 * (int)size;           // (the size the code kernel counted: nothing is OR-ed past it)
    for_tokens(bytes, len, r, [&](int lit, int mlen) {
      int extra = 0, nextra = 0;
      const int sym = mlen ? length_symbol(mlen, extra, nextra) : lit;
      const uint32_t c = L.codes[sym];
      const int cl = (int)(c >> 16);
      if (bitpos + cl + nextra + 1 > limit) return;
      or_bits(L.image, bitpos, c & 0xffffu, cl);
      if (mlen) {
        if (nextra) or_bits(L.image, bitpos, (uint32_t)extra, nextra);
        bitpos += 1;                             // the distance code 0, one bit: 0
      }
    });
    if (tid == kThreads - 1) {
      const uint32_t c = L.codes[256];
      if (bitpos + (int)(c >> 16) <= limit) or_bits(L.image, bitpos, c & 0xffffu, (int)(c >> 16));
    }
    __syncthreads();
    const uint8_t *img = reinterpret_cast<const uint8_t *>(L.image);
    for (int i = tid; i < (int)size; i += kThreads) {
      // the empty stored block behind a block that is not the last: 000 and padding (zero bits), then LEN = 0, NLEN = 0xffff
      const unsigned v = (!at.last && i >= (int)size - 2) ? 0xffu : (unsigned)img[i];
      store(o + i, v);
    }
  }
  if (at.last && tid == 0) {
    unsigned long long s1 = 1, s2 = 0;
    const int b0 = blk_first[at.stream];
    for (int k = b0; k <= b; ++k) {
      const BlockAt ak = locate(offsets, blk_first, S, k);
      const uint32_t *rk = blk_code + (size_t)k * kRecWords;
      s2 = (s2 + (unsigned long long)ak.len * s1 + rk[kRecAdlerB]) % kAdler;
      s1 = (s1 + rk[kRecAdlerA]) % kAdler;
    }
    const unsigned ad = ((unsigned)s2 << 16) | (unsigned)s1;
    store(o + size, ad >> 24);
    store(o + size + 1, (ad >> 16) & 0xffu);
    store(o + size + 2, (ad >> 8) & 0xffu);
    store(o + size + 3, ad & 0xffu);
  }
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filtered(int type, int x, int a, int b, int c) {
  const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (x - pred) & 0xff;
}

__global__ __launch_bounds__(kFilterWaves *kWave) void png_filter_kernel(const uint8_t *__restrict__ pix, const int32_t *__restrict__ hw,
                                                                         const int64_t *__restrict__ pix_off,
                                                                         const int64_t *__restrict__ stream_off, uint8_t *__restrict__ out,
                                                                         long long total_pixels, long long total_stream) {
  const int img = blockIdx.y, lane = threadIdx.x & 63;
  const int y = blockIdx.x * kFilterWaves + (threadIdx.x >> 6);
  const int h = hw[2 * img], w = hw[2 * img + 1];
  if (y >= h) return;                       // (whole waves leave; the kernel has no barrier)
  const long long p0 = pix_off[img], row_bytes = 3ll * w;
  if (p0 < 0 || p0 + (long long)h * w > total_pixels) return;
  const uint8_t *cur = pix + 3 * p0 + (long long)y * row_bytes;
  const uint8_t *up = cur - row_bytes;
  const bool has_up = y > 0;
  int sum[5] = {0, 0, 0, 0, 0};
  for (int x = lane; x < row_bytes; x += kWave) {
    const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, bb = has_up ? up[x] : 0, c = (has_up && x >= 3) ? up[x - 3] : 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int f = filtered(t, v, a, bb, c);
      sum[t] += min(f, 256 - f);
    }
  }
  int best = 0, best_sum = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    int s = sum[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (t == 0 || s < best_sum) {
      best = t;
      best_sum = s;
    }
  }
  const long long o = stream_off[img] + (long long)y * (row_bytes + 1);
  if (o < 0 || o + row_bytes + 1 > total_stream) return;
  if (lane == 0) out[o] = (uint8_t)best;
  for (int x = lane; x < row_bytes; x += kWave) {
    const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, bb = has_up ? up[x] : 0, c = (has_up && x >= 3) ? up[x - 3] : 0;
    out[o + 1 + x] = (uint8_t)filtered(best, v, a, bb, c);
  }
}

// h_offsets (HOST, S+1): starts at 0, never decreases, ends at `total`
const char *bad_offsets64(const int64_t *h_off, long S, long total) {
  if (h_off[0] != 0) return "do not start at 0";
  for (long s = 0; s < S; ++s)
    if (h_off[s + 1] < h_off[s]) return "are not ascending";
  if ((long)h_off[S] != total) return "do not end at the total given";
  return nullptr;
}

long blocks_of(const int64_t *h_off, long S) {
  long nb = 0;
  for (long s = 0; s < S; ++s) {
    const long n = (long)(h_off[s + 1] - h_off[s]);
    nb += n ? (n + kBlock - 1) / kBlock : 1;
  }
  return nb;
}

}  // namespace

#define SN_DEFLATE_COMMON(fn, h_offsets, S, total)                                                                                   \
  SN_REQUIRE(S >= 1 && S <= kMaxStreams, fn ": 1 <= S <= %d required (S = %ld)", kMaxStreams, (long)(S));                             \
  SN_REQUIRE(total >= 0 && total < (1L << 40), fn ": 0 <= total < 2^40 required (total = %ld)", (long)(total));                       \
  do {                                                                                                                                \
    const char *why__ = bad_offsets64(h_offsets, S, total);                                                                           \
    SN_REQUIRE(!why__, fn ": the offsets %s (S = %ld, total = %ld)", why__, (long)(S), (long)(total));                               \
  } while (0);                                                                                                                        \
  SN_REQUIRE(blocks_of(h_offsets, S) < 2147483647L, fn ": the blocks of a call must fit 32-bit indexing (%ld blocks)", blocks_of(h_offsets, S))

SN_EXPORT int sn_deflate_limits(int32_t *h_out6) {
  SN_REQUIRE(h_out6, "sn_deflate_limits: null pointer");
  h_out6[0] = kBlock;
  h_out6[1] = kThreads;
  h_out6[2] = kMaxStreams;
  h_out6[3] = kRecWords;
  h_out6[4] = (int32_t)sizeof(CodeLds);
  h_out6[5] = (int32_t)sizeof(WriteLds);
  return SN_OK;
}

SN_EXPORT long sn_deflate_bound(long n) {
  if (n < 0) return -1;
  const long nb = (n + kBlock - 1) / kBlock;
  return n + 5 * (nb + 1) + 6;
}

SN_EXPORT int sn_deflate_plan(const int64_t *offsets, const int64_t *h_offsets, long S, long total, int32_t *blk_first, sn_stream_t stream) {
  SN_REQUIRE(offsets && h_offsets && blk_first, "sn_deflate_plan: null pointer");
  SN_DEFLATE_COMMON("sn_deflate_plan", h_offsets, S, total);
  hipLaunchKernelGGL(deflate_plan_kernel, dim3(1), dim3(kWave), 0, sn_stream(stream), offsets, (int)S, blk_first);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_deflate_code(const uint8_t *data, const int64_t *offsets, const int64_t *h_offsets, long S, long total,
                              const int32_t *blk_first, long n_blocks, uint32_t *blk_code, int64_t *blk_size, sn_stream_t stream) {
  SN_REQUIRE(offsets && h_offsets && blk_first && blk_code && blk_size && (data || total == 0), "sn_deflate_code: null pointer");
  SN_DEFLATE_COMMON("sn_deflate_code", h_offsets, S, total);
  SN_REQUIRE(n_blocks == blocks_of(h_offsets, S), "sn_deflate_code: n_blocks = %ld, the offsets give %ld blocks of %d bytes", n_blocks,
             blocks_of(h_offsets, S), kBlock);
  hipLaunchKernelGGL(deflate_code_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, sn_stream(stream), data, offsets, blk_first, (int)S,
                     blk_code, blk_size);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_deflate_write(const uint8_t *data, const int64_t *offsets, const int64_t *h_offsets, long S, long total,
                               const int32_t *blk_first, long n_blocks, const uint32_t *blk_code, const int64_t *blk_pos, uint8_t *out,
                               long capacity, sn_stream_t stream) {
  SN_REQUIRE(offsets && h_offsets && blk_first && blk_code && blk_pos && out && (data || total == 0), "sn_deflate_write: null pointer");
  SN_DEFLATE_COMMON("sn_deflate_write", h_offsets, S, total);
  SN_REQUIRE(n_blocks == blocks_of(h_offsets, S), "sn_deflate_write: n_blocks = %ld, the offsets give %ld blocks of %d bytes", n_blocks,
             blocks_of(h_offsets, S), kBlock);
  long bound = 0;
  for (long s = 0; s < S; ++s) bound += sn_deflate_bound((long)(h_offsets[s + 1] - h_offsets[s]));
  SN_REQUIRE(capacity >= bound, "sn_deflate_write: capacity = %ld is below the bound %ld (the sum of n + 5 * (nb + 1) + 6 over the streams)",
             capacity, bound);
  SN_HIP(sn_once_per_device_max_lds(reinterpret_cast<const void *>(deflate_write_kernel), (int)sizeof(WriteLds)));
  hipLaunchKernelGGL(deflate_write_kernel, dim3((unsigned)n_blocks), dim3(kThreads), sizeof(WriteLds), sn_stream(stream), data, offsets,
                     blk_first, (int)S, blk_code, blk_pos, out, (long long)capacity);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_png_filter(const uint8_t *pix, const int32_t *hw, const int32_t *h_hw, const int64_t *pix_off, const int64_t *stream_off,
                            int I, long total_pixels, long total_stream, uint8_t *out, sn_stream_t stream) {
  SN_REQUIRE(pix && hw && h_hw && pix_off && stream_off && out, "sn_png_filter: null pointer");
  SN_REQUIRE(I >= 1 && I <= kMaxStreams, "sn_png_filter: 1 <= I <= %d required (I = %d)", kMaxStreams, I);
  long pixels = 0, bytes = 0;
  int max_h = 0;
  for (int i = 0; i < I; ++i) {
    const long h = h_hw[2 * i], w = h_hw[2 * i + 1];
    SN_REQUIRE(h >= 1 && w >= 1 && h * w < 2147483648L / 4, "sn_png_filter: picture %d is %ld x %ld: h >= 1, w >= 1, h * w < 2^29 required", i, h, w);
    pixels += h * w;
    bytes += h * (3 * w + 1);
    if (h > max_h) max_h = (int)h;
  }
  SN_REQUIRE(total_pixels == pixels, "sn_png_filter: total_pixels = %ld, the sizes give %ld", total_pixels, pixels);
  SN_REQUIRE(total_stream == bytes, "sn_png_filter: total_stream = %ld, the sizes give %ld (h * (3 * w + 1) per picture)", total_stream, bytes);
  SN_REQUIRE(total_pixels < (1L << 38), "sn_png_filter: total_pixels < 2^38 required (total_pixels = %ld)", total_pixels);
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((max_h + kFilterWaves - 1) / kFilterWaves), (unsigned)I), dim3(kFilterWaves * kWave), 0,
                     sn_stream(stream), pix, hw, pix_off, stream_off, out, (long long)total_pixels, (long long)total_stream);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
