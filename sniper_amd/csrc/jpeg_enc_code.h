// jpeg_enc_code.h -- the per-block part of baseline JPEG encoding (ITU T.81, 8 bit, the Annex K tables) for jpeg_encode.hip (DESIGN.md
// section 31): the quantisation tables and their exact reciprocals, libjpeg's slow-integer forward DCT, the Huffman coder of one block
// (its size and its bits) and the guarded bit writer.  Plain C++ that compiles for the host and for the device: the kernels call it
// on every lane, tests/jpeg_enc_main.cpp compiles it into a stand-alone program.  Integers only.  Internal, not part of the C ABI.
//   Safety: every loop has a bound; a table index is masked into its table; every store of the writer is guarded by the capacity it
//   was given (in 32-bit words) -- what does not fit is not written and sets the writer's `err`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SNE_HD __host__ __device__ inline
#else
#define SNE_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SNE_CONST __device__ __constant__ static const
#else
#define SNE_CONST static const
#endif

// the most bits of one block's code: a DC code of 11 bits with 11 extra bits (chroma, category 11), 63 AC codes of 16 + 10 bits
constexpr int kJpegEncMaxBlockBits = 22 + 63 * 26;
constexpr int kJpegEncRawBytesPerBlock = (kJpegEncMaxBlockBits + 7) / 8;      // 208 (the 4 bits to spare are not counted on)

enum { SNE_NO_ROOM = 1, SNE_BAD_COEF = 2 };      // a store past the capacity; a DC category above 11 / an AC category above 10

// zig-zag index -> natural (row-major) index
SNE_CONST uint8_t kJpegEncNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// T.81 annex K.1: luminance, chrominance (natural order)
SNE_CONST uint8_t kJpegEncBaseQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// T.81 annex K.3: the counts of the codes of 1 .. 16 bits, then the values: DC 0, DC 1, AC 0, AC 1
SNE_CONST uint8_t kJpegEncDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
SNE_CONST uint8_t kJpegEncAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
SNE_CONST uint8_t kJpegEncAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// ---- quantisation ------------------------------------------------------------------------------------------------------------------------
// entry `zz` (zig-zag order) of table `chroma` at `quality` 1 .. 100 (libjpeg's jpeg_quality_scaling, baseline clamp)
SNE_HD int sn_jpeg_enc_quant_entry(int chroma, int zz, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = ((int)kJpegEncBaseQuant[chroma & 1][kJpegEncNatural[zz & 63]] * s + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// n / d for 0 <= n < 2^14 and 8 <= d <= 2040 as the high word of n * m with m = floor(2^32 / d) + 1: m = (2^32 + e) / d with
// 0 < e <= d, so n * m / 2^32 = n / d + n * e / (d * 2^32), and the second term is below 2^14 / 2^32 < 1 / d: the floor is n / d's.
// (tests/jpeg_enc_main.cpp checks every pair.)
SNE_HD uint32_t sn_jpeg_enc_recip(uint32_t d) { return (uint32_t)(0x100000000ull / d) + 1u; }
SNE_HD uint32_t sn_jpeg_enc_mulhi(uint32_t n, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(n, m);
#else
  return (uint32_t)(((uint64_t)n * m) >> 32);
#endif
}
// c: 8 x the DCT coefficient, d = 8 * the table entry, m = sn_jpeg_enc_recip(d) -> sign(c) * ((|c| + (d >> 1)) / d)
SNE_HD int sn_jpeg_enc_quantise(int c, uint32_t d, uint32_t m) {
  const uint32_t a = (uint32_t)(c < 0 ? -c : c) + (d >> 1);
  const int q = (int)sn_jpeg_enc_mulhi(a, m);
  return c < 0 ? -q : q;
}

// ---- forward DCT: libjpeg's jfdctint (slow integer), rows then columns; d holds samples minus 128, and 8 x the DCT after ----------------
SNE_HD int sn_jpeg_enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <bool kRows>
SNE_HD void sn_jpeg_enc_fdct_pass(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7) {
  constexpr int n = kRows ? 11 : 15;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kRows) {
    d0 = (t10 + t11) * 4;
    d4 = (t10 - t11) * 4;
  } else {
    d0 = sn_jpeg_enc_descale(t10 + t11, 2);
    d4 = sn_jpeg_enc_descale(t10 - t11, 2);
  }
  const int z1e = (t12 + t13) * 4433;
  d2 = sn_jpeg_enc_descale(z1e + t13 * 6270, n);
  d6 = sn_jpeg_enc_descale(z1e - t12 * 15137, n);
  const int z5 = (t4 + t6 + t5 + t7) * 9633;
  const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
  d7 = sn_jpeg_enc_descale(t4 * 2446 + z1 + z3, n);
  d5 = sn_jpeg_enc_descale(t5 * 16819 + z2 + z4, n);
  d3 = sn_jpeg_enc_descale(t6 * 25172 + z2 + z3, n);
  d1 = sn_jpeg_enc_descale(t7 * 12299 + z1 + z4, n);
}

SNE_HD void sn_jpeg_enc_fdct(int *d /* 64, natural order, in place */) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 8; ++r)
    sn_jpeg_enc_fdct_pass<true>(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5], d[8 * r + 6], d[8 * r + 7]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int c = 0; c < 8; ++c)
    sn_jpeg_enc_fdct_pass<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
}

// ---- the Huffman coder ---------------------------------------------------------------------------------------------------------------------
// code | length << 16 per symbol; length 0: the table has no such symbol
struct SnJpegEncTables {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
};

// table t of 4: DC 0, DC 1, AC 0, AC 1 (the canonical codes of T.81 annex C)
SNE_HD void sn_jpeg_enc_build_table(SnJpegEncTables *T, int t) {
  const bool ac = t >= 2;
  const int id = t & 1;
  uint32_t *out = ac ? T->ac[id] : T->dc[id];
  const int n_out = ac ? 256 : 16, n_vals = ac ? 162 : 12;
  for (int i = 0; i < n_out; ++i) out[i] = 0;
  const uint8_t *bits = ac ? kJpegEncAcBits[id] : kJpegEncDcBits[id];
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int j = 0; j < (int)bits[l - 1] && k < n_vals; ++j, ++k) {
      const int sym = ac ? (int)kJpegEncAcVals[id][k] : k;
      out[sym] = code | ((uint32_t)l << 16);
      ++code;
    }
    code <<= 1;
  }
}

SNE_HD int sn_jpeg_enc_category(int v) {
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}

// A sink that only counts.
struct SnJpegEncCount {
  long bits = 0;
  int err = 0;
  SNE_HD void put(uint32_t, int n) { bits += n; }
};

// A sink that writes bits, MSB first, into a ZEROED stream of 32-bit words (bytes in stream order: a word is stored byte-swapped).
// Neighbouring blocks share the words at their borders, so a word is OR-ed in (atomically on the device: the order does not
// matter, the result is the same every run).  Nothing is stored at or past words + cap_words.
struct SnJpegEncWriter {
  uint32_t *words;
  long cap_words, w;
  uint64_t acc;      // bits at the top; the n highest are valid (the first (bit position & 31) of them are another block's: zero here)
  int n, err;
  SNE_HD SnJpegEncWriter(uint32_t *words_, long cap_words_, long bitpos) : words(words_), cap_words(cap_words_), w(bitpos >> 5), acc(0), n((int)(bitpos & 31)), err(0) {}
  SNE_HD void store(uint32_t v) {
    if (v) {
      if (w >= 0 && w < cap_words) {
        const uint32_t s = __builtin_bswap32(v);
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(&words[w], s);
#else
        words[w] |= s;
#endif
      } else {
        err |= SNE_NO_ROOM;
      }
    } else if (w < 0 || w >= cap_words) {
      err |= SNE_NO_ROOM;          // (zero bits need no store, but they need the room)
    }
    ++w;
  }
  // the n <= 26 low bits of v
  SNE_HD void put(uint32_t v, int nbits) {
    if (nbits <= 0) return;
    acc |= (uint64_t)(v & ((1u << nbits) - 1u)) << (64 - n - nbits);
    n += nbits;
    if (n >= 32) {
      store((uint32_t)(acc >> 32));
      acc <<= 32;
      n -= 32;
    }
  }
  SNE_HD void finish() {
    if (n > 0) store((uint32_t)(acc >> 32));
    n = 0;
    acc = 0;
  }
  SNE_HD long bitpos() const { return w * 32 + n; }
};

// One block: blk holds 64 quantised coefficients in zig-zag order, the DC not differenced; pred is the DC of the same component's
// previous block in scan order (0 for the first).  A code and its extra bits go to the sink in one put of at most 26 bits.
template <class Sink>
SNE_HD void sn_jpeg_enc_block(const int16_t *blk, int pred, int chroma, const SnJpegEncTables &T, Sink &sink) {
  chroma &= 1;
  {
    const int d = (int)blk[0] - pred;
    int s = sn_jpeg_enc_category(d);
    if (s > 11) {
      sink.err |= SNE_BAD_COEF;
      s = 11;
    }
    const uint32_t c = T.dc[chroma][s];
    const uint32_t extra = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u);
    sink.put(((c & 0xffffu) << s) | extra, (int)(c >> 16) + s);
  }
  int r = 0;
  for (int k = 1; k < 64; ++k) {
    const int a = blk[k];
    if (a == 0) {
      ++r;
      continue;
    }
    for (; r > 15; r -= 16) {          // (at most three times: r <= 62)
      const uint32_t z = T.ac[chroma][0xf0];
      sink.put(z & 0xffffu, (int)(z >> 16));
    }
    int s = sn_jpeg_enc_category(a);
    if (s > 10) {
      sink.err |= SNE_BAD_COEF;
      s = 10;
    }
    const uint32_t c = T.ac[chroma][((r << 4) | s) & 255];
    const uint32_t extra = (uint32_t)(a < 0 ? a - 1 : a) & ((1u << s) - 1u);
    sink.put(((c & 0xffffu) << s) | extra, (int)(c >> 16) + s);
    r = 0;
  }
  if (r) {
    const uint32_t e = T.ac[chroma][0];
    sink.put(e & 0xffffu, (int)(e >> 16));
  }
}

// the ones that fill the last byte of a scan that ends at bit `end`
template <class Sink>
SNE_HD void sn_jpeg_enc_fill(long end, Sink &sink) {
  const int n = (int)((8 - (end & 7)) & 7);
  sink.put((1u << n) - 1u, n);
}
