// inflate_code.h -- the decoder of zlib streams (RFC 1950 / 1951) that png_decode.hip runs with one wave per stream (DESIGN.md section
// 32).  Plain C++ that compiles for the host and for the device: the kernel runs it, tests/png_inflate_main.cpp compiles it into a
// stand-alone program (also under the address and undefined-behaviour sanitizers).  Internal, not part of the C ABI.
//
//   SnBits                the bounded bit reader: nothing is read at or past the stream's length
//   sn_inflate_build      canonical-code tables (count per length, symbols in code order) from code lengths; tells over-subscribed
//                         and incomplete sets apart
//   sn_inflate_zlib       the header, the blocks of the three types, the Adler-32, the bytes left over -> ONE status bit, or 0
//
// The bytes go to a sink (a template parameter): literal(byte), match(length, distance), raw(bytes of the input), adler().  The
// sink owns the capacity: a call that would pass it returns false and stores nothing.  On the device every lane of the wave runs
// this code with the same values (values read from LDS go through a readfirstlane so that the control flow stays scalar); only the
// sink divides work over the lanes.  No dynamic allocation, no recursion; every loop iteration consumes input bits or produces
// output bytes, and both are capped, so a damaged stream ends after a bounded number of steps.
#pragma once
#include <stdint.h>

// (always inlined on the device: a reader or a sink passed by reference to a real call would live in scratch memory)
#if defined(__HIPCC__)
#define SN_INF_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SN_INF_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define SN_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define SN_UNI(x) ((int)(x))
#endif

// one bit per cause; a stream gives exactly one of them (the first met) or 0
enum SnInflateStatus {
  SN_INF_HEADER = 1,        // zlib header: CM != 8, window above 32 KiB, FDICT, or the check bits
  SN_INF_BLOCK_TYPE = 2,    // BTYPE 3
  SN_INF_STORED = 4,        // stored block: LEN != ~NLEN
  SN_INF_LENGTHS = 8,       // code lengths: too many symbols, a repeat without a length before it or past the end, an over-subscribed
                            // set, an incomplete set other than one code of length 1, no end-of-block code
  SN_INF_SYMBOL = 16,       // literal/length 286 / 287, distance 30 / 31, or a code that no symbol has
  SN_INF_DISTANCE = 32,     // a distance beyond the start of the output
  SN_INF_INPUT = 64,        // the input ended early
  SN_INF_CAPACITY = 128,    // more output than the caller's capacity
  SN_INF_ADLER = 256,       // Adler-32 mismatch
  SN_INF_TRAILING = 512,    // bytes left after the Adler-32
};

constexpr int kInflateMaxBits = 15;
constexpr int kInflateLitSyms = 288;
constexpr int kInflateDistSyms = 32;
constexpr int kInflateFastBits = 9;
constexpr int kInflateRawPiece = 256;      // the most bytes of one raw() call
constexpr int kInflateMaxMatch = 258;
constexpr int kInflateWindow = 32768;
constexpr uint32_t kAdlerBase = 65521u;

// The decoder's tables: 2.3 KiB, in LDS on the device.  (Index arrays live here and not on the stack: a dynamically indexed local
// array would be scratch memory on the device.)
struct SnInflateTables {
  uint16_t lcount[kInflateMaxBits + 1], lsym[kInflateLitSyms];        // literal/length code
  uint16_t dcount[kInflateMaxBits + 1], dsym[kInflateDistSyms];       // distance code (the code-length code while the lengths are read)
  uint16_t offs[kInflateMaxBits + 1];                                // scratch of the construction
  uint16_t fast[1 << kInflateFastBits];                              // literal/length codes of <= 9 bits by their bits: sym << 4 | len
  uint8_t lens[kInflateLitSyms + kInflateDistSyms];
  uint8_t clen[20];
};

struct SnBits {
  const uint8_t *p;
  int n, pos;          // the stream's length; the next byte
  uint64_t buf;        // the bits not yet taken, the next one lowest
  int cnt;
};

SN_INF_HD void sn_bits_fill(SnBits &b) {
  if (b.cnt <= 32 && b.pos + 4 <= b.n) {
    const uint32_t w = (uint32_t)b.p[b.pos] | ((uint32_t)b.p[b.pos + 1] << 8) | ((uint32_t)b.p[b.pos + 2] << 16) | ((uint32_t)b.p[b.pos + 3] << 24);
    b.buf |= (uint64_t)(uint32_t)SN_UNI(w) << b.cnt;
    b.cnt += 32;
    b.pos += 4;
  }
  while (b.cnt <= 56 && b.pos < b.n) {
    b.buf |= (uint64_t)(uint32_t)SN_UNI(b.p[b.pos]) << b.cnt;
    b.cnt += 8;
    b.pos += 1;
  }
}

// k <= 32 bits, the first one lowest; false: the input ended
SN_INF_HD bool sn_bits_take(SnBits &b, int k, uint32_t &v) {
  if (b.cnt < k) {
    sn_bits_fill(b);
    if (b.cnt < k) return false;
  }
  v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
  b.buf >>= k;
  b.cnt -= k;
  return true;
}

// Code lengths lens[0 .. n) -> count[len], sym[] = the symbols in code order (by length, then by symbol).  Returns what is left of
// the code space in units of 2^-15 ... scaled as puff does: < 0 over-subscribed, 0 complete, > 0 incomplete; maxlen = the longest.
SN_INF_HD int sn_inflate_build(const uint8_t *lens, int n, uint16_t *count, uint16_t *sym, uint16_t *offs, int &maxlen) {
  for (int l = 0; l <= kInflateMaxBits; ++l) count[l] = 0;
  for (int s = 0; s < n; ++s) {
    const int l = SN_UNI(lens[s]);
    count[l] = (uint16_t)(SN_UNI(count[l]) + 1);
  }
  maxlen = 0;
  int left = 1;
  for (int l = 1; l <= kInflateMaxBits; ++l) {
    const int c = SN_UNI(count[l]);
    if (c) maxlen = l;
    left = (left << 1) - c;
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (int l = 1; l < kInflateMaxBits; ++l) offs[l + 1] = (uint16_t)(SN_UNI(offs[l]) + SN_UNI(count[l]));
  for (int s = 0; s < n; ++s) {
    const int l = SN_UNI(lens[s]);
    if (l) {
      const int o = SN_UNI(offs[l]);
      sym[o] = (uint16_t)s;
      offs[l] = (uint16_t)(o + 1);
    }
  }
  return left;
}

// the literal/length codes of <= 9 bits, indexed by the next 9 bits of the stream (a code's first bit is the stream's lowest)
SN_INF_HD void sn_inflate_fast(SnInflateTables &T, int n) {
  for (int i = 0; i < (1 << kInflateFastBits); ++i) T.fast[i] = 0;
  int code = 0;
  T.offs[0] = 0;
  for (int l = 1; l <= kInflateMaxBits; ++l) {          // offs[l] = the first code of length l
    code = (code + (l > 1 ? SN_UNI(T.lcount[l - 1]) : 0)) << 1;
    T.offs[l] = (uint16_t)code;                          // (a complete or incomplete set: fits 15 bits; 16 for the last, unused)
  }
  for (int s = 0; s < n; ++s) {
    const int l = SN_UNI(T.lens[s]);
    if (!l) continue;
    const int c = SN_UNI(T.offs[l]);
    T.offs[l] = (uint16_t)(c + 1);
    if (l > kInflateFastBits) continue;
    int rev = 0;
    for (int k = 0; k < l; ++k) rev |= ((c >> k) & 1) << (l - 1 - k);
    for (int i = rev; i < (1 << kInflateFastBits); i += 1 << l) T.fast[i] = (uint16_t)((s << 4) | l);
  }
}

// one symbol, bit by bit: >= 0 the symbol, -1 a code no symbol has, -2 the input ended
SN_INF_HD int sn_inflate_decode(SnBits &b, const uint16_t *count, const uint16_t *sym) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= kInflateMaxBits; ++l) {
    uint32_t bit;
    if (!sn_bits_take(b, 1, bit)) return -2;
    code |= (int)bit;
    const int c = SN_UNI(count[l]);
    if (code - c < first) return SN_UNI(sym[index + (code - first)]);
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

SN_INF_HD int sn_inflate_decode_lit(SnBits &b, const SnInflateTables &T) {
  if (b.cnt < kInflateMaxBits) sn_bits_fill(b);
  const int e = SN_UNI(T.fast[(int)(b.buf & ((1u << kInflateFastBits) - 1u))]);
  const int l = e & 15;
  if (l && l <= b.cnt) {
    b.buf >>= l;
    b.cnt -= l;
    return e >> 4;
  }
  return sn_inflate_decode(b, T.lcount, T.lsym);
}

// the order in which the lengths of the code-length code are sent (RFC 1951 3.2.7), five bits each
SN_INF_HD int sn_inflate_clen_order(int i) {
  const uint64_t lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) |
                      (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
  const uint64_t hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
  return (int)(((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12)))) & 31);
}

// what zlib's inflate accepts of a set: over-subscribed never; incomplete only as ONE code of length 1 (or no code at all, for
// the distances: a block of literals)
SN_INF_HD bool sn_inflate_set_ok(int left, int maxlen) { return left == 0 || (left > 0 && maxlen <= 1); }

// the two codes of a block from T.lens[0 .. nlen + ndist): 0 or SN_INF_LENGTHS
SN_INF_HD int sn_inflate_codes(SnInflateTables &T, int nlen, int ndist) {
  int maxlen = 0;
  if (!SN_UNI(T.lens[256])) return SN_INF_LENGTHS;
  int left = sn_inflate_build(T.lens, nlen, T.lcount, T.lsym, T.offs, maxlen);
  if (!sn_inflate_set_ok(left, maxlen)) return SN_INF_LENGTHS;
  left = sn_inflate_build(T.lens + nlen, ndist, T.dcount, T.dsym, T.offs, maxlen);
  if (!sn_inflate_set_ok(left, maxlen)) return SN_INF_LENGTHS;
  sn_inflate_fast(T, nlen);
  return 0;
}

SN_INF_HD int sn_inflate_fixed(SnInflateTables &T) {
  for (int s = 0; s < kInflateLitSyms; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  for (int s = 0; s < kInflateDistSyms; ++s) T.lens[kInflateLitSyms + s] = 5;
  return sn_inflate_codes(T, kInflateLitSyms, kInflateDistSyms);
}

// the header of a dynamic block: the code-length code, then the lengths with their repeat symbols
SN_INF_HD int sn_inflate_dynamic(SnBits &b, SnInflateTables &T) {
  uint32_t v;
  if (!sn_bits_take(b, 14, v)) return SN_INF_INPUT;
  const int nlen = (int)(v & 31) + 257, ndist = (int)((v >> 5) & 31) + 1, ncode = (int)(v >> 10) + 4;
  if (nlen > 286 || ndist > 30) return SN_INF_LENGTHS;
  for (int i = 0; i < 19; ++i) T.clen[i] = 0;
  for (int i = 0; i < ncode; ++i) {
    if (!sn_bits_take(b, 3, v)) return SN_INF_INPUT;
    T.clen[sn_inflate_clen_order(i)] = (uint8_t)v;
  }
  int maxlen = 0;
  if (sn_inflate_build(T.clen, 19, T.dcount, T.dsym, T.offs, maxlen) != 0) return SN_INF_LENGTHS;      // this one must be complete
  int at = 0;
  while (at < nlen + ndist) {
    const int s = sn_inflate_decode(b, T.dcount, T.dsym);
    if (s == -2) return SN_INF_INPUT;
    if (s < 0) return SN_INF_LENGTHS;
    if (s < 16) {
      T.lens[at++] = (uint8_t)s;
      continue;
    }
    int fill = 0, rep;
    if (s == 16) {
      if (at == 0) return SN_INF_LENGTHS;
      fill = SN_UNI(T.lens[at - 1]);
      if (!sn_bits_take(b, 2, v)) return SN_INF_INPUT;
      rep = 3 + (int)v;
    } else if (s == 17) {
      if (!sn_bits_take(b, 3, v)) return SN_INF_INPUT;
      rep = 3 + (int)v;
    } else {
      if (!sn_bits_take(b, 7, v)) return SN_INF_INPUT;
      rep = 11 + (int)v;
    }
    if (at + rep > nlen + ndist) return SN_INF_LENGTHS;
    for (int k = 0; k < rep; ++k) T.lens[at++] = (uint8_t)fill;
  }
  // (the distance lengths follow the literal/length lengths in T.lens: sn_inflate_codes reads them there)
  return sn_inflate_codes(T, nlen, ndist);
}

// the symbols of a block with codes, up to its end-of-block: 0 or a status bit
template <class Sink>
SN_INF_HD int sn_inflate_symbols(SnBits &b, const SnInflateTables &T, Sink &out) {
  for (;;) {
    const int s = sn_inflate_decode_lit(b, T);
    if (s == -2) return SN_INF_INPUT;
    if (s < 0) return SN_INF_SYMBOL;
    if (s < 256) {
      if (!out.literal(s)) return SN_INF_CAPACITY;
      continue;
    }
    if (s == 256) return 0;
    if (s > 285) return SN_INF_SYMBOL;
    uint32_t v;
    int len = 258;
    if (s < 285) {
      const int i = s - 257;
      if (i < 8) {
        len = 3 + i;
      } else {
        const int e = (i - 4) >> 2;
        if (!sn_bits_take(b, e, v)) return SN_INF_INPUT;
        len = 3 + ((4 + (i & 3)) << e) + (int)v;
      }
    }
    const int d = sn_inflate_decode(b, T.dcount, T.dsym);
    if (d == -2) return SN_INF_INPUT;
    if (d < 0 || d > 29) return SN_INF_SYMBOL;
    int dist = 1 + d;
    if (d >= 4) {
      const int e = (d >> 1) - 1;
      if (!sn_bits_take(b, e, v)) return SN_INF_INPUT;
      dist = 1 + ((2 + (d & 1)) << e) + (int)v;
    }
    if (dist > out.pos()) return SN_INF_DISTANCE;
    if (!out.match(len, dist)) return SN_INF_CAPACITY;
  }
}

// One zlib stream of n bytes -> the sink; T: the tables' storage.  Returns 0 or ONE status bit; out.pos() is what was produced.
template <class Sink>
SN_INF_HD int sn_inflate_zlib(const uint8_t *in, int n, Sink &out, SnInflateTables &T) {
  SnBits b;
  b.p = in;
  b.n = n < 0 ? 0 : n;
  b.pos = 0;
  b.buf = 0;
  b.cnt = 0;
  uint32_t v;
  if (!sn_bits_take(b, 16, v)) return SN_INF_INPUT;
  const uint32_t cmf = v & 255u, flg = v >> 8;
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 32u) || ((cmf << 8) | flg) % 31u) return SN_INF_HEADER;
  for (;;) {
    if (!sn_bits_take(b, 3, v)) return SN_INF_INPUT;
    const int last = (int)(v & 1u), type = (int)(v >> 1);
    if (type == 3) return SN_INF_BLOCK_TYPE;
    if (type == 0) {
      sn_bits_take(b, b.cnt & 7, v);
      if (!sn_bits_take(b, 32, v)) return SN_INF_INPUT;
      int len = (int)(v & 0xffffu);
      if ((uint32_t)len != ((v >> 16) ^ 0xffffu)) return SN_INF_STORED;
      while (len && b.cnt >= 8) {                      // the bytes the reader holds already
        sn_bits_take(b, 8, v);
        if (!out.literal((int)v)) return SN_INF_CAPACITY;
        len -= 1;
      }
      if (len > b.n - b.pos) return SN_INF_INPUT;
      while (len) {
        const int k = len < kInflateRawPiece ? len : kInflateRawPiece;
        if (!out.raw(b.p + b.pos, k)) return SN_INF_CAPACITY;
        b.pos += k;
        len -= k;
      }
    } else {
      const int bad = type == 1 ? sn_inflate_fixed(T) : sn_inflate_dynamic(b, T);
      if (bad) return bad;
      const int st = sn_inflate_symbols(b, T, out);
      if (st) return st;
    }
    if (last) break;
  }
  sn_bits_take(b, b.cnt & 7, v);
  uint32_t want = 0;
  for (int k = 0; k < 4; ++k) {
    if (!sn_bits_take(b, 8, v)) return SN_INF_INPUT;
    want = (want << 8) | v;
  }
  if (out.adler() != want) return SN_INF_ADLER;
  if (b.cnt > 0 || b.pos < b.n) return SN_INF_TRAILING;
  return 0;
}

// the sink of one thread: bytes into a buffer of `cap` bytes (the host program; any single-threaded caller)
struct SnByteSink {
  uint8_t *out;
  int cap, n;
  uint32_t a, b;
  SN_INF_HD void init(uint8_t *o, int capacity) {
    out = o;
    cap = capacity < 0 ? 0 : capacity;
    n = 0;
    a = 1;
    b = 0;
  }
  SN_INF_HD int pos() const { return n; }
  SN_INF_HD void put(uint8_t v) {
    out[n++] = v;
    a += v;
    if (a >= kAdlerBase) a -= kAdlerBase;
    b += a;
    if (b >= kAdlerBase) b -= kAdlerBase;
  }
  SN_INF_HD bool literal(int v) {
    if (n >= cap) return false;
    put((uint8_t)v);
    return true;
  }
  SN_INF_HD bool match(int len, int dist) {
    if (len > cap - n) return false;
    for (int i = 0; i < len; ++i) put(out[n - dist]);
    return true;
  }
  SN_INF_HD bool raw(const uint8_t *src, int k) {
    if (k > cap - n) return false;
    for (int i = 0; i < k; ++i) put(src[i]);
    return true;
  }
  SN_INF_HD uint32_t adler() const { return (b << 16) | a; }
};
