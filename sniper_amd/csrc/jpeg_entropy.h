// jpeg_entropy.h -- baseline JPEG entropy decoding (ITU T.81, Huffman, 8 bit) for jpeg_decode.hip.  Plain C++
// that compiles for the host and for the device: the kernel runs sn_jpeg_decode_span on every lane, tests/jpeg_entropy_main.cpp compiles
// it into a stand-alone program (the sequential decode that is the kernel's specification, and an emulation of its rounds).
// Internal, not part of the C ABI.
//   Safety: every loop has a bound; every load is guarded by the end of the segment, which the caller has clamped to the stream length;
//   every store is guarded by the block count the segment is expected to hold; a damaged stream yields a status, never an access.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SNJ_HD __host__ __device__ inline
#else
#define SNJ_HD inline
#endif

constexpr int kJpegMaxBpm = 10;             // blocks per MCU (T.81 B.2.3); the device path uses up to 6
constexpr int kJpegDhtBytes = 16 + 256;     // one table as the DHT segment holds it: 16 counts, then the values
constexpr uint32_t kJpegNoState = 0xffffffffu;
constexpr int kJpegNoLimit = 0x7fffffff;

// status bits (per segment, OR-ed into the image's word)
enum {
  SNJ_BAD_CODE = 1,      // no code of 1 .. 16 bits matches, or a DC category above 11 / an AC category above 10
  SNJ_BAD_RUN = 2,       // k + r > 63
  SNJ_OVERRUN = 4,       // a symbol reaches past the end of its segment (truncation, or a marker inside the data)
  SNJ_BLOCKS = 8,        // the segment holds fewer or more blocks than the frame header says
  SNJ_BAD_DC = 16,       // a DC value leaves int16
  SNJ_RANGE = 32,        // a sample leaves the range in which every IDCT implementation agrees (pixel kernel)
  SNJ_BAD_MARKER = 64,   // the two bytes after a segment are not the restart marker that is due
};

// zig-zag index -> natural (row-major) index
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__
#endif
static const uint8_t kJpegNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// A decoding table.  A code of l bits, left-aligned in 16 bits, is c; it has length l iff c < limit[l] and not c < limit[l - 1]
// (limit[l] = (last code of length <= l, plus one) << (16 - l), 0 while there is none); its value is vals[(c >> (16 - l)) + delta[l]].
// Codes of up to 8 bits are also found in one step: look[c >> 8] = (l << 8) | value, 0 for the longer ones.
struct SnJpegHuff {
  int32_t limit[17];
  int32_t delta[17];
  uint16_t look[256];
  uint8_t vals[256];
};

// Canonical codes from the DHT counts (T.81 annex C).  Over-subscribed counts (a code that would not fit its length) end the table
// there: the remaining lengths match nothing.  At most 256 values are read.
SNJ_HD void sn_jpeg_build_table(const uint8_t *dht, SnJpegHuff *t) {
  for (int i = 0; i < 256; ++i) {
    t->look[i] = 0;
    t->vals[i] = dht[16 + i];
  }
  int code = 0, k = 0;
  bool ok = true;
  t->limit[0] = 0;
  t->delta[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    int n = ok ? dht[l - 1] : 0;
    if (k + n > 256 || code + n > (1 << l)) {
      n = 0;
      ok = false;
    }
    t->delta[l] = k - code;
    if (l <= 8) {
      for (int j = 0; j < n; ++j) {
        const int first = (code + j) << (8 - l);
        for (int f = 0; f < (1 << (8 - l)); ++f) t->look[first + f] = (uint16_t)((l << 8) | dht[16 + k + j]);
      }
    }
    code += n;
    k += n;
    t->limit[l] = code << (16 - l);
    code <<= 1;
  }
}

// What a lane knows of one segment.  data points at the image's stream; [.., end) are the bytes the segment may read.
struct SnJpegCtx {
  const uint8_t *data;
  uint32_t end;               // byte index one past the segment's last byte (the caller guarantees end <= the stream's length)
  const SnJpegHuff *huff;     // four tables: DC 0, DC 1, AC 0, AC 1
  uint32_t bpm;               // blocks per MCU
  uint32_t nluma;             // the first nluma blocks of an MCU are component 0, then one block per further component
  uint32_t sel;               // bit 2c: the DC table of component c, bit 2c + 1: its AC table
};

// (bit position of the next symbol in the stream, stuffed bytes counted; block index inside the MCU << 8 | zig-zag index k).
// k = 0: the next symbol is a DC code.  p = kJpegNoState: no state (the lane before found no way through its bytes).
struct SnJpegState {
  uint32_t p;
  uint32_t bk;
};

// The bit reader.  acc holds cnt valid bits at its top; pos is the index of the next byte to load; bit j of ff says that the byte
// loaded j loads ago was a data byte FF, which takes two bytes of the stream (FF 00).  Past the end, or from a marker on, it loads
// zero bytes and keeps counting, so that the position of a symbol that overran is still past the end.
struct SnJpegBits {
  uint64_t acc;
  uint32_t cnt, pos, ff, end;
};

SNJ_HD void sn_jpeg_refill(SnJpegBits &b, const uint8_t *data) {
  for (int i = 0; i < 8 && b.cnt <= 56; ++i) {
    uint32_t v = 0, stuffed = 0;
    if (b.pos < b.end) {
      v = data[b.pos];
      if (v == 0xff) {
        if (b.pos + 1 < b.end && data[b.pos + 1] == 0) {
          stuffed = 1;
        } else {
          b.end = b.pos;      // a marker, or an FF that ends the segment: nothing is data from here on
          v = 0;
        }
      }
    }
    b.pos += 1 + stuffed;
    b.ff = (b.ff << 1) | stuffed;
    b.acc |= (uint64_t)v << (56 - b.cnt);
    b.cnt += 8;
  }
}

SNJ_HD uint32_t sn_jpeg_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}

// the stream position of the next unread bit
SNJ_HD uint32_t sn_jpeg_bitpos(const SnJpegBits &b) {
  const uint32_t k = (b.cnt + 7) >> 3;                       // bytes of acc not fully read (k <= 8)
  const uint32_t back = k + sn_jpeg_popc(b.ff & ((1u << k) - 1u));
  return (b.pos - back) * 8u + ((8u - (b.cnt & 7u)) & 7u);
}

SNJ_HD void sn_jpeg_start(SnJpegBits &b, const uint8_t *data, uint32_t p, uint32_t end) {
  b.acc = 0;
  b.cnt = 0;
  b.ff = 0;
  b.pos = p >> 3;
  b.end = end;
  sn_jpeg_refill(b, data);
  b.acc <<= (p & 7u);
  b.cnt -= (p & 7u);
}

// The entry of a lane that has nothing but a guess: a block starts at the first byte of its subsequence -- or one byte on where that
// byte is the zero stuffed after an FF, which is no data.
SNJ_HD SnJpegState sn_jpeg_guess(const uint8_t *data, uint32_t seg_first, uint32_t first_byte, uint32_t end) {
  SnJpegState s;
  uint32_t at = first_byte;
  if (at > seg_first && at < end && data[at] == 0 && data[at - 1] == 0xff) ++at;
  s.p = at * 8u;
  s.bk = 0;
  return s;
}

// Decodes the symbols (a Huffman code with its extra bits) that START before byte last_byte, from state `in` on (first_byte is the
// first byte of the range, kept for the record: a state never lies before it).  Returns the number of blocks completed; *out is the
// state of the first symbol that starts at or after last_byte.  With coef != nullptr the coefficients are written: block `block0`
// (counted inside the segment) is the one `in` stands in, int16, natural order, DC as decoded (a difference).  Decoding stops once
// block block_limit - 1 is complete: what follows the last block of a segment is padding, not symbols (a lane that does not know its
// block0 yet passes block0 = 0 and kJpegNoLimit).  *status collects SNJ_* bits; after one, *out is no state.
//   Without coef the span belongs to the rounds, where most entries are guesses: what a wrong guess meets (no matching code, a
//   category too large, a run past the block) must not end the chain that later lanes continue until it meets the true one, so such
//   a symbol is stepped over by a fixed rule instead.  On the true chain of a sound stream none of this happens, so both forms
//   decode it alike; a damaged stream is found by the writing pass, which is strict.
SNJ_HD int sn_jpeg_decode_span(const SnJpegCtx &c, SnJpegState in, uint32_t first_byte, uint32_t last_byte, int16_t *coef, int block0,
                               int block_limit, SnJpegState *out, int *status) {
  (void)first_byte;
  const bool tolerant = coef == nullptr;
  int done = 0;
  if (in.p == kJpegNoState) {
    *out = in;
    return 0;
  }
  const uint32_t last_bit = (last_byte < c.end ? last_byte : c.end) * 8u;
  uint32_t blk = in.bk >> 8, k = in.bk & 63u;
  if (blk >= c.bpm) blk = 0;
  uint32_t p = in.p;
  if (p >= last_bit) {
    *out = in;
    return 0;
  }
  SnJpegBits b;
  sn_jpeg_start(b, c.data, p, c.end);
  // each symbol takes at least one bit: (last_bit - p) iterations at the most
  const uint32_t max_iter = last_bit - p;
  int st = 0;
  for (uint32_t it = 0; it < max_iter && p < last_bit && block0 + done < block_limit; ++it) {
    sn_jpeg_refill(b, c.data);
    const uint32_t comp = blk < c.nluma ? 0u : 1u + (blk - c.nluma);
    const uint32_t tab = k == 0 ? ((c.sel >> (2u * comp)) & 1u) : 2u + ((c.sel >> (2u * comp + 1u)) & 1u);
    const SnJpegHuff &h = c.huff[tab];
    const uint32_t c16 = (uint32_t)(b.acc >> 48);
    uint32_t len, sym;
    const uint32_t e = h.look[c16 >> 8];
    if (e) {
      len = e >> 8;
      sym = e & 255u;
    } else {
      len = 0;
      for (uint32_t l = 9; l <= 16; ++l) {
        if ((int32_t)c16 < h.limit[l]) {
          len = l;
          break;
        }
      }
      const int32_t idx = len ? (int32_t)(c16 >> (16u - len)) + h.delta[len] : -1;
      if (idx < 0 || idx > 255) {
        if (!tolerant) {
          st |= SNJ_BAD_CODE;
          break;
        }
        b.acc <<= 1;          // a guess that met no code: one bit on
        b.cnt -= 1;
        p = sn_jpeg_bitpos(b);
        if (p > b.end * 8u) {
          st |= SNJ_OVERRUN;
          break;
        }
        continue;
      }
      sym = h.vals[idx];
    }
    b.acc <<= len;
    b.cnt -= len;
    uint32_t nbits, run = 0;
    bool end_block = false, has_value = true;
    if (k == 0) {
      nbits = sym;
      if (nbits > 11) {
        if (!tolerant) {
          st |= SNJ_BAD_CODE;
          break;
        }
        nbits = 11;
      }
    } else {
      run = sym >> 4;
      nbits = sym & 15u;
      if (nbits > 10) {
        if (!tolerant) {
          st |= SNJ_BAD_CODE;
          break;
        }
        nbits = 10;
      }
      if (nbits == 0) {
        has_value = false;
        if (run == 15) {
          run = 16;
        } else {
          end_block = true;
          run = 0;
        }
      }
      if (k + run > 63) {
        if (!tolerant) {
          st |= SNJ_BAD_RUN;
          break;
        }
        run = 63 - k;          // a guess that ran past the block: the block ends with this symbol
      }
      k += run;
    }
    if (has_value) {
      int32_t v = 0;
      if (nbits) {
        v = (int32_t)(b.acc >> (64u - nbits));
        b.acc <<= nbits;
        b.cnt -= nbits;
        if (v < (1 << (nbits - 1))) v = v - (1 << nbits) + 1;
      }
      const int blkno = block0 + done;
      if (coef && blkno >= 0 && blkno < block_limit && (k == 0 || nbits)) coef[(long)blkno * 64 + kJpegNatural[k]] = (int16_t)v;
      ++k;
    }
    p = sn_jpeg_bitpos(b);
    if (p > b.end * 8u) {
      st |= SNJ_OVERRUN;
      break;
    }
    if (end_block || k > 63) {
      k = 0;
      blk = blk + 1 < c.bpm ? blk + 1 : 0;
      ++done;
    }
  }
  if (st) {
    *status |= st;
    out->p = kJpegNoState;
    out->bk = 0;
  } else {
    out->p = p;
    out->bk = (blk << 8) | k;
  }
  return done;
}
