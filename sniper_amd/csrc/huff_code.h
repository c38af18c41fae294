// huff_code.h -- the length-limited prefix code of the deflate coder (png_encode.hip).  Plain C++ that compiles
// for the host and for the device: the kernel runs it on one lane, tests/test_png_cpu.py compiles it into a stand-alone program.
// Internal, not part of the C ABI.  Every loop has a bound that depends on the alphabet size and the length limit only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SN_HD __host__ __device__ inline
#else
#define SN_HD inline
#endif

constexpr int kHuffMaxSyms = 288;      // the largest alphabet (286 literal/length symbols, rounded up)
constexpr int kHuffMaxBits = 15;

// Code lengths of n >= 1 symbols whose frequencies fs[0 .. n) > 0 are sorted ascending (ties: by symbol index ascending, the caller's
// order) -> ls[0 .. n), 1 <= ls[i] <= maxbits, sum 2^-ls[i] == 1 exactly for n >= 2 (n == 1: the one length 1).
// Needs 2^maxbits >= n.  Scratch: w[2n] and par[2n].
//   1. Huffman's tree by the two-queue merge: nodes 0 .. n-1 are the leaves in the given order, node n + k is made at step k from the
//      two smallest heads of (leaf queue, internal queue); where a leaf and an internal node weigh the same the LEAF is taken.
//   2. Depths from the root down (a parent's index is above its children's).
//   3. Depths above maxbits are set to maxbits; that over-subscribes the code by fewer units of 2^-maxbits than symbols were moved
//      (each moved symbol weighed > 0 before and weighs 1 unit now, and the tree was complete), so at most n - 1 repair steps follow.
//      A step takes one code away from length maxbits, and splits the deepest code shorter than maxbits into two codes one bit longer:
//      the symbol count stays, the sum drops by exactly one unit.  A shorter code exists whenever the sum is too large, since n codes
//      of length maxbits alone sum to n <= 2^maxbits units.
//   4. Lengths are dealt in the given order, longest first: the rarest symbol gets the longest code.
SN_HD void sn_huff_sorted(const uint32_t *fs, int n, int maxbits, uint8_t *ls, uint32_t *w, uint16_t *par) {
  if (n == 1) {
    ls[0] = 1;
    return;
  }
  for (int i = 0; i < n; ++i) w[i] = fs[i];
  int li = 0, ii = n;
  for (int k = 0; k < n - 1; ++k) {
    const int node = n + k;
    uint32_t sum = 0;
    for (int pick = 0; pick < 2; ++pick) {
      const bool leaf = li < n && (ii >= node || w[li] <= w[ii]);
      const int c = leaf ? li++ : ii++;
      sum += w[c];
      par[c] = (uint16_t)node;
    }
    w[node] = sum;
  }
  w[2 * n - 2] = 0;                                   // the weights are spent: w now holds depths
  for (int i = 2 * n - 3; i >= 0; --i) w[i] = w[par[i]] + 1;
  int cnt[kHuffMaxBits + 1];
  for (int l = 0; l <= kHuffMaxBits; ++l) cnt[l] = 0;
  for (int i = 0; i < n; ++i) {
    const int d = (int)w[i] < maxbits ? (int)w[i] : maxbits;
#pragma unroll
    for (int l = 1; l <= kHuffMaxBits; ++l) cnt[l] += (l == d);          // (no dynamic index: cnt stays in registers on the device)
  }
  long total = 0;
#pragma unroll
  for (int l = 1; l <= kHuffMaxBits; ++l)
    if (l <= maxbits) total += (long)cnt[l] << (maxbits - l);
  const long full = 1L << maxbits;
  for (int it = 0; it < n; ++it) {
    if (total <= full) break;
    bool done = false;
#pragma unroll
    for (int l = kHuffMaxBits - 1; l >= 1; --l) {
      if (l < maxbits && !done && cnt[l] > 0) {
        cnt[l] -= 1;
        cnt[l + 1] += 2;
        done = true;
      }
    }
#pragma unroll
    for (int l = 1; l <= kHuffMaxBits; ++l) cnt[l] -= (l == maxbits);
    total -= 1;
  }
  int at = 0;
#pragma unroll
  for (int l = kHuffMaxBits; l >= 1; --l) {
    const int c = l <= maxbits ? cnt[l] : 0;
    for (int j = 0; j < kHuffMaxSyms; ++j) {
      if (j >= c) break;
      if (at < n) ls[at++] = (uint8_t)l;
    }
  }
}

// The whole construction from a histogram, sequentially: hist[0 .. nsym) -> lens[0 .. nsym) (0 where hist is 0).  The symbols that
// occur are ordered by (frequency, symbol index) ascending.  Scratch: fs[nsym], order[nsym], ls[nsym], w[2 nsym], par[2 nsym].
SN_HD int sn_huff_from_hist(const uint32_t *hist, int nsym, int maxbits, uint8_t *lens, uint32_t *fs, uint16_t *order, uint8_t *ls,
                            uint32_t *w, uint16_t *par) {
  int n = 0;
  for (int i = 0; i < nsym; ++i) {
    lens[i] = 0;
    if (!hist[i]) continue;
    int rank = 0;
    for (int j = 0; j < nsym; ++j) rank += (hist[j] != 0) & ((hist[j] < hist[i]) | ((hist[j] == hist[i]) & (j < i)));
    fs[rank] = hist[i];
    order[rank] = (uint16_t)i;
    ++n;
  }
  if (n == 0) return 0;
  sn_huff_sorted(fs, n, maxbits, ls, w, par);
  for (int i = 0; i < n; ++i) lens[order[i]] = ls[i];
  return n;
}

// RFC 1951 3.2.2: canonical codes of lens[0 .. nsym), each reversed (deflate packs codes from their most significant bit, and the
// packer here shifts least significant bits out first) -> codes[i] (unspecified where lens[i] == 0).
SN_HD void sn_huff_codes(const uint8_t *lens, int nsym, uint16_t *codes) {
  int cnt[kHuffMaxBits + 2];
  for (int l = 0; l <= kHuffMaxBits + 1; ++l) cnt[l] = 0;
  for (int i = 0; i < nsym; ++i) {
    const int d = lens[i];
#pragma unroll
    for (int l = 1; l <= kHuffMaxBits; ++l) cnt[l] += (l == d);
  }
  int next[kHuffMaxBits + 2];
  int code = 0;
  next[0] = 0;
#pragma unroll
  for (int l = 1; l <= kHuffMaxBits; ++l) {
    code = (code + cnt[l - 1]) << 1;
    next[l] = code;
  }
  for (int i = 0; i < nsym; ++i) {
    const int d = lens[i];
    int c = 0;
#pragma unroll
    for (int l = 1; l <= kHuffMaxBits; ++l) {
      if (l == d) {
        c = next[l];
        next[l] += 1;
      }
    }
    int r = 0;
    for (int b = 0; b < kHuffMaxBits; ++b)
      if (b < d) r |= ((c >> b) & 1) << (d - 1 - b);
    codes[i] = (uint16_t)r;
  }
}

// Sum over the used symbols of 2^(maxbits - len): == 2^maxbits for a complete code.
SN_HD long sn_huff_kraft(const uint8_t *lens, int nsym, int maxbits) {
  long t = 0;
  for (int i = 0; i < nsym; ++i)
    if (lens[i]) t += 1L << (maxbits - lens[i]);
  return t;
}

// ---- one deflate block's code, from the histogram of its tokens ------------------------------------------------------------------
constexpr int kDeflateLitSyms = 286;
constexpr int kDeflateClenSyms = 19;
constexpr int kDeflateHdrWords = 72;      // 17 + 19 * 3 + 287 * 7 = 2083 bits at the most

struct SnBlockCode {
  uint32_t hist[kHuffMaxSyms];            // in: the tokens' literal/length symbols, the end-of-block symbol counted once
  uint32_t fs[kHuffMaxSyms];              // in: the frequencies that occur, sorted by (frequency, symbol) ascending ...
  uint16_t order[kHuffMaxSyms];           // in: ... and their symbols
  int n_used;                             // in: how many occur
  uint32_t w[2 * kHuffMaxSyms];
  uint16_t par[2 * kHuffMaxSyms];
  uint8_t ls[kHuffMaxSyms];
  uint8_t lens[kHuffMaxSyms];             // out: code lengths (zeroed by the caller)
  uint16_t codes[kHuffMaxSyms];           // out: reversed codes
  uint32_t chist[32];                     // (zeroed by the caller)
  uint32_t cfs[32];
  uint16_t corder[32];
  uint16_t ccodes[32];
  uint8_t cls[32];
  uint8_t clens[32];
  uint32_t hdr[kDeflateHdrWords];         // out: the block header's bits (zeroed by the caller)
};

SN_HD void sn_put_bits(uint32_t *hdr, int &at, uint32_t v, int n) {
  const int w = at >> 5, sh = at & 31;
  hdr[w] |= v << sh;
  if (sh + n > 32) hdr[w + 1] |= v >> (32 - sh);
  at += n;
}

// extra bits of a literal/length symbol
SN_HD int sn_length_extra_bits(int sym) { return (sym >= 265 && sym < 285) ? (sym - 261) >> 2 : 0; }

// -> the bits of the whole block (header, tokens, end of block); hdr_bits = those of the header.  The header: BFINAL, BTYPE 2,
// HLIT = 29 (all 286 lengths), HDIST = 0 (one distance length: 1 where the block has a match, else 0), HCLEN = 15 (all 19), the
// code-length code's lengths in the order of RFC 1951 3.2.7, then the 287 lengths coded one by one (no repeat symbols).  Where all
// 287 lengths were equal a second code-length symbol would be forced, so that the code-length code is complete too.
SN_HD unsigned long long sn_deflate_block_code(SnBlockCode &L, int final_block, int &hdr_bits) {
  const uint8_t clen_order[kDeflateClenSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  const int n = L.n_used;
  sn_huff_sorted(L.fs, n, kHuffMaxBits, L.ls, L.w, L.par);
  for (int i = 0; i < kDeflateLitSyms; ++i)
    if (i < n) L.lens[L.order[i]] = L.ls[i];
  sn_huff_codes(L.lens, kDeflateLitSyms, L.codes);
  uint32_t matches = 0;
  for (int i = 257; i < kDeflateLitSyms; ++i) matches += L.hist[i];
  const int dist_len = matches ? 1 : 0;
  for (int i = 0; i < kDeflateLitSyms; ++i) L.chist[L.lens[i]] += 1;
  L.chist[dist_len] += 1;
  int kinds = 0;
  for (int i = 0; i < kDeflateClenSyms; ++i) kinds += L.chist[i] != 0;
  if (kinds < 2) L.chist[L.chist[0] ? 1 : 0] = 1;
  sn_huff_from_hist(L.chist, kDeflateClenSyms, 7, L.clens, L.cfs, L.corder, L.cls, L.w, L.par);
  sn_huff_codes(L.clens, kDeflateClenSyms, L.ccodes);
  int hb = 0;
  sn_put_bits(L.hdr, hb, (final_block ? 1u : 0u) | (2u << 1), 3);
  sn_put_bits(L.hdr, hb, kDeflateLitSyms - 257, 5);
  sn_put_bits(L.hdr, hb, 0, 5);
  sn_put_bits(L.hdr, hb, kDeflateClenSyms - 4, 4);
  for (int i = 0; i < kDeflateClenSyms; ++i) sn_put_bits(L.hdr, hb, L.clens[clen_order[i]], 3);
  unsigned long long bits = 0;
  for (int i = 0; i < kDeflateLitSyms; ++i) {
    const int l = L.lens[i];
    sn_put_bits(L.hdr, hb, L.ccodes[l], L.clens[l]);
    bits += (unsigned long long)L.hist[i] * (unsigned)(l + sn_length_extra_bits(i));
  }
  sn_put_bits(L.hdr, hb, L.ccodes[dist_len], L.clens[dist_len]);
  hdr_bits = hb;
  return bits + (unsigned long long)hb + matches;
}
