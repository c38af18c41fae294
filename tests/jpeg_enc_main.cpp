// Stand-alone host program over sniper_amd/csrc/jpeg_enc_code.h, the per-block code of the JPEG encoder's kernels; built and run by
// tests/test_jpeg_enc_cpu.py under the address and undefined-behaviour sanitizers.  Jobs on stdin, one answer per job on stdout:
//   recip                                   every n = |c| + (d >> 1), |c| <= 8192, d = 8 .. 2040: the reciprocal's quotient against n / d
//                                           -> "pairs mismatches"
//   quant Q T N, then a line of N * 64      N blocks of samples (0 .. 255, natural order) through the forward DCT and table T at quality Q
//                                           -> N * 64 quantised coefficients in zig-zag order
//   scan N NLUMA BPM SHORT, then N * 64     N blocks (zig-zag, DC not differenced) of a scan whose MCUs hold NLUMA luma blocks of BPM: every
//                                           block sized, the sizes scanned, every block written on its own at its bit offset into a zeroed
//                                           buffer of exactly the reported size less SHORT bytes (as the write kernel does, in any order)
//                                           -> "err bytes", the sizes, the bytes in hex
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../sniper_amd/csrc/jpeg_enc_code.h"

static bool read_ints(std::vector<int> &v, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i)
    if (scanf("%d", &v[i]) != 1) return false;
  return true;
}

int main() {
  SnJpegEncTables T;
  for (int t = 0; t < 4; ++t) sn_jpeg_enc_build_table(&T, t);
  char job[32];
  while (scanf("%31s", job) == 1) {
    if (!strcmp(job, "recip")) {
      long pairs = 0, bad = 0;
      for (uint32_t d = 8; d <= 2040; d += 8) {
        const uint32_t m = sn_jpeg_enc_recip(d);
        for (int c = -8192; c <= 8192; ++c) {
          const uint32_t n = (uint32_t)(c < 0 ? -c : c) + (d >> 1);
          const int want = (int)(n / d);
          ++pairs;
          if (sn_jpeg_enc_quantise(c, d, m) != (c < 0 ? -want : want)) ++bad;
        }
      }
      // and the whole range the derivation covers
      for (uint32_t d = 8; d <= 2040; ++d)
        for (uint32_t n = 0; n < (1u << 14); ++n, ++pairs)
          if (sn_jpeg_enc_mulhi(n, sn_jpeg_enc_recip(d)) != n / d) ++bad;
      printf("%ld %ld\n", pairs, bad);
    } else if (!strcmp(job, "quant")) {
      int q, t, n;
      std::vector<int> s;
      if (scanf("%d %d %d", &q, &t, &n) != 3 || n < 0 || n > 100000 || !read_ints(s, (size_t)n * 64)) return 2;
      for (int b = 0; b < n; ++b) {
        int d[64];
        for (int i = 0; i < 64; ++i) d[i] = s[(size_t)b * 64 + i] - 128;
        sn_jpeg_enc_fdct(d);
        for (int zz = 0; zz < 64; ++zz) {
          const uint32_t dv = 8u * (uint32_t)sn_jpeg_enc_quant_entry(t, zz, q);
          printf("%d ", sn_jpeg_enc_quantise(d[kJpegEncNatural[zz]], dv, sn_jpeg_enc_recip(dv)));
        }
      }
      printf("\n");
    } else if (!strcmp(job, "scan")) {
      int n, nluma, bpm, cut;
      std::vector<int> s;
      if (scanf("%d %d %d %d", &n, &nluma, &bpm, &cut) != 4 || n < 1 || n > 100000 || bpm < 1 || nluma < 1 || nluma > bpm ||
          !read_ints(s, (size_t)n * 64))
        return 2;
      std::vector<int16_t> coef((size_t)n * 64);
      for (size_t i = 0; i < coef.size(); ++i) coef[i] = (int16_t)s[i];
      auto pred_of = [&](int b) {
        const int k = b % bpm;
        int pb;
        if (k < nluma) pb = k > 0 ? b - 1 : (b < bpm ? -1 : b - bpm + nluma - 1);
        else pb = b < bpm ? -1 : b - bpm;
        return pb >= 0 ? (int)coef[(size_t)pb * 64] : 0;
      };
      std::vector<long> size(n), at(n + 1, 0);
      int err = 0;
      for (int b = 0; b < n; ++b) {
        SnJpegEncCount c;
        sn_jpeg_enc_block(&coef[(size_t)b * 64], pred_of(b), b % bpm >= nluma, T, c);
        size[b] = c.bits;
        err |= c.err;
        at[b + 1] = at[b] + c.bits;
      }
      const long bytes = (at[n] + 7) / 8, words = (bytes + 3) / 4;
      const long cap_bytes = 4 * words - cut, cap_words = cap_bytes / 4;
      // exactly the capacity: the sanitizer has the byte behind it
      uint32_t *raw = (uint32_t *)calloc(cap_words > 0 ? (size_t)cap_words : 1, 4);
      for (int b = n - 1; b >= 0; --b) {          // (backwards: the order must not matter)
        SnJpegEncWriter wr(raw, cap_words, at[b]);
        sn_jpeg_enc_block(&coef[(size_t)b * 64], pred_of(b), b % bpm >= nluma, T, wr);
        if (b == n - 1) sn_jpeg_enc_fill(wr.bitpos(), wr);
        wr.finish();
        err |= wr.err;
      }
      printf("%d %ld\n", err, bytes);
      for (int b = 0; b < n; ++b) printf("%ld ", size[b]);
      printf("\n");
      const unsigned char *p = (const unsigned char *)raw;
      for (long i = 0; i < bytes && i < 4 * cap_words; ++i) printf("%02x", p[i]);
      printf("\n");
      free(raw);
    } else {
      return 2;
    }
  }
  return 0;
}
