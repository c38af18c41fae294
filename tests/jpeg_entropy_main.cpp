// The stand-alone host program of sniper_amd/csrc/jpeg_entropy.h (tests/test_jpeg_cpu.py builds it with the sanitizers on).
// It reads jobs from standard input, one per five lines:
//   <mode> <bpm> <nluma> <sel> <sub> <nseg> <print>      mode: seq = every segment decoded in one span, the specification;
//                                                              rounds = the kernel's scheme on subsequences of <sub> bytes
//   <the four DHT tables, 4 * 272 bytes, in hex>
//   <the stream, in hex ('-' for an empty one)>
//   <first end blocks> per segment
// and prints per job: "<status> <total blocks> <rounds per segment ...>", then (print = 1) the coefficients with the DC values summed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../sniper_amd/csrc/jpeg_entropy.h"

static bool read_line(std::string &s) {
  s.clear();
  int ch;
  while ((ch = getchar()) != EOF && ch != '\n') s.push_back((char)ch);
  return ch != EOF || !s.empty();
}

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  auto d = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)(d(s[i]) * 16 + d(s[i + 1])));
  return v;
}

static bool same(const SnJpegState &a, const SnJpegState &b) { return a.p == b.p && a.bk == b.bk; }

int main() {
  std::string l1, l2, l3, l4;
  while (read_line(l1)) {
    if (l1.empty()) continue;
    if (!read_line(l2) || !read_line(l3) || !read_line(l4)) return 2;
    char mode[16];
    unsigned bpm, nluma, sel, sub, nseg, print;
    if (sscanf(l1.c_str(), "%15s %u %u %u %u %u %u", mode, &bpm, &nluma, &sel, &sub, &nseg, &print) != 7) return 2;
    if (bpm < 1 || bpm > (unsigned)kJpegMaxBpm || nluma < 1 || nluma > bpm || sub < 16 || nseg < 1) return 2;
    const std::vector<uint8_t> dht = unhex(l2);
    // the stream in an allocation of exactly its size: a read past it is the sanitizer's to find
    const std::vector<uint8_t> bytes = unhex(l3);
    if (dht.size() != 4 * kJpegDhtBytes) return 2;
    uint8_t *stream = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);
    if (bytes.size()) memcpy(stream, bytes.data(), bytes.size());
    std::vector<long> segs;
    {
      char *q = (char *)l4.c_str();
      for (;;) {
        char *e;
        const long v = strtol(q, &e, 10);
        if (e == q) break;
        segs.push_back(v);
        q = e;
      }
    }
    if (segs.size() != 3 * (size_t)nseg) return 2;
    SnJpegHuff huff[4];
    for (int t = 0; t < 4; ++t) sn_jpeg_build_table(dht.data() + t * kJpegDhtBytes, &huff[t]);
    long total = 0;
    for (unsigned s = 0; s < nseg; ++s) total += segs[3 * s + 2];
    int16_t *coef = (int16_t *)calloc((size_t)(total > 0 ? total : 1) * 64, sizeof(int16_t));
    int status = 0;
    std::vector<int> rounds(nseg, 1);
    long block_first = 0, decoded = 0;
    for (unsigned s = 0; s < nseg; ++s) {
      uint32_t first = (uint32_t)segs[3 * s], end = (uint32_t)segs[3 * s + 1];
      const int expect = (int)segs[3 * s + 2];
      if (end > bytes.size()) end = (uint32_t)bytes.size();          // what the kernel's entry point refuses is clamped here
      if (first > end) first = end;
      SnJpegCtx c;
      c.data = stream;
      c.end = end;
      c.huff = huff;
      c.bpm = bpm;
      c.nluma = nluma;
      c.sel = sel;
      int16_t *out = coef + block_first * 64;
      int got = 0;
      SnJpegState fin;
      if (!strcmp(mode, "seq")) {
        SnJpegState in = {first * 8u, 0u};
        got = sn_jpeg_decode_span(c, in, first, end, out, 0, expect, &fin, &status);
      } else {
        const uint32_t nsub = end - first > sub ? (end - first + sub - 1) / sub : 1;
        std::vector<SnJpegState> entry(nsub), ex[2];
        ex[0].resize(nsub);
        ex[1].resize(nsub);
        std::vector<int> n(nsub), base(nsub);
        int dummy = 0;
        auto lo = [&](uint32_t i) { return first + i * sub; };
        auto hi = [&](uint32_t i) { return i + 1 == nsub ? end : first + (i + 1) * sub; };
        for (uint32_t i = 0; i < nsub; ++i) {
          entry[i] = i == 0 ? SnJpegState{first * 8u, 0u} : sn_jpeg_guess(stream, first, lo(i), end);
          n[i] = sn_jpeg_decode_span(c, entry[i], lo(i), hi(i), nullptr, 0, kJpegNoLimit, &ex[0][i], &dummy);
        }
        int cur = 0;
        for (uint32_t t = 1; t < nsub; ++t) {
          const int prev = cur, next = cur ^ 1;
          bool changed = false;
          ex[next][0] = ex[prev][0];
          for (uint32_t i = 1; i < nsub; ++i) {
            const SnJpegState e = ex[prev][i - 1];
            if (!same(e, entry[i])) {
              entry[i] = e;
              n[i] = sn_jpeg_decode_span(c, e, lo(i), hi(i), nullptr, 0, kJpegNoLimit, &ex[next][i], &dummy);
              changed = true;
            } else {
              ex[next][i] = ex[prev][i];
            }
          }
          cur = next;
          if (!changed) break;
          ++rounds[s];
        }
        int run = 0;
        for (uint32_t i = 0; i < nsub; ++i) {
          base[i] = run;
          run += n[i];
        }
        // the lane whose span completes the segment's last block stops there; what the rounds counted after it was padding
        fin.p = kJpegNoState;
        fin.bk = 0;
        for (uint32_t i = 0; i < nsub; ++i) {
          SnJpegState o;
          const int n = sn_jpeg_decode_span(c, entry[i], lo(i), hi(i), out, base[i], expect, &o, &status);
          if (base[i] < expect) got = base[i] + n;
          if (base[i] < expect && base[i] + n == expect) fin = o;
        }
      }
      if (got != expect || fin.p == kJpegNoState || fin.bk != 0) status |= SNJ_BLOCKS;
      decoded += got;
      // DC: a running sum per component inside the segment
      int pred[kJpegMaxBpm] = {0};
      for (int b = 0; b < expect; ++b) {
        const unsigned j = (unsigned)b % bpm, comp = j < nluma ? 0 : 1 + j - nluma;
        pred[comp] += out[(long)b * 64];
        if (pred[comp] < -32768 || pred[comp] > 32767) status |= SNJ_BAD_DC;
        out[(long)b * 64] = (int16_t)pred[comp];
      }
      block_first += expect;
    }
    printf("%d %ld", status, decoded);
    for (unsigned s = 0; s < nseg; ++s) printf(" %d", rounds[s]);
    printf("\n");
    if (print) {
      for (long i = 0; i < total * 64; ++i) printf(i ? " %d" : "%d", coef[i]);
      printf("\n");
    }
    free(coef);
    free(stream);
  }
  return 0;
}
