// Stand-alone host program over sniper_amd/csrc/huff_code.h, the code construction the deflate kernel runs on one lane
// (tests/test_png_cpu.py compiles and runs it; it is also what a sanitizer build would run).  Commands on stdin, one per line:
//   lens  <maxbits> <nsym> <freq ...>     -> "<kraft units> <len ...>"        (sn_huff_from_hist; kraft in units of 2^-maxbits)
//   block <final> <286 freqs>             -> "<hdr_bits> <total_bits> <n hdr words> <hdr words ...> <286 lens> <286 reversed codes>"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../sniper_amd/csrc/huff_code.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "lens") {
      int maxbits = 0, nsym = 0;
      in >> maxbits >> nsym;
      if (nsym < 1 || nsym > kHuffMaxSyms || maxbits < 1 || maxbits > kHuffMaxBits) return 2;
      std::vector<uint32_t> hist(nsym), fs(nsym), w(2 * nsym);
      std::vector<uint16_t> order(nsym), par(2 * nsym);
      std::vector<uint8_t> lens(nsym), ls(nsym);
      for (int i = 0; i < nsym; ++i) in >> hist[i];
      sn_huff_from_hist(hist.data(), nsym, maxbits, lens.data(), fs.data(), order.data(), ls.data(), w.data(), par.data());
      std::printf("%ld", sn_huff_kraft(lens.data(), nsym, maxbits));
      for (int i = 0; i < nsym; ++i) std::printf(" %d", (int)lens[i]);
      std::printf("\n");
    } else if (cmd == "block") {
      int final_block = 0;
      in >> final_block;
      static SnBlockCode C;
      std::memset(&C, 0, sizeof(C));
      for (int i = 0; i < kDeflateLitSyms; ++i) in >> C.hist[i];
      // the rank sort the workgroup does in parallel
      for (int i = 0; i < kDeflateLitSyms; ++i) {
        if (!C.hist[i]) continue;
        int rank = 0;
        for (int j = 0; j < kDeflateLitSyms; ++j)
          rank += (C.hist[j] != 0) && (C.hist[j] < C.hist[i] || (C.hist[j] == C.hist[i] && j < i));
        C.fs[rank] = C.hist[i];
        C.order[rank] = (uint16_t)i;
        C.n_used += 1;
      }
      if (C.n_used < 2) return 3;
      int hb = 0;
      const unsigned long long bits = sn_deflate_block_code(C, final_block, hb);
      const int nw = (hb + 31) / 32;
      std::printf("%d %llu %d", hb, bits, nw);
      for (int i = 0; i < nw; ++i) std::printf(" %u", C.hdr[i]);
      for (int i = 0; i < kDeflateLitSyms; ++i) std::printf(" %d", (int)C.lens[i]);
      for (int i = 0; i < kDeflateLitSyms; ++i) std::printf(" %d", (int)C.codes[i]);
      std::printf("\n");
    } else {
      return 4;
    }
  }
  return 0;
}
