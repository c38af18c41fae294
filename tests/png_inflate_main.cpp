// Stand-alone host program over sniper_amd/csrc/inflate_code.h, the zlib decoder the inflate kernel runs with one wave per stream
// (tests/test_png_dec_cpu.py compiles and runs it, a second time under -fsanitize=address,undefined).  One stream per line on stdin:
//   <capacity> <the stream's bytes in hex, or - for none>
// -> "<status> <bytes produced> <1: the guard bytes behind the capacity are untouched> <the output in hex, or ->"
// The input lies in a heap block of exactly its size and the output in one of capacity + 32 bytes: a read past the stream or a store
// past the guard is the sanitizer's to report, a store into the guard this program's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../sniper_amd/csrc/inflate_code.h"

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main() {
  static SnInflateTables T;
  const int kGuard = 32;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    long cap = -1;
    std::string hex;
    if (!(in >> cap >> hex)) continue;
    if (cap < 0 || cap > (1L << 28)) return 2;
    if (hex == "-") hex.clear();
    if (hex.size() % 2) return 3;
    const size_t n = hex.size() / 2;
    uint8_t *src = (uint8_t *)std::malloc(n ? n : 1);
    uint8_t *dst = (uint8_t *)std::malloc((size_t)cap + kGuard);
    if (!src || !dst) return 4;
    for (size_t i = 0; i < n; ++i) {
      const int hi = nibble(hex[2 * i]), lo = nibble(hex[2 * i + 1]);
      if (hi < 0 || lo < 0) return 5;
      src[i] = (uint8_t)(hi * 16 + lo);
    }
    std::memset(dst, 0xA5, (size_t)cap + kGuard);
    SnByteSink sink;
    sink.init(dst, (int)cap);
    const int status = sn_inflate_zlib(src, (int)n, sink, T);
    int guard = 1;
    for (int i = 0; i < kGuard; ++i) guard &= dst[cap + i] == 0xA5;
    std::printf("%d %d %d ", status, sink.pos(), guard);
    if (sink.pos() == 0) std::printf("-");
    static const char *digits = "0123456789abcdef";
    std::string outhex((size_t)sink.pos() * 2, '0');
    for (int i = 0; i < sink.pos(); ++i) {
      outhex[2 * i] = digits[dst[i] >> 4];
      outhex[2 * i + 1] = digits[dst[i] & 15];
    }
    std::printf("%s\n", outhex.c_str());
    std::free(src);
    std::free(dst);
  }
  return 0;
}
