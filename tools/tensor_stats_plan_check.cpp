// tensor_stats_plan_check.cpp -- the planner of the per-tensor statistics (sniper_amd/csrc/tensor_stats_plan.cpp, plain host C++) under
// the sanitizers, as a stand-alone program on the CPU:
//
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/tensor_stats_plan_check.cpp sniper_amd/csrc/tensor_stats_plan.cpp -o plan_check && ./plan_check
//
// It plans the tables the tests use -- empty tensors, one tensor of many chunks, 1000 one-element tensors, T at the limit, the edge
// table of the device test, tables that must be refused -- into buffers of EXACTLY the size the library asks for, and checks that every
// element of every segment lies in exactly one item of its own tensor.  Exit status 0 and "ok" when all of it holds.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/sniper_hip.h"
#include "../sniper_amd/csrc/tensor_stats.h"

static char g_err[512];
void sn_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, g_err); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

using tstats::Item;
using tstats::Tensor;

static int plan_and_verify(const std::vector<int64_t> &segs) {
  const int T = (int)(segs.size() / 2);
  int32_t n_items = -1;
  CHECK(sn_tensor_stats_plan(segs.data(), T, nullptr, 0, &n_items) == SN_OK);
  const size_t bytes = sn_tensor_stats_plan_bytes(T, n_items);
  CHECK(bytes == (size_t)n_items * 32 + (size_t)T * 16);
  int64_t *buf = (int64_t *)malloc(bytes ? bytes : 1);       // exactly as large as asked for: a write past it is the sanitizer's
  int32_t again = -1;
  CHECK(sn_tensor_stats_plan(segs.data(), T, buf, bytes, &again) == SN_OK && again == n_items);
  if (bytes >= 8) CHECK(sn_tensor_stats_plan(segs.data(), T, buf, bytes - 8, &again) == SN_ERR_ARG);
  const Item *it = (const Item *)buf;
  const Tensor *tn = (const Tensor *)(it + n_items);
  int32_t k = 0;
  for (int t = 0; t < T; ++t) {
    CHECK(tn[t].n == segs[2 * t + 1] && tn[t].first == k);
    int64_t covered = 0;
    for (int32_t j = 0; j < tn[t].count; ++j, ++k) {
      CHECK(k < n_items && it[k].tensor == t && it[k].toff == covered && it[k].off == segs[2 * t] + covered);
      CHECK(it[k].len >= 1 && it[k].len <= tstats::kChunk && (it[k].len == tstats::kChunk || j == tn[t].count - 1));
      covered += it[k].len;
    }
    CHECK(covered == tn[t].n);
  }
  CHECK(k == n_items);
  CHECK(sn_tensor_stats_workspace_bytes(T, n_items) >= (size_t)n_items * 64);
  free(buf);
  return n_items;
}

int main() {
  int32_t lim[6];
  CHECK(sn_tensor_stats_limits(lim) == SN_OK);
  const int64_t S = lim[0], C = lim[1], S16 = lim[4];
  const int maxT = lim[2];
  CHECK(lim[3] == 8 && C % S == 0 && C % S16 == 0 && maxT >= 1000);
  int32_t n = -1;
  CHECK(sn_tensor_stats_plan(nullptr, 0, nullptr, 0, &n) == SN_OK && n == 0);
  CHECK(plan_and_verify({}) == 0);
  CHECK(plan_and_verify({0, 0, 5, 0, 5, 0}) == 0);                                // empty tensors, two at one offset
  CHECK(plan_and_verify({3, 100 * C + 17}) == 101);                                // one tensor of many chunks
  std::vector<int64_t> ones, edge, full;
  for (int t = 0; t < 1000; ++t) {
    ones.push_back(999 - t);
    ones.push_back(1);
  }
  CHECK(plan_and_verify(ones) == 1000);                                            // 1000 one-element tensors, descending offsets
  int64_t off = 0;
  int want = 0;
  const int64_t lens[] = {0, 1, 3, 4, 7, 8, 15, 16, S - 1, S, S + 1, S16 - 1, S16, S16 + 1, C - 1, C, C + 1, 3 * C + 5};
  for (size_t k = 0; k < sizeof(lens) / sizeof(lens[0]); ++k) {
    off += 1 + (int64_t)(k % 9);
    edge.push_back(off);
    edge.push_back(lens[k]);
    off += lens[k];
    want += (int)((lens[k] + C - 1) / C);
  }
  CHECK(plan_and_verify(edge) == want);                                            // the edge table of the device test
  for (int t = 0; t < maxT; ++t) {
    full.push_back((int64_t)t * 8);
    full.push_back(t % 8);
  }
  CHECK(plan_and_verify(full) == maxT - maxT / 8);                                 // T at the limit
  full.push_back((int64_t)maxT * 8);
  full.push_back(1);
  CHECK(sn_tensor_stats_plan(full.data(), maxT + 1, nullptr, 0, &n) == SN_ERR_ARG && strstr(g_err, "outside"));
  const int64_t over[] = {0, 10, 20, 5, 9, 3}, neg[] = {-1, 4}, negn[] = {0, -4}, wrap[] = {INT64_MAX - 2, 5}, touch[] = {0, 10, 10, 5};
  CHECK(sn_tensor_stats_plan(over, 3, nullptr, 0, &n) == SN_ERR_ARG && strstr(g_err, "overlap"));
  CHECK(sn_tensor_stats_plan(neg, 1, nullptr, 0, &n) == SN_ERR_ARG);
  CHECK(sn_tensor_stats_plan(negn, 1, nullptr, 0, &n) == SN_ERR_ARG);
  CHECK(sn_tensor_stats_plan(wrap, 1, nullptr, 0, &n) == SN_ERR_ARG);
  CHECK(sn_tensor_stats_plan(touch, 2, nullptr, 0, &n) == SN_OK && n == 2);
  CHECK(sn_tensor_stats_plan(touch, 2, nullptr, 0, nullptr) == SN_ERR_ARG);
  CHECK(sn_tensor_stats_plan(nullptr, 2, nullptr, 0, &n) == SN_ERR_ARG);
  CHECK(sn_tensor_stats_plan_bytes(-1, 0) == 0 && sn_tensor_stats_workspace_bytes(maxT + 1, 0) == 0);
  puts("ok");
  return 0;
}
