// tensor_stats_plan.cpp -- the host side of the per-tensor statistics (tensor_stats.hip): the limits, the sizes, and the planner that
// turns a segment table into the work items the pass walks.  Plain C++, no device call and no HIP header: the same file is compiled
// with a main of its own under -fsanitize=address,undefined (tools/tensor_stats_plan_check.cpp).
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/sniper_hip.h"
#include "tensor_stats.h"

void sn_set_error(const char *fmt, ...);

#define TS_EXPORT extern "C" __attribute__((visibility("default")))
#define TS_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      sn_set_error(__VA_ARGS__);   \
      return SN_ERR_ARG;           \
    }                              \
  } while (0)

using namespace tstats;

TS_EXPORT int sn_tensor_stats_limits(int32_t *h_out6) {
  TS_REQUIRE(h_out6, "sn_tensor_stats_limits: null pointer");
  h_out6[0] = kSpan32;
  h_out6[1] = kChunk;
  h_out6[2] = kMaxTensors;
  h_out6[3] = kRecord;
  h_out6[4] = kSpan16;
  h_out6[5] = kDefaultBlocks;
  return SN_OK;
}

TS_EXPORT size_t sn_tensor_stats_plan_bytes(int T, int n_items) {
  if (T < 0 || T > kMaxTensors || n_items < 0) return 0;
  return plan_bytes(T, n_items);
}

TS_EXPORT size_t sn_tensor_stats_workspace_bytes(int T, int n_items) {
  if (T < 0 || T > kMaxTensors || n_items < 0) return 0;
  const size_t b = (size_t)n_items * kRecord * sizeof(double);
  return (std::max(b, (size_t)1) + 255) / 256 * 256;
}

// h_segs: T records {int64 off; int64 n}.  h_plan == NULL: the segments are checked and *h_n_items is the number of items the plan
// will hold; else the plan is written into plan_bytes bytes (at least sn_tensor_stats_plan_bytes(T, that number)).
TS_EXPORT int sn_tensor_stats_plan(const int64_t *h_segs, int T, void *h_plan, size_t plan_bytes_given, int32_t *h_n_items) {
  TS_REQUIRE(h_n_items, "sn_tensor_stats_plan: null h_n_items");
  TS_REQUIRE(T >= 0 && T <= kMaxTensors, "sn_tensor_stats_plan: T = %d outside 0 .. %d", T, kMaxTensors);
  TS_REQUIRE(h_segs || T == 0, "sn_tensor_stats_plan: null h_segs");
  int64_t items = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t off = h_segs[2 * t], n = h_segs[2 * t + 1];
    TS_REQUIRE(off >= 0 && n >= 0 && n <= INT64_MAX - off, "sn_tensor_stats_plan: segment %d = (%lld, %lld) is negative or overflows", t,
               (long long)off, (long long)n);
    items += n / kChunk + (n % kChunk != 0);
    TS_REQUIRE(items <= INT32_MAX, "sn_tensor_stats_plan: more than 2^31 - 1 work items");
  }
  // disjoint: sorted by offset, every non-empty segment ends at or before the next one begins
  std::vector<int> order;
  order.reserve((size_t)T);
  for (int t = 0; t < T; ++t)
    if (h_segs[2 * t + 1] > 0) order.push_back(t);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return h_segs[2 * a] < h_segs[2 * b]; });
  for (size_t k = 1; k < order.size(); ++k) {
    const int a = order[k - 1], b = order[k];
    TS_REQUIRE(h_segs[2 * a] + h_segs[2 * a + 1] <= h_segs[2 * b], "sn_tensor_stats_plan: segments %d = (%lld, %lld) and %d = (%lld, %lld) overlap",
               a, (long long)h_segs[2 * a], (long long)h_segs[2 * a + 1], b, (long long)h_segs[2 * b], (long long)h_segs[2 * b + 1]);
  }
  *h_n_items = (int32_t)items;
  if (!h_plan) return SN_OK;
  TS_REQUIRE(plan_bytes_given >= plan_bytes(T, (int)items), "sn_tensor_stats_plan: plan buffer of %zu bytes, %zu needed", plan_bytes_given,
             plan_bytes(T, (int)items));
  TS_REQUIRE(((uintptr_t)h_plan & 7) == 0, "sn_tensor_stats_plan: h_plan must be 8-byte aligned");
  Item *it = (Item *)h_plan;
  Tensor *tn = (Tensor *)(it + items);
  int32_t k = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t off = h_segs[2 * t], n = h_segs[2 * t + 1];
    tn[t].n = n;
    tn[t].first = k;
    for (int64_t o = 0; o < n; o += kChunk, ++k) {
      it[k].off = off + o;
      it[k].toff = o;
      it[k].len = (int32_t)std::min<int64_t>(kChunk, n - o);
      it[k].tensor = t;
      it[k].pad[0] = it[k].pad[1] = 0;
    }
    tn[t].count = k - tn[t].first;
  }
  return SN_OK;
}
