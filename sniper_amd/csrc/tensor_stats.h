// tensor_stats.h -- what the planner (tensor_stats_plan.cpp, plain host C++: it is also compiled alone, under the sanitizers, by
// tools/tensor_stats_plan_check.cpp) and the kernels (tensor_stats.hip) of the per-tensor statistics share: the geometry, the
// layout of the plan, of a chunk's partial record and of the output.  Internal, not part of the C ABI.  No HIP header in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tstats {

constexpr int kThreads = 256;                    // threads per block
constexpr int kVec = 4;                          // 16-byte loads per lane per trip
constexpr int kSpan32 = kThreads * kVec * 4;     // fp32 elements per block trip
constexpr int kSpan16 = kThreads * kVec * 8;     // fp16 elements per block trip
constexpr int kChunk = 8 * kSpan32;              // elements of a work item (either dtype): 8 trips of fp32, 4 of fp16
constexpr int kMaxTensors = 65536;               // the header block keeps one bit per tensor in LDS (8 KiB)
constexpr int kRecord = 8;                       // doubles per output record, per header, per chunk partial
constexpr int kDefaultBlocks = 2048;             // the pass's grid cap (max_blocks = 0): eight blocks per CU
constexpr int kMaxBlocks = 65535;

// One work item: elements [off, off + len) of the arena are elements [toff, toff + len) of tensor `tensor`; len <= kChunk.
struct Item {
  int64_t off;
  int64_t toff;
  int32_t len;
  int32_t tensor;
  int32_t pad[2];
};
static_assert(sizeof(Item) == 32, "plan item is 32 bytes");

// One tensor: its length and its items, items[first .. first + count), in chunk order.
struct Tensor {
  int64_t n;
  int32_t first;
  int32_t count;
};
static_assert(sizeof(Tensor) == 16, "plan tensor is 16 bytes");

// The plan: n_items Item, then T Tensor.
inline size_t plan_bytes(int T, int n_items) { return (size_t)n_items * sizeof(Item) + (size_t)T * sizeof(Tensor); }

// A chunk's partial record in the workspace, eight 8-byte words: the same fields as an output record, the counts and the index as
// integers.  kNoIndex: no non-finite element.
enum { P_SUMSQ = 0, P_SUM = 1, P_BAD = 2, P_FIRST = 3, P_MAXABS = 4, P_ZEROS = 5 };
constexpr int64_t kNoIndex = INT64_MAX;

}  // namespace tstats
