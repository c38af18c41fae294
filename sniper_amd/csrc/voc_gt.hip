// voc_gt.hip -- the ground truth of the VOC mask evaluation from its two index maps: what the reference's
// parse_inst (lib/dataset/pascal_voc_eval.py:275-318) cuts on the host with one np.where per instance.
//
//   voc_inst_scan_kernel   one workgroup per image: per instance id 1 .. 255 the bound (min / max column and row) and the smallest and
//                          largest class under its pixels, by LDS min / max; an id whose two classes differ is flagged.
//   voc_inst_crop_kernel   the instances' boolean bitmaps, cropped to their bounds, into one pool at the caller's scanned offsets.
// No global atomics; the same bytes every run.
#include "common.h"

namespace {

constexpr int kIds = 256;
constexpr int kInstFields = 6;          // x1, y1, x2, y2, class, flag; x2 = -1: no such id in the image
constexpr int kRecFields = 6;           // image, id, x1, y1, bound width, bound height
constexpr int kMaxImages = 65535;
constexpr int kMaxRecs = kMaxImages * 255;
constexpr int kScanThreads = 256;

__global__ __launch_bounds__(kScanThreads) void voc_inst_scan_kernel(const uint64_t *__restrict__ obj_ptrs, const uint64_t *__restrict__ cls_ptrs,
                                                                     const int32_t *__restrict__ hw, int I, int32_t *__restrict__ inst) {
  __shared__ int x1[kIds], y1[kIds], x2[kIds], y2[kIds], c1[kIds], c2[kIds];
  const int i = blockIdx.x;
  if (i >= I) return;
  const int h = hw[2 * i], w = hw[2 * i + 1];
  const uint8_t *obj = reinterpret_cast<const uint8_t *>(obj_ptrs[i]);
  const uint8_t *cls = reinterpret_cast<const uint8_t *>(cls_ptrs[i]);
  for (int k = threadIdx.x; k < kIds; k += kScanThreads) {
    x1[k] = y1[k] = c1[k] = 0x7fffffff;
    x2[k] = y2[k] = c2[k] = -1;
  }
  __syncthreads();
  const long long pixels = (long long)h * w;
  for (long long p = threadIdx.x; p < pixels; p += kScanThreads) {
    const int id = obj[p];
    if (id == 0) continue;          // the background
    const int y = (int)(p / w), x = (int)(p - (long long)y * w), c = cls[p];
    atomicMin(&x1[id], x);
    atomicMax(&x2[id], x);
    atomicMin(&y1[id], y);
    atomicMax(&y2[id], y);
    atomicMin(&c1[id], c);
    atomicMax(&c2[id], c);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kIds; k += kScanThreads) {
    int32_t *o = inst + ((long long)i * kIds + k) * kInstFields;
    const bool there = k > 0 && x2[k] >= 0;
    o[0] = there ? x1[k] : 0;
    o[1] = there ? y1[k] : 0;
    o[2] = there ? x2[k] : -1;
    o[3] = there ? y2[k] : -1;
    o[4] = there ? c1[k] : 0;
    o[5] = there && c1[k] != c2[k] ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void voc_inst_crop_kernel(const uint64_t *__restrict__ obj_ptrs, const int32_t *__restrict__ hw,
                                                            const int32_t *__restrict__ rec, const int64_t *__restrict__ pool_off,
                                                            uint8_t *__restrict__ pool, long long pool_total) {
  const int n = blockIdx.y;
  const int i = rec[kRecFields * n], id = rec[kRecFields * n + 1], bx = rec[kRecFields * n + 2], by = rec[kRecFields * n + 3];
  const int bw = rec[kRecFields * n + 4], bh = rec[kRecFields * n + 5];
  const int w = hw[2 * i + 1];
  const uint8_t *obj = reinterpret_cast<const uint8_t *>(obj_ptrs[i]);
  const long long base = pool_off[n], area = (long long)bw * bh;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < area; q += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(q / bw), x = (int)(q - (long long)y * bw);
    if (base + q < pool_total) pool[base + q] = obj[(long long)(by + y) * w + bx + x] == id ? 1 : 0;
  }
}

const char *bad_sizes(const int32_t *h_hw, int I) {
  for (int i = 0; i < I; ++i) {
    const long long h = h_hw[2 * i], w = h_hw[2 * i + 1];
    if (h < 1 || w < 1 || h * w >= (1LL << 31)) return "h >= 1, w >= 1, h * w < 2^31 required of every map";
  }
  return nullptr;
}

}  // namespace

SN_EXPORT int sn_vocgt_scan(const uint64_t *obj_ptrs, const uint64_t *cls_ptrs, const int32_t *hw, const int32_t *h_hw, int I,
                               int32_t *inst, sn_stream_t stream) {
  SN_REQUIRE(obj_ptrs && cls_ptrs && hw && h_hw && inst, "sn_vocgt_scan: null pointer");
  SN_REQUIRE(I >= 1 && I <= kMaxImages, "sn_vocgt_scan: 1 <= I <= %d required (I = %d)", kMaxImages, I);
  const char *why = bad_sizes(h_hw, I);
  SN_REQUIRE(!why, "sn_vocgt_scan: %s", why);
  hipLaunchKernelGGL(voc_inst_scan_kernel, dim3((unsigned)I), dim3(kScanThreads), 0, sn_stream(stream), obj_ptrs, cls_ptrs, hw, I, inst);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_vocgt_crop(const uint64_t *obj_ptrs, const int32_t *hw, const int32_t *h_hw, int I, const int32_t *rec,
                               const int32_t *h_rec, const int64_t *pool_off, const int64_t *h_pool_off, long N, uint8_t *pool,
                               long pool_total, sn_stream_t stream) {
  SN_REQUIRE(obj_ptrs && hw && h_hw && rec && h_rec && pool_off && h_pool_off && pool, "sn_vocgt_crop: null pointer");
  SN_REQUIRE(I >= 1 && I <= kMaxImages, "sn_vocgt_crop: 1 <= I <= %d required (I = %d)", kMaxImages, I);
  SN_REQUIRE(N >= 1 && N <= kMaxRecs && N <= 65535, "sn_vocgt_crop: 1 <= N <= 65535 required (N = %ld)", N);
  const char *why = bad_sizes(h_hw, I);
  SN_REQUIRE(!why, "sn_vocgt_crop: %s", why);
  long long at = 0, most = 1;
  for (long n = 0; n < N; ++n) {
    const int32_t *r = h_rec + kRecFields * n;
    SN_REQUIRE(r[0] >= 0 && r[0] < I && r[1] >= 1 && r[1] <= 255, "sn_vocgt_crop: record %ld names image %d and id %d", n, r[0], r[1]);
    const long long h = h_hw[2 * r[0]], w = h_hw[2 * r[0] + 1];
    SN_REQUIRE(r[2] >= 0 && r[3] >= 0 && r[4] >= 1 && r[5] >= 1 && (long long)r[2] + r[4] <= w && (long long)r[3] + r[5] <= h,
               "sn_vocgt_crop: the bound of record %ld (%d, %d, %d x %d) leaves its %lld x %lld map", n, r[2], r[3], r[4], r[5], h, w);
    SN_REQUIRE(h_pool_off[n] == at, "sn_vocgt_crop: pool_off[%ld] = %ld, the bounds before it give %lld", n, (long)h_pool_off[n], at);
    at += (long long)r[4] * r[5];
    if ((long long)r[4] * r[5] > most) most = (long long)r[4] * r[5];
  }
  SN_REQUIRE(h_pool_off[N] == at && pool_total == at, "sn_vocgt_crop: pool_total = %ld and pool_off[N] = %ld, the bounds give %lld",
             pool_total, (long)h_pool_off[N], at);
  hipLaunchKernelGGL(voc_inst_crop_kernel, dim3((unsigned)sn_blocks((long)most, 64), (unsigned)N), dim3(256), 0, sn_stream(stream), obj_ptrs,
                     hw, rec, pool_off, pool, (long long)pool_total);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
