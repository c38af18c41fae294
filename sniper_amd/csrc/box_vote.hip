// box_vote.hip -- box voting after the test-time NMS (TEST.BBOX_VOTE).  Ours, modelled on Detectron's
// box_utils.box_voting: every box the NMS kept is replaced by the score-weighted mean of ALL pre-NMS boxes of its (image, class)
// problem that overlap it by at least `thresh`.
//
//   for a kept row t and the pre-NMS rows a = 0 .. n_a-1, ascending:
//     iou  = overlap_f64(t, a, mode 0)            the float64 overlap of lib/bbox/bbox.pyx (+1 pixel), from the float32 coordinates
//     vote = iou >= thresh
//     den += (double)s_a;   num_c += (double)s_a * (double)c_a      (c = x1, y1, x2, y2; the product of two float32 is exact)
//   no voter, or den not > 0: the row stays as it is;   else c_t = (float)(num_c / den) and the score by `method`:
//     0 'ID' unchanged;   1 'AVG' (float)(den / |V|);   2 'IOU_AVG' (float)(sum iou * s / sum iou)
//
// ONE launch for all P ragged problems of a pass, no host read of the post-NMS counts.  A workgroup is ONE wave: it takes one
// entry {problem, first top row} of the tile table the host built from the PRE-NMS sizes (an upper bound of the kept rows; a
// tile at or beyond d_top_count[q] returns) and holds one kept row per lane.  The pre-NMS rows stream through LDS in chunks of
// kChunk rows, widened to float64 once per chunk; every lane walks the chunk in index order, so all lanes read the same LDS
// address (a broadcast, no bank conflict) and each lane's sums are added in ascending row order by construction.  No cross-lane
// reduction, no atomics, no workspace: the same bits every run, the bits of the sequential float64 loop.  The overlap rejects
// on iw <= 0 / ih <= 0 before its divide.  The kept rows are written in place; the pre-NMS rows are a separate, read-only copy.
// Most problems of a pass hold a few dozen rows (2000 rows over 80 classes), hence the one-wave workgroup: a wider one would
// idle on them, and the waves of other problems on the same SIMD cover the LDS and divide latency (<= 64 VGPRs: 8 per SIMD).
#include "box_overlap.h"

namespace {

constexpr int kTile = kWave;        // kept rows per workgroup: one per lane
constexpr int kChunk = 128;         // pre-NMS rows per LDS chunk: 5 doubles each, 5 KB -- 32 one-wave workgroups in a CU's 160 KB

template <int METHOD>
__global__ __launch_bounds__(kTile) void box_vote_kernel(float *__restrict__ top, const float *__restrict__ all,
                                                         const int32_t *__restrict__ off, const int32_t *__restrict__ top_count,
                                                         const int32_t *__restrict__ tiles, int P, double thresh) {
  __shared__ __attribute__((aligned(16))) double s_a[kChunk * 5];
  const int q = tiles[2 * blockIdx.x], first = tiles[2 * blockIdx.x + 1];
  if (q < 0 || q >= P || first < 0) return;
  const long base = off[q];
  const int n_a = off[q + 1] - off[q];
  int n_t = top_count[q];
  n_t = n_t < n_a ? n_t : n_a;                    // the kept rows are a prefix of the problem's own rows, never beyond them
  if (first >= n_t) return;                       // (uniform over the wave: the barriers below see every lane or none)
  const int lane = threadIdx.x, r = first + lane;
  const bool live = r < n_t;
  float *trow = top + (base + (live ? r : first)) * 5;
  const double t0 = trow[0], t1 = trow[1], t2 = trow[2], t3 = trow[3];
  double den = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0, wsum = 0.0, wden = 0.0;
  int voters = 0;
  for (int c0 = 0; c0 < n_a; c0 += kChunk) {
    const int m = n_a - c0 < kChunk ? n_a - c0 : kChunk;
    __syncthreads();
    const float *src = all + (base + c0) * 5;
    for (int e = lane; e < m * 5; e += kTile) s_a[e] = (double)src[e];
    __syncthreads();
    if (live) {
      for (int j = 0; j < m; ++j) {
        const double *a = s_a + j * 5;
        const double iou = overlap_f64(t0, t1, t2, t3, a[0], a[1], a[2], a[3], 0);
        if (iou >= thresh) {
          const double s = a[4];
          ++voters;
          den += s;
          n0 += s * a[0];
          n1 += s * a[1];
          n2 += s * a[2];
          n3 += s * a[3];
          if (METHOD == 2) {
            wsum += iou * s;
            wden += iou;
          }
        }
      }
    }
  }
  if (live && voters > 0 && den > 0.0) {
    trow[0] = (float)(n0 / den);
    trow[1] = (float)(n1 / den);
    trow[2] = (float)(n2 / den);
    trow[3] = (float)(n3 / den);
    if (METHOD == 1) trow[4] = (float)(den / (double)voters);
    if (METHOD == 2) trow[4] = (float)(wsum / wden);
  }
}

}  // namespace

SN_EXPORT int sn_box_vote_limits(int32_t *h_out2) {
  SN_REQUIRE(h_out2, "sn_box_vote_limits: null pointer");
  h_out2[0] = kTile;
  h_out2[1] = kChunk;
  return SN_OK;
}

SN_EXPORT int sn_box_vote(float *d_top_rows, const float *d_all_rows, const int32_t *d_off, const int32_t *d_top_count,
                          const int32_t *d_tiles, int n_tiles, int P, double thresh, int method, sn_stream_t stream) {
  SN_REQUIRE(d_top_rows && d_all_rows && d_off && d_top_count && d_tiles, "sn_box_vote: null pointer");
  SN_REQUIRE(P >= 0, "sn_box_vote: P >= 0 required (P = %d)", P);
  SN_REQUIRE(n_tiles >= 0, "sn_box_vote: n_tiles >= 0 required (n_tiles = %d)", n_tiles);
  SN_REQUIRE(thresh > 0.0 && thresh <= 1.0, "sn_box_vote: thresh in (0, 1] required (thresh = %g)", thresh);      // NaN fails both
  SN_REQUIRE(method >= 0 && method <= 2, "sn_box_vote: unknown method %d (0 ID, 1 AVG, 2 IOU_AVG)", method);
  SN_REQUIRE(((uintptr_t)d_top_rows | (uintptr_t)d_all_rows | (uintptr_t)d_off | (uintptr_t)d_top_count | (uintptr_t)d_tiles) % 4 == 0,
             "sn_box_vote: misaligned array (4-byte alignment required)");
  SN_REQUIRE(d_top_rows != d_all_rows, "sn_box_vote: d_top_rows aliases d_all_rows (the pre-NMS rows are a separate copy)");
  if (P == 0 || n_tiles == 0) return SN_OK;
  const dim3 grid(n_tiles), block(kTile);
  hipStream_t s = sn_stream(stream);
  if (method == 0)
    hipLaunchKernelGGL(box_vote_kernel<0>, grid, block, 0, s, d_top_rows, d_all_rows, d_off, d_top_count, d_tiles, P, thresh);
  else if (method == 1)
    hipLaunchKernelGGL(box_vote_kernel<1>, grid, block, 0, s, d_top_rows, d_all_rows, d_off, d_top_count, d_tiles, P, thresh);
  else
    hipLaunchKernelGGL(box_vote_kernel<2>, grid, block, 0, s, d_top_rows, d_all_rows, d_off, d_top_count, d_tiles, P, thresh);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
