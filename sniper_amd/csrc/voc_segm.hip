// voc_segm.hip -- PASCAL VOC mask evaluation on the device: voc_eval_sds of lib/dataset/pascal_voc_eval.py:184-272 with mask_overlap
// of lib/mask/mask_transform.py:40-70.  Integer counts and one float64 division per overlap, so the matrix,
// tp / fp and -- through sn_voc_accumulate, unchanged, with an all-zero gt_difficult -- rec, prec and the 11-point AP are the
// reference's bits.  The one thing that is this project's and not the reference's is the resize of the probability map
// (paste_bit.h, shared with sn_rle_paste; the reference calls cv2.resize).
//
// sn_vocsds_mask_iou: ONE launch, one workgroup of 256 threads per detection.  The M x M map is staged in LDS once.  A thread owns box
//   columns (c = tid, tid + 256, ...) and walks the rows: the x coefficient of a column does not depend on the row, so the compiler
//   hoists it out of the row loop once paste_bit is inlined.  First the whole box (dt_area), then per instance of the detection's
//   problem the intersection rectangle only, reading the instance's byte where the resized map is set.  Every thread adds its counts
//   to LDS words with integer atomics (a sum of integers is the same in any order); after one barrier thread g writes entry g.
// sn_vocsds_match_iou: ONE launch, one workgroup per problem: sn_voc_match's kernel with the overlaps read from the matrix and the
//   rules of voc_eval_sds: the candidate is the FIRST instance with ov > cur starting from cur = -1000 (so an instance of overlap 0
//   is a candidate and a problem without instances has none), the match needs cur >= t (NOT strict), there is no difficult flag.
//   The candidate depends on no matching state, so the argument of voc_eval.hip carries over: among the detections of a problem
//   that claim an instance at threshold t, the first in rank is the true positive (an integer min in LDS), the others are false
//   positives.  voc_eval.hip is pinned by its resource test, so its body is restated here and that file is not touched.
// No float atomics, no scratch, no host read-back; every output element is written on every call; the same bits on every run.
#include <limits.h>

#include "common.h"
#include "paste_bit.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDt = SN_VOC_MAX_DT;
constexpr int kMaxGt = SN_VOC_MAX_GT;
constexpr int kMaxT = SN_VOC_MAX_T;
constexpr int kMaxM = SN_VOCSDS_MAX_M;    // the map lives in LDS: kMaxM * kMaxM floats
constexpr int kDtPerThread = kMaxDt / kThreads;
constexpr double kNoOverlap = -1000.0;      // cur_overlap before the first instance (pascal_voc_eval.py:244)

static_assert(kDtPerThread * kThreads == kMaxDt, "a thread owns a whole number of detections");

// the problem of detection n: the p with dt_off[p] <= n < dt_off[p + 1] (problems without detections are skipped)
__device__ __forceinline__ int problem_of(const int32_t *__restrict__ dt_off, int P, int n) {
  int lo = 0, hi = P;                       // the first index in [0, P] whose offset exceeds n, minus one
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (dt_off[mid] > n) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

__global__ __launch_bounds__(kThreads) void voc_mask_iou_kernel(
    const float *__restrict__ masks, const int32_t *__restrict__ dt_box, const int32_t *__restrict__ dt_off,
    const uint8_t *__restrict__ gt_bits, const int64_t *__restrict__ gt_pix_off, const int32_t *__restrict__ gt_bound,
    const int32_t *__restrict__ gt_area, const int32_t *__restrict__ gt_off, const int32_t *__restrict__ iou_off, int P, int M, float thr,
    int32_t *__restrict__ dt_area, double *__restrict__ iou) {
  __shared__ float s_map[kMaxM * kMaxM];
  __shared__ int s_inter[kMaxGt];
  __shared__ int s_area;
  const int n = blockIdx.x, tid = threadIdx.x;
  int p = problem_of(dt_off, P, n);
  p = p < 0 ? 0 : (p > P - 1 ? P - 1 : p);  // (offsets that do not cover n: still a row of the tables)
  const int g0 = gt_off[p];
  int G = gt_off[p + 1] - g0;
  G = G < kMaxGt ? G : kMaxGt;              // the entry point refuses larger problems; never index past the LDS counters
  G = G < 0 ? 0 : G;
  M = M < kMaxM ? M : kMaxM;

  const float *src = masks + (size_t)n * M * M;
  for (int e = tid; e < M * M; e += kThreads) s_map[e] = src[e];
  for (int g = tid; g < G; g += kThreads) s_inter[g] = 0;
  if (tid == 0) s_area = 0;
  __syncthreads();

  PasteBox b;
  const int dx1 = dt_box[4 * (size_t)n], dy1 = dt_box[4 * (size_t)n + 1], dx2 = dt_box[4 * (size_t)n + 2], dy2 = dt_box[4 * (size_t)n + 3];
  b.x1 = dx1;
  b.y1 = dy1;
  b.bw = dx2 - dx1 + 1;
  b.bh = dy2 - dy1 + 1;
  b.h = b.w = 0;
  b.sx = 1. / ((double)b.bw / M);
  b.sy = 1. / ((double)b.bh / M);
  b.area = 2 * b.bw == M && 2 * b.bh == M;

  // the whole box: pixels >= thr of the resized map
  int mine = 0;
  for (int c = tid; c < b.bw; c += kThreads)
    for (int r = 0; r < b.bh; ++r) mine += paste_bit(s_map, M, b, c, r, thr);
  if (mine) atomicAdd(&s_area, mine);

  // per instance: the pixels set in both inside the intersection of the two boxes (mask_transform.py:47-66)
  for (int g = 0; g < G; ++g) {
    const int32_t *gb = gt_bound + 4 * (size_t)(g0 + g);
    const int gx1 = gb[0], gy1 = gb[1], gx2 = gb[2], gy2 = gb[3];
    const int x1 = max(gx1, dx1), y1 = max(gy1, dy1), x2 = min(gx2, dx2), y2 = min(gy2, dy2);
    if (x1 > x2 || y1 > y2) continue;
    const long gw = (long)gx2 - gx1 + 1, gh = (long)gy2 - gy1 + 1;
    const int64_t pix = gt_pix_off[g0 + g];
    if (gw * gh != gt_pix_off[g0 + g + 1] - pix) continue;     // a bitmap that is not its bound's size is never read: overlap 0
    const uint8_t *bits = gt_bits + pix;
    int cnt = 0;
    for (int x = x1 + tid; x <= x2; x += kThreads) {
      const uint8_t *col = bits + (x - gx1);
      for (int y = y1; y <= y2; ++y)
        if (col[(long)(y - gy1) * gw]) cnt += paste_bit(s_map, M, b, x - dx1, y - dy1, thr);
    }
    if (cnt) atomicAdd(&s_inter[g], cnt);
  }
  __syncthreads();

  const int area = s_area;
  if (tid == 0) dt_area[n] = area;
  const size_t base = (size_t)iou_off[p] + (size_t)(n - dt_off[p]) * (size_t)(gt_off[p + 1] - g0);
  for (int g = tid; g < G; g += kThreads) {
    const long inter = s_inter[g];
    const long uni = (long)area + (long)gt_area[g0 + g] - inter;
    iou[base + g] = (inter == 0 || uni < 1) ? 0. : (double)inter / (double)uni;
  }
}

__global__ __launch_bounds__(kThreads) void voc_match_iou_kernel(
    const double *__restrict__ dt_score, const int32_t *__restrict__ dt_off, const int32_t *__restrict__ gt_off,
    const double *__restrict__ iou, const int32_t *__restrict__ iou_off, const double *__restrict__ iou_thrs, int T, long ND, long NG,
    int32_t *__restrict__ dt_best, double *__restrict__ dt_iou, uint8_t *__restrict__ dt_tp, uint8_t *__restrict__ dt_fp,
    int32_t *__restrict__ gt_det) {
  __shared__ double s_score[kMaxDt];
  __shared__ double s_thr[kMaxT];
  __shared__ int s_order[kMaxDt];           // arrival index of the detection of every rank
  __shared__ int s_first[kMaxT * kMaxGt];   // per (threshold, instance): the lowest rank among the detections that claim it
  const int p = blockIdx.x, tid = threadIdx.x;
  const int d0 = dt_off[p], g0 = gt_off[p];
  int D = dt_off[p + 1] - d0, G = gt_off[p + 1] - g0;
  D = D < kMaxDt ? D : kMaxDt;            // the entry point refuses larger problems; never index past the LDS images
  G = G < kMaxGt ? G : kMaxGt;
  const double *ov_p = iou + iou_off[p];

  for (int i = tid; i < D; i += kThreads) {
    s_score[i] = dt_score[d0 + i];
    s_order[i] = 0;                       // (a NaN score ranks nowhere: its slot still names a row of this problem)
  }
  for (int e = tid; e < T * G; e += kThreads) s_first[e] = INT_MAX;
  if (tid < T) s_thr[tid] = iou_thrs[tid];
  __syncthreads();

  double ov[kDtPerThread];
  int jm[kDtPerThread], rk[kDtPerThread];
#pragma unroll
  for (int q = 0; q < kDtPerThread; ++q) {
    const int i = tid + q * kThreads;
    ov[q] = kNoOverlap;
    jm[q] = -1;
    rk[q] = 0;
    if (i < D) {
      const double *row = ov_p + (size_t)i * G;
      double best = kNoOverlap;
      int arg = -1;
      for (int g = 0; g < G; ++g) {       // pascal_voc_eval.py:246-252: ascending g and a strict compare, the FIRST maximum stays
        const double o = row[g];
        if (o > best) {
          best = o;
          arg = g;
        }
      }
      const double si = s_score[i];
      int before = 0;
      for (int j = 0; j < D; ++j) {
        const double sj = s_score[j];
        before += (sj > si) | ((sj == si) & (j < i));
      }
      ov[q] = best;
      jm[q] = arg;
      rk[q] = before;
      s_order[before] = i;
      dt_best[d0 + i] = arg + 1;
      dt_iou[d0 + i] = best;
    }
  }
#pragma unroll
  for (int q = 0; q < kDtPerThread; ++q) {
    if (jm[q] >= 0)
      for (int t = 0; t < T; ++t)
        if (ov[q] >= s_thr[t]) atomicMin(&s_first[t * G + jm[q]], rk[q]);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kDtPerThread; ++q) {
    const int i = tid + q * kThreads;
    if (i < D) {
      for (int t = 0; t < T; ++t) {
        int tp = 0;                       // cur < t (or no instance at all: cur = -1000): a false positive
        if (jm[q] >= 0 && ov[q] >= s_thr[t]) tp = s_first[t * G + jm[q]] == rk[q];      // already_detect: a false positive
        dt_tp[(size_t)t * ND + d0 + i] = (uint8_t)tp;
        dt_fp[(size_t)t * ND + d0 + i] = (uint8_t)!tp;
      }
    }
  }
  for (int e = tid; e < T * G; e += kThreads) {
    const int t = e / G, g = e - t * G;
    const int f = s_first[e];
    gt_det[(size_t)t * NG + g0 + g] = f != INT_MAX ? s_order[f < D ? f : 0] + 1 : 0;
  }
}

}  // namespace

SN_EXPORT int sn_vocsds_limits(int32_t *h_out6) {
  SN_REQUIRE(h_out6, "sn_vocsds_limits: null pointer");
  const int v[6] = {kMaxDt, kMaxGt, kMaxT, kMaxM, kThreads, INT_MAX};
  for (int i = 0; i < 6; ++i) h_out6[i] = v[i];
  return SN_OK;
}

SN_EXPORT int sn_vocsds_mask_iou(const float *masks, const int32_t *dt_box, const int32_t *dt_off, const uint8_t *gt_bits,
                              const int64_t *gt_pix_off, const int32_t *gt_bound, const int32_t *gt_area, const int32_t *gt_off,
                              const int32_t *iou_off, int P, int M, float binary_thresh, int max_gt_per_problem, long ND, long NG,
                              long n_pairs, long max_box_pixels, int32_t *dt_area, double *iou, sn_stream_t stream) {
  SN_REQUIRE(masks && dt_box && dt_off && gt_bits && gt_pix_off && gt_bound && gt_area && gt_off && iou_off && dt_area && iou,
             "sn_vocsds_mask_iou: null pointer");
  SN_REQUIRE(P >= 1, "sn_vocsds_mask_iou: P >= 1 required (P = %d)", P);
  SN_REQUIRE(ND >= 1 && ND < 2147483648L, "sn_vocsds_mask_iou: 1 <= ND < 2^31 required (ND = %ld)", ND);
  SN_REQUIRE(M >= 1 && M <= kMaxM, "sn_vocsds_mask_iou: 1 <= M <= %d required, the map is staged in LDS (M = %d)", kMaxM, M);
  SN_REQUIRE(NG >= 0 && NG < 2147483648L, "sn_vocsds_mask_iou: 0 <= NG < 2^31 required (NG = %ld)", NG);
  SN_REQUIRE(max_gt_per_problem >= 0 && max_gt_per_problem <= kMaxGt,
             "sn_vocsds_mask_iou: a problem has %d instances, one workgroup counts at most %d", max_gt_per_problem, kMaxGt);
  SN_REQUIRE(n_pairs >= 0 && n_pairs < 2147483648L, "sn_vocsds_mask_iou: the pairs of a call must fit 32-bit indexing (n_pairs = %ld)", n_pairs);
  SN_REQUIRE(max_box_pixels >= 1 && max_box_pixels < 2147483648L,
             "sn_vocsds_mask_iou: 1 <= bw * bh < 2^31 required for every detection (max_box_pixels = %ld)", max_box_pixels);
  hipLaunchKernelGGL(voc_mask_iou_kernel, dim3((unsigned)ND), dim3(kThreads), 0, sn_stream(stream), masks, dt_box, dt_off, gt_bits, gt_pix_off,
                     gt_bound, gt_area, gt_off, iou_off, P, M, binary_thresh, dt_area, iou);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_vocsds_match_iou(const double *dt_score, const int32_t *dt_off, const int32_t *gt_off, const double *iou,
                               const int32_t *iou_off, const double *iou_thrs, int P, int T, int max_dt_per_problem,
                               int max_gt_per_problem, long ND, long NG, int32_t *dt_best, double *dt_iou, uint8_t *dt_tp,
                               uint8_t *dt_fp, int32_t *gt_det, sn_stream_t stream) {
  SN_REQUIRE(dt_score && dt_off && gt_off && iou && iou_off && iou_thrs && dt_best && dt_iou && dt_tp && dt_fp && gt_det,
             "sn_vocsds_match_iou: null pointer");
  SN_REQUIRE(P >= 1, "sn_vocsds_match_iou: P >= 1 required (P = %d)", P);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_vocsds_match_iou: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(max_dt_per_problem >= 0 && max_dt_per_problem <= kMaxDt,
             "sn_vocsds_match_iou: a problem has %d detections, one workgroup ranks at most %d", max_dt_per_problem, kMaxDt);
  SN_REQUIRE(max_gt_per_problem >= 0 && max_gt_per_problem <= kMaxGt,
             "sn_vocsds_match_iou: a problem has %d instances, one workgroup holds at most %d", max_gt_per_problem, kMaxGt);
  SN_REQUIRE(ND >= 0 && NG >= 0, "sn_vocsds_match_iou: ND >= 0 and NG >= 0 required (ND = %ld, NG = %ld)", ND, NG);
  SN_REQUIRE((double)ND * T < 2147483648. && (double)NG * T < 2147483648.,
             "sn_vocsds_match_iou: too many rows, T * ND and T * NG must fit 32-bit (ND = %ld, NG = %ld)", ND, NG);
  hipLaunchKernelGGL(voc_match_iou_kernel, dim3(P), dim3(kThreads), 0, sn_stream(stream), dt_score, dt_off, gt_off, iou, iou_off, iou_thrs, T,
                     ND, NG, dt_best, dt_iou, dt_tp, dt_fp, gt_det);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
