// voc_eval.hip -- PASCAL VOC box evaluation on the device: voc_eval and voc_ap of lib/dataset/pascal_voc_eval.py:39-70, 116-181,
// float64 and integer counts throughout, so that `rec`, `prec` and the 11-point AP come out on the reference's bits and the area
// AP within the rounding of its sum.
//
// What makes the matching parallel: a detection's candidate box jmax (the FIRST box of maximal IoU, np.argmax) and its ovmax depend
// on no matching state.  Only the det[jmax] flag is stateful, and it says: among the detections of one image whose jmax is this box
// and whose ovmax > t, the one earliest in the class's score order is the true positive, the others are false positives.  Within
// one image the class's order is the problem's own rank (descending score, equal scores by arrival order), so a problem is decided
// by itself and no walk over a class's detections is needed.
//
// sn_voc_match: ONE launch, one workgroup of 256 threads per problem = (class, image) pair with a detection or a box.  The boxes,
//   their areas and difficult flags and the scores sit in LDS.  Thread i owns detections i, i + 256, ... (four at most): it walks the
//   boxes (every lane reads the same box: broadcasts), keeps (ovmax, jmax) in registers, then counts the detections that precede
//   its own (the rank).  Per threshold every detection with ovmax > t offers its rank to its box by an integer min in LDS (a min
//   gives the same value whatever the order of arrival); the detection whose rank the box holds is the true positive.
// sn_voc_accumulate: two launches.
//   1. order: per class, the ordering of eval_order.h (shared with coco_eval.hip) straight on the score column.
//   2. curves: one workgroup per (threshold, class), chunks of kScanChunk detections: inclusive integer scans of tp / fp with a
//      carry, rec and prec, a reverse running max of prec into the workspace, the eleven searches of the VOC07 metric and the sum of
//      the area metric, reduced in a fixed order.
// No float atomics, no scratch, no host read-back; every output element is written on every call and the bits are the same on
// every run.  The file is compiled with -ffp-contract=off (sniper_amd/build.py) and says so itself below: numpy rounds the two
// products of `uni` and their sum separately.
#include <limits.h>

#include "common.h"
#include "eval_order.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxDt = SN_VOC_MAX_DT;      // detections of one problem: their scores are ranked in LDS
constexpr int kMaxGt = SN_VOC_MAX_GT;      // boxes of one problem: in LDS
constexpr int kMaxT = SN_VOC_MAX_T;
constexpr int kDtPerThread = kMaxDt / kThreads;
constexpr int kSortTile = kEvalSortTile, kScanChunk = kEvalScanChunk;
constexpr int kAp07 = 11;
constexpr double kEps = 2.220446049250313e-16;   // np.finfo(np.float64).eps

static_assert(kDtPerThread * kThreads == kMaxDt, "a thread owns a whole number of detections");
static_assert(kScanChunk == kThreads, "the curve kernel's reductions are written for four waves");

__global__ __launch_bounds__(kThreads) void voc_match_kernel(
    const double *__restrict__ dt_box, const double *__restrict__ dt_score, const int32_t *__restrict__ dt_off,
    const double *__restrict__ gt_box, const uint8_t *__restrict__ gt_difficult, const int32_t *__restrict__ gt_off,
    const double *__restrict__ iou_thrs, int T, long ND, long NG, int32_t *__restrict__ dt_best, double *__restrict__ dt_iou,
    uint8_t *__restrict__ dt_tp, uint8_t *__restrict__ dt_fp, int32_t *__restrict__ gt_det) {
  __shared__ double s_score[kMaxDt];
  __shared__ double s_gt[kMaxGt * 4];
  __shared__ double s_garea[kMaxGt];
  __shared__ double s_thr[kMaxT];
  __shared__ int s_order[kMaxDt];           // arrival index of the detection of every rank
  __shared__ int s_first[kMaxT * kMaxGt];   // per (threshold, box): the lowest rank among the detections that claim the box
  __shared__ int s_diff[kMaxGt];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int d0 = dt_off[p], g0 = gt_off[p];
  int D = dt_off[p + 1] - d0, G = gt_off[p + 1] - g0;
  D = D < kMaxDt ? D : kMaxDt;            // the entry point refuses larger problems; never index past the LDS images
  G = G < kMaxGt ? G : kMaxGt;

  for (int i = tid; i < D; i += kThreads) {
    s_score[i] = dt_score[d0 + i];
    s_order[i] = 0;                       // (a NaN score ranks nowhere: its slot still names a row of this problem)
  }
  for (int g = tid; g < G; g += kThreads) {
    const double *b = gt_box + (size_t)(g0 + g) * 4;
    const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    s_gt[g * 4 + 0] = x1;
    s_gt[g * 4 + 1] = y1;
    s_gt[g * 4 + 2] = x2;
    s_gt[g * 4 + 3] = y2;
    s_garea[g] = (x2 - x1 + 1.) * (y2 - y1 + 1.);
    s_diff[g] = gt_difficult[g0 + g] != 0;
  }
  for (int e = tid; e < T * G; e += kThreads) s_first[e] = INT_MAX;
  if (tid < T) s_thr[tid] = iou_thrs[tid];
  __syncthreads();

  double ov[kDtPerThread];
  int jm[kDtPerThread], rk[kDtPerThread];
#pragma unroll
  for (int q = 0; q < kDtPerThread; ++q) {
    const int i = tid + q * kThreads;
    ov[q] = -INFINITY;
    jm[q] = -1;
    rk[q] = 0;
    if (i < D) {
      const double *b = dt_box + (size_t)(d0 + i) * 4;
      const double bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
      const double darea = (bx2 - bx1 + 1.) * (by2 - by1 + 1.);
      double best = -INFINITY;
      int arg = -1;
      for (int g = 0; g < G; ++g) {       // pascal_voc_eval.py:146-160, operation for operation
        const double ixmin = fmax(s_gt[g * 4 + 0], bx1), iymin = fmax(s_gt[g * 4 + 1], by1);
        const double ixmax = fmin(s_gt[g * 4 + 2], bx2), iymax = fmin(s_gt[g * 4 + 3], by2);
        const double iw = fmax(ixmax - ixmin + 1., 0.), ih = fmax(iymax - iymin + 1., 0.);
        const double inters = iw * ih;
        const double uni = (darea + s_garea[g]) - inters;
        const double o = inters / uni;
        if (o > best) {                   // ascending g and a strict compare: the EARLIER box of equal IoU stays (np.argmax)
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
        if (ov[q] > s_thr[t]) atomicMin(&s_first[t * G + jm[q]], rk[q]);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kDtPerThread; ++q) {
    const int i = tid + q * kThreads;
    if (i < D) {
      for (int t = 0; t < T; ++t) {
        int tp = 0, fp = 1;               // ovmax <= t (or no box at all: ovmax = -inf): a false positive
        if (jm[q] >= 0 && ov[q] > s_thr[t]) {
          const bool diff = s_diff[jm[q]] != 0;
          tp = !diff && s_first[t * G + jm[q]] == rk[q];
          fp = !diff && !tp;              // a difficult box: neither
        }
        dt_tp[(size_t)t * ND + d0 + i] = (uint8_t)tp;
        dt_fp[(size_t)t * ND + d0 + i] = (uint8_t)fp;
      }
    }
  }
  for (int e = tid; e < T * G; e += kThreads) {
    const int t = e / G, g = e - t * G;
    const int f = s_first[e];
    gt_det[(size_t)t * NG + g0 + g] = (f != INT_MAX && !s_diff[g]) ? s_order[f < D ? f : 0] + 1 : 0;
  }
}

// grid (tiles, K): the order of class k's detections by (descending score, position), as positions in the whole detection list
__global__ __launch_bounds__(kSortTile) void voc_order_kernel(const int32_t *__restrict__ cat_off, const int32_t *__restrict__ dt_off,
                                                              const double *__restrict__ dt_score, int32_t *__restrict__ order) {
  __shared__ double s_tile[kSortTile];
  const int k = blockIdx.y;
  const int c0 = dt_off[cat_off[k]], N = dt_off[cat_off[k + 1]] - c0;
  sn_eval_order_tile(c0, N, dt_score, order, c0, s_tile);
}

struct Ap07Thrs {
  double v[kAp07];
};

// grid (T, K): rec[t], prec[t] of class k in sorted order, npos[k], ap07[t, k], ap_area[t, k]
__global__ __launch_bounds__(kScanChunk) void voc_curves_kernel(
    const int32_t *__restrict__ cat_off, const int32_t *__restrict__ dt_off, const int32_t *__restrict__ gt_off,
    const uint8_t *__restrict__ gt_difficult, const uint8_t *__restrict__ dt_tp, const uint8_t *__restrict__ dt_fp,
    const int32_t *__restrict__ order, Ap07Thrs thr07, int K, long ND, double *ws_mx, double *rec, double *prec,
    int32_t *__restrict__ npos_out, double *__restrict__ ap07, double *__restrict__ ap_area) {
  __shared__ int s_tp[kWaves], s_fp[kWaves], s_red[kWaves];
  __shared__ double s_mx[kWaves], s_sum[kWaves], s_p[kAp07];
  const int t = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int p0 = cat_off[k], p1 = cat_off[k + 1];
  const int c0 = dt_off[p0], N = dt_off[p1] - c0;
  const int g0 = gt_off[p0], g1 = gt_off[p1];

  // npos: the class's boxes that are not difficult
  int cnt = 0;
  for (int g = g0 + tid; g < g1; g += kScanChunk) cnt += gt_difficult[g] == 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) s_red[wave] = cnt;
  __syncthreads();
  int npos = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) npos += s_red[w];
  if (t == 0 && tid == 0) npos_out[k] = npos;
  const double dn = (double)npos;          // npos = 0 with detections: rec = 0 / 0 = nan, as the reference's
  const size_t slab = (size_t)t * ND + c0;
  double *rec_s = rec + slab, *prec_s = prec + slab, *mx_s = ws_mx + slab;

  // inclusive scans of tp and fp over the ordered detections, chunk by chunk with a carry
  int ctp = 0, cfp = 0;
  for (int base = 0; base < N; base += kScanChunk) {
    const int i = base + tid;
    int vt = 0, vf = 0;
    if (i < N) {
      const unsigned rel = (unsigned)(order[c0 + i] - c0);    // a permutation of the class; held in range if max_dt_per_class was understated
      const size_t j = (size_t)t * ND + c0 + (rel < (unsigned)N ? rel : 0u);
      vt = dt_tp[j] != 0;
      vf = dt_fp[j] != 0;
    }
    vt = wave_scan_add(vt, lane);
    vf = wave_scan_add(vf, lane);
    __syncthreads();                       // (the previous chunk's totals have been read)
    if (lane == kWave - 1) {
      s_tp[wave] = vt;
      s_fp[wave] = vf;
    }
    __syncthreads();
    int tot_t = 0, tot_f = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) {
        vt += s_tp[w];
        vf += s_fp[w];
      }
      tot_t += s_tp[w];
      tot_f += s_fp[w];
    }
    vt += ctp;
    vf += cfp;
    if (i < N) {
      rec_s[i] = (double)vt / dn;
      prec_s[i] = (double)vt / fmax((double)(vt + vf), kEps);
    }
    ctp += tot_t;
    cfp += tot_f;
  }
  __threadfence_block();
  __syncthreads();
  // mpre: prec non-increasing from the right (the trailing sentinel 0 changes nothing: prec >= 0), chunk by chunk from the end
  double cmx = -1.;
  const int nchunk = (N + kScanChunk - 1) / kScanChunk;
  for (int c = nchunk - 1; c >= 0; --c) {
    const int i = c * kScanChunk + tid;
    double v = i < N ? prec_s[i] : -1.;
    v = wave_scan_max_rev(v, lane);
    __syncthreads();
    if (lane == 0) s_mx[wave] = v;
    __syncthreads();
    double tot = cmx;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w > wave) v = fmax(v, s_mx[w]);
      tot = fmax(tot, s_mx[w]);
    }
    v = fmax(v, cmx);
    if (i < N) mx_s[i] = v;
    cmx = tot;
  }
  __threadfence_block();
  __syncthreads();

  // VOC07: per threshold the max of prec where rec >= thr = mpre at the first such index (rec is non-decreasing, or all nan), else 0
  if (tid < kAp07) {
    const double thr = thr07.v[tid];
    int lo = 0, hi = N;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rec_s[mid] >= thr) hi = mid; else lo = mid + 1;
    }
    s_p[tid] = lo < N ? mx_s[lo] : 0.;
  }
  // area: the sum of (mrec[i + 1] - mrec[i]) * mpre[i + 1] over the recall changes; a thread adds its own terms in ascending order,
  // the partial sums are added lane by lane, then wave by wave
  double part = 0.;
  for (int i = tid; i < N; i += kScanChunk) {
    const double r = rec_s[i], prev = i ? rec_s[i - 1] : 0.;
    if (r != prev) part += (r - prev) * mx_s[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if (lane == 0) s_sum[wave] = part;
  __syncthreads();
  if (tid == 0) {
    double a7 = 0.;
    for (int j = 0; j < kAp07; ++j) a7 += s_p[j] / 11.;
    ap07[(size_t)t * K + k] = a7;
    double area = 0.;
    for (int w = 0; w < kWaves; ++w) area += s_sum[w];
    const double last = N ? rec_s[N - 1] : 0.;
    if (1. != last) area += (1. - last) * 0.;     // the closing sentinels: 0, or nan where rec is
    ap_area[(size_t)t * K + k] = area;
  }
}

size_t ws_total(long ND, int T) { return sn_align((size_t)T * (size_t)(ND > 0 ? ND : 1) * sizeof(double)); }

}  // namespace

SN_EXPORT int sn_voc_limits(int32_t *h_out5) {
  SN_REQUIRE(h_out5, "sn_voc_limits: null pointer");
  const int v[5] = {kMaxDt, kMaxGt, kMaxT, kSortTile, kScanChunk};
  for (int i = 0; i < 5; ++i) h_out5[i] = v[i];
  return SN_OK;
}

SN_EXPORT int sn_voc_match(const double *dt_box, const double *dt_score, const int32_t *dt_off, const double *gt_box,
                           const uint8_t *gt_difficult, const int32_t *gt_off, const double *iou_thrs, int P, int T,
                           int max_dt_per_problem, int max_gt_per_problem, long ND, long NG, int32_t *dt_best, double *dt_iou,
                           uint8_t *dt_tp, uint8_t *dt_fp, int32_t *gt_det, sn_stream_t stream) {
  SN_REQUIRE(dt_box && dt_score && dt_off && gt_box && gt_difficult && gt_off && iou_thrs && dt_best && dt_iou && dt_tp && dt_fp && gt_det,
             "sn_voc_match: null pointer");
  SN_REQUIRE(P >= 1, "sn_voc_match: P >= 1 required (P = %d)", P);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_voc_match: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(max_dt_per_problem >= 0 && max_dt_per_problem <= kMaxDt,
             "sn_voc_match: a problem has %d detections, one workgroup ranks at most %d", max_dt_per_problem, kMaxDt);
  SN_REQUIRE(max_gt_per_problem >= 0 && max_gt_per_problem <= kMaxGt,
             "sn_voc_match: a problem has %d boxes, one workgroup holds at most %d", max_gt_per_problem, kMaxGt);
  SN_REQUIRE(ND >= 0 && NG >= 0, "sn_voc_match: ND >= 0 and NG >= 0 required (ND = %ld, NG = %ld)", ND, NG);
  SN_REQUIRE((double)ND * T < 2147483648. && (double)NG * T < 2147483648.,
             "sn_voc_match: too many rows, T * ND and T * NG must fit 32-bit (ND = %ld, NG = %ld)", ND, NG);
  hipLaunchKernelGGL(voc_match_kernel, dim3(P), dim3(kThreads), 0, sn_stream(stream), dt_box, dt_score, dt_off, gt_box, gt_difficult,
                     gt_off, iou_thrs, T, ND, NG, dt_best, dt_iou, dt_tp, dt_fp, gt_det);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT size_t sn_voc_accumulate_workspace_bytes(long ND, int T) {
  if (ND < 0 || T < 1 || T > kMaxT) return 0;
  return ws_total(ND, T);
}

SN_EXPORT int sn_voc_accumulate(const double *dt_score, const int32_t *dt_off, const int32_t *gt_off, const int32_t *cat_off,
                                const uint8_t *gt_difficult, const uint8_t *dt_tp, const uint8_t *dt_fp, const double *h_ap07_thrs,
                                int P, int K, int T, int max_dt_per_class, long ND, long NG, void *ws, size_t ws_bytes,
                                int32_t *order, double *rec, double *prec, int32_t *npos, double *ap07, double *ap_area,
                                sn_stream_t stream) {
  SN_REQUIRE(dt_score && dt_off && gt_off && cat_off && gt_difficult && dt_tp && dt_fp && h_ap07_thrs && order && rec && prec && npos &&
                 ap07 && ap_area,
             "sn_voc_accumulate: null pointer");
  SN_REQUIRE(P >= 1, "sn_voc_accumulate: P >= 1 required (P = %d)", P);
  SN_REQUIRE(K >= 1 && K <= 65535, "sn_voc_accumulate: 1 <= K <= 65535 required (K = %d)", K);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_voc_accumulate: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(ND >= 0 && NG >= 0, "sn_voc_accumulate: ND >= 0 and NG >= 0 required (ND = %ld, NG = %ld)", ND, NG);
  SN_REQUIRE(max_dt_per_class >= 0 && max_dt_per_class <= ND, "sn_voc_accumulate: 0 <= max_dt_per_class <= ND required (%d, ND = %ld)",
             max_dt_per_class, ND);
  SN_REQUIRE((double)ND * T < 2147483648. && (double)NG * T < 2147483648.,
             "sn_voc_accumulate: too many rows, T * ND and T * NG must fit 32-bit (ND = %ld, NG = %ld)", ND, NG);
  const size_t need = ws_total(ND, T);
  SN_REQUIRE(ws && ws_bytes >= need, "sn_voc_accumulate: short workspace (%zu bytes, sn_voc_accumulate_workspace_bytes = %zu)",
             ws ? ws_bytes : (size_t)0, need);
  Ap07Thrs thr07;
  for (int j = 0; j < kAp07; ++j) thr07.v[j] = h_ap07_thrs[j];
  hipStream_t s = sn_stream(stream);
  if (max_dt_per_class > 0) {
    hipLaunchKernelGGL(voc_order_kernel, dim3(sn_div_up(max_dt_per_class, kSortTile), K), dim3(kSortTile), 0, s, cat_off, dt_off, dt_score,
                       order);
    SN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(voc_curves_kernel, dim3(T, K), dim3(kScanChunk), 0, s, cat_off, dt_off, gt_off, gt_difficult, dt_tp, dt_fp, order, thr07,
                     K, ND, (double *)ws, rec, prec, npos, ap07, ap_area);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
