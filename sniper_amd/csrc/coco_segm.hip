// coco_segm.hip -- COCO mask evaluation on the device: the run-length arithmetic of lib/dataset/pycocotools/maskApi.c (rleArea :72-75,
// rleToBbox :111-124, rleIou :77-96 with the bbIou gate of :98-109) and the per-image matching of cocoeval.py:163-272 with the IoU read
// from a matrix.  Integer counts and one float64 division per IoU: the matrices are the reference's bits.
//
// A mask is a run of uint32 counts in column-major order, zeros first (the first count may be 0); the masks of a call lie in one pool
// behind (N+1) int32 prefix offsets.
// sn_rle_stats: ONE launch, a wave per mask.  The lanes take 64 runs at a time; an inclusive wave scan with a carry gives every run
//   its end position and the number of 1-pixels up to it, which are kept as (end, ones) pairs for sn_rle_iou; the minima and maxima of
//   rleToBbox and the area are reduced over the wave.
// sn_rle_iou: ONE launch, a wave per (detection, ground truth) pair of a problem.  The pair passes the reference's bounding-box gate or
//   scores 0.  The intersection is the sum over the detection's 1-runs [s, e) of F(e) - F(s), F(x) = the ground truth's 1-pixels below
//   x = a binary search in its (end, ones) pairs: exact, and no chain of dependent steps as in the reference's two-pointer walk.
// sn_coco_match_iou: coco_match_kernel of coco_eval.hip with the IoU of (detection, box) read from that matrix instead of computed
//   from boxes; ranking, tie rules, outputs and limits are the same (the box kernel is pinned by its resource test, so the body is
//   restated here and coco_eval.hip is untouched).
// No atomics, no scratch, no host read-back; every output element is written exactly once per call.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;       // masks (sn_rle_stats) and pairs (sn_rle_iou) per workgroup
constexpr int kMaxDt = SN_COCO_MAX_DT;
constexpr int kMaxGt = SN_COCO_MAX_GT;
constexpr int kGtPerLane = kMaxGt / kWave;
constexpr int kMaxT = SN_COCO_MAX_T, kMaxA = SN_COCO_MAX_A;
constexpr int kMaxGrid = 1 << 20;

static_assert(kGtPerLane * kWave == kMaxGt, "a lane holds a whole number of boxes");

__device__ __forceinline__ unsigned wave_scan_add_u(unsigned v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// rows6 (N,6) = x, y, w, h of rleToBbox, score (0 without scores), rleArea;  cum2 (total,2) = end position and 1-pixels up to it
__global__ __launch_bounds__(kThreads) void rle_stats_kernel(const uint32_t *__restrict__ cnts, const int32_t *__restrict__ rle_off,
                                                             const int32_t *__restrict__ hw, const double *__restrict__ score, long N,
                                                             double *__restrict__ rows6, uint2 *__restrict__ cum2) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (long n = (long)blockIdx.x * kWaves + wave; n < N; n += (long)gridDim.x * kWaves) {
    const int o0 = rle_off[n];
    int m = rle_off[n + 1] - o0;
    m = m < 0 ? 0 : m;
    const unsigned h = (unsigned)hw[2 * n], w = (unsigned)hw[2 * n + 1];
    const int me = m & ~1;                 // rleToBbox drops an odd last count
    unsigned cc = 0, ones = 0;             // carries: the same in every lane
    unsigned xs = w, ys = h, xe = 0, ye = 0;
    for (int base = 0; base < m; base += kWave) {
      const int j = base + lane;
      const unsigned c = j < m ? cnts[(size_t)o0 + j] : 0u;
      const unsigned sc = wave_scan_add_u(c, lane), so = wave_scan_add_u((j & 1) ? c : 0u, lane);
      const unsigned pos = cc + sc, on = ones + so;
      if (j < m) cum2[(size_t)o0 + j] = make_uint2(pos, on);
      if (j < me) {                        // run end points only: t = cc - j % 2 in unsigned arithmetic, like the reference
        const unsigned t = pos - (unsigned)(j & 1);
        const unsigned y = t % h, x = (t - y) / h;
        xs = x < xs ? x : xs;
        xe = x > xe ? x : xe;
        ys = y < ys ? y : ys;
        ye = y > ye ? y : ye;
      }
      cc += __shfl(sc, kWave - 1, 64);
      ones += __shfl(so, kWave - 1, 64);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned a = __shfl_xor(xs, off, 64), b = __shfl_xor(xe, off, 64), c = __shfl_xor(ys, off, 64), d = __shfl_xor(ye, off, 64);
      xs = a < xs ? a : xs;
      xe = b > xe ? b : xe;
      ys = c < ys ? c : ys;
      ye = d > ye ? d : ye;
    }
    if (lane == 0) {
      double *o = rows6 + (size_t)n * 6;
      const bool none = me == 0;           // an empty mask ([h * w], or no counts): four zeros
      o[0] = none ? 0. : (double)xs;
      o[1] = none ? 0. : (double)ys;
      o[2] = none ? 0. : (double)(xe - xs + 1u);
      o[3] = none ? 0. : (double)(ye - ys + 1u);
      o[4] = score ? score[n] : 0.;
      o[5] = (double)ones;
    }
  }
}

// the 1-pixels of a mask below position x, from its (end, ones) pairs
__device__ __forceinline__ unsigned ones_below(const uint2 *__restrict__ c, int m, unsigned x) {
  int lo = 0, hi = m;                      // k = the number of runs that end at or before x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid].x <= x) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0u;
  const uint2 prev = c[lo - 1];
  return prev.y + (((lo & 1) && lo < m) ? x - prev.x : 0u);
}

__global__ __launch_bounds__(kThreads) void rle_iou_kernel(
    const uint2 *__restrict__ dt_cum2, const int32_t *__restrict__ dt_rle_off, const double *__restrict__ dt_rows6,
    const uint2 *__restrict__ gt_cum2, const int32_t *__restrict__ gt_rle_off, const double *__restrict__ gt_rows6,
    const uint8_t *__restrict__ gt_flags, const int32_t *__restrict__ dt_off, const int32_t *__restrict__ gt_off,
    const int32_t *__restrict__ iou_off, int P, long n_pairs, double *__restrict__ iou) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int d_first = dt_off[0], g_first = gt_off[0];
  for (long e = (long)blockIdx.x * kWaves + wave; e < n_pairs; e += (long)gridDim.x * kWaves) {
    int lo = 0, hi = P;                    // the last p with iou_off[p] <= e: the problem that owns pair e
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (iou_off[mid] <= e) lo = mid; else hi = mid;
    }
    const int p = lo, G = gt_off[p + 1] - gt_off[p];
    if (G <= 0) continue;                  // (uniform; offsets that contradict each other: nothing to index)
    const int local = (int)(e - iou_off[p]), d = local / G, g = local - d * G;
    const size_t dn = (size_t)(dt_off[p] - d_first + d), gn = (size_t)(gt_off[p] - g_first + g);
    const double *D = dt_rows6 + dn * 6, *B = gt_rows6 + gn * 6;
    // bbIou of the two rleToBbox boxes is > 0 exactly when both extents are: the gate of rleIou
    const double bw = fmin(D[2] + D[0], B[2] + B[0]) - fmax(D[0], B[0]);
    const double bh = fmin(D[3] + D[1], B[3] + B[1]) - fmax(D[1], B[1]);
    double out = 0.;
    if (bw > 0 && bh > 0) {
      const int do0 = dt_rle_off[dn], md = dt_rle_off[dn + 1] - do0;
      const int go0 = gt_rle_off[gn], mg = gt_rle_off[gn + 1] - go0;
      const uint2 *dc = dt_cum2 + do0, *gc = gt_cum2 + go0;
      unsigned inter = 0;
      for (int j = 2 * lane + 1; j < md; j += 2 * kWave) {
        const unsigned s = dc[j - 1].x, t = dc[j].x;
        if (t > s) inter += ones_below(gc, mg, t) - ones_below(gc, mg, s);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) inter += __shfl_xor(inter, off, 64);
      const unsigned area_d = md > 0 ? dc[md - 1].y : 0u, area_g = mg > 0 ? gc[mg - 1].y : 0u;
      const unsigned u = (gt_flags[gn] & 1) ? area_d : area_d + area_g - inter;
      if (inter) out = (double)inter / (double)u;
    }
    if (lane == 0) iou[e] = out;
  }
}

struct Best {
  double iou;
  int idx;
};
// the winner of two candidates: higher IoU, on equal IoU the later box; idx < 0 = no candidate (its iou is -1)
__device__ __forceinline__ Best better(Best a, Best b) {
  const bool take = b.iou > a.iou || (b.iou == a.iou && b.idx > a.idx);
  return take ? b : a;
}
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Best o;
    o.iou = __shfl_xor(v.iou, off, 64);
    o.idx = __shfl_xor(v.idx, off, 64);
    v = better(v, o);
  }
  return v;
}

// one workgroup per problem: rank as coco_match_kernel does, then the A * T matchings dealt to the four waves; lane l holds boxes
// l, l + 64, l + 128, l + 192 and reads row `arrival` of the problem's D x G matrix for every detection (64 consecutive doubles)
__global__ __launch_bounds__(kThreads) void coco_match_iou_kernel(
    const double *__restrict__ dt, const int32_t *__restrict__ dt_off, const int32_t *__restrict__ kp_off,
    const double *__restrict__ gt_area, const uint8_t *__restrict__ gt_flags, const int32_t *__restrict__ gt_off,
    const double *__restrict__ iou, const int32_t *__restrict__ iou_off, const double *__restrict__ iou_thrs,
    const double *__restrict__ area_rng, int T, int A, int max_det, long NK, long NG, int32_t *__restrict__ dt_rank,
    int32_t *__restrict__ dt_match, uint8_t *__restrict__ dt_ignore, int32_t *__restrict__ gt_match, uint8_t *__restrict__ gt_ignore) {
  __shared__ double s_score[kMaxDt];
  __shared__ double s_area[kMaxDt];         // the kept detections' areas, in rank order
  __shared__ int s_order[kMaxDt];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int d0 = dt_off[p], g0 = gt_off[p], k0 = kp_off[p];
  const int Dall = dt_off[p + 1] - d0, G = gt_off[p + 1] - g0;     // (boxes past kMaxGt would have no lane: the entry point refuses them)
  const int D = Dall < kMaxDt ? Dall : kMaxDt;       // the entry point refuses larger problems; never index past the LDS image
  const int kept = D < max_det ? D : max_det;
  const double *drow = dt + (size_t)d0 * 6;
  const double *mat = iou + iou_off[p];               // row stride = the problem's own box count

  for (int i = tid; i < D; i += kThreads) {
    s_score[i] = drow[(size_t)i * 6 + 4];
    s_order[i] = 0;
  }
  __syncthreads();
  for (int i = tid; i < D; i += kThreads) {
    const double si = s_score[i];
    int before = 0;
    for (int j = 0; j < D; ++j) {
      const double sj = s_score[j];
      before += (sj > si) | ((sj == si) & (j < i));
    }
    if (before < kept) {
      s_order[before] = i;
      dt_rank[k0 + before] = i;
    }
  }
  __syncthreads();
  for (int r = tid; r < kept; r += kThreads) s_area[r] = drow[(size_t)s_order[r] * 6 + 5];
  __syncthreads();

  if (G == 0) {      // no box: nothing matches, a detection is ignored where its area lies outside the range
    for (int e = tid; e < A * T * kept; e += kThreads) {
      const int at = e / kept, r = e - at * kept, a = at / T;
      const double darea = s_area[r];
      const size_t o = (size_t)at * NK + k0 + r;
      dt_match[o] = 0;
      dt_ignore[o] = darea < area_rng[2 * a] || darea > area_rng[2 * a + 1] ? 1 : 0;
    }
    return;
  }

  double garea[kGtPerLane];
  int gflag[kGtPerLane];
#pragma unroll
  for (int i = 0; i < kGtPerLane; ++i) {
    const int g = lane + i * kWave;
    const bool ok = g < G;
    garea[i] = ok ? gt_area[g0 + g] : 0.;
    gflag[i] = ok ? (int)gt_flags[g0 + g] : 0;
  }

  // this lane's output addresses (per-lane values live in vector registers: the four scalar pointer pairs end here, and the matching
  // loop keeps within the scalar register file)
  int32_t *const dtm_lane = dt_match + k0 + lane, *const gtm_lane = gt_match + g0 + lane;
  uint8_t *const dtig_lane = dt_ignore + k0 + lane, *const gtig_lane = gt_ignore + g0 + lane;
  const double *const mat_lane = mat + lane;

  for (int at = wave; at < A * T; at += kWaves) {
    const int a = at / T, t = at - a * T;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = fmin(iou_thrs[t], 1 - 1e-10);
    bool gig[kGtPerLane];
    int gm[kGtPerLane];
#pragma unroll
    for (int i = 0; i < kGtPerLane; ++i) {
      gig[i] = (gflag[i] & 3) != 0 || garea[i] < lo || garea[i] > hi;
      gm[i] = 0;
    }
    const size_t orow = (size_t)at * NK;
    int out_m = 0, out_ig = 0;           // lane l holds the result of detection r with r % 64 == l until the 64 are stored together
    for (int r = 0; r < kept; ++r) {
      const double darea = s_area[r];    // every lane the same address: a broadcast
      const double *row = mat_lane + (size_t)s_order[r] * G;      // + i * 64: this lane's boxes
      Best first, second;
      first.iou = second.iou = -1.;
      first.idx = second.idx = -1;
#pragma unroll
      for (int i = 0; i < kGtPerLane; ++i) {
        if (i * kWave >= G) break;        // (uniform: boxes 64 i .. of this problem do not exist)
        const int g = lane + i * kWave;
        const bool crowd = gflag[i] & 1;
        const double v = g < G ? row[i * kWave] : 0.;
        const bool ok = g < G && v >= thr && (crowd || gm[i] == 0);
        Best c;
        c.iou = v;
        c.idx = g;
        if (ok && !gig[i]) first = better(first, c);      // ascending g within a lane: an equal IoU replaces
        if (ok && gig[i]) second = better(second, c);
      }
      first = wave_best(first);
      second = wave_best(second);
      const bool reg = first.idx >= 0;
      const int m = reg ? first.idx : second.idx;
#pragma unroll
      for (int i = 0; i < kGtPerLane; ++i)
        if (m == lane + i * kWave) gm[i] = r + 1;
      if (lane == (r & (kWave - 1))) {
        out_m = m + 1;
        out_ig = m >= 0 ? (reg ? 0 : 1) : (darea < lo || darea > hi ? 1 : 0);
      }
      if ((r & (kWave - 1)) == kWave - 1 || r == kept - 1) {
        const int r0 = r & ~(kWave - 1);
        if (r0 + lane <= r) {
          dtm_lane[orow + r0] = out_m;
          dtig_lane[orow + r0] = (uint8_t)out_ig;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kGtPerLane; ++i) {
      const int g = lane + i * kWave;
      if (g < G) {
        gtm_lane[(size_t)at * NG + i * kWave] = gm[i];
        if (t == 0) gtig_lane[(size_t)a * NG + i * kWave] = gig[i] ? 1 : 0;
      }
    }
  }
}

int wave_grid(long items) {
  const long b = (items + kWaves - 1) / kWaves;
  return (int)(b < 1 ? 1 : (b > kMaxGrid ? kMaxGrid : b));
}

}  // namespace

SN_EXPORT int sn_rle_limits(int32_t *h_out5) {
  SN_REQUIRE(h_out5, "sn_rle_limits: null pointer");
  const int v[5] = {kMaxDt, kMaxGt, kWave, kWaves, kThreads};
  for (int i = 0; i < 5; ++i) h_out5[i] = v[i];
  return SN_OK;
}

SN_EXPORT int sn_rle_stats(const uint32_t *cnts, const int32_t *rle_off, const int32_t *hw, const double *score, long N,
                           long total_runs, long max_hw, double *rows6, uint32_t *cum2, sn_stream_t stream) {
  SN_REQUIRE(cnts && rle_off && hw && rows6 && cum2, "sn_rle_stats: null pointer");
  SN_REQUIRE(N >= 1 && N < 2147483648L / 6, "sn_rle_stats: 1 <= N < 2^31 / 6 required (N = %ld)", N);
  SN_REQUIRE(total_runs >= 0 && total_runs < 2147483648L / 2,
             "sn_rle_stats: the run counts of a call must fit 32-bit indexing, 0 <= total_runs < 2^30 required (total_runs = %ld)",
             total_runs);
  SN_REQUIRE(max_hw >= 1 && max_hw < 2147483648L, "sn_rle_stats: 1 <= h * w < 2^31 required for every mask (max_hw = %ld)", max_hw);
  hipLaunchKernelGGL(rle_stats_kernel, dim3(wave_grid(N)), dim3(kThreads), 0, sn_stream(stream), cnts, rle_off, hw, score, N, rows6,
                     (uint2 *)cum2);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_rle_iou(const uint32_t *dt_cum2, const int32_t *dt_rle_off, const double *dt_rows6, const uint32_t *gt_cum2,
                         const int32_t *gt_rle_off, const double *gt_rows6, const uint8_t *gt_flags, const int32_t *dt_off,
                         const int32_t *gt_off, const int32_t *iou_off, int P, long n_pairs, double *iou, sn_stream_t stream) {
  SN_REQUIRE(dt_cum2 && dt_rle_off && dt_rows6 && gt_cum2 && gt_rle_off && gt_rows6 && gt_flags && dt_off && gt_off && iou_off && iou,
             "sn_rle_iou: null pointer");
  SN_REQUIRE(P >= 1, "sn_rle_iou: P >= 1 required (P = %d)", P);
  SN_REQUIRE(n_pairs >= 0 && n_pairs < 2147483648L, "sn_rle_iou: the pairs of a call must fit 32-bit indexing, 0 <= n_pairs < 2^31 required (n_pairs = %ld)",
             n_pairs);
  if (n_pairs == 0) return SN_OK;          // no problem has both a detection and a ground truth: no matrix entry exists
  hipLaunchKernelGGL(rle_iou_kernel, dim3(wave_grid(n_pairs)), dim3(kThreads), 0, sn_stream(stream), (const uint2 *)dt_cum2, dt_rle_off,
                     dt_rows6, (const uint2 *)gt_cum2, gt_rle_off, gt_rows6, gt_flags, dt_off, gt_off, iou_off, P, n_pairs, iou);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_coco_match_iou(const double *dt, const int32_t *dt_off, const int32_t *kp_off, const double *gt_area,
                                const uint8_t *gt_flags, const int32_t *gt_off, const double *iou, const int32_t *iou_off,
                                const double *iou_thrs, const double *area_rng, int P, int T, int A, int max_det, int max_dt_per_problem,
                                int max_gt_per_problem, long NK, long NG, int32_t *dt_rank, int32_t *dt_match, uint8_t *dt_ignore,
                                int32_t *gt_match, uint8_t *gt_ignore, sn_stream_t stream) {
  SN_REQUIRE(dt && dt_off && kp_off && gt_area && gt_flags && gt_off && iou && iou_off && iou_thrs && area_rng && dt_rank && dt_match &&
                 dt_ignore && gt_match && gt_ignore,
             "sn_coco_match_iou: null pointer");
  SN_REQUIRE(P >= 1, "sn_coco_match_iou: P >= 1 required (P = %d)", P);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_coco_match_iou: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(A >= 1 && A <= kMaxA, "sn_coco_match_iou: 1 <= A <= %d required (A = %d)", kMaxA, A);
  SN_REQUIRE(max_det >= 1, "sn_coco_match_iou: max_det >= 1 required (max_det = %d)", max_det);
  SN_REQUIRE(max_dt_per_problem >= 0 && max_dt_per_problem <= kMaxDt,
             "sn_coco_match_iou: a problem has %d detections, one workgroup ranks at most %d", max_dt_per_problem, kMaxDt);
  SN_REQUIRE(max_gt_per_problem >= 0 && max_gt_per_problem <= kMaxGt,
             "sn_coco_match_iou: a problem has %d masks of ground truth, one workgroup holds at most %d", max_gt_per_problem, kMaxGt);
  SN_REQUIRE(NK >= 0 && NG >= 0, "sn_coco_match_iou: NK >= 0 and NG >= 0 required (NK = %ld, NG = %ld)", NK, NG);
  SN_REQUIRE((double)NK * A * T < 2147483648. && (double)NG * A * T < 2147483648.,
             "sn_coco_match_iou: too many rows, A * T * NK and A * T * NG must fit 32-bit (NK = %ld, NG = %ld)", NK, NG);
  static_assert((size_t)kMaxDt * (2 * sizeof(double) + sizeof(int)) <= 64 * 1024, "LDS without an opt-in");
  hipLaunchKernelGGL(coco_match_iou_kernel, dim3(P), dim3(kThreads), 0, sn_stream(stream), dt, dt_off, kp_off, gt_area, gt_flags, gt_off,
                     iou, iou_off, iou_thrs, area_rng, T, A, max_det, NK, NG, dt_rank, dt_match, dt_ignore, gt_match, gt_ignore);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
