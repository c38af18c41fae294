// coco_eval.hip -- COCO box evaluation on the device: COCOeval.evaluateImg and COCOeval.accumulate of
// lib/dataset/pycocotools/cocoeval.py:163-272, 312-365 with the IoU of bbIou (maskApi.c:98-109), float64 and integer counts
// throughout, so that `precision` and `recall` come out on the reference's bits.
//
// sn_coco_match: ONE launch, one workgroup of 256 threads per problem = (category, image) pair with a detection or a box.
//   1. rank: the problem's scores sit in LDS; thread i counts the detections that precede detection i (higher score, equal score
//      by arrival order = Python's stable sorted(key=-score)) and writes its arrival index at its rank.  The first max_det stay.
//      The kept rows are staged in LDS in rank order (min(max_dt_per_problem, max_det) rows of dynamic LDS: the matching loop reads
//      a detection as a broadcast, not as a dependent global load per (a, t, detection)).
//   2. match: the A*T (area range, threshold) matchings are dealt to the four waves.  A wave walks the kept detections in rank
//      order; lane l holds boxes l, l+64, l+128, l+192 of the problem and their matched state in registers, recomputes the IoU of
//      the detection with each (cheaper than a D x G matrix) and the wave picks the winner by a butterfly over (IoU, arrival index):
//      the best IoU >= min(t, 1-1e-10), the LATER box on equal IoU (the reference's `<` lets an equal value replace).  Non-ignored
//      unmatched boxes are searched first; ignored boxes only when none of those qualifies, and among them a matched box is
//      skipped unless it is a crowd.
// sn_coco_accumulate: three launches.
//   1. keys: score and rank-within-problem of every kept detection (binary search of its problem in the kept offsets).
//   2. order: per category, tiles of kSortTile detections; thread i counts the category's detections that precede its own by
//      (descending score, position in the concatenation) -- the total order a stable mergesort of -score yields -- tile by tile
//      through LDS, and writes its position at its rank.  One ordering per category serves every (a, m).
//   3. curves: one workgroup per (category, area range, threshold), chunks of kScanChunk detections: inclusive integer scans of
//      tp / fp with a carry, pr = tp / (fp + tp + eps) into the workspace, a reverse running max over it, then one thread per
//      recall threshold searches rc = tp / npig.  A detection whose rank is >= max_dets[m] counts neither way and is NOT compacted
//      away: it repeats its predecessor's (tp, fp), which changes neither the running max, nor the first index with rc >= thr, nor
//      whether that index is past the end.
// No atomics, no scratch, no host read-back; every output element is written exactly once per call and the bits are the same on
// every run.  The file is compiled with -ffp-contract=off (sniper_amd/build.py) and says so itself below: the reference is built
// for baseline x86-64 and rounds da+ga-w*h twice.
#include "common.h"
#include "eval_order.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxDt = SN_COCO_MAX_DT;     // detections of one problem: their scores are ranked in LDS
constexpr int kMaxGt = SN_COCO_MAX_GT;     // boxes of one problem: four per lane, in registers
constexpr int kGtPerLane = kMaxGt / kWave;
constexpr int kMaxT = 16, kMaxA = 8, kMaxM = 4, kMaxR = 128;
constexpr int kSortTile = kEvalSortTile, kScanChunk = kEvalScanChunk;     // eval_order.h: shared with voc_eval.hip
constexpr double kEps = 2.220446049250313e-16;   // np.spacing(1)

static_assert(kGtPerLane * kWave == kMaxGt, "a lane holds a whole number of boxes");

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

__global__ __launch_bounds__(kThreads) void coco_match_kernel(
    const double *__restrict__ dt, const int32_t *__restrict__ dt_off, const int32_t *__restrict__ kp_off,
    const double *__restrict__ gt, const uint8_t *__restrict__ gt_flags, const int32_t *__restrict__ gt_off,
    const double *__restrict__ iou_thrs, const double *__restrict__ area_rng, int T, int A, int max_det, int kept_cap, long NK,
    long NG, int32_t *__restrict__ dt_rank, int32_t *__restrict__ dt_match, uint8_t *__restrict__ dt_ignore, int32_t *__restrict__ gt_match,
    uint8_t *__restrict__ gt_ignore) {
  __shared__ double s_score[kMaxDt];
  __shared__ int s_order[kMaxDt];
  // the kept detections in rank order, six doubles each: x, y, x + w, y + h, w * h, area (kept_cap rows of dynamic LDS)
  extern __shared__ __attribute__((aligned(16))) double s_det[];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int d0 = dt_off[p], g0 = gt_off[p], k0 = kp_off[p];
  int D = dt_off[p + 1] - d0, G = gt_off[p + 1] - g0;
  D = D < kMaxDt ? D : kMaxDt;          // the entry point refuses larger problems; never index past the LDS image
  G = G < kMaxGt ? G : kMaxGt;
  int kept = D < max_det ? D : max_det;
  kept = kept < kept_cap ? kept : kept_cap;      // = kept unless the caller understated max_dt_per_problem: never past s_det
  const double *drow = dt + (size_t)d0 * 6;

  for (int i = tid; i < D; i += kThreads) {
    s_score[i] = drow[(size_t)i * 6 + 4];
    s_order[i] = 0;                     // (a NaN score ranks nowhere: its slot still names a row of this problem)
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
  for (int r = tid; r < kept; r += kThreads) {
    const double *d = drow + (size_t)s_order[r] * 6;
    const double x = d[0], y = d[1], w = d[2], h = d[3];
    double *o = s_det + r * 6;
    o[0] = x;
    o[1] = y;
    o[2] = w + x;
    o[3] = h + y;
    o[4] = w * h;
    o[5] = d[5];
  }
  __syncthreads();

  if (G == 0) {      // no box: nothing matches, a detection is ignored where its area lies outside the range
    for (int e = tid; e < A * T * kept; e += kThreads) {
      const int at = e / kept, r = e - at * kept, a = at / T;
      const double darea = s_det[r * 6 + 5];
      const size_t o = (size_t)at * NK + k0 + r;
      dt_match[o] = 0;
      dt_ignore[o] = darea < area_rng[2 * a] || darea > area_rng[2 * a + 1] ? 1 : 0;
    }
    return;
  }

  // this lane's boxes: x, y, x + w, y + h, w * h, the annotation's area and its flags
  double gx[kGtPerLane], gy[kGtPerLane], gx2[kGtPerLane], gy2[kGtPerLane], gwh[kGtPerLane], garea[kGtPerLane];
  int gflag[kGtPerLane];
#pragma unroll
  for (int i = 0; i < kGtPerLane; ++i) {
    const int g = lane + i * kWave;
    const bool ok = g < G;
    const double *b = gt + (size_t)(g0 + (ok ? g : 0)) * 5;
    const double x = ok ? b[0] : 0., y = ok ? b[1] : 0., w = ok ? b[2] : 0., h = ok ? b[3] : 0.;
    gx[i] = x;
    gy[i] = y;
    gx2[i] = w + x;
    gy2[i] = h + y;
    gwh[i] = w * h;
    garea[i] = ok ? b[4] : 0.;
    gflag[i] = ok ? (int)gt_flags[g0 + g] : 0;
  }

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
    const size_t orow = (size_t)at * NK + k0;
    int out_m = 0, out_ig = 0;           // lane l holds the result of detection r with r % 64 == l until the 64 are stored together
    for (int r = 0; r < kept; ++r) {
      const double *d = s_det + r * 6;   // every lane the same address: a broadcast
      const double dx = d[0], dy = d[1], dx2 = d[2], dy2 = d[3], da = d[4], darea = d[5];
      Best first, second;
      first.iou = second.iou = -1.;
      first.idx = second.idx = -1;
#pragma unroll
      for (int i = 0; i < kGtPerLane; ++i) {
        if (i * kWave >= G) break;        // (uniform: boxes 64 i .. of this problem do not exist)
        const int g = lane + i * kWave;
        const bool crowd = gflag[i] & 1;
        double iou = 0.;
        const double w = fmin(dx2, gx2[i]) - fmax(dx, gx[i]);
        const double h = fmin(dy2, gy2[i]) - fmax(dy, gy[i]);
        if (w > 0 && h > 0) {
          const double in = w * h;
          const double u = crowd ? da : da + gwh[i] - in;
          iou = in / u;
        }
        const bool ok = g < G && iou >= thr && (crowd || gm[i] == 0);
        Best c;
        c.iou = iou;
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
          dt_match[orow + r0 + lane] = out_m;
          dt_ignore[orow + r0 + lane] = (uint8_t)out_ig;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kGtPerLane; ++i) {
      const int g = lane + i * kWave;
      if (g < G) {
        gt_match[(size_t)at * NG + g0 + g] = gm[i];
        if (t == 0) gt_ignore[(size_t)a * NG + g0 + g] = gig[i] ? 1 : 0;
      }
    }
  }
}

// (x1, y1, x2, y2, score) rows, float32 or float64, -> (x, y, w = x2 - x1 + 1, h = y2 - y1 + 1, score, w * h) float64 rows; row j of the
// output reads row src[j] of the input (src = NULL: row j)
template <typename TIn>
__global__ __launch_bounds__(256) void coco_pack_rows_kernel(const TIn *__restrict__ rows, const int32_t *__restrict__ src, long n,
                                                             double *__restrict__ dt6) {
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
    const TIn *r = rows + (size_t)(src ? src[j] : j) * 5;
    const double x1 = (double)r[0], y1 = (double)r[1], x2 = (double)r[2], y2 = (double)r[3];
    const double w = x2 - x1 + 1, h = y2 - y1 + 1;
    double *o = dt6 + (size_t)j * 6;
    o[0] = x1;
    o[1] = y1;
    o[2] = w;
    o[3] = h;
    o[4] = (double)r[4];
    o[5] = w * h;
  }
}

// score and rank-within-problem of every kept detection
__global__ __launch_bounds__(256) void coco_keys_kernel(const double *__restrict__ dt, const int32_t *__restrict__ dt_off,
                                                        const int32_t *__restrict__ kp_off, const int32_t *__restrict__ dt_rank,
                                                        int P, long NK, double *__restrict__ ws_score,
                                                        int32_t *__restrict__ ws_rank) {
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < NK; j += (long)gridDim.x * 256) {
    int lo = 0, hi = P;                  // the last p with kp_off[p] <= j (kp_off[0] = 0, kp_off[P] = NK > j)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (kp_off[mid] <= j) lo = mid; else hi = mid;
    }
    const int D = dt_off[lo + 1] - dt_off[lo];
    int arrival = dt_rank[j];            // written by sn_coco_match; held inside the problem's rows whatever the caller passes
    arrival = arrival < 0 ? 0 : (arrival < D ? arrival : D - 1);
    ws_score[j] = dt[((size_t)dt_off[lo] + arrival) * 6 + 4];
    ws_rank[j] = (int)(j - kp_off[lo]);
  }
}

// grid (tiles, K): the order of category k's kept detections by (descending score, position) -- eval_order.h
__global__ __launch_bounds__(kSortTile) void coco_order_kernel(const int32_t *__restrict__ cat_off, const int32_t *__restrict__ kp_off,
                                                               const double *__restrict__ ws_score, int32_t *__restrict__ ws_order) {
  __shared__ double s_tile[kSortTile];
  const int k = blockIdx.y;
  const int c0 = kp_off[cat_off[k]], N = kp_off[cat_off[k + 1]] - c0;
  sn_eval_order_tile(c0, N, ws_score, ws_order, 0, s_tile);
}

struct MaxDets {
  int n, v[kMaxM];
};

// grid (A*T, K): precision[t, :, k, a, :] and recall[t, k, a, :]
__global__ __launch_bounds__(kScanChunk) void coco_curves_kernel(
    const int32_t *__restrict__ cat_off, const int32_t *__restrict__ kp_off, const int32_t *__restrict__ gt_off,
    const int32_t *__restrict__ dt_match, const uint8_t *__restrict__ dt_ignore, const uint8_t *__restrict__ gt_ignore,
    const int32_t *__restrict__ ws_rank, const int32_t *__restrict__ ws_order, const double *__restrict__ rec_thrs, MaxDets md,
    int T, int A, int K, int R, long NK, long NG, int32_t *__restrict__ ws_tp, double *__restrict__ ws_pr,
    double *__restrict__ precision, double *__restrict__ recall) {
  __shared__ int s_tp[kWaves], s_fp[kWaves], s_red[kWaves];
  __shared__ double s_mx[kWaves];
  const int at = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int a = at / T, t = at - a * T, M = md.n;
  const int p0 = cat_off[k], p1 = cat_off[k + 1];
  const int c0 = kp_off[p0], N = kp_off[p1] - c0;
  const int g0 = gt_off[p0], g1 = gt_off[p1];

  // npig: the category's boxes that area range a does not ignore
  int cnt = 0;
  for (int g = g0 + tid; g < g1; g += kScanChunk) cnt += gt_ignore[(size_t)a * NG + g] == 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) s_red[wave] = cnt;
  __syncthreads();
  int npig = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) npig += s_red[w];
  __syncthreads();

  const size_t rec_at = ((size_t)(t * K + k) * A + a) * M;
  if (p0 == p1 || npig == 0) {           // cocoeval.py:319-320, 331-332: the -1 of an absent category stays
    for (int e = tid; e < R * M; e += kScanChunk) {
      const int r = e / M, m = e - r * M;
      precision[(((size_t)(t * R + r) * K + k) * A + a) * M + m] = -1.;
    }
    if (tid < M) recall[rec_at + tid] = -1.;
    return;
  }
  const double dn = (double)npig;
  const size_t slab = (size_t)at * NK + c0;
  int32_t *tp_s = ws_tp + slab;
  double *pr_s = ws_pr + slab;
  const int32_t *order = ws_order + c0;

  for (int m = 0; m < M; ++m) {
    const int cap = md.v[m];
    // inclusive scans of tp and fp over the ordered detections, chunk by chunk with a carry
    int ctp = 0, cfp = 0;
    for (int base = 0; base < N; base += kScanChunk) {
      const int i = base + tid;
      int vt = 0, vf = 0;
      if (i < N) {
        const unsigned o = (unsigned)order[i];     // a permutation of [0, N); held in range if max_kept_per_category was understated
        const int j = c0 + (int)(o < (unsigned)N ? o : 0u);
        const bool in = ws_rank[j] < cap && dt_ignore[(size_t)at * NK + j] == 0;
        const bool hit = dt_match[(size_t)at * NK + j] != 0;
        vt = in && hit;
        vf = in && !hit;
      }
      vt = wave_scan_add(vt, lane);
      vf = wave_scan_add(vf, lane);
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
        tp_s[i] = vt;
        pr_s[i] = (double)vt / ((double)(vf + vt) + kEps);
      }
      ctp += tot_t;
      cfp += tot_f;
      __syncthreads();
    }
    if (tid == 0) recall[rec_at + m] = N ? (double)ctp / dn : 0.;
    // pr non-increasing from the right: a reverse running max, chunk by chunk from the end
    double cmx = -1.;                    // below every pr (pr >= 0)
    const int nchunk = (N + kScanChunk - 1) / kScanChunk;
    for (int c = nchunk - 1; c >= 0; --c) {
      const int i = c * kScanChunk + tid;
      double v = i < N ? pr_s[i] : -1.;
      v = wave_scan_max_rev(v, lane);
      if (lane == 0) s_mx[wave] = v;
      __syncthreads();
      double tot = cmx;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        if (w > wave) v = fmax(v, s_mx[w]);
        tot = fmax(tot, s_mx[w]);
      }
      v = fmax(v, cmx);
      if (i < N) pr_s[i] = v;
      cmx = tot;
      __syncthreads();
    }
    // q[r] = pr[searchsorted(rc, thr, left)]; from the first threshold whose index is N onward q stays 0 (the reference's
    // try/except leaves the loop there)
    __threadfence_block();
    __syncthreads();
    int fail = R;
    for (int r = tid; r < R; r += kScanChunk) {
      const double thr = rec_thrs[r];
      int lo = 0, hi = N;                // the first i with rc[i] >= thr
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)tp_s[mid] / dn < thr) lo = mid + 1; else hi = mid;
      }
      if (lo == N && r < fail) fail = r;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(fail, off, 64);
      fail = o < fail ? o : fail;
    }
    if (lane == 0) s_red[wave] = fail;
    __syncthreads();
    fail = R;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) fail = s_red[w] < fail ? s_red[w] : fail;
    for (int r = tid; r < R; r += kScanChunk) {
      double q = 0.;
      if (r < fail) {
        const double thr = rec_thrs[r];
        int lo = 0, hi = N;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((double)tp_s[mid] / dn < thr) lo = mid + 1; else hi = mid;
        }
        q = pr_s[lo];                    // lo < N: r is below the first failing threshold
      }
      precision[(((size_t)(t * R + r) * K + k) * A + a) * M + m] = q;
    }
    __syncthreads();
  }
}

struct Ws {
  size_t score, rank, order, tp, pr, total;
};
Ws ws_layout(long NK, int T, int A) {
  const size_t n = NK > 0 ? (size_t)NK : 1, at = (size_t)A * T;
  Ws w;
  size_t o = 0;
  w.score = o; o += sn_align(n * sizeof(double));
  w.rank = o;  o += sn_align(n * sizeof(int32_t));
  w.order = o; o += sn_align(n * sizeof(int32_t));
  w.tp = o;    o += sn_align(at * n * sizeof(int32_t));
  w.pr = o;    o += sn_align(at * n * sizeof(double));
  w.total = o;
  return w;
}

}  // namespace

SN_EXPORT int sn_coco_limits(int32_t *h_out8) {
  SN_REQUIRE(h_out8, "sn_coco_limits: null pointer");
  const int v[8] = {kMaxDt, kMaxGt, kMaxT, kMaxA, kMaxM, kMaxR, kSortTile, kScanChunk};
  for (int i = 0; i < 8; ++i) h_out8[i] = v[i];
  return SN_OK;
}

SN_EXPORT int sn_coco_pack_rows(const void *rows, int rows_f32, const int32_t *src, long n, double *dt6, sn_stream_t stream) {
  SN_REQUIRE(rows && dt6, "sn_coco_pack_rows: null pointer");
  SN_REQUIRE(n >= 1 && n < 2147483648L / 6, "sn_coco_pack_rows: 1 <= n < 2^31 / 6 required (n = %ld)", n);
  SN_REQUIRE(rows_f32 == 0 || rows_f32 == 1, "sn_coco_pack_rows: rows_f32 must be 0 (float64) or 1 (float32), got %d", rows_f32);
  if (rows_f32)
    hipLaunchKernelGGL(coco_pack_rows_kernel<float>, dim3(sn_blocks(n, 4096)), dim3(256), 0, sn_stream(stream), (const float *)rows, src,
                       n, dt6);
  else
    hipLaunchKernelGGL(coco_pack_rows_kernel<double>, dim3(sn_blocks(n, 4096)), dim3(256), 0, sn_stream(stream), (const double *)rows,
                       src, n, dt6);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT size_t sn_coco_match_workspace_bytes(void) { return 0; }

SN_EXPORT int sn_coco_match(const double *dt, const int32_t *dt_off, const int32_t *kp_off, const double *gt, const uint8_t *gt_flags,
                            const int32_t *gt_off, const double *iou_thrs, const double *area_rng, int P, int T, int A, int max_det,
                            int max_dt_per_problem, int max_gt_per_problem, long NK, long NG, int32_t *dt_rank, int32_t *dt_match,
                            uint8_t *dt_ignore, int32_t *gt_match, uint8_t *gt_ignore, sn_stream_t stream) {
  SN_REQUIRE(dt && dt_off && kp_off && gt && gt_flags && gt_off && iou_thrs && area_rng && dt_rank && dt_match && dt_ignore &&
                 gt_match && gt_ignore,
             "sn_coco_match: null pointer");
  SN_REQUIRE(P >= 1, "sn_coco_match: P >= 1 required (P = %d)", P);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_coco_match: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(A >= 1 && A <= kMaxA, "sn_coco_match: 1 <= A <= %d required (A = %d)", kMaxA, A);
  SN_REQUIRE(max_det >= 1, "sn_coco_match: max_det >= 1 required (max_det = %d)", max_det);
  SN_REQUIRE(max_dt_per_problem >= 0 && max_dt_per_problem <= kMaxDt,
             "sn_coco_match: a problem has %d detections, one workgroup ranks at most %d", max_dt_per_problem, kMaxDt);
  SN_REQUIRE(max_gt_per_problem >= 0 && max_gt_per_problem <= kMaxGt,
             "sn_coco_match: a problem has %d boxes, one workgroup holds at most %d", max_gt_per_problem, kMaxGt);
  SN_REQUIRE(NK >= 0 && NG >= 0, "sn_coco_match: NK >= 0 and NG >= 0 required (NK = %ld, NG = %ld)", NK, NG);
  SN_REQUIRE((double)NK * A * T < 2147483648. && (double)NG * A * T < 2147483648.,
             "sn_coco_match: too many rows, A * T * NK and A * T * NG must fit 32-bit (NK = %ld, NG = %ld)", NK, NG);
  static_assert(SN_COCO_MAX_T == kMaxT && SN_COCO_MAX_A == kMaxA && SN_COCO_MAX_M == kMaxM && SN_COCO_MAX_R == kMaxR,
                "the header states the limits");
  // dynamic LDS: the kept rows of the largest problem, at most 1024 * 48 bytes beside the 12 KB of scores and order: 60 KB
  int kept_cap = max_dt_per_problem < max_det ? max_dt_per_problem : max_det;
  kept_cap = kept_cap < 1 ? 1 : kept_cap;
  static_assert((size_t)kMaxDt * 6 * sizeof(double) + kMaxDt * (sizeof(double) + sizeof(int)) <= 64 * 1024, "LDS without an opt-in");
  hipLaunchKernelGGL(coco_match_kernel, dim3(P), dim3(kThreads), (size_t)kept_cap * 6 * sizeof(double), sn_stream(stream), dt, dt_off, kp_off, gt, gt_flags, gt_off,
                     iou_thrs, area_rng, T, A, max_det, kept_cap, NK, NG, dt_rank, dt_match, dt_ignore, gt_match, gt_ignore);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT size_t sn_coco_accumulate_workspace_bytes(long NK, int T, int A) {
  if (NK < 0 || T < 1 || A < 1 || T > kMaxT || A > kMaxA) return 0;
  return ws_layout(NK, T, A).total;
}

SN_EXPORT int sn_coco_accumulate(const double *dt, const int32_t *dt_off, const int32_t *kp_off, const int32_t *gt_off,
                                 const int32_t *cat_off, const int32_t *dt_rank, const int32_t *dt_match, const uint8_t *dt_ignore,
                                 const uint8_t *gt_ignore, const double *rec_thrs, const int32_t *h_max_dets, int P, int K, int T,
                                 int A, int M, int R, int max_det, int max_kept_per_category, long NK, long NG, void *ws,
                                 size_t ws_bytes, double *precision, double *recall, sn_stream_t stream) {
  SN_REQUIRE(dt && dt_off && kp_off && gt_off && cat_off && dt_rank && dt_match && dt_ignore && gt_ignore && rec_thrs &&
                 h_max_dets && precision && recall,
             "sn_coco_accumulate: null pointer");
  SN_REQUIRE(P >= 1, "sn_coco_accumulate: P >= 1 required (P = %d)", P);
  SN_REQUIRE(K >= 1 && K <= 65535, "sn_coco_accumulate: 1 <= K <= 65535 required (K = %d)", K);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_coco_accumulate: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(A >= 1 && A <= kMaxA, "sn_coco_accumulate: 1 <= A <= %d required (A = %d)", kMaxA, A);
  SN_REQUIRE(M >= 1 && M <= kMaxM, "sn_coco_accumulate: 1 <= M <= %d required (M = %d)", kMaxM, M);
  SN_REQUIRE(R >= 1 && R <= kMaxR, "sn_coco_accumulate: 1 <= R <= %d required (R = %d)", kMaxR, R);
  SN_REQUIRE(max_det >= 1, "sn_coco_accumulate: max_det >= 1 required (max_det = %d)", max_det);
  MaxDets md;
  md.n = M;
  for (int m = 0; m < kMaxM; ++m) md.v[m] = m < M ? h_max_dets[m] : 0;
  SN_REQUIRE(md.v[0] >= 1, "sn_coco_accumulate: max_dets[0] >= 1 required (max_dets[0] = %d)", md.v[0]);
  for (int m = 1; m < M; ++m)
    SN_REQUIRE(md.v[m] > md.v[m - 1], "sn_coco_accumulate: max_dets must be ascending (max_dets[%d] = %d after %d)", m, md.v[m],
               md.v[m - 1]);
  SN_REQUIRE(md.v[M - 1] == max_det, "sn_coco_accumulate: the last of max_dets must equal max_det (%d != %d)", md.v[M - 1], max_det);
  SN_REQUIRE(NK >= 0 && NG >= 0, "sn_coco_accumulate: NK >= 0 and NG >= 0 required (NK = %ld, NG = %ld)", NK, NG);
  SN_REQUIRE(max_kept_per_category >= 0 && max_kept_per_category <= NK,
             "sn_coco_accumulate: 0 <= max_kept_per_category <= NK required (%d, NK = %ld)", max_kept_per_category, NK);
  SN_REQUIRE((double)NK * A * T < 2147483648. && (double)NG * A * T < 2147483648.,
             "sn_coco_accumulate: too many rows, A * T * NK and A * T * NG must fit 32-bit (NK = %ld, NG = %ld)", NK, NG);
  SN_REQUIRE((double)T * R * K * A * M < 2147483648., "sn_coco_accumulate: too many precision entries for 32-bit indexing");
  const Ws w = ws_layout(NK, T, A);
  SN_REQUIRE(ws && ws_bytes >= w.total, "sn_coco_accumulate: short workspace (%zu bytes, sn_coco_accumulate_workspace_bytes = %zu)",
             ws ? ws_bytes : (size_t)0, w.total);
  char *b = (char *)ws;
  double *ws_score = (double *)(b + w.score);
  int32_t *ws_rank = (int32_t *)(b + w.rank), *ws_order = (int32_t *)(b + w.order), *ws_tp = (int32_t *)(b + w.tp);
  double *ws_pr = (double *)(b + w.pr);
  hipStream_t s = sn_stream(stream);
  if (NK > 0) {
    hipLaunchKernelGGL(coco_keys_kernel, dim3(sn_blocks(NK, 4096)), dim3(256), 0, s, dt, dt_off, kp_off, dt_rank, P, NK, ws_score,
                       ws_rank);
    SN_CHECK_LAUNCH();
    if (max_kept_per_category > 0) {
      hipLaunchKernelGGL(coco_order_kernel, dim3(sn_div_up(max_kept_per_category, kSortTile), K), dim3(kSortTile), 0, s, cat_off,
                         kp_off, ws_score, ws_order);
      SN_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(coco_curves_kernel, dim3(A * T, K), dim3(kScanChunk), 0, s, cat_off, kp_off, gt_off, dt_match, dt_ignore,
                     gt_ignore, ws_rank, ws_order, rec_thrs, md, T, A, K, R, NK, NG, ws_tp, ws_pr, precision, recall);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
