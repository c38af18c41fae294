// prop_roidb.hip -- the proposal roidb on the device: what lib/dataset/imdb.py does between an RPN proposals pickle and the roidb
// of the negative-chip training run.
//   sn_prop_nms     nmsp (lib/nms/nms.py:48-86) for I images of unsorted (n,5) float32 rows: float32 IoU, suppress at `> thresh`.
//   sn_prop_assign  the body of create_roidb_from_box_list (imdb.py:168-191): float64 bbox_overlaps, row max and first argmax.
//   sn_prop_recall  the greedy one-to-one matching of evaluate_recall (imdb.py:329-374), one (image, area range) pair per workgroup.
// Ragged batches through (I+1) int32 prefix offsets.  The IoU expressions are the ones nms.hip and data_path.hip compute
// (box_overlap.h), the ordering and the wave scan are the evaluators' (eval_order.h).  No float atomics, no scratch, no host
// read-back: the only accumulation across workgroups is integer (num_pos, hits), so the bytes are the same on every run.  The file
// is compiled with -ffp-contract=off (sniper_amd/build.py) and says so itself below.
#include <limits.h>

#include "common.h"
#include "box_overlap.h"
#include "eval_order.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxGt = SN_PROP_MAX_GT;     // ground-truth boxes of one image: in LDS (assign) / one or two per thread (recall)
constexpr int kMaxT = SN_PROP_MAX_T;
constexpr int kBlock = 256;                // proposals per workgroup of the assign launch; threads of the recall workgroup
constexpr int kWaves = kBlock / kWave;
constexpr int kNmsTile = 64;               // candidates resolved per step of the NMS walk
constexpr int kNmsCols = kNmsTile / kWaves;
constexpr int kCols = kMaxGt / kBlock;     // columns a recall thread owns
constexpr int kRetBits = 32768;            // the recall's filter of retired boxes, one bit per (box index mod kRetBits)

static_assert(kCols * kBlock == kMaxGt, "a recall thread owns a whole number of columns");
static_assert(kEvalSortTile == kBlock, "the key and order launches share one grid");

// ---- NMS ---------------------------------------------------------------------------------------------------------------------
// grid (tiles, I): the score column as float64 keys (exact, order-preserving), an image's rows REVERSED: the ordering of
// eval_order.h ranks equal keys by position, so on the reversed rows the LATER row of equal score comes first.
__global__ __launch_bounds__(kBlock) void prop_keys_kernel(const float *__restrict__ rows, const int32_t *__restrict__ off,
                                                           double *__restrict__ keys) {
  const int b = blockIdx.y, c0 = off[b], N = off[b + 1] - c0;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < N) keys[c0 + (N - 1 - i)] = (double)rows[(size_t)(c0 + i) * 5 + 4];
}

// grid (tiles, I): order[c0 + rank] = reversed position (N - 1 - row) of the image's row of that rank
__global__ __launch_bounds__(kEvalSortTile) void prop_order_kernel(const int32_t *__restrict__ off, const double *__restrict__ keys,
                                                                   int32_t *__restrict__ order) {
  __shared__ double s_tile[kEvalSortTile];
  const int b = blockIdx.y, c0 = off[b], N = off[b + 1] - c0;
  sn_eval_order_tile(c0, N, keys, order, 0, s_tile);
}

// One workgroup per image walks the ordered candidates kNmsTile at a time, as nms_lazy_kernel (nms.hip) does for its dense batch:
//   1. every candidate of the chunk against the survivors so far (wave w takes survivors w, w + 4, ...; lane = candidate);
//   2. the upper triangle inside the chunk (wave w computes columns 16 w .. 16 w + 15 of every row);
//   3. wave 0 resolves the chunk in order on those diagonal words and appends the new survivors.
// The survivors' boxes live in the caller's workspace, not in LDS: an image's proposal count has no cap.  The workgroup reads back
// what it wrote itself, across a workgroup barrier.
__global__ __launch_bounds__(kBlock) void prop_nms_kernel(const float *__restrict__ rows, const int32_t *__restrict__ off,
                                                          const int32_t *__restrict__ order, float thresh, float *kept_box,
                                                          int32_t *__restrict__ keep, int32_t *__restrict__ nkeep) {
  __shared__ float cand[kNmsTile * 4];
  __shared__ int cidx[kNmsTile];
  __shared__ unsigned long long dead_w[kWaves];
  __shared__ unsigned dpart[kWaves][kNmsTile];
  __shared__ int nk_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int c0 = off[b], n = off[b + 1] - c0;
  float *kb = kept_box + (size_t)c0 * 4;
  int32_t *kp = keep + c0;
  if (tid == 0) nk_s = 0;
  __syncthreads();
  const int nchunks = (n + kNmsTile - 1) / kNmsTile;
  for (int c = 0; c < nchunks; ++c) {
    const int nk = nk_s;
    const int csize = min(n - c * kNmsTile, kNmsTile);
    if (wave == 0 && lane < csize) {
      const unsigned rev = (unsigned)order[c0 + c * kNmsTile + lane];      // a permutation of the image; held in range regardless
      const int idx = n - 1 - (int)(rev < (unsigned)n ? rev : 0u);
      const float *p = rows + (size_t)(c0 + idx) * 5;
      cand[lane * 4 + 0] = p[0]; cand[lane * 4 + 1] = p[1]; cand[lane * 4 + 2] = p[2]; cand[lane * 4 + 3] = p[3];
      cidx[lane] = idx;
    }
    __syncthreads();
    const bool in = lane < csize;
    float me[4] = {0.f, 0.f, 0.f, 0.f};
    if (in) { me[0] = cand[lane * 4]; me[1] = cand[lane * 4 + 1]; me[2] = cand[lane * 4 + 2]; me[3] = cand[lane * 4 + 3]; }
    // 1. suppressed by an earlier survivor?
    bool dead = false;
    for (int k = wave; k < nk; k += kWaves) {
      const float sv[4] = {kb[k * 4 + 0], kb[k * 4 + 1], kb[k * 4 + 2], kb[k * 4 + 3]};
      dead = dead || (dev_iou(sv, me) > thresh);
    }
    const unsigned long long dw = __ballot(dead && in);
    if (lane == 0) dead_w[wave] = dw;
    // 2. this wave's columns of the chunk's upper triangle
    unsigned bits = 0u;
    if (in) {
#pragma unroll
      for (int jj = 0; jj < kNmsCols; ++jj) {
        const int j = wave * kNmsCols + jj;
        if (j > lane && j < csize && dev_iou(me, cand + j * 4) > thresh) bits |= 1u << jj;
      }
    }
    dpart[wave][lane] = bits;
    __syncthreads();
    // 3. sequential resolution of the chunk: one iteration per new survivor
    if (wave == 0) {
      unsigned long long diag = 0ull, dead_all = 0ull;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        diag |= (unsigned long long)dpart[w][lane] << (w * kNmsCols);
        dead_all |= dead_w[w];
      }
      unsigned long long avail = __ballot(in) & ~dead_all, kept = 0ull;
      int nk2 = nk;
      while (avail != 0ull) {              // wave-uniform
        const int r = __ffsll((long long)avail) - 1;
        const unsigned long long d =
            ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(diag >> 32), r) << 32) |
            (unsigned)__builtin_amdgcn_readlane((int)(diag & 0xffffffffu), r);
        kept |= 1ull << r;
        avail &= ~(d | (1ull << r));
        ++nk2;
      }
      if ((kept >> lane) & 1ull) {
        const int pos = nk + __popcll(kept & ((1ull << lane) - 1ull));     // pos < n: at most one survivor per candidate
        kb[pos * 4 + 0] = me[0]; kb[pos * 4 + 1] = me[1]; kb[pos * 4 + 2] = me[2]; kb[pos * 4 + 3] = me[3];
        kp[pos] = cidx[lane];
      }
      if (lane == 0) nk_s = nk2;
    }
    __threadfence_block();
    __syncthreads();
  }
  const int nk = nk_s;
  for (int j = nk + tid; j < n; j += kBlock) kp[j] = -1;
  if (tid == 0) nkeep[b] = nk;
}

// ---- assignment --------------------------------------------------------------------------------------------------------------
// grid (I, blocks): the image's boxes in LDS (every lane reads the same box: broadcasts), one proposal per thread
__global__ __launch_bounds__(kBlock) void prop_assign_kernel(const double *__restrict__ boxes, const int32_t *__restrict__ box_off,
                                                             const double *__restrict__ gt_box, const int32_t *__restrict__ gt_classes,
                                                             const int32_t *__restrict__ gt_off, float *__restrict__ max_ov,
                                                             int32_t *__restrict__ max_cls, int32_t *__restrict__ argmax) {
  __shared__ double s_gt[kMaxGt * 4];
  __shared__ int s_cls[kMaxGt];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int b0 = box_off[i], N = box_off[i + 1] - b0;
  if ((int)blockIdx.y * kBlock >= N) return;         // the whole workgroup leaves: no barrier is skipped by a part of it
  const int g0 = gt_off[i];
  int G = gt_off[i + 1] - g0;
  G = G < kMaxGt ? G : kMaxGt;                        // the entry point refuses larger images; never index past the LDS image
  for (int e = tid; e < G * 4; e += kBlock) s_gt[e] = gt_box[(size_t)g0 * 4 + e];
  for (int g = tid; g < G; g += kBlock) s_cls[g] = gt_classes[g0 + g];
  __syncthreads();
  const int n = blockIdx.y * kBlock + tid;
  if (n >= N) return;
  const double *b = boxes + (size_t)(b0 + n) * 4;
  const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  double best = -INFINITY;
  int arg = -1;
  for (int g = 0; g < G; ++g) {
    const double o = overlap_f64(x1, y1, x2, y2, s_gt[g * 4 + 0], s_gt[g * 4 + 1], s_gt[g * 4 + 2], s_gt[g * 4 + 3], 0);
    if (o > best) {                                   // ascending g and a strict compare: the FIRST index of the maximum (np.argmax)
      best = o;
      arg = g;
    }
  }
  max_ov[b0 + n] = arg >= 0 ? (float)best : 0.f;      // the assignment into the float32 `overlaps` array
  max_cls[b0 + n] = (arg >= 0 && best > 0.) ? s_cls[arg] : 0;
  argmax[b0 + n] = arg;
}

// ---- recall ------------------------------------------------------------------------------------------------------------------
// the best (overlap, box) of one ground-truth column over the boxes not yet retired; ascending n and a strict compare: the LOWEST
// box index of the maximum (argmax(axis=0)).  A box is retired iff its filter bit is set AND it is in the list: the filter alone
// decides for the boxes never retired, whatever N is.
__device__ __forceinline__ void column_best(const double *__restrict__ boxes, int N, const double q0, const double q1, const double q2,
                                            const double q3, const unsigned *s_bits, const int *s_ret, int nret, double &best, int &arg) {
  best = -1.;
  arg = -1;
  for (int n = 0; n < N; ++n) {
    if (nret && ((s_bits[(n & (kRetBits - 1)) >> 5] >> (n & 31)) & 1u)) {
      bool ret = false;
      for (int k = 0; k < nret; ++k) ret = ret || s_ret[k] == n;
      if (ret) continue;
    }
    const double *b = boxes + (size_t)n * 4;
    const double o = overlap_f64(b[0], b[1], b[2], b[3], q0, q1, q2, q3, 0);
    if (o > best) {
      best = o;
      arg = n;
    }
  }
}

// grid (I, A): one (image, area range) problem per workgroup.  The N x G overlap matrix never exists: a thread owns up to kCols
// columns (ground-truth boxes of the range, in their order) and keeps each one's best (value, box) over the boxes still in play.
// A round is an arg-max over the columns (largest value, then lowest column); it retires that column and its box, and only the
// columns whose best box was the one retired walk the boxes again, with the same expression and hence the same bits.
__global__ __launch_bounds__(kBlock) void prop_recall_kernel(const double *__restrict__ boxes, const int32_t *__restrict__ box_off,
                                                             const double *__restrict__ gt_box, const uint8_t *__restrict__ gt_mask,
                                                             const int32_t *__restrict__ gt_off, const double *__restrict__ thrs, int T,
                                                             long NG, double *__restrict__ gt_ov, int32_t *num_pos, int32_t *hits) {
  __shared__ double s_gt[kMaxGt * 4];
  __shared__ double s_rec[kMaxGt];
  __shared__ double s_thr[kMaxT];
  __shared__ double s_wv[kWaves];
  __shared__ int s_wg[kWaves], s_wb[kWaves], s_cnt[kWaves];
  __shared__ int s_ret[kMaxGt];
  __shared__ unsigned s_bits[kRetBits / 32];
  const int i = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int b0 = box_off[i], N = box_off[i + 1] - b0;
  const int g0 = gt_off[i];
  int G = gt_off[i + 1] - g0;
  G = G < kMaxGt ? G : kMaxGt;
  const double *bx = boxes + (size_t)b0 * 4;

  // the boxes of the range, compacted in their own order
  int Ga = 0;
  for (int c = 0; c < G; c += kBlock) {
    const int g = c + tid;
    const int in = g < G && ((gt_mask[g0 + g] >> a) & 1);
    const int incl = wave_scan_add(in, lane);
    __syncthreads();                       // (the previous chunk's totals have been read)
    if (lane == kWave - 1) s_cnt[wave] = incl;
    __syncthreads();
    int before = Ga, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += s_cnt[w];
      tot += s_cnt[w];
    }
    if (in) {
      const double *q = gt_box + (size_t)(g0 + g) * 4;
      const int pos = before + incl - 1;
      s_gt[pos * 4 + 0] = q[0]; s_gt[pos * 4 + 1] = q[1]; s_gt[pos * 4 + 2] = q[2]; s_gt[pos * 4 + 3] = q[3];
    }
    Ga += tot;
  }
  for (int w = tid; w < kRetBits / 32; w += kBlock) s_bits[w] = 0u;
  if (tid < T) s_thr[tid] = thrs[tid];
  __syncthreads();
  const int rounds = N < Ga ? N : Ga;

  double q[kCols][4], bv[kCols];
  int bb[kCols];
  bool alive[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    const int g = tid + c * kBlock;
    alive[c] = g < Ga && rounds > 0;
    bv[c] = -1.;
    bb[c] = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[c][e] = alive[c] ? s_gt[g * 4 + e] : 0.;
    if (alive[c]) column_best(bx, N, q[c][0], q[c][1], q[c][2], q[c][3], s_bits, s_ret, 0, bv[c], bb[c]);
  }
  for (int r = 0; r < rounds; ++r) {
    double v = -2.;
    int g = INT_MAX, box = -1;
#pragma unroll
    for (int c = 0; c < kCols; ++c)
      if (alive[c] && bv[c] > v) {         // ascending column and a strict compare: the lowest column of equal value
        v = bv[c];
        g = tid + c * kBlock;
        box = bb[c];
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(v, off, 64);
      const int og = __shfl_xor(g, off, 64), ob = __shfl_xor(box, off, 64);
      if (ov > v || (ov == v && og < g)) {
        v = ov;
        g = og;
        box = ob;
      }
    }
    if (lane == 0) {
      s_wv[wave] = v;
      s_wg[wave] = g;
      s_wb[wave] = box;
    }
    __syncthreads();
    v = s_wv[0];
    g = s_wg[0];
    box = s_wb[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
      if (s_wv[w] > v || (s_wv[w] == v && s_wg[w] < g)) {
        v = s_wv[w];
        g = s_wg[w];
        box = s_wb[w];
      }
    if (tid == 0) {
      s_rec[r] = v;
      s_ret[r] = box;
      if (box >= 0) s_bits[(box & (kRetBits - 1)) >> 5] |= 1u << (box & 31);
    }
#pragma unroll
    for (int c = 0; c < kCols; ++c)
      if (tid + c * kBlock == g) alive[c] = false;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kCols; ++c)
      if (alive[c] && bb[c] == box) column_best(bx, N, q[c][0], q[c][1], q[c][2], q[c][3], s_bits, s_ret, r + 1, bv[c], bb[c]);
  }
  __syncthreads();
  // the image's G slots of this range: the recorded values in round order, then zeros (np.zeros(G_a), the unused tail never read)
  double *ov = gt_ov + (size_t)a * NG + g0;
  for (int j = tid; j < G; j += kBlock) ov[j] = j < rounds ? s_rec[j] : 0.;
  if (tid == 0 && Ga > 0) atomicAdd(&num_pos[a], Ga);
  if (N > 0) {                             // imdb.py:348 `continue`: an image without boxes adds no values, only its num_pos
    for (int t = 0; t < T; ++t) {
      const double thr = s_thr[t];
      int cnt = 0;
      for (int j = tid; j < Ga; j += kBlock) cnt += (j < rounds ? s_rec[j] : 0.) >= thr;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
      if (lane == 0 && cnt > 0) atomicAdd(&hits[a * T + t], cnt);
    }
  }
}

size_t nms_ws_keys(long total) { return sn_align((size_t)(total > 0 ? total : 1) * sizeof(double)); }
size_t nms_ws_order(long total) { return sn_align((size_t)(total > 0 ? total : 1) * sizeof(int32_t)); }
size_t nms_ws_kept(long total) { return sn_align((size_t)(total > 0 ? total : 1) * 4 * sizeof(float)); }

}  // namespace

SN_EXPORT int sn_prop_limits(int32_t *h_out6) {
  SN_REQUIRE(h_out6, "sn_prop_limits: null pointer");
  const int v[6] = {kMaxGt, kMaxT, kBlock, kBlock, kNmsTile, kEvalSortTile};
  for (int i = 0; i < 6; ++i) h_out6[i] = v[i];
  return SN_OK;
}

SN_EXPORT size_t sn_prop_nms_workspace_bytes(long total) {
  if (total < 0 || total >= 2147483648L / 5) return 0;
  return nms_ws_keys(total) + nms_ws_order(total) + nms_ws_kept(total);
}

SN_EXPORT int sn_prop_nms(const float *rows, const int32_t *off, int I, int max_n, long total, float thresh, void *ws, size_t ws_bytes,
                          int32_t *keep, int32_t *nkeep, sn_stream_t stream) {
  SN_REQUIRE(rows && off && keep && nkeep, "sn_prop_nms: null pointer");
  SN_REQUIRE(I >= 1 && I <= 65535, "sn_prop_nms: 1 <= I <= 65535 required (I = %d)", I);
  SN_REQUIRE(total >= 0 && total < 2147483648L / 5, "sn_prop_nms: 0 <= total and 5 * total must fit 32-bit (total = %ld)", total);
  SN_REQUIRE(max_n >= 0 && max_n <= total, "sn_prop_nms: 0 <= max_n <= total required (%d, total = %ld)", max_n, total);
  const size_t need = sn_prop_nms_workspace_bytes(total);
  SN_REQUIRE(ws && ws_bytes >= need, "sn_prop_nms: short workspace (%zu bytes, sn_prop_nms_workspace_bytes = %zu)", ws ? ws_bytes : (size_t)0,
             need);
  hipStream_t s = sn_stream(stream);
  double *keys = (double *)ws;
  int32_t *order = (int32_t *)((char *)ws + nms_ws_keys(total));
  float *kept = (float *)((char *)ws + nms_ws_keys(total) + nms_ws_order(total));
  if (max_n > 0) {
    const dim3 grid(sn_div_up(max_n, kBlock), I);
    hipLaunchKernelGGL(prop_keys_kernel, grid, dim3(kBlock), 0, s, rows, off, keys);
    SN_CHECK_LAUNCH();
    hipLaunchKernelGGL(prop_order_kernel, grid, dim3(kEvalSortTile), 0, s, off, keys, order);
    SN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(prop_nms_kernel, dim3(I), dim3(kBlock), 0, s, rows, off, order, thresh, kept, keep, nkeep);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_prop_assign(const double *boxes, const int32_t *box_off, const double *gt_box, const int32_t *gt_classes,
                             const int32_t *gt_off, int I, int max_n, int max_g, long total, long NG, float *max_ov, int32_t *max_cls,
                             int32_t *argmax, sn_stream_t stream) {
  SN_REQUIRE(boxes && box_off && gt_box && gt_classes && gt_off && max_ov && max_cls && argmax, "sn_prop_assign: null pointer");
  SN_REQUIRE(I >= 1, "sn_prop_assign: I >= 1 required (I = %d)", I);
  SN_REQUIRE(total >= 0 && NG >= 0 && total < 2147483648L / 4 && NG < 2147483648L / 4,
             "sn_prop_assign: 0 <= total, NG and 4 * rows must fit 32-bit (total = %ld, NG = %ld)", total, NG);
  SN_REQUIRE(max_n >= 0 && max_n <= total, "sn_prop_assign: 0 <= max_n <= total required (%d, total = %ld)", max_n, total);
  SN_REQUIRE(max_g >= 0 && max_g <= kMaxGt, "sn_prop_assign: an image has %d ground-truth boxes, one workgroup holds at most %d", max_g,
             kMaxGt);
  SN_REQUIRE(sn_div_up(max_n, kBlock) <= 65535, "sn_prop_assign: an image has %d boxes, the launch covers at most %d", max_n, 65535 * kBlock);
  if (max_n == 0) return SN_OK;
  hipLaunchKernelGGL(prop_assign_kernel, dim3(I, sn_div_up(max_n, kBlock)), dim3(kBlock), 0, sn_stream(stream), boxes, box_off, gt_box,
                     gt_classes, gt_off, max_ov, max_cls, argmax);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_prop_recall(const double *boxes, const int32_t *box_off, const double *gt_box, const uint8_t *gt_mask,
                             const int32_t *gt_off, const double *thrs, int I, int A, int T, int max_g, long total, long NG, double *gt_ov,
                             int32_t *num_pos, int32_t *hits, sn_stream_t stream) {
  SN_REQUIRE(boxes && box_off && gt_box && gt_mask && gt_off && thrs && gt_ov && num_pos && hits, "sn_prop_recall: null pointer");
  SN_REQUIRE(I >= 1, "sn_prop_recall: I >= 1 required (I = %d)", I);
  SN_REQUIRE(A >= 1 && A <= 8, "sn_prop_recall: 1 <= A <= 8 required, a range is a bit of gt_mask (A = %d)", A);
  SN_REQUIRE(T >= 1 && T <= kMaxT, "sn_prop_recall: 1 <= T <= %d required (T = %d)", kMaxT, T);
  SN_REQUIRE(total >= 0 && NG >= 0 && total < 2147483648L / 4 && (double)NG * A < 2147483648. / 4,
             "sn_prop_recall: 0 <= total, NG and 4 * rows must fit 32-bit (total = %ld, NG = %ld)", total, NG);
  SN_REQUIRE(max_g >= 0 && max_g <= kMaxGt, "sn_prop_recall: an image has %d ground-truth boxes, one workgroup holds at most %d", max_g,
             kMaxGt);
  hipStream_t s = sn_stream(stream);
  SN_HIP(hipMemsetAsync(num_pos, 0, sizeof(int32_t) * A, s));
  SN_HIP(hipMemsetAsync(hits, 0, sizeof(int32_t) * A * T, s));
  hipLaunchKernelGGL(prop_recall_kernel, dim3(I, A), dim3(kBlock), 0, s, boxes, box_off, gt_box, gt_mask, gt_off, thrs, T, NG, gt_ov, num_pos,
                     hits);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
