// ohem.hip -- BoxAnnotatorOHEM on the device (lib/operator_py/box_annotator_ohem.py:27-78): per image keep the roi_per_img RoIs
// of largest classification + box loss, ignore the rest.  The operator has no gradient.
//
//   valid = label >= 0
//   loss  = valid ? -log(softmax(score)[min(label, C-1)] + 1e-14) + sum_j w_j * smooth_l1(pred_j - target_j, sigma = 1) : 0
//           (fp32, max-subtracted log-sum-exp)
//   the roi_per_img RoIs of largest loss keep their label and weights (a label < 0 is written as -1, like the reference does);
//   every other RoI gets label -1 and weights 0;   fg_labels = labels_ohem with 0 replaced by -1
//
// ORDER (ours where numpy's argsort is unspecified): RoIs rank by descending loss, equal losses by ascending RoI index, and a NaN
// loss ranks above every number (np.argsort puts NaN last and the reference reverses the order).  The key is sn_float_key(loss)
// with -0 folded into +0 and NaN mapped to the largest key.
//
// ONE launch, one workgroup of 1024 threads per image:
//   1. loss: one wave per RoI row, lanes across the C classes (a row is read coalesced, once; the wave's next row is in flight
//      while the current one is reduced), three wave64 butterfly reductions (max, sum of exponentials, box loss) -> key in LDS.
//   2. rank: thread i counts the keys that beat key i (4 keys per ds_read_b128, every lane the same address: a broadcast, no bank
//      conflict) and writes label / weights / fg label of RoI i -- every output element exactly once, so no fill precedes the call.
// No atomics, no workspace, no host read-back; the result is the same bits every run.  The LDS image is R keys (4 bytes each) in
// the 64 KB a workgroup gets without an opt-in: R <= SN_OHEM_MAX_ROIS = 16384.  The ranking is O(R^2 / 1024) per thread: 300 RoIs
// (the launch shape) cost 75 LDS reads per thread; 6000 (RPN_PRE_NMS_TOP_N) about 9000.
#include "common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxRois = 16384;
constexpr unsigned kKeyNaN = 0xFFFFFFFFu;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float smooth_l1(float d) {   // sigma = 1
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

// what a lane holds of one RoI row while the row before it is reduced
struct RowRegs {
  float v0, v1, label, bp, bt, bw;
};
__device__ __forceinline__ RowRegs load_row(const float *__restrict__ score, const float *__restrict__ pred,
                                            const float *__restrict__ target, const float *__restrict__ weight,
                                            const float *__restrict__ labels, int r, int C, int box_dim, int lane) {
  RowRegs q;
  const float *s = score + (size_t)r * C;
  q.v0 = lane < C ? s[lane] : -INFINITY;
  q.v1 = lane + kWave < C ? s[lane + kWave] : -INFINITY;
  q.label = labels[r];
  const bool b = lane < box_dim;
  const size_t o = (size_t)r * box_dim + lane;
  q.bp = b ? pred[o] : 0.f;
  q.bt = b ? target[o] : 0.f;
  q.bw = b ? weight[o] : 0.f;
  return q;
}

__global__ __launch_bounds__(kThreads) void box_annotator_ohem_kernel(
    const float *__restrict__ cls_score, const float *__restrict__ bbox_pred, const float *__restrict__ labels,
    const float *__restrict__ bbox_targets, const float *__restrict__ bbox_weights, float *__restrict__ labels_ohem,
    float *__restrict__ bbox_weights_ohem, float *__restrict__ fg_labels, int R, int C, int box_dim, int keep) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_key[];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t row0 = (size_t)img * R;
  const float *score = cls_score + row0 * C;
  const float *pred = bbox_pred + row0 * box_dim, *target = bbox_targets + row0 * box_dim, *weight = bbox_weights + row0 * box_dim;
  const float *label = labels + row0;
  const int Rp = (R + 3) & ~3;

  if (keep < R) {
    if (wave < R) {
      RowRegs q = load_row(score, pred, target, weight, label, wave, C, box_dim, lane);
      for (int r = wave; r < R; r += kWaves) {
        const RowRegs c = q;
        if (r + kWaves < R) q = load_row(score, pred, target, weight, label, r + kWaves, C, box_dim, lane);
        const float *s = score + (size_t)r * C;
        float m = fmaxf(c.v0, c.v1);
        for (int k = lane + 2 * kWave; k < C; k += kWave) m = fmaxf(m, s[k]);
        m = wave_max(m);
        float z = (lane < C ? expf(c.v0 - m) : 0.f) + (lane + kWave < C ? expf(c.v1 - m) : 0.f);
        for (int k = lane + 2 * kWave; k < C; k += kWave) z += expf(s[k] - m);
        float box = c.bw * smooth_l1(c.bp - c.bt);
        for (int j = lane + kWave; j < box_dim; j += kWave) {
          const size_t o = (size_t)r * box_dim + j;
          box += weight[o] * smooth_l1(pred[o] - target[o]);
        }
        z = wave_sum(z);
        box = wave_sum(box);
        if (lane == 0) {
          unsigned key = sn_float_key(0.f);
          if (c.label >= 0.f) {
            const int li = (int)fminf(c.label, (float)(C - 1));      // a label >= C reads class C-1, never past the row
            const float p = expf(s[li] - m) / z;
            const float loss = -logf(p + 1e-14f) + box;
            key = loss != loss ? kKeyNaN : sn_float_key(loss == 0.f ? 0.f : loss);
          }
          s_key[r] = key;
        }
      }
    }
    if (tid < Rp - R) s_key[R + tid] = 0u;      // padding of the last ds_read_b128: below every key, beats nothing
    __syncthreads();
  }

  for (int i = tid; i < R; i += kThreads) {
    bool kept = true;
    if (keep < R) {
      const unsigned ki = s_key[i];
      int above = 0;
      for (int j = 0; j < Rp; j += 4) {
        const uint4 k4 = *reinterpret_cast<const uint4 *>(s_key + j);
        above += (k4.x > ki) | ((k4.x == ki) & (j < i));
        above += (k4.y > ki) | ((k4.y == ki) & (j + 1 < i));
        above += (k4.z > ki) | ((k4.z == ki) & (j + 2 < i));
        above += (k4.w > ki) | ((k4.w == ki) & (j + 3 < i));
      }
      kept = above < keep;
    }
    const float l = label[i];
    const float lo = (kept && l >= 0.f) ? l : -1.f;
    labels_ohem[row0 + i] = lo;
    if (fg_labels) fg_labels[row0 + i] = lo == 0.f ? -1.f : lo;
    const size_t o = (row0 + i) * box_dim;
    for (int j = 0; j < box_dim; ++j) bbox_weights_ohem[o + j] = kept ? bbox_weights[o + j] : 0.f;
  }
}

}  // namespace

SN_EXPORT int sn_box_annotator_ohem(const float *cls_score, const float *bbox_pred, const float *labels, const float *bbox_targets,
                                    const float *bbox_weights, float *labels_ohem, float *bbox_weights_ohem, float *fg_labels, int B,
                                    int R, int C, int box_dim, int roi_per_img, sn_stream_t stream) {
  SN_REQUIRE(cls_score && bbox_pred && labels && bbox_targets && bbox_weights && labels_ohem && bbox_weights_ohem,
             "sn_box_annotator_ohem: null pointer");
  SN_REQUIRE(B >= 1, "sn_box_annotator_ohem: B >= 1 required (B = %d)", B);
  SN_REQUIRE(R >= 1, "sn_box_annotator_ohem: R >= 1 required (R = %d)", R);
  SN_REQUIRE(R <= kMaxRois, "sn_box_annotator_ohem: R <= %d required, the keys of one image are ranked in LDS (R = %d)", kMaxRois, R);
  SN_REQUIRE(C >= 2, "sn_box_annotator_ohem: C >= 2 required (C = %d)", C);
  SN_REQUIRE(box_dim >= 1, "sn_box_annotator_ohem: box_dim >= 1 required (box_dim = %d)", box_dim);
  SN_REQUIRE(roi_per_img >= 1, "sn_box_annotator_ohem: roi_per_img >= 1 required (roi_per_img = %d)", roi_per_img);
  static_assert(SN_OHEM_MAX_ROIS == kMaxRois, "the header states the limit");
  const int keep = roi_per_img < R ? roi_per_img : R;
  const size_t lds = keep < R ? (size_t)((R + 3) & ~3) * sizeof(unsigned) : 0;
  hipLaunchKernelGGL(box_annotator_ohem_kernel, dim3(B), dim3(kThreads), lds, sn_stream(stream), cls_score, bbox_pred, labels,
                     bbox_targets, bbox_weights, labels_ohem, bbox_weights_ohem, fg_labels, R, C, box_dim, keep);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
