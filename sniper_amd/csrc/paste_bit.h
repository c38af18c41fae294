// paste_bit.h -- the ONE copy of the resize-and-threshold arithmetic of a mask probability map in its box: included by mask_rle.hip
// (the paste of mask_voc2coco into an image, sn_rle_paste), by voc_segm.hip (the region overlap of voc_eval_sds, sn_vocsds_mask_iou)
// and by render.hip (the mask overlay of sn_render_dets).  All must be compiled with -ffp-contract=off (sniper_amd/build.py): the two passes round every product and sum on their own.
//
// Detection n: an (M, M) float32 mask resized to its box (bw = x2 - x1 + 1, bh = y2 - y1 + 1) and thresholded.  The resize is THIS
// PROJECT'S statement of the float32 INTER_LINEAR path of the algorithm oracle/cv_resize.py documents for uint8 (not pinned to OpenCV):
// scale = 1 / (b / M) in double per axis; coefficient f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; in x both ends clamp
// (s < 0: s = 0, f = 0; s >= M - 1: s = M - 1 and the value is S[s]); in y the two source rows are clipped to [0, M - 1] and the
// coefficient is kept; horizontal pass S[s] * (1 - f) + S[s + 1] * f, then vertical pass r0 * (1 - g) + r1 * g, all float32, no fused
// multiply-add; the exact 2 x 2 decimation (both scales 2) is the area average (((a + b) + c) + d) * 0.25f of the block in row-major
// order.
#pragma once
#include "common.h"

struct PasteBox {
  int x1, y1, bw, bh, h, w;      // h, w: the image (the paste only; the region overlap knows no image and leaves them 0)
  double sx, sy;
  bool area;
};
// detection n of a call: its box (x1, y1, x2, y2) inclusive, its image's (h, w)
__device__ __forceinline__ PasteBox paste_box(const int32_t *__restrict__ boxes, const int32_t *__restrict__ hw, int n, int M) {
  PasteBox b;
  b.x1 = boxes[4 * n];
  b.y1 = boxes[4 * n + 1];
  b.bw = boxes[4 * n + 2] - b.x1 + 1;
  b.bh = boxes[4 * n + 3] - b.y1 + 1;
  b.h = hw[2 * n];
  b.w = hw[2 * n + 1];
  b.sx = 1. / ((double)b.bw / M);
  b.sy = 1. / ((double)b.bh / M);
  b.area = 2 * b.bw == M && 2 * b.bh == M;
  return b;
}
// the mask bit of column c, row r of the box; S may be global or LDS memory, M * M floats
__device__ __forceinline__ bool paste_bit(const float *__restrict__ S, int M, const PasteBox &b, int c, int r, float thr) {
  float v;
  if (b.area) {
    const float *q = S + (size_t)(2 * r) * M + 2 * c;
    v = (((q[0] + q[1]) + q[M]) + q[M + 1]) * 0.25f;
  } else {
    float fx = (float)((c + 0.5) * b.sx - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    float fy = (float)((r + 0.5) * b.sy - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    const int r0 = sy < 0 ? 0 : (sy > M - 1 ? M - 1 : sy), r1 = sy + 1 < 0 ? 0 : (sy + 1 > M - 1 ? M - 1 : sy + 1);
    const float *p0 = S + (size_t)r0 * M, *p1 = S + (size_t)r1 * M;
    float h0, h1;
    if (sx >= M - 1) {
      h0 = p0[M - 1];
      h1 = p1[M - 1];
    } else {
      const float a0 = 1.f - fx;
      h0 = p0[sx] * a0 + p0[sx + 1] * fx;
      h1 = p1[sx] * a0 + p1[sx + 1] * fx;
    }
    v = h0 * (1.f - fy) + h1 * fy;
  }
  return v >= thr;
}
