// box_overlap.h -- the two box-overlap expressions the library computes on the reference's bits, each written once: the float64
// overlap of lib/bbox/bbox.pyx (data_path.hip, prop_roidb.hip) and the float32 IoU of lib/nms/nms_kernel.cu, which is also the
// arithmetic of lib/nms/nms.py (nms.hip, prop_roidb.hip).  Internal, not part of the C ABI.  Every including file is compiled with
// -ffp-contract=off: the reference rounds after every multiply.
#pragma once
#include "common.h"

__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }

// bbox.pyx:17-57 (mode 0) / :59-95 (mode 1); b = box, q = query box.
__device__ __forceinline__ double overlap_f64(const double b0, const double b1, const double b2, const double b3,
                                              const double q0, const double q1, const double q2, const double q3,
                                              const int mode) {
  const double box_area = (q2 - q0 + 1) * (q3 - q1 + 1);
  const double iw = dmin(b2, q2) - dmax(b0, q0) + 1;
  if (iw > 0) {
    const double ih = dmin(b3, q3) - dmax(b1, q1) + 1;
    if (ih > 0) {
      if (mode == 0) {
        const double ua = (b2 - b0 + 1) * (b3 - b1 + 1) + box_area - iw * ih;
        return iw * ih / ua;
      }
      return iw * ih / box_area;
    }
  }
  return 0.0;
}

// nms_kernel.cu:24-32 devIoU; nms.py:66-81 computes the same float32 operations in the same order
__device__ __forceinline__ float dev_iou(const float *a, const float *b) {
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float width = fmaxf(right - left + 1, 0.f), height = fmaxf(bottom - top + 1, 0.f);
  const float interS = width * height;
  const float Sa = (a[2] - a[0] + 1) * (a[3] - a[1] + 1);
  const float Sb = (b[2] - b[0] + 1) * (b[3] - b[1] + 1);
  return interS / (Sa + Sb - interS);
}
