// deform_sample.h -- the DCN v1 bilinear sampling point, shared by the column kernels of roi_deform.hip and the fused grouped
// kernels of gdeform.hip (one copy: both sides of a layer's forward and backward must agree on every border case).
//   p = lattice point + offset (float32);  the sample is zero unless 0 <= p < dim on both axes (ok)
//   low = floor(p); if low >= dim-1: high = low = dim-1, frac = 0; else high = low+1
// The corner indices are only meaningful -- and only inside the map -- under ok: loads are issued under ok alone.
#pragma once
#include "common.h"

struct DeformSample {
  bool ok;
  int y0, y1, x0, x1;
  float ly, lx;
};

__device__ __forceinline__ DeformSample deform_sample(float py, float px, int H, int W) {
  DeformSample s;
  s.ok = py >= 0.f && px >= 0.f && py < (float)H && px < (float)W;
  s.y0 = (int)floorf(py);
  s.x0 = (int)floorf(px);
  if (s.y0 >= H - 1) { s.y0 = s.y1 = H - 1; s.ly = 0.f; } else { s.y1 = s.y0 + 1; s.ly = py - (float)s.y0; }
  if (s.x0 >= W - 1) { s.x0 = s.x1 = W - 1; s.lx = 0.f; } else { s.x1 = s.x0 + 1; s.lx = px - (float)s.x0; }
  return s;
}
