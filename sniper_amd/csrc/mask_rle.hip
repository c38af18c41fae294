// mask_rle.hip -- polygons to run-length encoded masks on the device: rleFrPoly (lib/dataset/pycocotools/maskApi.c:139-179) per
// polygon and the union of an annotation's parts (rleMerge with intersect = 0, :49-70), on the reference's counts (DESIGN.md
// section 22).  float64 with the C casts that truncate toward zero; compiled with -ffp-contract=off.
//
// The reference walks the 5x upsampled boundary, keeps a point (x * h + y) wherever x changes, sorts them with the sentinel h * w and
// compacts sequentially: a position of odd multiplicity toggles the mask, an even one cancels, and whatever equals h * w shares the
// end with the sentinel.  So the mask is the parity of the crossings at or before a pixel, and its runs end at the distinct
// positions of odd multiplicity below h * w, in ascending order.  Three kernels, a workgroup of 256 threads per polygon / annotation:
//   poly_cross_kernel   the boundary walk, closed form per point: the edge of point j by binary search in the prefix of the edges'
//                       point counts (built on the host from the same integer vertices), then (u, v) of points j and j - 1 and
//                       the reference's filter.  Run twice: a count pass, and -- after the host has turned the counts into
//                       offsets -- a fill pass whose slots come from a block scan with a carry (the same order every run).
//   poly_runs_kernel    per crossing: is it the first of its value and is the value's multiplicity odd (a count over the polygon's
//                       crossings), then its rank among such values (a second count).  No sort, hence no LDS path and no size
//                       at which another path takes over; quadratic in the crossings of ONE polygon.
//   poly_union_kernel   an annotation of one part is copied.  With several parts, a pixel is set when any part's parity is odd: the
//                       candidates are the parts' run ends, a candidate is a run end of the union when the OR changes there (binary
//                       searches in every part), counted once (by the first part that holds it) and ranked by counting.
// Outputs land in pools with slack (crossings + 1 counts per polygon, the sum of that over an annotation's parts), sized on the host
// after the one read-back of the crossing counts; m_out holds the real lengths.  No atomics, no scratch.
#include "common.h"
#include "paste_bit.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

__device__ __forceinline__ int wave_scan_add_i(int v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}
// sum over the workgroup, the same value in every thread (s_red: kWaves ints; two barriers)
__device__ __forceinline__ int block_sum(int v, int *s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += s_red[w];
  return t;
}

struct Pt {
  int u, v;
};
// point d of the edge from vertex a to vertex b of the upsampled polygon (maskApi.c:147-157)
__device__ __forceinline__ Pt edge_point(int xa, int ya, int xb, int yb, int d) {
  int xs = xa, xe = xb, ys = ya, ye = yb;
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (flip) {
    int t = xs; xs = xe; xe = t;
    t = ys; ys = ye; ye = t;
  }
  Pt p;
  if (dx >= dy) {
    const int t = flip ? dx - d : d;
    p.u = t + xs;
    // dx == 0 (then dy == 0 too): a zero-length edge, s = 0 / 0 in the reference; its v is never read there and is not formed here
    p.v = dx == 0 ? ys : (int)(ys + ((double)(ye - ys) / dx) * t + .5);
  } else {
    const int t = flip ? dy - d : d;
    p.v = t + ys;
    p.u = (int)(xs + ((double)(xe - xs) / dy) * t + .5);
  }
  return p;
}

// cross_off == NULL: count pass (cross_count[p] = crossings below h * w); else fill pass (cross[cross_off[p] ..] in boundary order)
__global__ __launch_bounds__(kThreads) void poly_cross_kernel(const double *__restrict__ xy, const int32_t *__restrict__ poly_off,
                                                              const int32_t *__restrict__ edge_pt_off, const int32_t *__restrict__ poly_hw,
                                                              const int32_t *__restrict__ cross_off, int32_t *__restrict__ cross_count,
                                                              uint32_t *__restrict__ cross) {
  __shared__ int s_red[kWaves];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int v0 = poly_off[p], nv = poly_off[p + 1] - v0;
  const int h = poly_hw[2 * p], w = poly_hw[2 * p + 1];
  const unsigned hw = (unsigned)h * (unsigned)w;
  const int pt0 = nv > 0 ? edge_pt_off[v0] : 0, m = nv > 0 ? edge_pt_off[v0 + nv] - pt0 : 0;
  const double scale = 5;
  int carry = 0, mine = 0;
  for (int base = 1; base < m || base == 1; base += kThreads) {      // (at least one round: every thread reaches the barriers)
    const int j = base + tid;
    bool keep = false;
    unsigned val = 0;
    if (j < m) {
      Pt cur, prev;
      {
        int lo = 0, hi = nv;               // the edge that holds point j: the last e with edge_pt_off[v0 + e] - pt0 <= j
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (edge_pt_off[v0 + mid] - pt0 <= j) lo = mid; else hi = mid;
        }
        const int e = lo, e2 = e + 1 == nv ? 0 : e + 1;
        const int xa = (int)(scale * xy[2 * (size_t)(v0 + e)] + .5), ya = (int)(scale * xy[2 * (size_t)(v0 + e) + 1] + .5);
        const int xb = (int)(scale * xy[2 * (size_t)(v0 + e2)] + .5), yb = (int)(scale * xy[2 * (size_t)(v0 + e2) + 1] + .5);
        const int d = j - (edge_pt_off[v0 + e] - pt0);
        cur = edge_point(xa, ya, xb, yb, d);
        if (d > 0) {
          prev = edge_point(xa, ya, xb, yb, d - 1);
        } else {                           // the last point of the edge before (e >= 1 here: point 0 of edge 0 is j = 0).  Not simply
                                           // its end vertex: (int)(y + .5) of a negative y is y + 1
          const int xz = (int)(scale * xy[2 * (size_t)(v0 + e - 1)] + .5), yz = (int)(scale * xy[2 * (size_t)(v0 + e - 1) + 1] + .5);
          prev = edge_point(xz, yz, xa, ya, edge_pt_off[v0 + e] - edge_pt_off[v0 + e - 1] - 1);
        }
      }
      if (cur.u != prev.u) {
        double xd = (double)(cur.u < prev.u ? cur.u : cur.u - 1);
        xd = (xd + .5) / scale - .5;
        if (!(floor(xd) != xd || xd < 0 || xd > w - 1)) {
          double yd = (double)(cur.v < prev.v ? cur.v : prev.v);
          yd = (yd + .5) / scale - .5;
          if (yd < 0) yd = 0; else if (yd > h) yd = h;
          yd = ceil(yd);
          val = (unsigned)((int)xd * h + (int)yd);
          keep = val < hw;                 // a point at h * w shares the end with the sentinel: it is no run end
        }
      }
    }
    if (cross_off == nullptr) {
      mine += keep;
    } else {
      const int inc = wave_scan_add_i(keep ? 1 : 0, lane);
      __syncthreads();
      if (lane == kWave - 1) s_red[wave] = inc;
      __syncthreads();
      int before = carry, total = 0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) {
        if (k < wave) before += s_red[k];
        total += s_red[k];
      }
      if (keep) cross[(size_t)cross_off[p] + before + inc - 1] = val;
      carry += total;
    }
  }
  if (cross_off == nullptr) {
    const int total = block_sum(mine, s_red);
    if (tid == 0) cross_count[p] = total;
  }
}

// runs (slack pool, cross_off[p] + p onward: k_p + 1 slots) and m_out[p]; flag / bpos: workspaces as long as `cross`
__global__ __launch_bounds__(kThreads) void poly_runs_kernel(const uint32_t *__restrict__ cross, const int32_t *__restrict__ cross_off,
                                                             const int32_t *__restrict__ poly_hw, uint8_t *__restrict__ flag,
                                                             uint32_t *__restrict__ bpos, uint32_t *__restrict__ runs,
                                                             int32_t *__restrict__ m_out) {
  __shared__ int s_red[kWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int c0 = cross_off[p], k = cross_off[p + 1] - c0;
  const unsigned hw = (unsigned)poly_hw[2 * p] * (unsigned)poly_hw[2 * p + 1];
  const uint32_t *a = cross + c0;
  uint8_t *f = flag + c0;
  uint32_t *b = bpos + c0;
  int mine = 0;
  for (int i = tid; i < k; i += kThreads) {
    const unsigned v = a[i];
    int mult = 0, earlier = 0;
    for (int j = 0; j < k; ++j) {
      const bool same = a[j] == v;
      mult += same;
      earlier += same & (j < i);
    }
    const int run_end = earlier == 0 && (mult & 1);
    f[i] = (uint8_t)run_end;
    mine += run_end;
  }
  const int nb = block_sum(mine, s_red);   // (its barriers also publish f to the workgroup)
  for (int i = tid; i < k; i += kThreads) {
    if (!f[i]) continue;
    const unsigned v = a[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += (f[j] != 0) & (a[j] < v);
    b[rank] = v;
  }
  __syncthreads();
  uint32_t *out = runs + (size_t)c0 + p;
  for (int r = tid; r <= nb; r += kThreads) {
    const unsigned lo = r == 0 ? 0u : b[r - 1], hi = r == nb ? hw : b[r];
    out[r] = hi - lo;
  }
  if (tid == 0) m_out[p] = nb + 1;
}

// number of entries of the ascending list b[0 .. n) that are <= q
__device__ __forceinline__ int count_le(const uint32_t *__restrict__ b, int n, unsigned q) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] <= q) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// annotation a = polygons [ann_off[a], ann_off[a+1]); its counts go to out_runs at cross_off[first part] + first part + ... slack as for
// the parts together, m to ann_m[a].  bpos / m_out: what poly_runs_kernel left; uflag / upos: workspaces as long as `cross`.
__global__ __launch_bounds__(kThreads) void poly_union_kernel(const int32_t *__restrict__ ann_off, const int32_t *__restrict__ cross_off,
                                                              const int32_t *__restrict__ poly_hw, const uint32_t *__restrict__ runs,
                                                              const uint32_t *__restrict__ bpos, const int32_t *__restrict__ m_out,
                                                              uint8_t *__restrict__ uflag, uint32_t *__restrict__ upos,
                                                              uint32_t *__restrict__ out_runs, int32_t *__restrict__ ann_m) {
  __shared__ int s_red[kWaves];
  const int a = blockIdx.x, tid = threadIdx.x;
  const int p0 = ann_off[a], p1 = ann_off[a + 1];
  uint32_t *out = out_runs + (size_t)cross_off[p0] + p0;
  if (p1 - p0 == 1) {
    const int m = m_out[p0];
    const uint32_t *src = runs + (size_t)cross_off[p0] + p0;
    for (int r = tid; r < m; r += kThreads) out[r] = src[r];
    if (tid == 0) ann_m[a] = m;
    return;
  }
  if (p1 == p0) {                           // an annotation without polygons: no mask (the host refuses it; nothing is indexed)
    if (tid == 0) ann_m[a] = 0;
    return;
  }
  const unsigned hw = (unsigned)poly_hw[2 * p0] * (unsigned)poly_hw[2 * p0 + 1];
  const int c0 = cross_off[p0], n = cross_off[p1] - c0;      // candidate slots: part q's run ends are its first m_out[q] - 1
  uint8_t *f = uflag + c0;
  uint32_t *u = upos + c0;
  int mine = 0;
  for (int i = tid; i < n; i += kThreads) {
    int q = p0, hi = p1;                   // the part that owns slot i: the last q with cross_off[q] - c0 <= i
    while (hi - q > 1) {
      const int mid = (q + hi) >> 1;
      if (cross_off[mid] - c0 <= i) q = mid; else hi = mid;
    }
    const int idx = i - (cross_off[q] - c0);
    int is_end = 0;
    if (idx < m_out[q] - 1) {
      const unsigned v = bpos[cross_off[q] + idx];
      bool first = true, now = false, before = false;
      for (int r = p0; r < p1; ++r) {
        const uint32_t *b = bpos + cross_off[r];
        const int nb = m_out[r] - 1;
        const int le = count_le(b, nb, v);
        const bool has = le > 0 && b[le - 1] == v;
        if (r < q && has) first = false;
        now |= (le & 1) != 0;
        before |= ((has ? le - 1 : le) & 1) != 0;          // the parity one pixel earlier: without v itself
      }
      is_end = first && now != before;
    }
    f[i] = (uint8_t)is_end;
    mine += is_end;
  }
  const int nb = block_sum(mine, s_red);
  for (int i = tid; i < n; i += kThreads) {
    if (!f[i]) continue;
    int q = p0, hi = p1;
    while (hi - q > 1) {
      const int mid = (q + hi) >> 1;
      if (cross_off[mid] - c0 <= i) q = mid; else hi = mid;
    }
    const unsigned v = bpos[cross_off[q] + (i - (cross_off[q] - c0))];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      if (!f[j]) continue;
      int qj = p0, hj = p1;
      while (hj - qj > 1) {
        const int mid = (qj + hj) >> 1;
        if (cross_off[mid] - c0 <= j) qj = mid; else hj = mid;
      }
      rank += bpos[cross_off[qj] + (j - (cross_off[qj] - c0))] < v;
    }
    u[rank] = v;
  }
  __syncthreads();
  for (int r = tid; r <= nb; r += kThreads) {
    const unsigned lo = r == 0 ? 0u : u[r - 1], hi = r == nb ? hw : u[r];
    out[r] = hi - lo;
  }
  if (tid == 0) ann_m[a] = nb + 1;
}

// ---- the paste of mask probabilities (lib/mask/mask_voc2coco.py:39-49) -----------------------------------------------------
// Detection n: an (M, M) float32 mask resized to its box (bw = x2 - x1 + 1, bh = y2 - y1 + 1), thresholded, zeros outside the box, the
// whole (h, w) image run-length encoded column-major.  The resize and the threshold -- PasteBox, paste_box, paste_bit -- live in
// paste_bit.h, shared with the region overlap of voc_segm.hip and the mask overlay of render.hip.
// the value changes of box column c in column-major order: calls emit(position) for each, in ascending order.  A box of full image
// height is contiguous from one column to the next; otherwise a column starts after zeros and a set last bit is closed behind it
// (unless the image ends there).
template <typename F>
__device__ __forceinline__ int paste_column(const float *__restrict__ S, int M, const PasteBox &b, int c, float thr, F emit) {
  const bool full = b.y1 == 0 && b.bh == b.h;
  bool prev = full && c > 0 ? paste_bit(S, M, b, c - 1, b.bh - 1, thr) : false;
  const unsigned base = (unsigned)(b.x1 + c) * (unsigned)b.h + (unsigned)b.y1;
  int t = 0;
  for (int r = 0; r < b.bh; ++r) {
    const bool bit = paste_bit(S, M, b, c, r, thr);
    if (bit != prev) {
      emit(t, base + (unsigned)r);
      ++t;
    }
    prev = bit;
  }
  const unsigned after = base + (unsigned)b.bh;
  if (prev && !(full && c + 1 < b.bw) && after < (unsigned)b.h * (unsigned)b.w) {
    emit(t, after);
    ++t;
  }
  return t;
}

// a workgroup per detection: col_pre[col_off[n] + c] = value changes before column c, det_t[n] = their number
__global__ __launch_bounds__(kThreads) void paste_count_kernel(const float *__restrict__ masks, const int32_t *__restrict__ boxes,
                                                               const int32_t *__restrict__ hw, const int32_t *__restrict__ col_off, int M,
                                                               float thr, int32_t *__restrict__ col_pre, int32_t *__restrict__ det_t) {
  __shared__ int s_red[kWaves];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const PasteBox b = paste_box(boxes, hw, n, M);
  const float *S = masks + (size_t)n * M * M;
  const int c0 = col_off[n];
  int carry = 0;
  for (int base = 0; base < b.bw; base += kThreads) {
    const int c = base + tid;
    const int t = c < b.bw ? paste_column(S, M, b, c, thr, [](int, unsigned) {}) : 0;
    const int inc = wave_scan_add_i(t, lane);
    __syncthreads();
    if (lane == kWave - 1) s_red[wave] = inc;
    __syncthreads();
    int before = carry, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      if (k < wave) before += s_red[k];
      total += s_red[k];
    }
    if (c < b.bw) col_pre[c0 + c] = before + inc - t;
    carry += total;
  }
  if (tid == 0) det_t[n] = carry;
}

// a workgroup per detection: the positions of its value changes into tpos, then the counts between them (rle_off[n+1] - rle_off[n] =
// det_t[n] + 1 of them: from 0 to the first change -- 0 where the first pixel is set --, between changes, from the last to h * w)
__global__ __launch_bounds__(kThreads) void paste_fill_kernel(const float *__restrict__ masks, const int32_t *__restrict__ boxes,
                                                              const int32_t *__restrict__ hw, const int32_t *__restrict__ col_off,
                                                              const int32_t *__restrict__ col_pre, const int32_t *__restrict__ rle_off, int M,
                                                              float thr, uint32_t *__restrict__ tpos, uint32_t *__restrict__ cnts) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const PasteBox b = paste_box(boxes, hw, n, M);
  const float *S = masks + (size_t)n * M * M;
  const int c0 = col_off[n], o0 = rle_off[n], T = rle_off[n + 1] - o0 - 1;
  uint32_t *tp = tpos + o0;
  for (int c = tid; c < b.bw; c += kThreads) {
    const int at = col_pre[c0 + c];
    paste_column(S, M, b, c, thr, [&](int t, unsigned pos) {
      if (at + t < T) tp[at + t] = pos;          // (T is what the count pass found: never past the detection's slots)
    });
  }
  __syncthreads();
  const unsigned total = (unsigned)b.h * (unsigned)b.w;
  for (int r = tid; r <= T; r += kThreads) {
    const unsigned lo = r == 0 ? 0u : tp[r - 1], hi = r == T ? total : tp[r];
    cnts[(size_t)o0 + r] = hi - lo;
  }
}

}  // namespace

SN_EXPORT int sn_rle_poly_cross(const double *xy, const int32_t *poly_off, const int32_t *edge_pt_off, const int32_t *poly_hw,
                                const int32_t *cross_off, int NP, long total_vertices, long total_points, long max_hw,
                                int32_t *cross_count, uint32_t *cross, sn_stream_t stream) {
  SN_REQUIRE(xy && poly_off && edge_pt_off && poly_hw, "sn_rle_poly_cross: null pointer");
  SN_REQUIRE(cross_off ? cross != nullptr : cross_count != nullptr,
             "sn_rle_poly_cross: null pointer (the count pass writes cross_count, the fill pass -- cross_off given -- writes cross)");
  SN_REQUIRE(NP >= 1, "sn_rle_poly_cross: NP >= 1 required (NP = %d)", NP);
  SN_REQUIRE(total_vertices >= 0 && total_vertices < 2147483648L / 2 && total_points >= 0 && total_points < 2147483648L,
             "sn_rle_poly_cross: vertices and boundary points of a call must fit 32-bit indexing (total_vertices = %ld, total_points = %ld)",
             total_vertices, total_points);
  SN_REQUIRE(max_hw >= 1 && max_hw < 2147483648L, "sn_rle_poly_cross: 1 <= h * w < 2^31 required for every polygon (max_hw = %ld)", max_hw);
  hipLaunchKernelGGL(poly_cross_kernel, dim3(NP), dim3(kThreads), 0, sn_stream(stream), xy, poly_off, edge_pt_off, poly_hw, cross_off,
                     cross_count, cross);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT size_t sn_rle_from_polys_workspace_bytes(long total_cross) {
  if (total_cross < 0 || total_cross >= 2147483648L / 2) return 0;
  const size_t n = total_cross > 0 ? (size_t)total_cross : 1;
  return 2 * sn_align(n) + 2 * sn_align(n * sizeof(uint32_t));        // flag, uflag, bpos, upos
}

SN_EXPORT int sn_rle_from_polys(const uint32_t *cross, const int32_t *cross_off, const int32_t *poly_hw, const int32_t *ann_off, int NP,
                                int NA, long total_cross, void *ws, size_t ws_bytes, uint32_t *part_runs, int32_t *part_m,
                                uint32_t *runs, int32_t *ann_m, sn_stream_t stream) {
  SN_REQUIRE(cross && cross_off && poly_hw && ann_off && part_runs && part_m && runs && ann_m, "sn_rle_from_polys: null pointer");
  SN_REQUIRE(NP >= 1 && NA >= 1, "sn_rle_from_polys: NP >= 1 and NA >= 1 required (NP = %d, NA = %d)", NP, NA);
  SN_REQUIRE(total_cross >= 0 && total_cross < 2147483648L / 2 - NP,
             "sn_rle_from_polys: crossings plus polygons of a call must fit 32-bit indexing (total_cross = %ld, NP = %d)", total_cross, NP);
  const size_t need = sn_rle_from_polys_workspace_bytes(total_cross);
  SN_REQUIRE(ws && ws_bytes >= need, "sn_rle_from_polys: short workspace (%zu bytes, sn_rle_from_polys_workspace_bytes = %zu)",
             ws ? ws_bytes : (size_t)0, need);
  const size_t n = total_cross > 0 ? (size_t)total_cross : 1;
  char *b = (char *)ws;
  uint8_t *flag = (uint8_t *)b, *uflag = (uint8_t *)(b + sn_align(n));
  uint32_t *bpos = (uint32_t *)(b + 2 * sn_align(n)), *upos = (uint32_t *)(b + 2 * sn_align(n) + sn_align(n * sizeof(uint32_t)));
  hipStream_t s = sn_stream(stream);
  hipLaunchKernelGGL(poly_runs_kernel, dim3(NP), dim3(kThreads), 0, s, cross, cross_off, poly_hw, flag, bpos, part_runs, part_m);
  SN_CHECK_LAUNCH();
  hipLaunchKernelGGL(poly_union_kernel, dim3(NA), dim3(kThreads), 0, s, ann_off, cross_off, poly_hw, part_runs, bpos, part_m, uflag, upos,
                     runs, ann_m);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_rle_paste_count(const float *masks, const int32_t *boxes, const int32_t *hw, const int32_t *col_off, int n, int M,
                                 float binary_thresh, long total_cols, long max_hw, int32_t *col_pre, int32_t *det_t,
                                 sn_stream_t stream) {
  SN_REQUIRE(masks && boxes && hw && col_off && col_pre && det_t, "sn_rle_paste_count: null pointer");
  SN_REQUIRE(n >= 1, "sn_rle_paste_count: n >= 1 required (n = %d)", n);
  SN_REQUIRE(M >= 1 && M <= 1024 && (double)n * M * M < 2147483648., "sn_rle_paste_count: 1 <= M <= 1024 and n * M * M < 2^31 required (M = %d, n = %d)", M, n);
  SN_REQUIRE(total_cols >= 1 && total_cols < 2147483648L, "sn_rle_paste_count: the box columns of a call must fit 32-bit indexing (total_cols = %ld)", total_cols);
  SN_REQUIRE(max_hw >= 1 && max_hw < 2147483648L, "sn_rle_paste_count: 1 <= h * w < 2^31 required for every image (max_hw = %ld)", max_hw);
  hipLaunchKernelGGL(paste_count_kernel, dim3(n), dim3(kThreads), 0, sn_stream(stream), masks, boxes, hw, col_off, M, binary_thresh, col_pre, det_t);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_rle_paste(const float *masks, const int32_t *boxes, const int32_t *hw, const int32_t *col_off, const int32_t *col_pre,
                           const int32_t *rle_off, int n, int M, float binary_thresh, long total_cols, long total_runs, long max_hw,
                           uint32_t *tpos, uint32_t *cnts, sn_stream_t stream) {
  SN_REQUIRE(masks && boxes && hw && col_off && col_pre && rle_off && tpos && cnts, "sn_rle_paste: null pointer");
  SN_REQUIRE(n >= 1, "sn_rle_paste: n >= 1 required (n = %d)", n);
  SN_REQUIRE(M >= 1 && M <= 1024 && (double)n * M * M < 2147483648., "sn_rle_paste: 1 <= M <= 1024 and n * M * M < 2^31 required (M = %d, n = %d)", M, n);
  SN_REQUIRE(total_cols >= 1 && total_cols < 2147483648L, "sn_rle_paste: the box columns of a call must fit 32-bit indexing (total_cols = %ld)", total_cols);
  SN_REQUIRE(total_runs >= n && total_runs < 2147483648L / 2, "sn_rle_paste: n <= total_runs < 2^30 required (total_runs = %ld, n = %d)", total_runs, n);
  SN_REQUIRE(max_hw >= 1 && max_hw < 2147483648L, "sn_rle_paste: 1 <= h * w < 2^31 required for every image (max_hw = %ld)", max_hw);
  hipLaunchKernelGGL(paste_fill_kernel, dim3(n), dim3(kThreads), 0, sn_stream(stream), masks, boxes, hw, col_off, col_pre, rle_off, M, binary_thresh, tpos, cnts);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
