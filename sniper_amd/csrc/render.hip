// render.hip -- detections drawn into images on the device: boxes, labels and mask overlays (the raster is this
// project's, in integer arithmetic: lib/data_utils/visualization.py:21-57 draws with matplotlib, whose anti-aliasing pins nothing).
// One launch renders a batch.  The grid is tiles x images, a tile is kTileW x kTileH pixels, a workgroup of kThreads threads owns one:
// lane = column, and each of the kWaves waves owns kRows whole rows, so a wave writes runs of 3 * kTileW contiguous bytes.
//
// Layers per pixel, in this order, items in list order inside a layer:
//   base     the source pixel (uint8 RGB, or the network input: trunc(x + mean) clamped to 0 .. 255)
//   mask     where paste_bit holds (paste_bit.h: the bits of sn_rle_paste): p = (p * (256 - a) + c * a + 128) >> 8, a = mask_alpha
//   outline  inside rect and not inside rect shrunk by line_width: the item's colour, opaque, the last item wins
//   label    a box of len * gw + 2 by gh + 2 pixels at (x1, y1 - (gh + 2)), or at (x1, y1 + line_width) when that top would be
//            negative: the blend with a = 128 toward the item's colour, then every glyph pixel toward white with a = cov + (cov >> 7)
// A later layer reads what the earlier one left, so the walk over an image's items is made twice: masks and outlines (the outline is
// kept beside the pixel, as "colour of the last item that covers it"), then labels.
//
// Culling: a workgroup walks its image's items kRound at a time, a wave 64 of them; an item whose rect and label rect both miss the
// tile -- or, without a mask, whose outline does: a tile inside the shrunk rect -- is dropped, the others are compacted IN ORDER into an
// LDS list of 32-byte entries (wave ballot, prefix popcount, the waves' counts summed in wave order).  The pixels loop over that list
// only and read an item from LDS, never from the tables; an image of at most kRound items is culled once for both walks.  No atomics, no
// scratch, no host read-back; the same bits every run.
#include "common.h"
#include "paste_bit.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTileW = kWave, kTileH = 16, kThreads = 256, kWaves = kThreads / kWave, kRows = kTileH / kWaves, kRound = 256;
constexpr int kMaxItems = SN_RENDER_MAX_ITEMS;
constexpr int kCoord = 1 << 29;          // rect coordinates are clamped to +-2^29: every sum below stays inside int32
enum { kRects, kColors, kMaskIdx, kTextOff, kText, kAtlas, kMasks, kPtrs };
static_assert(kRound == kThreads, "a culling round is one item per thread");

struct RenderArgs {
  const void *src;
  const int32_t *hw;
  const int64_t *pix_off;
  const int32_t *item_off, *rects, *mask_idx, *text_off, *text;
  const uint8_t *colors, *atlas;
  const float *masks;
  uint8_t *out;
  int G, gh, gw, n_masks, M, mask_alpha, line_width;
  float thr, mean[3];
};

__device__ __forceinline__ int clampc(int v) { return v < -kCoord ? -kCoord : (v > kCoord ? kCoord : v); }
// p, c: 0x00BBGGRR packed; every channel (p * (256 - a) + c * a + 128) >> 8, 0 <= a <= 256
__device__ __forceinline__ unsigned blend(unsigned p, unsigned c, int a) {
  unsigned out = 0;
#pragma unroll
  for (int s = 0; s < 24; s += 8) {
    const unsigned pv = (p >> s) & 255u, cv = (c >> s) & 255u;
    out |= ((pv * (unsigned)(256 - a) + cv * (unsigned)a + 128u) >> 8) << s;
  }
  return out;
}

// one survivor of the culling in LDS: what the pixel loops read of an item (32 bytes; the tables stay in global memory)
struct Entry {
  int x1, y1, x2, y2;
  unsigned c;                            // 0x00BBGGRR
  int m, t0, len;                        // mask row or -1; the text's first glyph and its length (0: no label)
};
struct Label {
  int x, y, bw, bh;
};
__device__ __forceinline__ Label label_of(const RenderArgs &a, int x1, int y1, int len) {
  Label l;
  l.bw = len * a.gw + 2;
  l.bh = a.gh + 2;
  l.x = x1;
  l.y = y1 - l.bh >= 0 ? y1 - l.bh : y1 + a.line_width;
  return l;
}

template <bool TENSOR>
__global__ __launch_bounds__(kThreads) void render_kernel(const RenderArgs a) {
  __shared__ Entry s_list[kRound];
  __shared__ int s_cnt[kWaves];
  __shared__ const void *s_ptr[kPtrs];          // the tables' addresses: read where they are used, not held in scalar registers throughout
  const int img = blockIdx.z;
  const int h = a.hw[2 * img], w = a.hw[2 * img + 1];
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  if (tx0 >= w || ty0 >= h) return;                          // (the whole workgroup: the grid covers the largest image)
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tx1 = min(tx0 + kTileW, w) - 1, ty1 = min(ty0 + kTileH, h) - 1;
  const int x = tx0 + lane, yb = ty0 + wave * kRows, ye = min(yb + kRows, h) - 1;          // this wave's rows yb .. ye (none: ye < yb)
  const size_t base = (size_t)a.pix_off[img];
  const size_t plane = (size_t)h * (size_t)w;

  unsigned p[kRows], o[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    p[r] = 0;
    o[r] = 0;
    const int y = yb + r;
    if (x < w && y < h) {
      const size_t at = (size_t)y * w + x;
      if (TENSOR) {
        const float *s = (const float *)a.src + 3 * base + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = s[c * plane] + a.mean[c];
          const unsigned q = v >= 255.f ? 255u : (v >= 1.f ? (unsigned)(int)v : 0u);          // (a NaN: 0)
          p[r] |= q << (8 * c);
        }
      } else {
        const uint8_t *s = (const uint8_t *)a.src + 3 * (base + at);
        p[r] = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16);
      }
    }
  }

  if (tid == 0) {
    s_ptr[kRects] = a.rects; s_ptr[kColors] = a.colors; s_ptr[kMaskIdx] = a.mask_idx; s_ptr[kTextOff] = a.text_off;
    s_ptr[kText] = a.text; s_ptr[kAtlas] = a.atlas; s_ptr[kMasks] = a.masks;
  }
  __syncthreads();
  const int i0 = a.item_off[img];
  int n = a.item_off[img + 1] - i0;
  n = n < 0 || !a.rects ? 0 : (n > kMaxItems ? kMaxItems : n);          // (no item tables: nothing is read through them)
  const int nrounds = (n + kRound - 1) / kRound;
  int cnt = 0;
#pragma unroll
  for (int phase = 0; phase < 2; ++phase) {
    for (int round = 0; round < nrounds; ++round) {
      if (phase == 0 || nrounds > 1) {
        const int k = round * kRound + tid;
        bool hit = false;
        Entry en;
        if (k < n) {
          const int it = i0 + k;
          const int32_t *rect = (const int32_t *)s_ptr[kRects] + 4 * (size_t)it, *toff = (const int32_t *)s_ptr[kTextOff] + it;
          const uint8_t *col = (const uint8_t *)s_ptr[kColors] + 3 * (size_t)it;
          en.x1 = clampc(rect[0]);
          en.y1 = clampc(rect[1]);
          en.x2 = clampc(rect[2]);
          en.y2 = clampc(rect[3]);
          en.c = (unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16);
          en.m = ((const int32_t *)s_ptr[kMaskIdx])[it];
          if (en.m >= a.n_masks) en.m = -1;                    // (n_masks is 0 without masks)
          en.t0 = toff[0];
          en.len = a.G > 0 ? toff[1] - en.t0 : 0;              // (G is 0 without glyphs)
          if (en.len < 0) en.len = 0;
          const int lw = a.line_width;
          hit = en.x1 <= tx1 && en.x2 >= tx0 && en.y1 <= ty1 && en.y2 >= ty0;
          // without a mask only the outline draws: a tile wholly inside the rect shrunk by line_width sees nothing of it
          if (en.m < 0 && tx0 >= en.x1 + lw && tx1 <= en.x2 - lw && ty0 >= en.y1 + lw && ty1 <= en.y2 - lw) hit = false;
          const Label l = label_of(a, en.x1, en.y1, en.len);
          hit |= en.len > 0 && l.x <= tx1 && l.x + l.bw - 1 >= tx0 && l.y <= ty1 && l.y + l.bh - 1 >= ty0;
        }
        const unsigned long long b = __ballot(hit);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();                                       // (the list of the round before has been read by every wave)
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int off = 0;
        cnt = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
          if (q < wave) off += s_cnt[q];
          cnt += s_cnt[q];
        }
        if (hit) s_list[off + before] = en;
        __syncthreads();
      }
      for (int e = 0; e < cnt; ++e) {
        const Entry en = s_list[e];
        const int x1 = en.x1, y1 = en.y1, x2 = en.x2, y2 = en.y2;
        const unsigned c = en.c;
        if (phase == 0) {
          if (y1 > ye || y2 < yb) continue;                     // (wave-uniform: none of this wave's rows)
          const bool in_x = x >= x1 && x <= x2;
          const int m = en.m, lw = a.line_width;
          // (wave-uniform too: these rows of the tile lie wholly inside the shrunk rect of an item without a mask)
          if (m < 0 && tx0 >= x1 + lw && tx1 <= x2 - lw && yb >= y1 + lw && ye <= y2 - lw) continue;
          if (m >= 0) {
            const int32_t box[4] = {x1, y1, x2, y2}, ihw[2] = {h, w};
            const PasteBox pb = paste_box(box, ihw, 0, a.M);
            const float *S = (const float *)s_ptr[kMasks] + (size_t)m * a.M * a.M;
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
              const int y = yb + r;
              if (in_x && x < w && y >= y1 && y <= y2 && y <= ye && paste_bit(S, a.M, pb, x - x1, y - y1, a.thr)) p[r] = blend(p[r], c, a.mask_alpha);
            }
          }
          const bool core_x = x >= x1 + lw && x <= x2 - lw;
#pragma unroll
          for (int r = 0; r < kRows; ++r) {
            const int y = yb + r;
            const bool inside = in_x && y >= y1 && y <= y2, core = core_x && y >= y1 + lw && y <= y2 - lw;
            if (inside && !core) o[r] = c | 0x1000000u;
          }
        } else {
          if (en.len == 0) continue;
          const Label l = label_of(a, x1, y1, en.len);
          if (l.y > ye || l.y + l.bh - 1 < yb) continue;
          if (x < l.x || x > l.x + l.bw - 1) continue;         // (per lane: nothing below synchronises)
          const int gx = x - l.x - 1;
          const bool in_gx = gx >= 0 && gx < en.len * a.gw;
          int g = -1, cx = 0;
          if (in_gx) {
            const int q = gx / a.gw;
            cx = gx - q * a.gw;
            g = ((const int32_t *)s_ptr[kText])[en.t0 + q];
          }
          const bool glyph = g >= 0 && g < a.G;
#pragma unroll
          for (int r = 0; r < kRows; ++r) {
            const int y = yb + r, gy = y - l.y - 1;
            if (y < l.y || y > l.y + l.bh - 1) continue;
            p[r] = blend(p[r], c, 128);
            if (glyph && gy >= 0 && gy < a.gh) {
              const int cov = ((const uint8_t *)s_ptr[kAtlas])[((size_t)g * a.gh + gy) * a.gw + cx];
              p[r] = blend(p[r], 0xFFFFFFu, cov + (cov >> 7));
            }
          }
        }
      }
    }
    if (phase == 0) {
#pragma unroll
      for (int r = 0; r < kRows; ++r)
        if (o[r] >> 24) p[r] = o[r] & 0xFFFFFFu;
    }
  }

#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = yb + r;
    if (x < w && y < h) {
      uint8_t *d = a.out + 3 * (base + (size_t)y * w + x);
      d[0] = (uint8_t)(p[r] & 255u);
      d[1] = (uint8_t)((p[r] >> 8) & 255u);
      d[2] = (uint8_t)((p[r] >> 16) & 255u);
    }
  }
}

}  // namespace

SN_EXPORT int sn_render_limits(int32_t *h_out5) {
  SN_REQUIRE(h_out5, "sn_render_limits: null pointer");
  const int v[5] = {kMaxItems, kTileW, kTileH, kRound, kThreads};
  for (int i = 0; i < 5; ++i) h_out5[i] = v[i];
  return SN_OK;
}

SN_EXPORT int sn_render_dets(int form, const void *src, const int32_t *hw, const int64_t *pix_off, int I, int max_h, int max_w,
                             long total_pixels, const int32_t *item_off, int max_items, long total_items, const int32_t *rects,
                             const uint8_t *colors, const int32_t *mask_idx, const int32_t *text_off, const int32_t *text,
                             const int32_t *h_text, long total_text, const uint8_t *atlas, int G, int gh, int gw, const float *masks,
                             int n_masks, int M, float binary_thresh, int mask_alpha, int line_width, float mean0, float mean1,
                             float mean2, uint8_t *out, sn_stream_t stream) {
  SN_REQUIRE(form == SN_RENDER_UINT8 || form == SN_RENDER_TENSOR, "sn_render_dets: form is SN_RENDER_UINT8 (0) or SN_RENDER_TENSOR (1) (form = %d)", form);
  SN_REQUIRE(src && hw && pix_off && item_off && out, "sn_render_dets: null pointer (src, hw, pix_off, item_off and out are always needed)");
  SN_REQUIRE(I >= 1 && I <= 65535, "sn_render_dets: 1 <= I <= 65535 required (I = %d)", I);
  SN_REQUIRE(max_h >= 1 && max_w >= 1 && (long)max_h * max_w < 2147483648L && max_h <= 65535 * kTileH,
             "sn_render_dets: every image needs h >= 1, w >= 1, h * w < 2^31 and h <= %d (max_h = %d, max_w = %d)", 65535 * kTileH, max_h, max_w);
  SN_REQUIRE(total_pixels >= I && total_pixels < (1L << 40), "sn_render_dets: I <= total_pixels < 2^40 required (total_pixels = %ld, I = %d)", total_pixels, I);
  SN_REQUIRE(max_items >= 0 && max_items <= kMaxItems, "sn_render_dets: an image has %d items, at most %d are drawn (SN_RENDER_MAX_ITEMS)", max_items, kMaxItems);
  SN_REQUIRE(total_items >= 0 && total_items < 2147483648L / 4 && total_items <= (long)I * kMaxItems,
             "sn_render_dets: the items of a call must fit 32-bit indexing, 0 <= total_items < 2^29 required (total_items = %ld)", total_items);
  SN_REQUIRE(total_items == 0 || (rects && colors && mask_idx && text_off), "sn_render_dets: null pointer (rects, colors, mask_idx and text_off are needed when there are items)");
  SN_REQUIRE(mask_alpha >= 0 && mask_alpha <= 256, "sn_render_dets: 0 <= mask_alpha <= 256 required (mask_alpha = %d)", mask_alpha);
  SN_REQUIRE(line_width >= 1 && line_width <= 65536, "sn_render_dets: 1 <= line_width <= 65536 required (line_width = %d)", line_width);
  SN_REQUIRE(total_text >= 0 && total_text < 2147483648L / 512, "sn_render_dets: the glyphs of a call must fit 32-bit indexing, 0 <= total_text < 2^22 required (total_text = %ld)", total_text);
  if (total_text > 0) {
    SN_REQUIRE(text && atlas, "sn_render_dets: null pointer (text and atlas are needed when there are glyphs)");
    SN_REQUIRE(G >= 1 && gh >= 1 && gw >= 1 && gh <= 256 && gw <= 256 && (long)G * gh * gw < 2147483648L,
               "sn_render_dets: an atlas of G >= 1 glyphs of 1 .. 256 by 1 .. 256 pixels required (G = %d, gh = %d, gw = %d)", G, gh, gw);
    if (h_text)
      for (long t = 0; t < total_text; ++t)
        SN_REQUIRE(h_text[t] >= 0 && h_text[t] < G, "sn_render_dets: glyph index %d at position %ld of text is outside [0, G = %d)", h_text[t], t, G);
  }
  SN_REQUIRE(n_masks >= 0, "sn_render_dets: n_masks >= 0 required (n_masks = %d)", n_masks);
  if (n_masks > 0) {
    SN_REQUIRE(masks, "sn_render_dets: null pointer (masks are needed when n_masks > 0)");
    SN_REQUIRE(M >= 1 && M <= 1024 && (double)n_masks * M * M < 2147483648., "sn_render_dets: 1 <= M <= 1024 and n_masks * M * M < 2^31 required (M = %d, n_masks = %d)", M, n_masks);
  }
  RenderArgs a;
  a.src = src; a.hw = hw; a.pix_off = pix_off; a.item_off = item_off; a.rects = rects; a.mask_idx = mask_idx; a.text_off = text_off;
  a.text = total_text > 0 ? text : nullptr; a.colors = colors; a.atlas = total_text > 0 ? atlas : nullptr; a.masks = n_masks > 0 ? masks : nullptr;
  a.out = out; a.G = total_text > 0 ? G : 0; a.gh = total_text > 0 ? gh : 1; a.gw = total_text > 0 ? gw : 1; a.n_masks = n_masks; a.M = n_masks > 0 ? M : 1;
  a.mask_alpha = mask_alpha; a.line_width = line_width; a.thr = binary_thresh; a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  const dim3 grid(sn_div_up(max_w, kTileW), sn_div_up(max_h, kTileH), I);
  if (form == SN_RENDER_TENSOR)
    hipLaunchKernelGGL(render_kernel<true>, grid, dim3(kThreads), 0, sn_stream(stream), a);
  else
    hipLaunchKernelGGL(render_kernel<false>, grid, dim3(kThreads), 0, sn_stream(stream), a);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
