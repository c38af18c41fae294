"""The raster of sniper_amd/csrc/render.hip in plain numpy: the specification the GPU tests compare against
with np.array_equal.  The mask bits are tests/coco_segm_ref.paste's (the run-length encoding of the pasted detection, decoded).

An image's draw list is a dict: rects (n, 4) int x1, y1, x2, y2 inclusive; colors (n, 3) uint8; text: one int glyph-index array per item
(may be empty); mask_idx (n) int into masks (k, M, M) float32, -1 = none.  Layers per pixel, items in list order inside a layer:
  base     the source pixel
  mask     where the pasted mask is set:  p = (p * (256 - a) + c * a + 128) >> 8,  a = mask_alpha
  outline  inside rect and not inside rect shrunk by line_width on every side: the colour, opaque
  label    a box of len * gw + 2 by gh + 2 pixels, left edge x1, top y1 - (gh + 2) when that is >= 0, else y1 + line_width: the blend
           with a = 128; glyph k's cell starts one pixel inside, at x1 + 1 + k * gw; a glyph pixel blends toward white with
           a = cov + (cov >> 7)"""
import numpy as np

import coco_segm_ref as segm

COORD = 1 << 29


def blend(p, c, a):
    """p (..., 3) int64, c (3,), 0 <= a (scalar or array broadcast over the channels) <= 256"""
    a = np.asarray(a, np.int64)
    if a.ndim:
        a = a[..., None]
    return (p * (256 - a) + np.asarray(c, np.int64) * a + 128) >> 8


def from_tensor(x, means):
    """(3, h, w) float32 + means -> (h, w, 3) uint8: the sum in float32, truncated toward zero, clamped to 0 .. 255"""
    v = np.asarray(x, np.float32) + np.asarray(means, np.float32).reshape(3, 1, 1)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8).transpose(1, 2, 0)


def mask_bits(mask, rect, h, w, thr):
    """(h, w) bool: the detection pasted into its image, from the run-length encoding coco_segm_ref.paste returns"""
    cnts = segm.paste(mask, rect, h, w, thr)
    flat = np.repeat(np.arange(len(cnts)) & 1, cnts.astype(np.int64)).astype(bool)
    return flat.reshape(w, h).T


def label_rect(rect, n_glyphs, gh, gw, line_width):
    x1, y1 = int(rect[0]), int(rect[1])
    top = y1 - (gh + 2)
    return x1, (top if top >= 0 else y1 + line_width), n_glyphs * gw + 2, gh + 2


def render(image, items, atlas=None, mask_alpha=102, line_width=3, thr=0.4):
    """image (h, w, 3) uint8 -> the picture, (h, w, 3) uint8"""
    h, w = image.shape[:2]
    p = image.astype(np.int64)
    rects = np.clip(np.asarray(items['rects'], np.int64).reshape(-1, 4), -COORD, COORD)
    n = len(rects)
    colors = np.asarray(items['colors'], np.int64).reshape(-1, 3)
    mask_idx = np.asarray(items.get('mask_idx', -np.ones(n)), np.int64).reshape(-1)
    ys, xs = np.mgrid[0:h, 0:w]
    for k in range(n):
        if mask_idx[k] >= 0:
            bits = mask_bits(items['masks'][mask_idx[k]], rects[k], h, w, thr)
            p[bits] = blend(p[bits], colors[k], mask_alpha)
    for k in range(n):
        x1, y1, x2, y2 = rects[k]
        inside = (xs >= x1) & (xs <= x2) & (ys >= y1) & (ys <= y2)
        core = (xs >= x1 + line_width) & (xs <= x2 - line_width) & (ys >= y1 + line_width) & (ys <= y2 - line_width)
        p[inside & ~core] = colors[k]
    texts = items.get('text') if atlas is not None else None
    if texts is not None:
        G, gh, gw = atlas.shape
        for k in range(n):
            t = np.asarray(texts[k], np.int64).reshape(-1)
            if len(t) == 0:
                continue
            lx, ly, bw, bh = label_rect(rects[k], len(t), gh, gw, line_width)
            box = (xs >= lx) & (xs < lx + bw) & (ys >= ly) & (ys < ly + bh)
            p[box] = blend(p[box], colors[k], 128)
            strip = np.concatenate([atlas[g] for g in t], axis=1).astype(np.int64)          # (gh, len * gw)
            gx, gy = xs - lx - 1, ys - ly - 1
            on = (gx >= 0) & (gx < len(t) * gw) & (gy >= 0) & (gy < gh)
            cov = strip[gy[on], gx[on]]
            p[on] = blend(p[on], (255, 255, 255), cov + (cov >> 7))
    return p.astype(np.uint8)
