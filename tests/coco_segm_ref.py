"""A restatement of the reference's COCO mask evaluation in plain Python and numpy: the run-length arithmetic of
lib/dataset/pycocotools/maskApi.c (rleEncode :32-41, rleMerge :49-70, rleArea :72-75, rleIou :77-96, rleToBbox :111-124, rleFrPoly
:139-179, rleFrString :195-208) and COCOeval with useSegm = 1.  It depends neither on the kernels nor on the reference;
tests/golden/cocosegm_v1.npz (written from the reference itself) pins it on the bits, and it in turn is what the device is compared
with where no golden exists.  It walks like the reference does -- two pointers over the runs -- and deliberately not like the
kernels (no prefix sums, no binary search).

A mask is a numpy uint32 array of counts, column-major, zeros first.  Matching and accumulation are tests/coco_eval_ref.py's: its
evaluate_img asks the module-level bb_iou for the IoU of two rows, and `evaluate` below hands it rows that name the masks and a
bb_iou that looks their rle_iou up.  Layout of the results: coco_eval_ref.py's docstring.
"""
import math

import numpy as np

import coco_eval_ref as box_ref

Params = box_ref.Params
_bb_iou = box_ref.bb_iou          # the box IoU itself (evaluate() below swaps the module's name for the mask lookup while it runs)
U32 = 0xFFFFFFFF


def rle_from_string(s):
    """rleFrString: 6 bits per character from chr(48), 5 of them payload, bit 0x20 = more, bit 0x10 of the last = sign; from the
    third count on the value is a difference to the count two before"""
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & U32)
    return np.array(cnts, np.uint32)


def rle_encode(mask):
    """rleEncode of one (h,w) bitmap"""
    flat = np.asarray(mask, np.uint8).T.reshape(-1)
    cnts, p, c = [], 0, 0
    for v in flat:
        if v != p:
            cnts.append(c)
            c, p = 0, v
        c += 1
    cnts.append(c)
    return np.array(cnts, np.uint32)


def rle_area(cnts):
    return int(sum(int(c) for c in cnts[1::2])) & U32


def rle_to_bbox(cnts, h, w):
    """rleToBbox: run end points only, t = cc - j % 2 (unsigned), an odd last count dropped, an empty mask gives four zeros"""
    m = len(cnts) // 2 * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, ys, xe, ye, cc = w, h, 0, 0, 0
    for j in range(m):
        cc = (cc + int(cnts[j])) & U32
        t = (cc - j % 2) & U32
        y = t % h
        x = (t - y) // h
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [float(xs), float(ys), float((xe - xs + 1) & U32), float((ye - ys + 1) & U32)]


def rle_iou(d, g, hw, crowd):
    """rleIou of one pair of masks of the same image: 0 unless bbIou of the rleToBbox boxes is > 0, then the two-pointer walk"""
    h, w = int(hw[0]), int(hw[1])
    if not _bb_iou(rle_to_bbox(d, h, w), rle_to_bbox(g, h, w), crowd) > 0:
        return 0.0
    ca, cb, ka, kb = int(d[0]), int(g[0]), len(d), len(g)
    va = vb = False
    a = b = 1
    i = u = 0
    ct = 1
    while ct > 0:
        c = min(ca, cb)
        if va or vb:
            u += c
            if va and vb:
                i += c
        ct = 0
        ca -= c
        if not ca and a < ka:
            ca = int(d[a])
            a += 1
            va = not va
        ct += ca
        cb -= c
        if not cb and b < kb:
            cb = int(g[b])
            b += 1
            vb = not vb
        ct += cb
    if i == 0:
        u = 1
    elif crowd:
        u = rle_area(d)
    return float(i) / float(u)


def rle_merge(rles, h, w, intersect=False):
    """rleMerge (the reference's walk; intersect = False is the union of an annotation's parts)"""
    cnts = [int(c) for c in rles[0]]
    for B in rles[1:]:
        A = cnts
        B = [int(c) for c in B]
        ca, cb = A[0], B[0]
        v = va = vb = False
        cnts, a, b, cc, ct = [], 1, 1, 0, 1
        while ct > 0:
            c = min(ca, cb)
            cc += c
            ct = 0
            ca -= c
            if not ca and a < len(A):
                ca = A[a]
                a += 1
                va = not va
            ct += ca
            cb -= c
            if not cb and b < len(B):
                cb = B[b]
                b += 1
                vb = not vb
            ct += cb
            vp = v
            v = (va and vb) if intersect else (va or vb)
            if v != vp or ct == 0:
                cnts.append(cc)
                cc = 0
    return np.array(cnts, np.uint32)


def _cint(x):
    """the C cast (int) of a double: truncation toward zero"""
    return int(x)


def poly_crossings(xy, h, w):
    """the first half of rleFrPoly: the 5x upsampled boundary walk and the x-change filter -> the points x * h + y, in boundary order"""
    k = len(xy) // 2
    scale = 5.0
    x = [_cint(scale * xy[2 * j] + .5) for j in range(k)]
    y = [_cint(scale * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else float('nan')         # 0 / 0 in the reference: the only point of such an edge has t = 0 ...
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(ys if dx == 0 else _cint(ys + s * t + .5))      # ... and its v is never read (no x change next to it)
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(_cint(xs + s * t + .5))
    pts = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / scale - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / scale - .5
            yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
            yd = math.ceil(yd)
            pts.append((int(xd) * h + int(yd)) & U32)
    return pts


def rle_from_poly(xy, h, w):
    """rleFrPoly: the boundary walk and filter of poly_crossings, the sort with the sentinel h * w, the sequential compaction"""
    a = sorted(poly_crossings(xy, h, w) + [h * w])
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b, j = [a[0]], 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return np.array(b, np.uint32)


def rle_from_polys(polys, h, w):
    """an annotation's polygons -> one mask: rleFrPoly each, then rleMerge (union) when there are several (cocoeval.py:92-101)"""
    parts = [rle_from_poly(p, h, w) for p in polys]
    return parts[0] if len(parts) == 1 else rle_merge(parts, h, w)


def resize_linear_f32(S, bh, bw):
    """The resize of the paste, as this project specifies it (include/sniper_hip.h; the float32 INTER_LINEAR path of the algorithm
    oracle/cv_resize.py documents for uint8; NOT pinned to OpenCV).  Operation order, all in float32 unless said otherwise:
      scale = 1 / (b / M) in float64 per axis;  f = float32((d + 0.5) * scale - 0.5);  s = floor(f);  f = f - s
      x: s < 0 -> s = 0, f = 0;  s >= M - 1 -> the value is S[., M - 1];  else  H = S[., s] * (1 - f) + S[., s + 1] * f
      y: rows r0 = clip(s, 0, M - 1), r1 = clip(s + 1, 0, M - 1), the coefficient as it is:  D = H[r0] * (1 - g) + H[r1] * g
      both scales exactly 2: the area average (((a + b) + c) + d) * 0.25 of the 2 x 2 block, row-major"""
    S = np.asarray(S, np.float32)
    M = S.shape[0]
    one = np.float32(1)
    if 2 * bw == M and 2 * bh == M:
        return (((S[0::2, 0::2] + S[0::2, 1::2]) + S[1::2, 0::2]) + S[1::2, 1::2]) * np.float32(0.25)

    def table(n):
        scale = 1.0 / (np.float64(n) / np.float64(M))
        f = ((np.arange(n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        return s, (f - s.astype(np.float32)).astype(np.float32)
    sx, fx = table(bw)
    fx[sx < 0], sx[sx < 0] = 0, 0
    last = sx >= M - 1
    s0, s1 = np.where(last, M - 1, sx), np.minimum(np.where(last, M - 1, sx) + 1, M - 1)
    H = (S[:, s0] * (one - fx)[None, :] + S[:, s1] * fx[None, :]).astype(np.float32)
    H[:, last] = S[:, M - 1][:, None]
    sy, fy = table(bh)
    r0, r1 = np.clip(sy, 0, M - 1), np.clip(sy + 1, 0, M - 1)
    return (H[r0] * (one - fy)[:, None] + H[r1] * fy[:, None]).astype(np.float32)


def paste(mask, box, h, w, binary_thresh=0.4):
    """mask_voc2coco for one detection: the mask resized to its integer box x1, y1, x2, y2, >= float32(binary_thresh), zeros
    outside, rleEncode of the whole image"""
    x1, y1, x2, y2 = (int(v) for v in box)
    img = np.zeros((h, w), np.uint8)
    img[y1:y2 + 1, x1:x2 + 1] = resize_linear_f32(mask, y2 - y1 + 1, x2 - x1 + 1) >= np.float32(binary_thresh)
    return rle_encode(img)


def stats_rows(rles, hw, score=None):
    """(N,6) float64 rows x, y, w, h, score, area: what COCO.loadRes derives from a segmentation (pycocotools/coco.py:315-321)"""
    out = np.zeros((len(rles), 6))
    for n, r in enumerate(rles):
        out[n, :4] = rle_to_bbox(r, int(hw[n][0]), int(hw[n][1]))
        out[n, 4] = 0.0 if score is None else float(score[n])
        out[n, 5] = float(rle_area(r))
    return out


def pair_iou(gt, dt, d, g, cache=None):
    """rle_iou of detection d and annotation g (indices into the sets); `cache` (a dict) keeps the value for a second evaluation
    of the same set with other parameters"""
    if cache is None:
        return rle_iou(dt['rle'][d], gt['rle'][g], dt['hw'][d], int(gt['iscrowd'][g]))
    if (d, g) not in cache:
        cache[d, g] = rle_iou(dt['rle'][d], gt['rle'][g], dt['hw'][d], int(gt['iscrowd'][g]))
    return cache[d, g]


def iou_matrices(gt, dt, K, cache=None):
    """-> (iou pool, iou_off (P+1)): every problem's D x G matrix, detection-major in arrival order, problems category-major"""
    parts, off = [], [0]
    for _, _, gi, di in box_ref.group(gt, dt, K):
        m = np.array([[pair_iou(gt, dt, d, g, cache) for g in gi] for d in di], np.float64)
        parts.append(m.reshape(-1))
        off.append(off[-1] + len(di) * len(gi))
    return (np.concatenate(parts) if parts else np.zeros(0)), np.array(off, np.int32)


def evaluate(gt, dt, K, params=None, defect=None, cache=None):
    """the per-image evaluation of coco_eval_ref.evaluate with the IoU of masks; the detection's area is its rleArea"""
    gt_rows = dict(gt, bbox=np.array([[n, 0, 0, 0] for n in range(len(gt['image']))], np.float64).reshape(-1, 4))
    dt_rows = dict(dt, bbox=np.array([[n, 0, 0, 0] for n in range(len(dt['image']))], np.float64).reshape(-1, 4),
                   area=np.array([rle_area(r) for r in dt['rle']], np.float64))
    lookup = lambda d, g, crowd: pair_iou(gt, dt, int(d[0]), int(g[0]), cache)
    keep = box_ref.bb_iou
    box_ref.bb_iou = lookup
    try:
        return box_ref.evaluate(gt_rows, dt_rows, K, params, defect)
    finally:
        box_ref.bb_iou = keep


def run(gt, dt, K, params=None, summary=True, cache=None):
    """everything: the flat per-image arrays, the IoU matrices, precision, recall and (for the default parameter shapes) stats"""
    params = params or Params()
    ev = evaluate(gt, dt, K, params, cache=cache)
    ev['iou'], ev['iou_off'] = iou_matrices(gt, dt, K, cache)
    ev['precision'], ev['recall'] = box_ref.accumulate(ev, K, params)
    if summary:
        ev['stats'], ev['summary'] = box_ref.summarize(ev['precision'], ev['recall'], params)
    return ev
