"""Detections drawn into images on the device: boxes, labels and mask overlays (lib/data_utils/visualization.py:21-57, which pays a
matplotlib figure per image).  The raster is this project's, in integer arithmetic (restated in numpy by
tests/render_ref.py); one launch of sn_render_dets (csrc/render.hip) draws a batch.  The host's share is the draw list -- which rows
pass the threshold, their rounded boxes, colours and label strings -- and the file encoding (PIL, as data/im_worker.py reads images).

Where this departs from the reference, on purpose: the colours are a fixed palette (class_colors; the reference draws
random.random() per class and run), the blends are integer, the network-input form clamps where numpy's astype(uint8) wraps, and file
names carry no wall clock."""
import os
import warnings

import numpy as np

__all__ = ['visualize_dets', 'render_batch', 'render_lists', 'render_results', 'draw_list', 'class_colors', 'default_atlas', 'encode_text']

MASK_ALPHA = 102            # 0.4 of 256, rounded
LINE_WIDTH = 3
COORD = 1 << 29             # rect coordinates are clamped to +-2^29 (the kernel does the same)


def class_colors(n):
    """(n, 3) uint8 RGB, one colour per class index: the PASCAL VOC colour map -- bit 3q + c of the index (q = 0 .. 7) becomes bit 7 - q of
    channel c.  A bijection of the low 24 bits, so any two indices below 2^24 differ; index 0 (the background, never drawn) is black and
    white would need the index 2^24 - 1.  The same colours every run."""
    k = np.arange(int(n), dtype=np.int64)
    out = np.zeros((int(n), 3), np.int64)
    for q in range(8):
        for c in range(3):
            out[:, c] |= ((k >> (3 * q + c)) & 1) << (7 - q)
    return out.astype(np.uint8)


_ATLAS = []


def default_atlas():
    """(95, gh, gw) uint8 coverage of ASCII 32 .. 126 in equal cells, rendered once per process with PIL's ImageFont.load_default();
    None, after one warning, where PIL or its font is missing (labels are then dropped, boxes and masks are still drawn)."""
    if not _ATLAS:
        try:
            from PIL import Image, ImageDraw, ImageFont
            font = ImageFont.load_default()
            chars = [chr(c) for c in range(32, 127)]
            boxes = [font.getbbox(c) for c in chars]
            gw = max(1, max(int(b[2]) for b in boxes))
            gh = max(1, max(int(b[3]) for b in boxes))
            atlas = np.zeros((len(chars), gh, gw), np.uint8)
            for g, c in enumerate(chars):
                im = Image.new('L', (gw, gh), 0)
                ImageDraw.Draw(im).text((0, 0), c, fill=255, font=font)
                atlas[g] = np.asarray(im)
            _ATLAS.append(atlas)
        except Exception as e:          # noqa: BLE001 (no PIL, no FreeType, no bundled font: all mean "no labels")
            warnings.warn('sniper_amd.visualization: no label font (%s: %s); boxes and masks are drawn without labels' % (type(e).__name__, e))
            _ATLAS.append(None)
    return _ATLAS[0]


def encode_text(label, G=95):
    """a label string -> int32 glyph indices of the default atlas' order (ASCII 32 .. 126); any other character becomes '?'"""
    q = ord('?') - 32
    idx = [ord(c) - 32 if 32 <= ord(c) <= 126 else q for c in label]
    return np.array([i if i < G else 0 for i in idx], np.int32)


def draw_list(dets, scale, class_names, threshold=0.5, masks=None, hw=None):
    """The items visualize_dets draws, in its order: classes ascending from index 1, the rows of dets[j] in order, a row kept when
    score >= threshold (the reference skips score < threshold).  bbox = det[:4] * scale in float32 (numpy's result for a float32 row and a
    Python float), rounded half to even in float64, clamped to +-2^29, int32.  The label is '{:s} {:.1f}'.format(name, score).
    masks[j] (n, M, M) aligned with dets[j]: the item's rect is then evaluation.paste_boxes of the scaled box in its (h, w) = hw image
    -- clipped and rounded as the results files do -- and must satisfy the paste's precondition 0 <= x1 <= x2 < w (likewise y);
    ValueError otherwise.
    -> dict: rects (n, 4) int32, colors (n, 3) uint8, labels [str], mask_idx (n) int32 into masks (k, M, M) float32 or None."""
    palette = class_colors(max(len(class_names), 1))
    rects, colors, labels, mask_idx, kept = [], [], [], [], []
    for j in range(1, min(len(class_names), len(dets))):
        rows = np.asarray(dets[j], np.float32).reshape(-1, 5) if len(dets[j]) else np.zeros((0, 5), np.float32)
        mj = None
        if masks is not None and j < len(masks) and masks[j] is not None and len(masks[j]):
            mj = np.asarray(masks[j], np.float32)
            if mj.ndim != 3 or mj.shape[0] != len(rows) or mj.shape[1] != mj.shape[2]:
                raise ValueError('draw_list: masks[%d] is %s, dets[%d] has %d rows: (n, M, M) aligned with the rows required' % (j, mj.shape, j, len(rows)))
        for r, det in enumerate(rows):
            score = det[-1]
            if not score >= threshold:
                continue
            bbox = det[:4] * scale
            if mj is None:
                rect = np.clip(np.rint(bbox.astype(np.float64)), -COORD, COORD).astype(np.int32)
            else:
                if hw is None:
                    raise ValueError('draw_list: masks need the image size hw')
                from .evaluation import paste_boxes
                h, w = int(hw[0]), int(hw[1])
                rect = paste_boxes(bbox[None], h, w, what='draw_list: class %d row %d' % (j, r))[0].astype(np.int32)
                if not (0 <= rect[0] <= rect[2] < w and 0 <= rect[1] <= rect[3] < h):
                    raise ValueError('draw_list: class %d row %d has the mask box %s outside its %d x %d image' % (j, r, rect.tolist(), h, w))
                mask_idx.append(len(kept))
                kept.append(mj[r])
            if mj is None:
                mask_idx.append(-1)
            rects.append(rect)
            colors.append(palette[j])
            labels.append('{:s} {:.1f}'.format(class_names[j], score))
    Ms = set(m.shape[0] for m in kept)
    if len(Ms) > 1:
        raise ValueError('draw_list: masks of sizes %s in one image, one size per call' % sorted(Ms))
    return {'rects': np.array(rects, np.int32).reshape(-1, 4), 'colors': np.array(colors, np.uint8).reshape(-1, 3), 'labels': labels,
            'mask_idx': np.array(mask_idx, np.int32), 'masks': np.stack(kept) if kept else None}


def _limits():
    import ctypes
    from . import hip
    out = (ctypes.c_int32 * 5)()
    hip.lib().call('sn_render_limits', out)
    return dict(zip(('max_items', 'tile_w', 'tile_h', 'round', 'threads'), (int(v) for v in out)))


def render_lists(source, lists, atlas='default', means=None, mask_alpha=MASK_ALPHA, line_width=LINE_WIDTH, binary_thresh=0.4, timing=None,
                 repeat=1):
    """One sn_render_dets call: `source` is a list of (h, w, 3) uint8 RGB images (numpy arrays or device tensors, sizes may differ) or
    one (B, 3, Hm, Wm) float32 network input (numpy or device tensor; `means` = the three values added back, in its channel order).
    lists[i]: a draw_list dict -- rects, colors, mask_idx, masks, and either `text` (one int32 glyph-index array per item) or `labels`
    (strings, encoded for the default atlas).  atlas: 'default', a (G, gh, gw) uint8 array, or None (no labels).
    -> one (h, w, 3) uint8 array per image: device tensors when the source was on the device, numpy arrays otherwise.
    timing: a dict that receives pack_s, upload_s, kernel_s (of `repeat` launches) and download_s, each closed by a synchronise
    (tools/render_bench.py)."""
    import time
    import torch
    from . import hip
    dev = hip.require_gpu()
    t0 = time.perf_counter()
    if isinstance(atlas, str):
        atlas = default_atlas()
    tensor_form = not isinstance(source, (list, tuple))
    if tensor_form:
        on_device = isinstance(source, torch.Tensor) and source.is_cuda
        if len(source.shape) != 4 or source.shape[1] != 3:
            raise ValueError('render_lists: the tensor form is (B, 3, Hm, Wm), got %s' % (tuple(source.shape),))
        I = int(source.shape[0])
        hw = np.tile(np.array([[source.shape[2], source.shape[3]]], np.int64), (I, 1))
        m3 = [float(np.float32(v)) for v in (means if means is not None else (0, 0, 0))]
    else:
        I = len(source)
        on_device = I > 0 and all(isinstance(s, torch.Tensor) and s.is_cuda for s in source)
        for s in source:
            if tuple(s.shape[2:]) != (3,) or len(s.shape) != 3 or not str(s.dtype).endswith('uint8'):
                raise ValueError('render_lists: the uint8 form takes (h, w, 3) uint8 images, got %s %s' % (tuple(s.shape), s.dtype))
        hw = np.array([[s.shape[0], s.shape[1]] for s in source], np.int64).reshape(-1, 2)
        m3 = [0.0, 0.0, 0.0]
    if I < 1 or len(lists) != I:
        raise ValueError('render_lists: %d images and %d draw lists' % (I, len(lists)))
    if hw.min() < 1:
        raise ValueError('render_lists: an empty image')
    pix_off = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])]).astype(np.int64)
    counts = [len(l['rects']) for l in lists]
    cap = _limits()['max_items']
    if max(counts) > cap:
        raise ValueError('render_lists: image %d has %d items, at most %d are drawn (SN_RENDER_MAX_ITEMS)' % (int(np.argmax(counts)), max(counts), cap))
    item_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(item_off[-1])
    rects = np.concatenate([np.asarray(l['rects'], np.int32).reshape(-1, 4) for l in lists]) if total else np.zeros((0, 4), np.int32)
    colors = np.concatenate([np.asarray(l['colors'], np.uint8).reshape(-1, 3) for l in lists]) if total else np.zeros((0, 3), np.uint8)
    G = gh = gw = 0
    texts = []
    if atlas is not None:
        atlas = np.ascontiguousarray(atlas, np.uint8)
        G, gh, gw = atlas.shape
    for l in lists:
        if atlas is None:
            texts.extend(np.zeros(0, np.int32) for _ in range(len(l['rects'])))
        elif l.get('text') is not None:
            texts.extend(np.asarray(t, np.int32).reshape(-1) for t in l['text'])
        else:
            texts.extend(encode_text(s, G) for s in l.get('labels') or [''] * len(l['rects']))
    assert len(texts) == total, 'one text per item'
    text_off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int32)
    text = np.concatenate(texts).astype(np.int32) if total and text_off[-1] else np.zeros(0, np.int32)
    mask_idx, pools, n_masks, M = [], [], 0, 0
    for i, l in enumerate(lists):
        mi = np.asarray(l['mask_idx'], np.int32).reshape(-1).copy() if len(l['rects']) else np.zeros(0, np.int32)
        mk = l.get('masks')
        if (mi >= 0).any():
            mk = np.ascontiguousarray(mk, np.float32)
            if M and mk.shape[1] != M:
                raise ValueError('render_lists: masks of sizes %d and %d in one call' % (M, mk.shape[1]))
            M = int(mk.shape[1])
            r = np.asarray(l['rects'], np.int64).reshape(-1, 4)[mi >= 0]
            if mi.max() >= len(mk) or not ((0 <= r[:, 0]) & (r[:, 0] <= r[:, 2]) & (r[:, 2] < hw[i, 1]) & (0 <= r[:, 1]) & (r[:, 1] <= r[:, 3]) & (r[:, 3] < hw[i, 0])).all():
                raise ValueError('render_lists: image %d has a mask item whose rect is not a paste box inside its %d x %d image, or whose mask is missing' % (i, hw[i, 0], hw[i, 1]))
            mi[mi >= 0] += n_masks
            pools.append(mk)
            n_masks += len(mk)
        mask_idx.append(mi)
    mask_idx = np.concatenate(mask_idx) if total else np.zeros(0, np.int32)

    def lap(key):          # (timing given: every stage is closed by a synchronise)
        nonlocal t0
        if timing is not None:
            torch.cuda.synchronize()
            timing[key] = timing.get(key, 0.0) + time.perf_counter() - t0
            t0 = time.perf_counter()
    lap('pack_s')
    if tensor_form:
        src = hip.dev(source, torch.float32)
    else:
        flat = [hip.dev(s).reshape(-1) for s in source]
        src = flat[0] if I == 1 else torch.cat(flat)
    d = lambda a: hip.dev(a) if a.size else None
    args = ['sn_render_dets', 1 if tensor_form else 0, src, hip.dev(hw.astype(np.int32)), hip.dev(pix_off), I, int(hw[:, 0].max()), int(hw[:, 1].max()),
            int(pix_off[-1]), hip.dev(item_off), max(counts), total, d(rects), d(colors), d(mask_idx), hip.dev(text_off) if total else None,
            d(text), text if text.size else None, int(text.size), hip.dev(atlas) if atlas is not None and text.size else None, int(G), int(gh), int(gw),
            hip.dev(np.concatenate(pools)) if n_masks else None, n_masks, M, float(np.float32(binary_thresh)), int(mask_alpha), int(line_width),
            m3[0], m3[1], m3[2], torch.empty((int(pix_off[-1]) * 3,), dtype=torch.uint8, device=dev), hip.stream()]
    out = args[-2]
    lap('upload_s')
    for _ in range(max(1, int(repeat))):
        hip.call(*args)
    lap('kernel_s')
    views = [out[3 * pix_off[i]:3 * pix_off[i + 1]].view(int(hw[i, 0]), int(hw[i, 1]), 3) for i in range(I)]
    if on_device:
        return views
    host = out.cpu().numpy()
    lap('download_s')
    return [host[3 * pix_off[i]:3 * pix_off[i + 1]].reshape(int(hw[i, 0]), int(hw[i, 1]), 3) for i in range(I)]


def render_batch(source, dets_per_image, class_names, scale=1.0, means=None, threshold=0.5, masks_per_image=None, binary_thresh=0.4,
                 atlas='default', mask_alpha=MASK_ALPHA, line_width=LINE_WIDTH):
    """Draw dets_per_image[i] (dets[j] = the (n, 5) rows of class j, as visualize_dets takes them) into image i: one device call for
    the batch.  source / means / atlas / the return value: as render_lists; scale: one value or one per image;
    masks_per_image[i][j]: (n, M, M) maps aligned with dets_per_image[i][j]."""
    tensor_form = not isinstance(source, (list, tuple))
    I = int(source.shape[0]) if tensor_form else len(source)
    scales = [scale] * I if np.ndim(scale) == 0 else list(scale)
    lists = []
    for i in range(I):
        hw = tuple(source.shape[2:4]) if tensor_form else tuple(source[i].shape[:2])
        lists.append(draw_list(dets_per_image[i], scales[i], class_names, threshold, masks_per_image[i] if masks_per_image is not None else None, hw))
    return render_lists(source, lists, atlas, means, mask_alpha, line_width, binary_thresh)


def _save(arr, path):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


ENCODERS = ('pil', 'device')


def _check_encoder(encoder):
    if encoder not in ENCODERS:
        raise ValueError("encoder=%r: 'pil' (the default) or 'device'" % (encoder,))


def _save_all(pics, paths, encoder='pil'):
    """pics[i] -> paths[i].  encoder='device': a '.png' path (any letter case) is encoded on the device by sniper_amd/png.py, a '.jpg' or
    '.jpeg' path by sniper_amd/jpeg_encode.py (byte for byte the file PIL writes: quality 75, 4:2:0), device tensors without their raw
    bytes coming to the host; every other file, and every file of encoder='pil', is written by PIL."""
    import torch
    _check_encoder(encoder)
    ext = [os.path.splitext(path)[1].lower() if encoder == 'device' else '' for path in paths]
    dev = [k for k, e in enumerate(ext) if e == '.png']
    jpg = [k for k, e in enumerate(ext) if e in ('.jpg', '.jpeg')]
    if dev:
        from .png import write_png
        write_png([paths[k] for k in dev], [pics[k] for k in dev])
    if jpg:
        from .jpeg_encode import write_jpeg
        write_jpeg([paths[k] for k in jpg], [pics[k] for k in jpg])
    for k in sorted(set(range(len(paths))) - set(dev) - set(jpg)):
        _save(pics[k].cpu().numpy() if isinstance(pics[k], torch.Tensor) else pics[k], paths[k])


def visualize_dets(im, dets, scale, pixel_means, class_names, threshold=0.5, save_path='debug.png', transform=True, dpi=80, masks=None,
                   binary_thresh=0.4, encoder='pil'):
    """The reference's entry point, signature and meaning (lib/data_utils/visualization.py:21-57): transform=True takes the (3, h, w)
    network input and adds pixel_means[[2, 1, 0]] back (transform_im; clamped here); transform=False an (h, w, 3) uint8 RGB image.
    masks[j]: (n, M, M) maps aligned with dets[j].  `dpi` is accepted and unused: a pixel of the image is a pixel of the file.  The
    file's extension decides its format (PIL); encoder='device' writes a '.png' file with this project's encoder (sniper_amd/png.py)
    and a '.jpg' / '.jpeg' file with sniper_amd/jpeg_encode.py, which writes the bytes PIL would.
    -> the (h, w, 3) uint8 picture."""
    import torch
    _check_encoder(encoder)
    if transform:
        t = im if isinstance(im, torch.Tensor) else torch.as_tensor(np.asarray(im, np.float32))
        pic = render_batch(t[None], [dets], class_names, scale, np.asarray(pixel_means, np.float32)[[2, 1, 0]], threshold,
                           [masks] if masks is not None else None, binary_thresh)[0]
    else:
        pic = render_batch([im if isinstance(im, torch.Tensor) else np.ascontiguousarray(im, np.uint8)], [dets], class_names, scale, None,
                           threshold, [masks] if masks is not None else None, binary_thresh)[0]
    if save_path and encoder == 'device':
        _save_all([pic], [save_path], encoder)
    if isinstance(pic, torch.Tensor):
        pic = pic.cpu().numpy()
    if save_path and encoder != 'device':
        _save(pic, save_path)
    return pic


def _load_rgb(entry):
    from PIL import Image
    im = np.array(Image.open(entry['image']).convert('RGB'))
    return np.ascontiguousarray(im[:, ::-1] if entry.get('flipped') else im)


def render_results(roidb, all_boxes, class_names, out_dir, all_masks=None, threshold=0.5, vis_ext='.png', names=None,
                   binary_thresh=0.4, budget_bytes=256 << 20, encoder='pil'):
    """A data set's final detections as pictures: image i of roidb (its file `image`, mirrored when `flipped`) with
    all_boxes[j][i] -- and all_masks[j][i], what mask_inference.predict_masks returns -- drawn at scale 1, saved as
    out_dir/{names[i] or i}{vis_ext}.  Images are rendered in batches whose source bytes stay under budget_bytes (one device call
    each).  encoder='device': '.png' and '.jpg' / '.jpeg' files are encoded on the device, a batch per call, from the rendered pictures
    where they lie (sniper_amd/png.py, sniper_amd/jpeg_encode.py: the JPEG files are byte for byte the files PIL writes).
    -> the paths written, in image order."""
    _check_encoder(encoder)
    if not os.path.isdir(out_dir):
        os.makedirs(out_dir)
    K = len(all_boxes)
    class_names = list(class_names) if class_names is not None else ['__background__'] + ['class %d' % j for j in range(1, K)]
    paths, batch, size = [], [], 0

    def flush():
        ims = [b[1] for b in batch]
        dets = [[[]] + [all_boxes[j][b[0]] for j in range(1, K)] for b in batch]
        masks = [[None] + [all_masks[j][b[0]] for j in range(1, K)] for b in batch] if all_masks is not None else None
        if encoder == 'device':
            import torch
            from . import hip
            ims = [torch.as_tensor(im).to(hip.require_gpu()) for im in ims]          # device sources: the pictures stay in HBM
        pics = render_batch(ims, dets, class_names, 1.0, None, threshold, masks, binary_thresh)
        out = [os.path.join(out_dir, '{}{}'.format(names[b[0]] if names is not None else b[0], vis_ext)) for b in batch]
        if encoder == 'device':
            _save_all(pics, out, encoder)
        else:
            for pic, path in zip(pics, out):
                _save(pic, path)
        paths.extend(out)
        del batch[:]

    for i, entry in enumerate(roidb):
        im = _load_rgb(entry)
        if batch and size + im.nbytes > budget_bytes:
            flush()
            size = 0
        batch.append((i, im))
        size += im.nbytes
    if batch:
        flush()
    return paths
