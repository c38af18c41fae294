"""What the results-file tests share: the loader of tests/golden/cocoresults_v1.npz (made by tests/golden/make_cocoresults_golden.py from
the reference's maskApi.c, coco.py and pascal_voc.py) and the device coders run at the C ABI with every operand between guard bytes."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cocoresults_v1.npz')
_CACHE = {}


def _split(pool, off):
    return [pool[off[n]:off[n + 1]] for n in range(len(off) - 1)]


def _texts(pool, off):
    return [bytes(b).decode('ascii') for b in _split(pool, off)]


def load_golden():
    """dict: counts (list of uint32 arrays) and strings (list of str) of the string cases; image_ids, cat_ids, sizes; all_boxes
    [class][image] float32 rows and all_rles[class][image] lists of RLE dicts with uint32 counts (class 0 = background); bbox / segm:
    the reference's records as lists of dicts; voc_files (bytes per class), voc_images, voc_classes"""
    if not _CACHE:
        z = np.load(GOLDEN)
        g = {'counts': _split(z['str_cnts'], z['str_cnt_off']), 'strings': _texts(z['str_chars'], z['str_off'])}
        g['image_ids'], g['cat_ids'], g['sizes'] = [int(v) for v in z['det_image_ids']], [int(v) for v in z['det_cat_ids']], z['det_sizes']
        K, I = len(g['cat_ids']), len(g['image_ids'])
        cells, masks = _split(z['det_rows'], z['det_cell_off']), _split(z['det_cnts'], z['det_cnt_off'])
        off = z['det_cell_off']
        g['all_boxes'] = [[np.zeros((0, 5), np.float32) for _ in range(I)]] + [[cells[k * I + i] for i in range(I)] for k in range(K)]
        g['all_rles'] = [[[] for _ in range(I)]] + [[[{'size': [int(v) for v in g['sizes'][i]], 'counts': m}
                                                      for m in masks[off[k * I + i]:off[k * I + i + 1]]] for i in range(I)] for k in range(K)]
        g['bbox'] = [{'image_id': int(i), 'category_id': int(c), 'bbox': [float(v) for v in b], 'score': float(s)}
                     for i, c, b, s in zip(z['bbox_image'], z['bbox_cat'], z['bbox_box'], z['bbox_score'])]
        g['segm'] = [{'image_id': int(i), 'category_id': int(c), 'segmentation': {'size': [int(v) for v in hw], 'counts': t}, 'score': float(s)}
                     for i, c, hw, t, s in zip(z['segm_image'], z['segm_cat'], z['segm_size'], _texts(z['segm_chars'], z['segm_off']), z['segm_score'])]
        g['voc_files'] = [bytes(b) for b in _split(z['voc_chars'], z['voc_off'])]
        g['voc_images'], g['voc_classes'] = _texts(z['voc_images'], z['voc_image_off']), _texts(z['voc_classes'], z['voc_class_off'])
        _CACHE.update(g)
    return _CACHE


def same_records(got, want):
    """two record lists are equal key for key with floats compared on their bits (== on floats, and the types are Python's own)"""
    assert len(got) == len(want), (len(got), len(want))
    for n, (a, b) in enumerate(zip(got, want)):
        assert a == b and sorted(a) == sorted(b), (n, a, b)
        assert type(a['score']) is float and isinstance(a['image_id'], int) and isinstance(a['category_id'], int), (n, a)
        if 'bbox' in a:
            assert all(type(v) is float for v in a['bbox']), (n, a)
        else:
            assert type(a['segmentation']['counts']) is str and all(type(v) is int for v in a['segmentation']['size']), (n, a)


# ---- the device, at the C ABI, with every operand in a guarded buffer ---------------------------------
def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int32)


def device_encode(rles):
    """sn_rle_string_len + sn_rle_to_string -> (list of bytes, str_len (N) int32)"""
    import torch
    from coco_eval_util import Guarded
    from sniper_amd import hip
    N = len(rles)
    run_off = offsets([len(r) for r in rles])
    total = int(run_off[-1])
    cnts = np.concatenate([np.asarray(r, np.uint32) for r in rles]) if total else np.zeros(0, np.uint32)
    G = Guarded()
    d_c, d_roff, o_len = G.put(cnts), G.put(run_off), G.out((N,), np.int32)
    hip.call('sn_rle_string_len', d_c, d_roff, run_off, N, total, o_len, hip.stream())
    torch.cuda.synchronize()
    G.check()
    lens = Guarded.read(o_len, (N,), np.int32)
    str_off = offsets(lens)
    chars = int(str_off[-1])
    d_soff, o_s = G.put(str_off), G.out((chars,), np.uint8)
    hip.call('sn_rle_to_string', d_c, d_roff, run_off, d_soff, str_off, N, total, chars, o_s, hip.stream())
    torch.cuda.synchronize()
    G.check()
    pool = Guarded.read(o_s, (chars,), np.uint8)
    return [pool[str_off[n]:str_off[n + 1]].tobytes() for n in range(N)], lens


def device_decode(strings, fill=0xA5A5A5A5):
    """sn_rle_string_count + sn_rle_from_string -> (list of uint32 arrays, m (N), status (N)).  A string whose status is not 0 gets
    the slots of its m all the same, and they must come back untouched (`fill`)."""
    import torch
    from coco_eval_util import Guarded
    from sniper_amd import hip
    raw = [s if isinstance(s, bytes) else s.encode('latin-1') for s in strings]
    N = len(raw)
    str_off = offsets([len(b) for b in raw])
    chars = int(str_off[-1])
    G = Guarded()
    d_s, d_soff = G.put(np.frombuffer(b''.join(raw), np.uint8)), G.put(str_off)
    o_m, o_st = G.out((N,), np.int32), G.out((N,), np.int32)
    hip.call('sn_rle_string_count', d_s, d_soff, str_off, N, chars, o_m, o_st, hip.stream())
    torch.cuda.synchronize()
    G.check()
    m, status = Guarded.read(o_m, (N,), np.int32), Guarded.read(o_st, (N,), np.int32)
    run_off = offsets(m)
    total = int(run_off[-1])
    d_roff, d_st = G.put(run_off), G.put(status)
    o_c = G.put(np.full(total, fill, np.uint32))
    G.items[-1] = (G.items[-1][0], G.items[-1][1], None)          # an output that starts from a known pattern
    hip.call('sn_rle_from_string', d_s, d_soff, str_off, d_roff, run_off, d_st, N, chars, total, o_c, hip.stream())
    torch.cuda.synchronize()
    G.check()
    pool = Guarded.read(o_c, (total,), np.uint32)
    return [pool[run_off[n]:run_off[n + 1]] for n in range(N)], m, status
