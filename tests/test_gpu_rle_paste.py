"""-m gpu: the paste of mask probabilities (sn_rle_paste_count + sn_rle_paste through sniper_amd.evaluation.rle_paste) against the
restatement tests/coco_segm_ref.py (resize_linear_f32 + rleEncode), on the bits: mask sizes 1, 14 and 28; boxes of 1 x 1, one row,
one column, the exact 2 x decimation, scale 1 and the full image; box widths on both sides of the workgroup size sn_rle_limits
reports; probabilities exactly on the threshold.  The resize is specified by this project and not pinned to OpenCV; the ENCODING
half is pinned to the reference: at scale 1 with probabilities in {0, 1} the stage is an encoder, compared with the golden's
rleEncode counts.  Through COCOSegmEvaluator the pasted detections evaluate like the same masks handed over as RLE."""
import ctypes

import numpy as np
import pytest

import coco_segm_ref as ref
import coco_segm_util as U

pytestmark = pytest.mark.gpu
THR = 0.4


def _device(masks, boxes, hw, thr=THR):
    from sniper_amd.evaluation import rle_paste
    got = rle_paste(masks, boxes, hw, thr)
    again = rle_paste(masks, boxes, hw, thr)
    assert all(a.dtype == np.uint32 and a.tobytes() == b.tobytes() for a, b in zip(got, again)), 'two runs differ'
    return got


def _check(masks, boxes, hw, thr=THR):
    got = _device(masks, boxes, hw, thr)
    for n in range(len(masks)):
        want = ref.paste(masks[n], boxes[n], int(hw[n][0]), int(hw[n][1]), thr)
        assert np.array_equal(got[n], want), (n, list(boxes[n]), list(hw[n]), got[n][:10], want[:10], len(got[n]), len(want))
        assert int(got[n].sum()) == int(hw[n][0]) * int(hw[n][1])
    return got


def _boxes_for(M, h, w, T):
    """the kinds of box the paste must handle in an h x w image (w > 2 T + 1), as x1, y1, x2, y2"""
    out = [(5, 7, 5, 7), (3, 9, 3 + 20, 9), (8, 2, 8, 2 + 17),                     # 1 x 1, one row, one column
           (4, 6, 4 + M - 1, 6 + M - 1), (0, 0, w - 1, h - 1),                      # scale 1, the full image
           (0, 0, 10, h - 1), (w - 12, 0, w - 1, h - 1), (w - 9, h - 6, w - 1, h - 1),      # full height (columns join), the last pixel
           (2, 3, 2 + 2 * M, 3 + 3 * M), (1, 1, 1 + M // 3, 1 + M // 2 + 1), (6, 0, 6 + M - 1, 2 * M - 1)]      # up, down, one axis at scale 1
    if M % 2 == 0:
        out += [(7, 5, 7 + M // 2 - 1, 5 + M // 2 - 1), (7, 5, 7 + M // 2 - 1, 5 + M - 1)]      # exact 2 x decimation; 2 x in x only (linear)
    out += [(1, 4, 1 + bw - 1, 4 + 6) for bw in (T - 1, T, T + 1, 2 * T + 1)]       # box columns across the rounds of the block scan
    return np.array(out, np.int32)


@pytest.mark.parametrize('M', (1, 14, 28))
def test_paste_against_the_restatement(M):
    from sniper_amd import hip
    lim = (ctypes.c_int32 * 5)()
    hip.lib().call('sn_rle_limits', lim)
    T = int(lim[4])
    rng = np.random.RandomState(M)
    h, w = 97, 2 * T + 30
    boxes = _boxes_for(M, h, w, T)
    n = len(boxes)
    masks = rng.rand(n, M, M).astype(np.float32)
    _check(masks, boxes, np.tile([[h, w]], (n, 1)))
    # probabilities exactly on the threshold: kept as they are at scale 1 and in constant masks (>= keeps them), beside values one
    # float32 step below
    thr = np.float32(THR)
    on = np.where(rng.rand(n, M, M) < 0.5, thr, np.nextafter(thr, np.float32(0))).astype(np.float32)
    on[0] = thr
    got = _check(on, boxes, np.tile([[h, w]], (n, 1)))
    assert int(got[3][1::2].sum()) == int((on[3] >= thr).sum())            # the scale-1 box: exactly the entries on the threshold
    ones = _check(np.ones((n, M, M), np.float32), boxes, np.tile([[h, w]], (n, 1)))
    assert [int(v) for v in ones[4]] == [0, h * w]                           # the full image, all set: a leading 0


def test_scale_1_is_the_references_encoder():
    """{0, 1} probabilities over the whole of a square image: the output is rleEncode of the bitmap, the golden's counts"""
    d, made = U.load_golden()['hand'], U.make_sets()['hand']
    by_size = {}
    for n, a in enumerate(made['dt']):
        h, w = (int(v) for v in d['sizes'][a['image']])
        if h == w:
            by_size.setdefault(h, []).append(n)
    assert sum(len(v) for v in by_size.values()) >= 10
    for M, rows in by_size.items():
        masks = np.stack([made['dt'][n]['mask'].astype(np.float32) for n in rows])
        got = _device(masks, np.tile([[0, 0, M - 1, M - 1]], (len(rows), 1)), np.tile([[M, M]], (len(rows), 1)))
        for g, n in zip(got, rows):
            assert np.array_equal(g, d['dt_counts'][n]), (M, n, g, d['dt_counts'][n])


def test_pasted_detections_evaluate_like_their_run_length_encoding():
    from sniper_amd.evaluation import COCOSegmEvaluator, paste_boxes
    d = U.load_golden()['seeded']
    rng = np.random.RandomState(9)
    K, I = d['K'], d['I']
    boxes = [[np.zeros((0, 5)) for _ in range(I)] for _ in range(K + 1)]
    probs = [[np.zeros((0, 14, 14), np.float32) for _ in range(I)] for _ in range(K + 1)]
    rles = [[[] for _ in range(I)] for _ in range(K + 1)]
    for i in range(I):
        h, w = (int(v) for v in d['sizes'][i])
        for k in range(1, K + 1):
            n = int(rng.randint(0, 3))
            if not n:
                continue
            x1, y1 = rng.uniform(-3, w - 6, n), rng.uniform(-3, h - 6, n)
            rows = np.stack((x1, y1, x1 + rng.uniform(2, 25, n), y1 + rng.uniform(2, 25, n), np.round(rng.rand(n), 2)), axis=1)
            m = rng.rand(n, 14, 14).astype(np.float32)
            boxes[k][i], probs[k][i] = rows, m
            b = paste_boxes(rows, h, w)
            rles[k][i] = [{'size': [h, w], 'counts': ref.paste(m[j], b[j], h, w, 0.5)} for j in range(n)]
    ev = COCOSegmEvaluator(U.gt_dict(d, polygons=False), range(I), range(K), d['sizes'])
    a = ev.evaluate(boxes, probs, binary_thresh=0.5, return_matches=True)
    b = ev.evaluate(boxes, rles, return_matches=True)
    assert a.precision.tobytes() == b.precision.tobytes() and a.matches['iou'].tobytes() == b.matches['iou'].tobytes()
    assert (a.matches['iou'] > 0).any() and a.timing['detections'] > 50
    other = ev.evaluate(boxes, probs, binary_thresh=0.4, return_matches=True)           # the threshold is not ignored
    assert other.matches['dt'][:, 5].sum() > a.matches['dt'][:, 5].sum()
