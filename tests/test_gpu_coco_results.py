"""-m gpu: sniper_amd.results end to end on the seeded set of tests/coco_segm_util.py (24 images of at most 64 x 48 pixels): a results
file written and evaluated from the file gives the bits of the evaluation of the detections themselves, for boxes and for masks; the
strings of pasted probabilities are those of rle_paste's counts; the file parses to the records."""
import json

import numpy as np
import pytest

import coco_results_util as RU
import coco_segm_util as SU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seeded():
    """the set, its detections as all_boxes / all_masks (RLE dicts), and a roidb; the box columns -- which the mask golden leaves at
    zero -- are the masks' own extents, jittered for the detections (float32, as a Tester hands them over)"""
    d = SU.load_golden()['seeded']
    rng = np.random.RandomState(17)

    def extent(counts, i):
        h, w = (int(v) for v in d['sizes'][i])
        ys, xs = np.nonzero(SU.from_counts(counts, h, w))
        return [xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else [0, 0, 0, 0]
    boxes, masks = SU.detections_of(d)
    at = {}
    for n in range(len(d['dt_image'])):
        k, i = int(d['dt_category'][n]) + 1, int(d['dt_image'][n])
        r = at.get((k, i), 0)
        at[(k, i)] = r + 1
        boxes[k][i][r, :4] = np.array(extent(d['dt_counts'][n], i)) + rng.uniform(0, 1.5, 4) * [-1, -1, 1, 1]
    boxes = [[np.asarray(c, np.float32).reshape(-1, 5) for c in per_image] for per_image in boxes]
    roidb, num_classes = SU.roidb_of(d)
    for i, r in enumerate(roidb):
        rows = np.flatnonzero(d['gt_image'] == i)
        r['boxes'] = np.array([extent(d['gt_counts'][n], i) for n in rows], np.float64).reshape(-1, 4)
    return dict(d=d, boxes=boxes, masks=masks, roidb=roidb, num_classes=num_classes, image_ids=range(1, d['I'] + 1),
                cat_ids=range(1, d['K'] + 1))


def test_bbox_file_evaluates_to_the_bits_of_evaluate_detections(seeded, tmp_path):
    from sniper_amd.evaluation import evaluate_detections
    from sniper_amd.results import evaluate_results_file, write_coco_results
    s = seeded
    path = str(tmp_path / 'detections_val_results.json')
    n = write_coco_results(path, s['boxes'], s['image_ids'], s['cat_ids'])
    assert n == len(s['d']['dt_image'])
    got = evaluate_results_file(path, s['roidb'], s['num_classes'], 'bbox')
    want = evaluate_detections(s['boxes'], s['roidb'], s['num_classes'])
    assert got.precision.tobytes() == want.precision.tobytes() and got.recall.tobytes() == want.recall.tobytes()
    assert (want.precision > -1).mean() > 0.5 and 0.05 < want.stats[0] < 1
    assert got.summary() == want.summary()


def test_segm_file_evaluates_to_the_bits_of_evaluate_sds(seeded, tmp_path):
    from sniper_amd.evaluation import evaluate_sds
    from sniper_amd.results import evaluate_results_file, load_coco_results, write_coco_results
    s = seeded
    path = str(tmp_path / 'detections_val_results.json')
    n = write_coco_results(path, s['boxes'], s['image_ids'], s['cat_ids'], 'segm', s['masks'], s['d']['sizes'])
    assert n == len(s['d']['dt_image'])
    got = evaluate_results_file(path, s['roidb'], s['num_classes'], 'segm')
    want = evaluate_sds(s['boxes'], s['masks'], s['roidb'], s['num_classes'])
    assert got.iou_type == 'segm'
    assert got.precision.tobytes() == want.precision.tobytes() and got.recall.tobytes() == want.recall.tobytes()
    assert (want.precision > -1).mean() > 0.5 and 0.05 < want.stats[0] < 1
    # the cells that come back: the counts that went in, and the masks' own bounding boxes (the reference's rleToBbox, from the golden)
    boxes, masks = load_coco_results(path, s['image_ids'], s['cat_ids'], s['d']['sizes'])
    seen = 0
    order = sorted(range(n), key=lambda m: (int(s['d']['dt_category'][m]), int(s['d']['dt_image'][m]), m))
    it = iter(order)
    for k in range(1, s['num_classes']):
        for i in range(s['d']['I']):
            assert len(masks[k][i]) == len(s['masks'][k][i]) == len(boxes[k][i])
            for r, (a, b) in enumerate(zip(masks[k][i], s['masks'][k][i])):
                m = next(it)
                assert a['size'] == b['size'] and a['counts'].dtype == np.uint32 and np.array_equal(a['counts'], b['counts'])
                x, y, w, h = s['d']['dt_bbox'][m]
                assert boxes[k][i][r].tolist() == ([x, y, x + w - 1, y + h - 1] if w > 0 else [0., 0., 0., 0.]) + [float(np.float32(s['d']['dt_score'][m]))]
                seen += 1
    assert seen == n


def test_strings_of_pasted_probabilities_and_the_parsed_file(seeded, tmp_path):
    from sniper_amd.evaluation import paste_boxes, rle_paste
    from sniper_amd.results import coco_results, rle_to_strings, write_coco_results
    s = seeded
    rng = np.random.RandomState(23)
    yy, xx = np.mgrid[0:28, 0:28]
    probs = [[None] * len(per_image) for per_image in s['boxes']]
    for k, per_image in enumerate(s['boxes']):
        for i, rows in enumerate(per_image):
            cy, cx, ry, rx = rng.uniform(8, 20, (4, len(rows), 1, 1))
            probs[k][i] = np.clip(1.2 - ((yy - cy) / ry) ** 2 - ((xx - cx) / rx) ** 2, 0, 1).astype(np.float32).reshape(len(rows), 28, 28)
    boxes = [[c.copy() for c in per_image] for per_image in s['boxes']]
    for i in range(len(boxes[0])):
        boxes[2][i] = boxes[2][i][:0]                  # a class without detections
        probs[2][i] = probs[2][i][:0]
    for k in range(len(boxes)):
        boxes[k][3] = boxes[k][3][:0]                  # an image without detections
        probs[k][3] = probs[k][3][:0]
    sizes = s['d']['sizes']
    recs = coco_results(boxes, s['image_ids'], s['cat_ids'], 'segm', probs, sizes)
    assert len(recs) == sum(len(c) for per_image in boxes for c in per_image) > 20
    assert all(r['category_id'] != s['cat_ids'][1] and r['image_id'] != s['image_ids'][3] for r in recs)
    want, scores = [], []
    for k in range(1, len(boxes)):
        for i, rows in enumerate(boxes[k]):
            if len(rows):
                h, w = (int(v) for v in sizes[i])
                rles = rle_paste(probs[k][i], paste_boxes(rows.astype(np.float64), h, w), np.tile([[h, w]], (len(rows), 1)))
                want += rle_to_strings(rles)
                scores += [float(v) for v in rows[:, 4]]
                assert all(int(r.sum()) == h * w for r in rles)
    assert [r['segmentation']['counts'] for r in recs] == want and [r['score'] for r in recs] == scores
    assert len(set(want)) > len(want) // 2
    path = str(tmp_path / 'detections_test-dev_results.json')
    assert write_coco_results(path, boxes, s['image_ids'], s['cat_ids'], 'segm', probs, sizes) == len(recs)
    with open(path) as fh:
        text = fh.read()
    assert text == json.dumps(recs, sort_keys=True, indent=4)
    RU.same_records(json.loads(text), recs)
    brecs = coco_results(boxes, s['image_ids'], s['cat_ids'])
    bpath = str(tmp_path / 'detections_bbox_results.json')
    write_coco_results(bpath, boxes, s['image_ids'], s['cat_ids'])
    with open(bpath) as fh:
        RU.same_records(json.load(fh), brecs)
    assert len(brecs) == len(recs)
