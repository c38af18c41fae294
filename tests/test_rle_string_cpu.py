"""CPU: the string coders' closed-form restatement (tests/rle_string_ref.py) against the reference's own strings, and the host side of
sniper_amd.results -- the records, the json layout, the VOC lines, every ValueError -- against tests/golden/cocoresults_v1.npz.
Nothing here needs a device; everything is bytes or bits."""
import json

import numpy as np
import pytest

import coco_results_util as RU
import coco_segm_util as SU
import rle_string_ref as ref


@pytest.fixture(scope='module')
def golden():
    return RU.load_golden()


def test_restatement_equals_the_references_strings_and_inverts_them(golden):
    from sniper_amd.evaluation import rle_from_string
    assert len(golden['counts']) == len(golden['strings']) >= 40
    widths = set()
    for c, s in zip(golden['counts'], golden['strings']):
        assert ref.to_string(c) == s and ref.string_len(c) == len(s)
        assert ref.status_of(s) == (0, len(c))
        back = ref.from_string(s)
        assert back.dtype == np.uint32 and np.array_equal(back, c)
        assert np.array_equal(rle_from_string(s), c)
        widths |= set(ref.widths(ref.differences(c)).tolist())
    assert widths == {1, 2, 3, 4, 5, 6}          # the reference is defined up to six characters; seven are this project's


def test_restatement_equals_the_strings_of_the_mask_golden():
    n = 0
    for s, d in SU.load_golden().items():
        for form, counts, text in zip(d['gt_form'], d['gt_counts'], d['gt_strings']):
            if form == SU.FORM_STRING:
                assert ref.to_string(counts) == text and np.array_equal(ref.from_string(text), counts), s
                n += 1
    assert n >= 5


def test_restatement_past_the_reference_seven_characters_and_modulo():
    from sniper_amd.evaluation import rle_from_string
    c = np.array([0, 2 ** 32 - 1, 5, 0, 2 ** 32 - 1, 2 ** 29, 2 ** 32 - 1 - 2 ** 29, 2 ** 31], np.uint32)
    s = ref.to_string(c)
    assert sorted(set(ref.widths(ref.differences(c)).tolist()))[-1] == 7
    assert np.array_equal(ref.from_string(s), c) and np.array_equal(rle_from_string(s), c)
    assert ref.widths(np.array([2 ** 29 - 1, 2 ** 29, -2 ** 29, -2 ** 29 - 1, 2 ** 32 - 1, -(2 ** 32 - 1)])).tolist() == [6, 7, 6, 7, 7, 7]
    assert [ref.status_of(t)[0] for t in ('', '0', 'P', '0P', 'PPPPPP0', 'PPPPPPP0', '0~', '0/', '~P')] == [0, 0, 1, 1, 0, 3, 2, 2, 2]


def test_bbox_records_equal_the_references(golden):
    from sniper_amd.results import coco_results
    got = coco_results(golden['all_boxes'], golden['image_ids'], golden['cat_ids'])
    RU.same_records(got, golden['bbox'])
    assert len(got) >= 12


def test_segm_records_from_string_cells_equal_the_references(golden):
    """cells passed as RLE dicts whose counts are already strings: order, ids, sizes and the unrounded score, without a device"""
    from sniper_amd.results import coco_results
    it = iter(golden['segm'])
    cells = [[[dict(next(it)['segmentation']) for _ in range(len(rows))] for rows in per_image] for per_image in golden['all_boxes']]
    got = coco_results(golden['all_boxes'], golden['image_ids'], golden['cat_ids'], 'segm', cells, golden['sizes'])
    RU.same_records(got, golden['segm'])
    assert any(r['score'] != round(r['score'], 8) for r in got)            # unrounded: coco.py:57


def test_json_layout_and_the_way_back(golden, tmp_path):
    from sniper_amd.results import load_coco_results, write_coco_results
    path = str(tmp_path / 'detections_val_results.json')
    n = write_coco_results(path, golden['all_boxes'], golden['image_ids'], golden['cat_ids'])
    assert n == len(golden['bbox'])
    with open(path) as fh:
        text = fh.read()
    assert text == json.dumps(golden['bbox'], sort_keys=True, indent=4)
    assert text.startswith('[\n    {\n        "bbox": [\n            ')
    RU.same_records(json.loads(text), golden['bbox'])
    boxes, masks = load_coco_results(path, golden['image_ids'], golden['cat_ids'])
    assert masks is None and len(boxes) == len(golden['cat_ids']) + 1
    it = iter(golden['bbox'])
    for k, per_image in enumerate(boxes):
        for i, rows in enumerate(per_image):
            assert rows.dtype == np.float64 and len(rows) == len(golden['all_boxes'][k][i])
            for row in rows:
                r = next(it)
                x, y, w, h = r['bbox']
                assert row.tolist() == [x, y, x + w - 1, y + h - 1, r['score']]


def test_voc_lines_equal_the_references(golden, tmp_path):
    from sniper_amd.results import write_voc_results
    template = str(tmp_path / 'comp4_det_test_{:s}.txt')
    lines = write_voc_results(template, golden['all_boxes'], golden['voc_images'], golden['voc_classes'])
    assert lines == sum(f.count(b'\n') for f in golden['voc_files']) >= 12
    for cls, want in zip(golden['voc_classes'], golden['voc_files']):
        with open(template.format(cls), 'rb') as fh:
            assert fh.read() == want, cls
    assert any(len(f) == 0 for f in golden['voc_files'])                   # a class without detections: an empty file


def _raises(words, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert all(w in str(e.value) for w in words), str(e.value)


def test_value_errors_by_message(golden):
    from sniper_amd import results as R
    g = golden
    ids, cats, sizes = g['image_ids'], g['cat_ids'], g['sizes']
    _raises(('ann_type', "'keypoints'"), R.coco_results, g['all_boxes'], ids, cats, 'keypoints')
    _raises(('segm records need all_masks',), R.coco_results, g['all_boxes'], ids, cats, 'segm')
    _raises(('all_masks[class][image]', '2 classes'), R.coco_results, g['all_boxes'], ids, cats, 'segm', g['all_rles'][:2], sizes)
    k, i = [(k, i) for k in range(1, len(cats) + 1) for i in range(len(ids)) if len(g['all_boxes'][k][i])][0]
    short = [[list(c) for c in per_image] for per_image in g['all_rles']]
    short[k][i] = short[k][i][:-1]
    _raises(('all_masks[%d][%d] has %d masks' % (k, i, len(short[k][i])),), R.coco_results, g['all_boxes'], ids, cats, 'segm', short, sizes)
    wrong = [[list(c) for c in per_image] for per_image in g['all_rles']]
    wrong[k][i][0] = {'size': [3, 3], 'counts': '9'}
    _raises(('detection 0 of all_masks[%d][%d]' % (k, i), 'the mask is 3 x 3'), R.coco_results, g['all_boxes'], ids, cats, 'segm', wrong, sizes)
    # probabilities: the boxes of all cells are clipped and rounded together, and a refused one is still named by its cell
    probs = [[np.zeros((len(rows), 28, 28), np.float32) for rows in per_image] for per_image in g['all_boxes']]
    flipped = [[rows.copy() for rows in per_image] for per_image in g['all_boxes']]
    flipped[k][i][-1, :4] = [9, 4, 3, 8]
    _raises(('all_boxes[%d][%d]' % (k, i), 'detection %d' % (len(flipped[k][i]) - 1), 'x2 < x1'), R.coco_results, flipped, ids, cats, 'segm',
            probs, sizes)
    _raises(('mask 1', 'non-negative integers below 2^32'), R.rle_to_strings, [np.array([1, 2]), np.array([-1, 4])])
    _raises(('mask 0', 'non-negative integers below 2^32'), R.rle_to_strings, [np.array([1.5, 2])])
    _raises(('string 1', 'outside chr(48) .. chr(111)'), R.rle_from_strings, ['0', u'€'])
    rec = dict(g['bbox'][0])
    _raises(('record 1', 'unknown image_id 777'), R.load_coco_results, [rec, dict(rec, image_id=777)], ids, cats)
    _raises(('record 0', 'unknown category_id 2'), R.load_coco_results, [dict(rec, category_id=2)], ids, cats)
    _raises(('record 0', 'neither bbox nor segmentation'), R.load_coco_results, [{'image_id': ids[0], 'category_id': cats[0], 'score': 1.}], ids, cats)
    seg = dict(g['segm'][0])
    _raises(('needs image_sizes',), R.load_coco_results, [seg], ids, cats)
    bad = dict(seg, segmentation={'size': [2, 2], 'counts': seg['segmentation']['counts']})
    _raises(('record 1', 'the mask is 2 x 2'), R.load_coco_results, [seg, bad], ids, cats, sizes)
    _raises(('record 0', "'counts': str"), R.load_coco_results, [dict(seg, segmentation={'size': [2, 2], 'counts': [4]})], ids, cats, sizes)
    _raises(('ann_type', "'keypoints'"), R.evaluate_results_file, 'nowhere.json', [], 2, 'keypoints')
    _raises(('3 classes', '1 class names'), R.write_voc_results, 'x_{:s}.txt', [[], [], []], [], ['cat'])
