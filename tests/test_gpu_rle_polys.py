"""-m gpu: polygons to run-length encoded masks (sn_rle_poly_cross + sn_rle_from_polys through sniper_amd.evaluation.rle_from_polys)
against the reference's counts in tests/golden/cocosegm_v1.npz and against the restatement (tests/coco_segm_ref.py): boundary-point
and crossing counts at 0, 1 and the three values around once and twice the workgroup size that sn_rle_limits reports, a zigzag of tens of thousands of crossings, annotations of 1, 2
and 65 parts, two runs with the same bytes, and the closed loop over the synthetic mask roidb.  Counts are integers: no tolerance."""
import numpy as np
import pytest

import coco_segm_ref as ref
import coco_segm_util as U

pytestmark = pytest.mark.gpu



@pytest.fixture(scope='module')
def chunk():
    """threads of a workgroup = boundary points per round of the walk = crossings per round of the slot scan (sn_rle_limits)"""
    import ctypes
    from sniper_amd import hip
    out = (ctypes.c_int32 * 5)()
    hip.lib().call('sn_rle_limits', out)
    return int(out[4])


def _device(polys, hw):
    from sniper_amd.evaluation import rle_from_polys
    got = rle_from_polys(polys, hw)
    again = rle_from_polys(polys, hw)
    assert all(a.dtype == np.uint32 and a.tobytes() == b.tobytes() for a, b in zip(got, again)), 'two runs differ'
    return got


def _same(got, want, what):
    assert len(got) == len(want)
    for n, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, n, a[:12], np.asarray(b)[:12], len(a), len(b))


@pytest.mark.parametrize('s', U.SETS)
def test_golden_polygons(s):
    d = U.load_golden()[s]
    rows = [n for n in range(len(d['gt_form'])) if int(d['gt_form'][n]) == U.FORM_POLY]
    if not rows:
        assert s != 'edge'
        return
    got = _device([[list(p) for p in d['gt_polys'][n]] for n in rows], d['sizes'][d['gt_image'][rows]])
    _same(got, [d['gt_counts'][n] for n in rows], s)


def seam_values(T):
    return (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)


def crossing_candidates(T, h, w):
    """rectangles, triangles and clipped shapes of every width around T / 2 and T columns (about two crossings per column; the
    clipped ones drop some), and points / segments for 0 and 1"""
    polys = [[3.0, 3.0], [3.0, 3.0, 3.2, 3.0], [3.0, 3.0, 4.0, 3.0], [2.5, 1.0, 3.5, 9.0]]
    for n in list(range(1, 4)) + list(range(T // 2 - 4, T // 2 + 5)) + list(range(T - 4, T + 5)):
        polys.append([2.0, 5.0, 2.0 + n, 5.0, 2.0 + n, 12.0, 2.0, 12.0])                  # two crossings per column
        polys.append([2.0, 5.0, 2.0 + n, 5.0, 2.0 + n / 2.0, 30.0])                        # a triangle
        polys.append([-3.0, 37.0, -3.0 + n, 37.0, -3.0 + n, 45.0, -3.0, 45.0])             # clipped at the left and at the bottom
        polys.append([w - n + 0.0, 35.0, w + 2.0, 35.0, w + 2.0, 40.0, w - n + 0.0, 40.0])  # reaches the last pixel
    return polys


def point_polygon(P):
    """a polygon of exactly P >= 1 boundary points (the sum over its edges of max(|dx|, |dy|) + 1 in the 5x grid): one vertex for 1, a
    segment of (P - 2) / 2 grid steps for an even P, a flat triangle 0 -> 1 -> (P - 3) / 2 for an odd one"""
    if P == 1:
        return [1.0, 2.0]
    if P % 2 == 0:
        return [0.0, 2.0, (P // 2 - 1) / 5.0, 2.0]
    assert P >= 7
    return [0.0, 2.0, 1 / 5.0, 2.0, ((P - 3) // 2) / 5.0, 2.0]


def _counts_of(polys, h, w):
    """boundary points and kept crossings (below h * w) of every polygon, by the restatement"""
    pts, cross = [], []
    for p in polys:
        x = [int(5.0 * v + .5) for v in p[0::2]]
        y = [int(5.0 * v + .5) for v in p[1::2]]
        k = len(x)
        pts.append(sum(max(abs(x[j] - x[(j + 1) % k]), abs(y[j] - y[(j + 1) % k])) + 1 for j in range(k)))
        cross.append(sum(1 for v in ref.poly_crossings(p, h, w) if v < h * w))
    return pts, cross


def test_seams_against_the_restatement(chunk):
    """crossings per polygon of exactly 0, 1, T - 1, T, T + 1, 2T - 1, 2T, 2T + 1 and boundary points of exactly 1, T - 1 .. 2T + 1 (a
    polygon has a vertex, hence a point: 0 does not exist), T = the workgroup size sn_rle_limits reports; each value asserted present"""
    T = chunk
    h, w = 40, T + 44
    cand = crossing_candidates(T, h, w)
    _, cross = _counts_of(cand, h, w)
    polys = []
    for want in seam_values(T):
        assert want in cross, (want, sorted(set(cross)))
        polys.append(cand[cross.index(want)])
    n_cross = len(polys)
    point_values = [v for v in seam_values(T) if v >= 1]
    polys += [point_polygon(P) for P in point_values]
    pts, cross = _counts_of(polys, h, w)
    assert cross[:n_cross] == list(seam_values(T)) and pts[n_cross:] == point_values
    got = _device([[p] for p in polys], np.tile([[h, w]], (len(polys), 1)))
    want = [ref.rle_from_poly(p, h, w) for p in polys]
    _same(got, want, 'seams')
    # run counts per polygon across the same seams: the counts written per round of the last pass
    runs = sorted(set(len(r) for r in want))
    assert any(v <= 1 for v in runs) and any(T - 4 <= v <= T + 4 for v in runs) and any(v > 2 * T - 4 for v in runs), runs


def test_a_zigzag_of_tens_of_thousands_of_crossings():
    h, w = 4, 12000
    top = [v for x in range(0, w, 2) for v in (x + 0.0, 0.0, x + 1.0, 4.0)]
    poly = top + [w - 1.0, 4.5, 0.0, 4.5]
    want = ref.rle_from_poly(poly, h, w)
    n_cross = len(ref.poly_crossings(poly, h, w))
    assert n_cross > 20000
    got = _device([[poly]], [[h, w]])
    _same(got, [want], 'zigzag')


def test_annotations_of_1_2_and_65_parts():
    rng = np.random.RandomState(3)
    h, w = 48, 64

    def rect():
        x0, y0 = rng.uniform(-4, w - 2), rng.uniform(-4, h - 2)
        ww, hh = rng.uniform(1, 20), rng.uniform(1, 20)
        return [round(float(v), 2) for v in (x0, y0, x0 + ww, y0, x0 + ww, y0 + hh, x0, y0 + hh)]

    def tri():
        return [round(float(v), 2) for v in rng.uniform(-3, 66, 6)]
    anns = [[rect()], [tri()], [rect(), rect()], [rect(), tri()], [[5.0, 5.0, 30.0, 5.0, 30.0, 30.0, 5.0, 30.0], [10.0, 10.0, 20.0, 10.0, 20.0, 20.0, 10.0, 20.0]],
            [[0.0, 0.0, 64.0, 0.0, 64.0, 48.0, 0.0, 48.0], tri()], [rect() if n % 3 else tri() for n in range(65)], [[1.0, 1.0]], [[1.0, 1.0], rect()],
            [[70.0, 50.0, 80.0, 50.0, 80.0, 60.0], [60.0, 44.0, 64.0, 44.0, 64.0, 48.0, 60.0, 48.0]]]
    got = _device(anns, np.tile([[h, w]], (len(anns), 1)))
    _same(got, [ref.rle_from_polys(a, h, w) for a in anns], 'parts')
    assert sum(len(a) for a in anns) >= 80 and any(len(g) > 20 for g in got)


def test_closed_loop_over_the_synthetic_mask_roidb():
    """gt_masks (polygons) -> from_roidb -> detections made from the ground truth, each with a constant-1 mask -> a finite AP above 0"""
    from sniper_amd import synthetic
    from sniper_amd.evaluation import COCOSegmEvaluator, evaluate_sds
    num_classes = 5
    # the roidb's polygons are noisy ellipses inscribed in (a part of) their box and fill about a third of it; a constant-1 mask reaches
    # IoU 0.5 only where an object fills half of its box, which two objects of the first 12 images do (images 6 and 10: 0.51, 0.53)
    roidb = synthetic.make_roidb(n_images=12, seed=0, num_classes=num_classes, with_masks=True)
    ev = COCOSegmEvaluator.from_roidb(roidb, num_classes)
    assert len(ev.gt_rle) == sum(int((np.asarray(r['gt_classes']) > 0).sum()) for r in roidb) > 0
    for n in range(len(ev.gt_rle)):          # the conversion against the restatement, and the area against the mask's own
        r = roidb[ev.gt['image'][n]]
        keep = np.flatnonzero(np.asarray(r['gt_classes']) > 0)
        j = keep[n - int(np.searchsorted(ev.gt['image'], ev.gt['image'][n]))]
        want = ref.rle_from_polys(r['gt_masks'][j], r['height'], r['width'])
        assert np.array_equal(ev.gt_rle[n], want), n
        if 'gt_areas' not in r:
            assert ev.gt['area'][n] == ref.rle_area(want)
    # detections from the ground truth itself: its box and a constant-1 mask, pasted into the image
    boxes = [[np.zeros((0, 5)) for _ in roidb] for _ in range(num_classes)]
    masks = [[np.zeros((0, 28, 28), np.float32) for _ in roidb] for _ in range(num_classes)]
    n = 0
    for i, r in enumerate(roidb):
        for j in np.flatnonzero(np.asarray(r['gt_classes']) > 0):
            k = int(r['gt_classes'][j])
            boxes[k][i] = np.concatenate((boxes[k][i], [list(np.asarray(r['boxes'], np.float64)[j]) + [0.9 - 0.001 * n]]))
            masks[k][i] = np.concatenate((masks[k][i], np.ones((1, 28, 28), np.float32)))
            n += 1
    res = evaluate_sds(boxes, masks, roidb, num_classes)
    assert np.isfinite(res.stats[0]) and res.stats[0] > 0
    lines = res.summary().split('\n')
    assert len(lines) == 12 and lines[0].startswith(' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ')
