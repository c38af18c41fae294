"""CPU: the host pieces of sniper_amd.visualization (draw list order, the >= threshold, half-to-even rounding, label strings, the
palette, the default atlas) and the numpy restatement's own layer order on a hand-made case."""
import numpy as np
import pytest

import render_ref as ref
from sniper_amd import visualization as V

NAMES = ['__background__', 'cat', 'dog', 'emu']


def _row(x1, y1, x2, y2, s):
    return [x1, y1, x2, y2, s]


def test_draw_list_walks_classes_then_rows_and_skips_the_background():
    dets = [np.array([_row(0, 0, 9, 9, 0.99)], np.float32),                        # index 0: never drawn
            np.array([_row(1, 1, 5, 5, 0.9), _row(2, 2, 6, 6, 0.1), _row(3, 3, 7, 7, 0.8)], np.float32),
            np.zeros((0, 5), np.float32),
            np.array([_row(4, 4, 8, 8, 0.7)], np.float32)]
    L = V.draw_list(dets, 1.0, NAMES)
    assert L['rects'].dtype == np.int32 and L['colors'].dtype == np.uint8 and L['mask_idx'].dtype == np.int32
    assert L['rects'].tolist() == [[1, 1, 5, 5], [3, 3, 7, 7], [4, 4, 8, 8]]
    assert L['labels'] == ['cat 0.9', 'cat 0.8', 'emu 0.7']
    pal = V.class_colors(4)
    assert L['colors'].tolist() == [pal[1].tolist(), pal[1].tolist(), pal[3].tolist()]
    assert L['mask_idx'].tolist() == [-1, -1, -1] and L['masks'] is None
    empty = V.draw_list([[], [], [], []], 1.0, NAMES)
    assert empty['rects'].shape == (0, 4) and empty['colors'].shape == (0, 3) and empty['labels'] == []


def test_a_score_exactly_at_the_threshold_is_kept():
    half = np.float32(0.5)
    dets = [[], np.array([_row(0, 0, 1, 1, half), _row(0, 0, 2, 2, np.nextafter(half, np.float32(0))), _row(0, 0, 3, 3, np.nan)], np.float32)]
    L = V.draw_list(dets, 1.0, NAMES[:2], threshold=0.5)
    assert L['rects'].tolist() == [[0, 0, 1, 1]]                       # the reference skips score < threshold: 0.5 stays
    assert V.draw_list(dets, 1.0, NAMES[:2], threshold=0.0)['rects'][:, 2].tolist() == [1, 2]


def test_boxes_are_scaled_in_float32_and_rounded_half_to_even():
    dets = [[], np.array([_row(0.5, 1.5, 2.5, 3.5, 1), _row(-0.5, -1.5, 4.25, 4.75, 1), _row(1, 3, 5, 7, 1)], np.float32)]
    assert V.draw_list(dets, 1.0, NAMES[:2])['rects'].tolist() == [[0, 2, 2, 4], [0, -2, 4, 5], [1, 3, 5, 7]]
    assert V.draw_list(dets, 0.5, NAMES[:2])['rects'][2].tolist() == [0, 2, 2, 4]          # .5 products: 0.5, 1.5, 2.5, 3.5
    # float32, not float64: 16777217 is no float32, and 0.1f * 3 rounds like float32
    d = [[], np.array([_row(0.1, 0.7, 16777216, 1e30, 1)], np.float32)]
    want = np.clip(np.rint((d[1][0, :4] * 3.0).astype(np.float64)), -V.COORD, V.COORD).astype(np.int32)
    assert (d[1][0, :4] * 3.0).dtype == np.float32
    got = V.draw_list(d, 3.0, NAMES[:2])['rects'][0]
    assert got.tolist() == want.tolist() and got[3] == V.COORD


def test_label_strings_and_their_encoding():
    dets = [[], np.array([_row(0, 0, 1, 1, 0.96), _row(0, 0, 1, 1, 0.949), _row(0, 0, 1, 1, 1.0)], np.float32)]
    assert V.draw_list(dets, 1.0, ['__background__', 'traffic light'])['labels'] == ['traffic light 1.0', 'traffic light 0.9', 'traffic light 1.0']
    assert V.encode_text(' A~').tolist() == [0, 33, 94] and V.encode_text('é\n').tolist() == [31, 31] and V.encode_text('').dtype == np.int32


def test_mask_items_take_the_box_of_the_paste():
    from sniper_amd.evaluation import paste_boxes
    dets = [[], np.array([_row(-3.2, 1.5, 30.6, 8.5, 0.9), _row(2, 2, 4, 4, 0.2), _row(1.4, 0, 5, 3, 0.8)], np.float32)]
    masks = [None, np.arange(3 * 4 * 4, dtype=np.float32).reshape(3, 4, 4)]
    L = V.draw_list(dets, 1.0, NAMES[:2], masks=masks, hw=(10, 20))
    assert L['rects'].tolist() == paste_boxes(dets[1][[0, 2]], 10, 20).tolist() == [[0, 2, 19, 8], [1, 0, 5, 3]]
    assert L['mask_idx'].tolist() == [0, 1] and np.array_equal(L['masks'], masks[1][[0, 2]])
    with pytest.raises(ValueError):
        V.draw_list(dets, 1.0, NAMES[:2], masks=masks)                 # no image size
    with pytest.raises(ValueError):
        V.draw_list(dets, 1.0, NAMES[:2], masks=[None, masks[1][:2]], hw=(10, 20))


def test_palette_is_deterministic_distinct_and_never_white():
    a, b = V.class_colors(81), V.class_colors(81)
    assert a.dtype == np.uint8 and a.shape == (81, 3) and np.array_equal(a, b)
    assert len({tuple(c) for c in a.tolist()}) == 81
    big = V.class_colors(4096)
    assert len({tuple(c) for c in big.tolist()}) == 4096 and not (big == 255).all(axis=1).any()
    assert np.array_equal(big[:81], a) and a[1].tolist() == [128, 0, 0] and a[2].tolist() == [0, 128, 0] and a[8].tolist() == [64, 0, 0]


def test_default_atlas():
    try:
        from PIL import ImageFont
        ImageFont.load_default()
    except Exception as e:          # noqa: BLE001
        pytest.skip('PIL\'s default font cannot be loaded: %s' % e)
    atlas = V.default_atlas()
    assert atlas is not None and atlas.dtype == np.uint8 and atlas.ndim == 3 and atlas.shape[0] == 95
    assert atlas.shape[1] >= 5 and atlas.shape[2] >= 3
    assert atlas[0].max() == 0 and atlas[ord('A') - 32].max() > 128 and not np.array_equal(atlas[ord('A') - 32], atlas[ord('B') - 32])
    assert V.default_atlas() is atlas


def test_restatement_layer_order_on_a_hand_made_case():
    """8 x 8, grey 100.  Item 0: a red rect (1,3)-(6,7), line width 1, with a full mask at alpha 128 and a one-glyph label that does not
    fit above (top 3 - 4 < 0), so it sits inside at y = 4.  Item 1: a blue rect (5,2)-(9,4) cut by the right edge, no label."""
    img = np.full((8, 8, 3), 100, np.uint8)
    atlas = np.zeros((1, 2, 2), np.uint8)
    atlas[0] = [[255, 0], [128, 64]]
    items = {'rects': [[1, 3, 6, 7], [5, 2, 9, 4]], 'colors': [[200, 0, 0], [0, 0, 250]], 'text': [[0], []], 'mask_idx': [0, -1],
             'masks': np.ones((1, 2, 2), np.float32)}
    out = ref.render(img, items, atlas, mask_alpha=128, line_width=1)
    assert out.dtype == np.uint8 and out.shape == (8, 8, 3)
    assert out[0, 0].tolist() == [100, 100, 100]                                  # untouched
    assert out[5, 5].tolist() == [150, 50, 50]                                    # mask only: (100 * 128 + 200 * 128 + 128) >> 8
    assert out[3, 2].tolist() == [200, 0, 0]                                      # outline over the mask
    assert out[3, 5].tolist() == [0, 0, 250] and out[4, 6].tolist() == [0, 0, 250]      # the later outline wins over outline and mask
    # inside the blue rect's core (x 6 .. 8, y 3) nothing of it is drawn: the red outline and the source show
    assert out[2, 7].tolist() == [0, 0, 250] and out[3, 6].tolist() == [200, 0, 0] and out[3, 7].tolist() == [100, 100, 100]
    # the label box: x 1 .. 4, y 4 .. 7, over outline (x = 1) and mask: blend with 128 toward red
    assert out[4, 1].tolist() == [200, 0, 0]                                      # red toward red stays red
    assert out[4, 4].tolist() == [175, 25, 25]                                    # (150, 50, 50) toward (200, 0, 0)
    # glyph at (2, 5): coverage 255 -> a = 256 -> white; (3, 5): 0 -> unchanged; (2, 6): 128 -> a = 129; (3, 6): 64 -> a = 64
    assert out[5, 2].tolist() == [255, 255, 255] and out[5, 3].tolist() == [175, 25, 25]
    assert out[6, 2].tolist() == [(175 * 127 + 255 * 129 + 128) >> 8, (25 * 127 + 255 * 129 + 128) >> 8, (25 * 127 + 255 * 129 + 128) >> 8]
    assert out[6, 3].tolist() == [(175 * 192 + 255 * 64 + 128) >> 8, (25 * 192 + 255 * 64 + 128) >> 8, (25 * 192 + 255 * 64 + 128) >> 8]
    # a rect thinner than twice the line width is filled
    thin = ref.render(img, {'rects': [[2, 1, 5, 6]], 'colors': [[9, 9, 9]], 'text': [[]], 'mask_idx': [-1]}, None, line_width=2)
    assert (thin[1:7, 2:6] == 9).all() and (thin[:, :2] == 100).all() and (thin[0] == 100).all()
    # the tensor form clamps and truncates
    x = np.array([-300.7, -0.9, 0.9, 1.0, 254.99, 255.0, 300.0, 77.5], np.float32).reshape(1, 1, 8).repeat(3, axis=0)
    assert ref.from_tensor(x, (0.5, 0.0, -0.25))[0, :, 0].tolist() == [0, 0, 1, 1, 255, 255, 255, 78]
    assert ref.from_tensor(x, (0.5, 0.0, -0.25))[0, :, 2].tolist() == [0, 0, 0, 0, 254, 254, 255, 77]
