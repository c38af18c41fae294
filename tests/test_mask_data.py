"""CPU: the mask branch's polygon plumbing (sniper_amd/data/mask_utils.py) against the REFERENCE's anchor_worker output
(tests/golden/mask_polys_v1.npz, made by tests/golden/make_mask_golden.py) and against lib/data_utils/mask_utils.py
directly (tests/golden/mask_utils_v1.npz, made by tests/golden/make_mask_utils_golden.py)."""
import os
import sys

import numpy as np

from golden_util import anchor_case, golden
from sniper_amd.data import mask_utils
from sniper_amd.synthetic import make_roidb

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_mask_utils_golden import ENCODINGS, cases  # noqa: E402


def test_encoded_polys_match_reference_anchor_worker():
    z = np.load(os.path.join(HERE, 'golden', 'mask_polys_v1.npz'))
    g = golden()
    roidb = make_roidb(6, seed=5, n_proposals=300, with_masks=True)
    plain = make_roidb(6, seed=5, n_proposals=300)
    assert all(np.array_equal(a['boxes'], b['boxes']) for a, b in zip(roidb, plain))      # polygons come from a separate stream
    n = int(z['count'])
    rows = trunc = 0
    for k in range(n):
        args, _, _ = anchor_case(k)
        i = int(g['anchor_%02d_src' % k][0])
        enc = mask_utils.encode_chip_masks(args[0], args[1], args[2], args[5], args[7], roidb[i]['gt_masks'])
        want = z['enc_%02d' % k]
        assert enc.dtype == np.float32 and np.array_equal(enc, want), k
        ids, boxes = mask_utils.kept_gt(args[0], args[1], args[2], args[5])
        gt = z['gt_%02d' % k]
        assert int((gt[:, 4] >= 0).sum()) == len(ids) and np.array_equal(gt[:len(ids), :4], boxes[ids])
        rows += len(ids)
        trunc += int((want[:len(ids), 1] < np.array([len(roidb[i]['gt_masks'][j]) for j in ids])).sum())
    assert rows > 150 and trunc > 0          # the 500-float budget truncated some objects


def test_crop_and_encode_match_reference_mask_utils():
    """lib/data_utils/mask_utils.py's crop_polys / poly_encoder on seeded polygons (tests/golden/mask_utils_v1.npz)."""
    z = np.load(os.path.join(HERE, 'golden', 'mask_utils_v1.npz'))
    for i, (polys, crop, scale, cats) in enumerate(cases()):
        b = mask_utils.crop_polys(polys, crop, scale)
        assert [len(p) for p in b] == z['nseg_%d' % i].tolist()
        for j, p in enumerate(b):
            for k, y in enumerate(p):
                x = z['crop_%d_%d_%d' % (i, j, k)]
                assert np.array_equal(x, y) and x.dtype == y.dtype, (i, j, k)
        for mlen, mg in ENCODINGS:
            assert np.array_equal(z['enc_%d_%d_%d' % (i, mlen, mg)], mask_utils.poly_encoder(b, cats, mlen, mg))
