"""Generate tests/golden/mask_utils_v1.npz from the REFERENCE's own lib/data_utils/mask_utils.py (build container only):
`crop_polys` and `poly_encoder` on the seeded polygon cases of `cases()` (synthetic COCO-style polygons of
sniper_amd.synthetic.make_roidb, random crops, scales and categories), every output array with its dtype.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mask_utils_golden.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mask_utils_v1.npz')
ENCODINGS = ((500, 100), (60, 3))        # (max_poly_len, max_n_gts) of poly_encoder


def cases():
    """(polygons, crop, scale, categories) per synthetic image."""
    from sniper_amd.synthetic import make_roidb
    rs = np.random.RandomState(3)
    for r in make_roidb(4, seed=9, with_masks=True):
        polys = r['gt_masks']
        crop, scale = [float(rs.uniform(0, 100)), float(rs.uniform(0, 100)), 0, 0], float(rs.uniform(0.5, 3))
        yield polys, crop, scale, rs.randint(0, 80, len(polys))


def main():
    sys.path.insert(0, ROOT)
    from oracle.build import REF
    sys.path.insert(0, os.path.join(REF, 'lib', 'data_utils'))
    sys.dont_write_bytecode = True
    ref = importlib.import_module('mask_utils')
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(REF))
    out = {}
    for i, (polys, crop, scale, cats) in enumerate(cases()):
        cropped = ref.crop_polys(polys, crop, scale)
        out['nseg_%d' % i] = np.array([len(p) for p in cropped], np.int64)
        for j, p in enumerate(cropped):
            for k, seg in enumerate(p):
                out['crop_%d_%d_%d' % (i, j, k)] = seg
        for mlen, mg in ENCODINGS:
            out['enc_%d_%d_%d' % (i, mlen, mg)] = ref.poly_encoder(cropped, cats, mlen, mg)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
