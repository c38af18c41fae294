"""Generate tests/golden/iterator_order_v1.json from the REFERENCE's own iterator `reset` bodies (build container only): the
lib2to3 translation oracle/build.py makes of lib/iterators (oracle/_ref/py3; MNIteratorBase.py:59-82, MNIteratorTest.py:52-65,
MNIteratorTestAutoFocus.py:96-134), each `reset` compiled alone and run on stub objects over the seeded roidbs of `roidb()`
for every case tests/test_iterator_order.py checks.  Records the epoch order and, for training, the next numpy draw after
`reset` (the number of draws it made).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_iterator_golden.py
"""
import ast
import copy
import json
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, 'oracle', '_ref', 'py3', 'lib')
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'iterator_order_v1.json')

TRAIN_CASES = [(37, 4, False), (37, 4, True), (16, 8, False), (5, 4, False), (64, 20, False)]
TRAIN_SEEDS = (0, 3)
TEST_CASES = [(37, 4), (9, 8), (3, 4)]
AUTOFOCUS_CASES = [(23, 4), (9, 8), (40, 2)]


def roidb(rs, n, crops=False):
    out = []
    for _ in range(n):
        w, h = int(rs.randint(200, 700)), int(rs.randint(200, 700))
        r = {'width': w, 'height': h}
        if crops:
            k = int(rs.randint(0, 4))
            x1, y1 = rs.randint(0, 100, k), rs.randint(0, 100, k)
            r['inference_crops'] = np.stack([x1, y1, x1 + rs.randint(50, 300, k), y1 + rs.randint(50, 300, k)], 1).astype(np.float64)
        out.append(r)
    return out


def train_key(n, bs, single, seed):
    return '%d_%d_%d_%d' % (n, bs, int(single), seed)


def case_key(n, bs):
    return '%d_%d' % (n, bs)


def load():
    with open(OUT) as fh:
        return json.load(fh)


def _ref_reset(mod, cls):
    """The class's `reset`, compiled ALONE from the translated file (the module's import chain reaches mxnet, cv2 and the
    compiled extensions; `reset` itself is numpy only)."""
    path = os.path.join(REF, 'iterators', mod + '.py')
    tree = ast.parse(open(path).read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    fn = next(n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name == 'reset')
    ns = {'np': np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, 'exec'), ns)
    return ns['reset']


def main():
    out = {'train': {}, 'test': {}, 'autofocus': {}}
    reset = _ref_reset('MNIteratorBase', 'MNIteratorBase')
    for n, bs, single in TRAIN_CASES:
        rdb = roidb(np.random.RandomState(n + bs), n)
        for seed in TRAIN_SEEDS:
            a = types.SimpleNamespace(roidb=rdb, batch_size=bs, single_size_change=single)
            np.random.seed(seed)
            reset(a)
            out['train'][train_key(n, bs, single, seed)] = {'inds': a.inds.tolist(), 'size': int(a.size),
                                                            'next_draw': int(np.random.randint(1 << 30))}
    reset = _ref_reset('MNIteratorTest', 'MNIteratorTest')
    for n, bs in TEST_CASES:
        a = types.SimpleNamespace(roidb=roidb(np.random.RandomState(n), n), batch_size=bs)
        reset(a)
        out['test'][case_key(n, bs)] = {'inds': a.inds.tolist()}
    reset = _ref_reset('MNIteratorTestAutoFocus', 'MNIteratorTestAutoFocus')
    for n, bs in AUTOFOCUS_CASES:
        rdb = copy.deepcopy(roidb(np.random.RandomState(n), n, crops=True))
        a = types.SimpleNamespace(roidb=rdb, batch_size=bs)
        reset(a)
        out['autofocus'][case_key(n, bs)] = {
            'inds': a.inds.tolist(), 'size': int(a.size), 'crop2im': sorted([int(k), int(v)] for k, v in a.crop2im.items()),
            'crop_mapping': [sorted([int(k), int(v)] for k, v in r['crop_mapping'].items()) for r in rdb]}
    with open(OUT, 'w') as fh:
        json.dump(out, fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
