"""CPU: the epoch order of the three iterator mirrors (sniper_amd/iterators: `orientation_order` and the `reset` methods built on it)
against the reference's own `reset` bodies (MNIteratorBase.py:59-82, MNIteratorTest.py:52-65, MNIteratorTestAutoFocus.py:96-134)
under the same numpy seed.  The reference's results are the golden tests/golden/iterator_order_v1.json, generated from the
reference itself by tests/golden/make_iterator_golden.py on the same seeded roidbs."""
import copy
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_iterator_golden import (AUTOFOCUS_CASES, TEST_CASES, TRAIN_CASES, TRAIN_SEEDS, case_key, load,  # noqa: E402
                                  roidb, train_key)


@pytest.fixture(scope='module')
def golden():
    return load()


@pytest.mark.parametrize('n,bs,single', TRAIN_CASES)
def test_training_order_equals_the_reference_reset(golden, n, bs, single):
    from sniper_amd.iterators.MNIteratorBase import MNIteratorBase
    rdb = roidb(np.random.RandomState(n + bs), n)
    b = types.SimpleNamespace(roidb=rdb, batch_size=bs, single_size_change=single)
    b._set_order = lambda order: MNIteratorBase._set_order(b, order)
    for seed in TRAIN_SEEDS:
        want = golden['train'][train_key(n, bs, single, seed)]
        np.random.seed(seed)
        MNIteratorBase.reset(b)
        assert np.array_equal(b.inds, want['inds']) and b.size == want['size'] and b.cur_i == 0
        assert np.random.randint(1 << 30) == want['next_draw']   # same number of draws


@pytest.mark.parametrize('n,bs', TEST_CASES)
def test_single_scale_test_order_equals_the_reference_reset(golden, n, bs):
    from sniper_amd.iterators.MNIteratorBase import orientation_order
    rdb = roidb(np.random.RandomState(n), n)
    ours = orientation_order([r['width'] for r in rdb], [r['height'] for r in rdb], bs, 'first')
    assert np.array_equal(golden['test'][case_key(n, bs)]['inds'], ours)


@pytest.mark.parametrize('n,bs', AUTOFOCUS_CASES)
def test_autofocus_order_and_chip_maps_equal_the_reference_reset(golden, n, bs):
    from sniper_amd.iterators.MNIteratorBase import MNIteratorBase
    from sniper_amd.iterators.MNIteratorTestAutoFocus import MNIteratorTestAutoFocus
    want = golden['autofocus'][case_key(n, bs)]
    rdb = copy.deepcopy(roidb(np.random.RandomState(n), n, crops=True))
    b = types.SimpleNamespace(roidb=rdb, batch_size=bs)
    b._set_order = lambda order: MNIteratorBase._set_order(b, order)
    MNIteratorTestAutoFocus.reset(b)
    assert np.array_equal(b.inds, want['inds']) and b.size == want['size']
    assert sorted([k, v] for k, v in b.crop2im.items()) == want['crop2im']
    assert [sorted([k, v] for k, v in r['crop_mapping'].items()) for r in rdb] == want['crop_mapping']
