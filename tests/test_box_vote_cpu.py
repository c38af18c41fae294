"""CPU: the restatement of box voting (tests/box_vote_ref.py) against the vote sets the reference's own compiled
bbox_overlaps_cython gave (tests/golden/boxvote_v1.npz), against Detectron's statement of the same operator, and the switch that
turns voting on: config keys, SNIPER_BBOX_VOTE, precedence, refusals.  No kernel is launched here."""
import os

import numpy as np
import pytest

import box_vote_ref as R
from sniper_amd.ext import box_vote as BV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'boxvote_v1.npz')


def golden_sets():
    """-> list of (top, all, {thresh: (n_t, n_a) bool}, nonneg)"""
    g = np.load(GOLDEN)
    a_off = np.concatenate(([0], np.cumsum(g['all_sizes'])))
    t_off = np.concatenate(([0], np.cumsum(g['top_sizes'])))
    cells = g['top_sizes'].astype(np.int64) * g['all_sizes']
    c_off = np.concatenate(([0], np.cumsum(cells)))
    bits = {t: np.unpackbits(g['member_%d' % round(100 * t)])[:c_off[-1]].astype(bool) for t in R.THRESHOLDS}
    out = []
    for k in range(len(cells)):
        n_t, n_a = int(g['top_sizes'][k]), int(g['all_sizes'][k])
        member = {t: bits[t][c_off[k]:c_off[k + 1]].reshape(n_t, n_a) for t in R.THRESHOLDS}
        out.append((g['top_rows'][t_off[k]:t_off[k + 1]], g['all_rows'][a_off[k]:a_off[k + 1]], member, bool(g['nonneg'][k])))
    return out


def test_golden_inputs_are_the_generators():
    sets = golden_sets()
    want = R.golden_inputs()
    assert len(sets) == len(want) + 3
    for (top, alld, _, _), (wt, wa) in zip(sets, want):
        assert np.array_equal(top, wt) and np.array_equal(alld, wa)
    assert sum(nn for _, _, _, nn in sets[:len(want)]) == 20


def test_restated_overlap_gives_the_reference_vote_sets():
    rows = two = 0
    for top, alld, member, _ in golden_sets():
        ov = R.overlaps(top, alld)
        for t in R.THRESHOLDS:
            assert np.array_equal(ov >= t, member[t]), t
        rows += len(top)
        two += int((member[0.8].sum(1) >= 2).sum())
    assert 2 * two >= rows > 700            # a set where nobody votes shows nothing


@pytest.mark.parametrize('method', R.METHODS)
def test_restatement_agrees_with_detectrons_statement(method):
    """Sequential float64 sums against np.average's: with non-negative terms only, both carry a relative error of about
    n * 2^-53, so the float32 roundings can differ only at a rounding boundary -- at most 1 float32 ulp."""
    worst = moved = 0
    for top, alld, _, nonneg in golden_sets():
        if not nonneg:
            continue
        for t in R.THRESHOLDS:
            mine, theirs = R.box_vote_ref(top, alld, t, method), R.box_vote_detectron(top, alld, t, method)
            worst = max(worst, R.ulp_distance(mine, theirs))
            moved += int((mine[:, :4] != top[:, :4]).sum())
            if method == 'ID':
                assert np.array_equal(mine[:, 4], top[:, 4])
    print('largest distance: %d ulp' % worst)
    assert worst <= 1 and moved > 0


def test_exact_half_votes_and_forty_percent_does_not():
    top, alld = R.problem_sets(64, 128)['IoU exactly 0.5']
    ov = R.overlaps(top, alld)
    assert ov[0, 1] == 0.5 and ov[0, 2] == 0.4
    got = R.box_vote_ref(top, alld, 0.5, 'AVG')
    assert got[0, 4] == np.float32((np.float64(np.float32(0.9)) + np.float64(np.float32(0.6))) / 2)
    assert got[0, 3] == np.float32((np.float64(np.float32(0.9)) * 9 + np.float64(np.float32(0.6)) * 4) / (np.float64(np.float32(0.9)) + np.float64(np.float32(0.6))))
    assert np.array_equal(R.box_vote_ref(top, alld, 0.51, 'AVG')[:, :4], top[:, :4])        # alone, a box votes for itself


def test_tile_table_covers_every_pre_nms_row_once():
    tab = BV.tile_table([0, 1, 64, 65, 0, 130], tile=64)
    assert tab.dtype == np.int32 and tab.tolist() == [[1, 0], [2, 0], [3, 0], [3, 64], [5, 0], [5, 64], [5, 128]]
    assert BV.tile_table([], tile=64).shape == (0, 2) and BV.tile_table([0, 0], tile=64).shape == (0, 2)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def test_switch_is_off_by_default_and_read_from_the_config():
    from sniper_amd import config as cfgmod
    cfg = cfgmod.res101_e2e()
    assert cfg.TEST.BBOX_VOTE is False and cfg.TEST.BBOX_VOTE_TH == 0.8 and cfg.TEST.BBOX_VOTE_SCORING == 'ID'
    assert BV.vote_options(cfg.TEST, environ={}) is None
    cfg.TEST.BBOX_VOTE = True
    assert BV.vote_options(cfg.TEST, environ={}) == (0.8, 'ID')
    cfg.TEST.BBOX_VOTE_TH, cfg.TEST.BBOX_VOTE_SCORING = 0.5, 'IOU_AVG'
    assert BV.vote_options(cfg.TEST, environ={}) == (0.5, 'IOU_AVG')
    # a config object without the keys (the reference's own): off, and the defaults once BBOX_VOTE alone is set
    assert BV.vote_options(_Cfg(NMS=-1), environ={}) is None
    assert BV.vote_options(_Cfg(BBOX_VOTE=True), environ={}) == (0.8, 'ID')

    class Plain(object):            # attribute access only
        BBOX_VOTE, BBOX_VOTE_TH = True, 0.75
    assert BV.vote_options(Plain(), environ={}) == (0.75, 'ID')


def test_environment_spelling_and_precedence():
    off = _Cfg(NMS=-1)
    assert BV.vote_options(off, environ={'SNIPER_BBOX_VOTE': '0.8'}) == (0.8, 'ID')
    assert BV.vote_options(off, environ={'SNIPER_BBOX_VOTE': ' 0.65:AVG '}) == (0.65, 'AVG')
    assert BV.vote_options(off, environ={'SNIPER_BBOX_VOTE': '1:IOU_AVG'}) == (1.0, 'IOU_AVG')
    assert BV.vote_options(off, environ={'SNIPER_BBOX_VOTE': ''}) is None
    assert BV.vote_options(_Cfg(BBOX_VOTE=False), environ={'SNIPER_BBOX_VOTE': '0.7:AVG'}) == (0.7, 'AVG')
    # the config key wins over the variable
    on = _Cfg(BBOX_VOTE=True, BBOX_VOTE_TH=0.9, BBOX_VOTE_SCORING='AVG')
    assert BV.vote_options(on, environ={'SNIPER_BBOX_VOTE': '0.5:ID'}) == (0.9, 'AVG')
    assert BV.vote_options(on, environ={'SNIPER_BBOX_VOTE': 'nonsense'}) == (0.9, 'AVG')


@pytest.mark.parametrize('value,words', [
    ('abc', ('SNIPER_BBOX_VOTE', '<thresh>[:<method>]')),
    ('0', ('SNIPER_BBOX_VOTE', '(0, 1]')),
    ('1.01', ('SNIPER_BBOX_VOTE', '(0, 1]')),
    ('-0.5:AVG', ('SNIPER_BBOX_VOTE', '(0, 1]')),
    ('nan', ('SNIPER_BBOX_VOTE', '(0, 1]')),
    ('0.8:MEDIAN', ('SNIPER_BBOX_VOTE', 'unknown scoring method', 'MEDIAN')),
    ('0.8:', ('SNIPER_BBOX_VOTE', 'unknown scoring method')),
    ('0.8:TEMP_AVG', ('SNIPER_BBOX_VOTE', 'TEMP_AVG', 'exp / pow')),
])
def test_environment_refusals(value, words):
    with pytest.raises((ValueError, NotImplementedError)) as e:
        BV.vote_options(_Cfg(), environ={'SNIPER_BBOX_VOTE': value})
    assert all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.parametrize('name', BV.UNPINNED)
def test_transcendental_scoring_methods_are_refused_by_name(name):
    with pytest.raises(NotImplementedError) as e:
        BV.method_id(name)
    assert name in str(e.value)
    with pytest.raises(NotImplementedError):
        BV.vote_options(_Cfg(BBOX_VOTE=True, BBOX_VOTE_SCORING=name), environ={})
    with pytest.raises(NotImplementedError):
        BV.box_voting(np.zeros((1, 5), np.float32), np.zeros((1, 5), np.float32), 0.8, name)


@pytest.mark.parametrize('thresh', [0, 0.0, -0.1, 1.0000001, 2, float('nan'), float('inf'), None, 'x'])
def test_thresholds_outside_the_half_open_interval_are_refused(thresh):
    with pytest.raises(ValueError):
        BV.check_thresh(thresh)
    with pytest.raises(ValueError):
        BV.vote_options(_Cfg(BBOX_VOTE=True, BBOX_VOTE_TH=thresh), environ={})
    with pytest.raises(ValueError):
        BV.box_voting(np.zeros((1, 5), np.float32), np.zeros((1, 5), np.float32), thresh)
    assert BV.check_thresh(1) == 1.0 and BV.check_thresh(1e-9) == 1e-9


def test_tester_reads_the_switch_once():
    from sniper_amd import config as cfgmod
    from sniper_amd import inference

    class Imdb(object):
        num_classes, classes, name, result_path = 3, None, 'synthetic', None
    cfg = cfgmod.res101_e2e()
    old = os.environ.pop('SNIPER_BBOX_VOTE', None)
    try:
        t = inference.Tester(None, Imdb(), [{}], None, cfg=cfg, batch_size=1)
        assert t._bbox_vote() is None
        cfg.TEST.BBOX_VOTE = True                         # read once: a Tester keeps what it was built with
        assert t._bbox_vote() is None
        assert inference.Tester(None, Imdb(), [{}], None, cfg=cfg, batch_size=1)._bbox_vote() == (0.8, 'ID')
        cfg.TEST.BBOX_VOTE_SCORING = 'QUASI_SUM'
        with pytest.raises(NotImplementedError):
            inference.Tester(None, Imdb(), [{}], None, cfg=cfg, batch_size=1)._bbox_vote()
    finally:
        if old is not None:
            os.environ['SNIPER_BBOX_VOTE'] = old
