"""GPU: box voting inside Tester.aggregate (TEST.BBOX_VOTE): the device aggregation, the host statement and an independent
statement -- the NMS, then tests/box_vote_ref.py per (image, class) problem, then the MAX_PER_IMAGE rule -- agree bit for bit,
for soft and hard NMS; voting moves boxes; voting off is the aggregation as it was.  The fixture is the one of
tests/test_gpu_inference.py::test_device_aggregation_equals_the_host_statement with its boxes drawn in clusters, so that the
chips and scales of an image see the same objects and there is something to vote on."""
import numpy as np
import pytest
import torch

import box_vote_ref as R
from gpu_util import dev

pytestmark = pytest.mark.gpu

NC, N_IMG = 9, 7                                  # 8 foreground classes


def _fixture():
    from sniper_amd import inference
    rs = np.random.RandomState(3)
    centres = rs.uniform(0, 300, (N_IMG, NC - 1, 2, 2))                       # two objects per (image, class)
    sides = rs.uniform(12, 70, (N_IMG, NC - 1, 2, 2))
    dets = []
    for s_i in range(3):
        d = inference._Detections([[[] for _ in range(N_IMG)] for _ in range(NC)])
        for i in range(N_IMG):
            n_chips = 0 if (s_i == 2 and i == 4) else 1 + (i + s_i) % 3
            for j in range(NC):
                d[j][i] = [np.zeros((0, 5)) for _ in range(n_chips)]
            for c in range(n_chips):
                lens = rs.randint(0, 9, NC - 1) * (rs.rand(NC - 1) < 0.7)
                if i == 5:
                    lens = np.minimum(lens, 1) * (np.arange(NC - 1) < 3)           # an image that stays below the cap
                if (i + c) % 5 == 0:
                    lens[:] = 0                                                    # a chip without detections
                n = int(lens.sum())
                cls = np.repeat(np.arange(NC - 1), lens)
                obj = rs.randint(0, 2, n)
                xy, wh = centres[i, cls, obj], sides[i, cls, obj]
                jit = rs.normal(0.0, 0.03, (n, 4)) * np.hstack((wh, wh))
                sc = np.round(rs.uniform(0.01, 1.0, (n, 1)), 2 if i == 2 else 6)    # image 2: many tied scores
                big = np.ascontiguousarray(np.hstack((xy + jit[:, :2], xy + wh + jit[:, 2:], sc)), np.float64)
                ends = np.cumsum(lens)
                for j in range(1, NC):
                    d[j][i][c] = big[ends[j - 1] - lens[j - 1]:ends[j - 1]]
                d.compact[(i, c)] = (big, lens.astype(np.int64))
                cap = n + 5                                                        # (the device buffer is a capacity, not a count)
                dev_rows = torch.full((cap, 5), 7.0, dtype=torch.float64, device=dev())
                dev_rows[:n] = torch.from_numpy(big).to(dev())
                d.device_parts[(i, c)] = (dev_rows, torch.from_numpy(lens.astype(np.int32)).to(dev()))
        dets.append(d)
    return dets


def _tester(vote=None, hard=False):
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    cfg = cfgmod.res101_e2e_autofocus()
    cfg.TEST.VALID_RANGES = ((30, -1), (-1, 60), (10, 45))
    cfg.TEST.MAX_PER_IMAGE = 40
    if hard:
        cfg.TEST.NMS, cfg.TEST.NMS_SIGMA = 0.45, -1
    if vote is not None:
        cfg.TEST.BBOX_VOTE, cfg.TEST.BBOX_VOTE_TH, cfg.TEST.BBOX_VOTE_SCORING = True, vote[0], vote[1]

    class Imdb(object):
        num_classes, classes, name, result_path = NC, None, 'synthetic', None
    return inference.Tester(None, Imdb(), [{} for _ in range(N_IMG)], None, cfg=cfg, batch_size=2)


def _host(tester, dets):
    for d in dets:
        d.device_parts = {}
    return tester.aggregate(dets)


def _independent(tester, dets, vote):
    """aggregate_problems, the NMS, box_vote_ref per problem, cap_detections_per_image: the order of DESIGN.md section 35"""
    from sniper_amd import inference
    rows, sizes = inference.aggregate_problems(dets, tester.cfg.TEST.VALID_RANGES, N_IMG, NC, stacked=True)
    final = tester.nms_worker.nms_wrapper.process_stacked(rows, sizes)
    pre = inference._split_rows(np.asarray(rows, np.float32), sizes)
    stats = {'rows': 0, 'two': 0, 'moved': 0}
    if vote is not None:
        voted = []
        for t, a in zip(final, pre):
            ov = R.overlaps(t, a)
            voted.append(R.box_vote_ref(t, a, vote[0], vote[1], ov=ov))
            stats['rows'] += len(t)
            stats['two'] += int(((ov >= vote[0]).sum(1) >= 2).sum())
            stats['moved'] += int((voted[-1][:, :4] != np.asarray(t, np.float32).reshape(-1, 5)[:, :4]).sum())
        final = voted
    out = [[np.zeros((0, 5), np.float32) for _ in range(N_IMG)] for _ in range(NC)]
    nc = NC - 1
    for i in range(N_IMG):
        per = final[i * nc:(i + 1) * nc]
        kept = inference.cap_detections_per_image(per, tester.cfg.TEST.MAX_PER_IMAGE)
        for j in range(1, NC):
            out[j][i] = (kept if kept is not None else per)[j - 1]
    return out, stats


def _same(a, b):
    n = 0
    for i in range(N_IMG):
        for j in range(1, NC):
            x, y = np.asarray(a[j][i], np.float32).reshape(-1, 5), np.asarray(b[j][i], np.float32).reshape(-1, 5)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (i, j, x.shape, y.shape)
            n += len(x)
    return n


def _differs(a, b):
    return any(np.asarray(a[j][i], np.float32).reshape(-1, 5).tobytes() != np.asarray(b[j][i], np.float32).reshape(-1, 5).tobytes()
               for i in range(N_IMG) for j in range(1, NC))


@pytest.mark.parametrize('method', ['ID', 'AVG'])
def test_soft_nms_device_host_and_independent_statement_agree(method):
    vote = (0.8, method)
    tester = _tester(vote)
    assert tester._bbox_vote() == vote
    got = tester.aggregate_device(_fixture())
    assert got is not None
    want = _host(tester, _fixture())
    assert _same(got, want) > 100
    ind, stats = _independent(tester, _fixture(), vote)
    _same(got, ind)
    assert stats['moved'] > 0 and 2 * stats['two'] >= stats['rows'], stats           # there was something to vote on
    off = _tester(None)
    plain = off.aggregate_device(_fixture())
    assert _differs(got, plain)                                                      # at least one box differs from voting off
    capped = sum(sum(len(got[j][i]) for j in range(1, NC)) >= 40 for i in range(N_IMG))
    assert capped >= 3


@pytest.mark.parametrize('method', ['ID', 'AVG'])
def test_hard_nms_host_statement_votes_with_the_same_operator(method):
    vote = (0.8, method)
    tester = _tester(vote, hard=True)
    dets = _fixture()
    assert tester.aggregate_device(dets) is None                 # hard NMS: the host statement drives, the vote runs on the device
    got = tester.aggregate(dets)
    ind, stats = _independent(tester, _fixture(), vote)
    assert _same(got, ind) >= N_IMG and stats['moved'] > 0       # (hard NMS keeps about one row per object; every image has some)
    assert _differs(got, _tester(None, hard=True).aggregate(_fixture()))


def test_voting_off_is_the_aggregation_as_it_was(monkeypatch):
    from sniper_amd.ext import box_vote
    monkeypatch.delenv('SNIPER_BBOX_VOTE', raising=False)

    def refuse(*a, **k):
        raise AssertionError('voting is off: no call')
    monkeypatch.setattr(box_vote, 'box_vote_stacked', refuse)
    clones = []
    real_clone = torch.Tensor.clone
    monkeypatch.setattr(torch.Tensor, 'clone', lambda self, *a, **k: (clones.append(1), real_clone(self, *a, **k))[1])
    tester = _tester(None)
    assert tester._bbox_vote() is None
    got = tester.aggregate_device(_fixture())
    assert not clones                                             # and no copy of the rows
    want = _host(tester, _fixture())
    ind, _ = _independent(tester, _fixture(), None)
    assert _same(got, want) > 100 and _same(got, ind) > 100


def test_environment_variable_alone_turns_voting_on(monkeypatch):
    monkeypatch.setenv('SNIPER_BBOX_VOTE', '0.8:AVG')
    tester = _tester(None)
    assert tester.cfg.TEST.BBOX_VOTE is False and tester._bbox_vote() == (0.8, 'AVG')
    got = tester.aggregate_device(_fixture())
    monkeypatch.delenv('SNIPER_BBOX_VOTE')
    want = _tester((0.8, 'AVG')).aggregate_device(_fixture())
    assert _same(got, want) > 100
    assert _differs(got, _tester(None).aggregate_device(_fixture()))
