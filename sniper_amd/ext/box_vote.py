"""Box voting after the test-time NMS (TEST.BBOX_VOTE), modelled on Detectron's `box_utils.box_voting`:
every box the NMS kept becomes the score-weighted mean of all pre-NMS boxes of its (image, class) problem that overlap it by at
least `thresh`.  One `sn_box_vote` launch (sniper_amd/csrc/box_vote.hip) serves every problem of a pass; float64 sums in a fixed
order, so the result is the same bits every run and equals the sequential restatement (tests/box_vote_ref.py)."""
import ctypes
import os

import numpy as np

METHODS = {'ID': 0, 'AVG': 1, 'IOU_AVG': 2}
# Detectron's other scoring methods need exp / pow, which no two libraries round alike: refused, not approximated
UNPINNED = ('TEMP_AVG', 'GENERALIZED_AVG', 'QUASI_SUM')
ENV = 'SNIPER_BBOX_VOTE'


def method_id(scoring_method):
    if scoring_method in UNPINNED:
        raise NotImplementedError('box voting: scoring method %r needs exp / pow and cannot be reproduced bit for bit; '
                                  'use one of %s' % (scoring_method, sorted(METHODS)))
    if scoring_method not in METHODS:
        raise ValueError('box voting: unknown scoring method %r (known: %s)' % (scoring_method, sorted(METHODS)))
    return METHODS[scoring_method]


def check_thresh(thresh):
    try:
        t = float(thresh)
    except (TypeError, ValueError):
        raise ValueError('box voting: the threshold must be a number in (0, 1], got %r' % (thresh,))
    if not (0.0 < t <= 1.0):           # (NaN fails both comparisons)
        raise ValueError('box voting: the threshold must lie in (0, 1], got %r' % (thresh,))
    return t


def limits():
    """sn_box_vote_limits -> {'tile': kept rows per workgroup, 'chunk': pre-NMS rows per LDS chunk}; needs no device"""
    from .._lib import lib
    out = (ctypes.c_int32 * 2)()
    lib().call('sn_box_vote_limits', out)
    return {'tile': int(out[0]), 'chunk': int(out[1])}


def tile_table(sizes, tile=None):
    """(n_tiles, 2) int32 {problem, first kept row}: one entry per `tile` rows of every problem's PRE-NMS size -- an upper bound of
    what the NMS keeps, and known on the host, so the launch needs no read of the post-NMS counts"""
    tile = tile or limits()['tile']
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    per = -(-sizes // tile)
    q = np.repeat(np.arange(len(sizes), dtype=np.int64), per)
    first = (np.arange(len(q), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)) * tile
    return np.ascontiguousarray(np.stack((q, first), 1), np.int32)


def parse_env(value):
    """'<thresh>[:<method>]' of SNIPER_BBOX_VOTE -> (thresh, method name)"""
    text = value.strip()
    head, sep, tail = text.partition(':')
    try:
        thresh = float(head)
    except ValueError:
        raise ValueError('%s=%r: expected <thresh>[:<method>], e.g. 0.8 or 0.8:AVG' % (ENV, value))
    method = tail.strip() if sep else 'ID'
    try:
        method_id(method)
        return check_thresh(thresh), method
    except (ValueError, NotImplementedError) as e:
        raise type(e)('%s=%r: %s' % (ENV, value, e))


def vote_options(test_cfg, environ=None):
    """The voting switch of a Tester -> None (off) or (thresh, method name).  TEST.BBOX_VOTE / BBOX_VOTE_TH / BBOX_VOTE_SCORING
    when the config turns it on; otherwise SNIPER_BBOX_VOTE=<thresh>[:<method>] (the reference's own config object rejects
    unknown keys, so its unchanged main_test.py reaches the switch through the environment).  The config wins over the variable."""
    environ = os.environ if environ is None else environ
    get = test_cfg.get if hasattr(test_cfg, 'get') else (lambda k, d=None: getattr(test_cfg, k, d))
    if get('BBOX_VOTE', False):
        method = get('BBOX_VOTE_SCORING', 'ID')
        method_id(method)
        return check_thresh(get('BBOX_VOTE_TH', 0.8)), method
    value = environ.get(ENV)
    if value is None or not value.strip():
        return None
    return parse_env(value)


def box_vote_stacked(top_rows, top_counts, all_rows, sizes, thresh, scoring_method='ID', d_off=None):
    """Vote on P stacked problems.  Problem q owns `sizes[q]` rows of both (total, 5) float32 arrays, back to back: `all_rows`
    the rows handed to the NMS, `top_rows` what it left in place, of which the first `top_counts[q]` rows are the kept boxes.
    `sizes` is a host array (the caller built the problems from it).  Device tensors are voted IN PLACE and never leave HBM
    (`top_rows` is returned; `d_off` may pass the int32 offsets already on the device); numpy arrays are uploaded, and the voted
    copy of `top_rows` comes back."""
    import torch

    from .. import hip
    method, thresh = method_id(scoring_method), check_thresh(thresh)
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    P, total = len(sizes), int(sizes.sum())
    on_device = isinstance(top_rows, torch.Tensor)
    if on_device:
        if not (isinstance(all_rows, torch.Tensor) and isinstance(top_counts, torch.Tensor)):
            raise TypeError('box_vote_stacked: device top_rows need device all_rows and top_counts')
        if top_rows.dtype != torch.float32 or all_rows.dtype != torch.float32 or top_counts.dtype != torch.int32:
            raise TypeError('box_vote_stacked: rows must be float32 and top_counts int32 on the device')
        if not (top_rows.is_contiguous() and all_rows.is_contiguous() and top_counts.is_contiguous()):
            raise ValueError('box_vote_stacked: device arrays must be contiguous')
        d_top, d_all, d_cnt = top_rows, all_rows, top_counts
    else:
        top_rows = np.ascontiguousarray(top_rows, np.float32).reshape(-1, 5)
        all_rows = np.ascontiguousarray(all_rows, np.float32).reshape(-1, 5)
        top_counts = np.ascontiguousarray(top_counts, np.int32).reshape(-1)
    if tuple(top_rows.shape) != (total, 5) or tuple(all_rows.shape) != (total, 5) or int(top_counts.numel() if on_device else top_counts.size) != P:
        raise ValueError('box_vote_stacked: %d problems of %d rows need (%d, 5) rows twice and %d counts' % (P, total, total, P))
    assert total < 2 ** 31
    if P == 0 or total == 0:
        return top_rows if on_device else top_rows.copy()
    if not on_device:
        d_top, d_all, d_cnt = hip.dev(top_rows), hip.dev(all_rows), hip.dev(top_counts)
    if d_off is None:
        off = np.zeros(P + 1, np.int32)
        off[1:] = np.cumsum(sizes)
        d_off = hip.dev(off, device=d_top.device)
    tiles = tile_table(sizes)
    d_tiles = hip.dev(tiles, device=d_top.device)
    hip.call('sn_box_vote', d_top, d_all, d_off, d_cnt, d_tiles, len(tiles), P, thresh, method, hip.stream())
    return d_top if on_device else d_top.cpu().numpy()


def box_voting(top_dets, all_dets, thresh, scoring_method='ID', beta=1.0):
    """Detectron's `box_utils.box_voting` for one problem, numpy in and out: `top_dets` (n_t, 5) are the boxes the NMS kept (a
    subset of `all_dets` by coordinates, at most as many), `all_dets` (n_a, 5) the boxes it was handed.  -> the voted copy of
    `top_dets`, float32.  `beta` only parametrises the scoring methods that are refused here."""
    top = np.ascontiguousarray(top_dets, np.float32).reshape(-1, 5)
    alld = np.ascontiguousarray(all_dets, np.float32).reshape(-1, 5)
    n_t, n_a = len(top), len(alld)
    if n_t > n_a:
        raise ValueError('box_voting: %d kept boxes out of %d: the kept boxes are a subset of all_dets' % (n_t, n_a))
    method_id(scoring_method), check_thresh(thresh)
    if n_t == 0:
        return top.copy()
    rows = np.zeros((n_a, 5), np.float32)
    rows[:n_t] = top
    return box_vote_stacked(rows, [n_t], alld, [n_a], thresh, scoring_method)[:n_t]
