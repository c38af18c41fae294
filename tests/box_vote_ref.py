"""Box voting restated in plain numpy / Python, the statement the device operator is compared with bit
for bit, plus a second statement in Detectron's own words (np.average / np.mean) and the input sets both tests and the golden
script use.

    overlaps(top, all)           the float64 +1-pixel overlap of lib/bbox/bbox.pyx, operation for operation
    box_vote_ref(...)            the semantics: voters in ascending row index, sequential float64 sums, one divide, float32
    box_vote_detectron(...)      Detectron's box_utils.box_voting for 'ID' / 'AVG' / 'IOU_AVG'
    clustered(rs, ...)           the clustered generator;  problem_sets(tile, chunk)  the edge set;  golden_sets()  the recorded sets
"""
import numpy as np

METHODS = ('ID', 'AVG', 'IOU_AVG')
THRESHOLDS = (0.5, 0.8, 1.0)


def overlaps(top, alld):
    """bbox_overlaps_cython(top, all) of lib/bbox/bbox.pyx:17-57: float64 from the float32 coordinates, each product and sum
    rounded on its own.  -> (n_t, n_a) float64"""
    t = np.asarray(top, np.float32).reshape(-1, 5)[:, :4].astype(np.float64)[:, None, :]
    a = np.asarray(alld, np.float32).reshape(-1, 5)[:, :4].astype(np.float64)[None, :, :]
    box_area = (a[..., 2] - a[..., 0] + 1) * (a[..., 3] - a[..., 1] + 1)               # the query box
    iw = np.minimum(t[..., 2], a[..., 2]) - np.maximum(t[..., 0], a[..., 0]) + 1
    ih = np.minimum(t[..., 3], a[..., 3]) - np.maximum(t[..., 1], a[..., 1]) + 1
    with np.errstate(all='ignore'):           # element-wise float64: the same operations in the same order as the pyx loop
        ua = (t[..., 2] - t[..., 0] + 1) * (t[..., 3] - t[..., 1] + 1) + box_area - iw * ih
        iou = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), iou, 0.0)


def membership(top, alld, thresh, ov=None):
    """(n_t, n_a) bool: who votes for whom"""
    return (overlaps(top, alld) if ov is None else ov) >= thresh


def box_vote_ref(top, alld, thresh, method='ID', ov=None, member=None):
    """The semantics, one sequential float64 loop per kept row.  -> the voted (n_t, 5) float32 copy of `top`.  `ov`: overlaps
    computed before; `member`: the (n_t, n_a) vote sets to use in place of `ov >= thresh` (the golden ones)"""
    assert method in METHODS and 0.0 < thresh <= 1.0
    top = np.array(top, np.float32).reshape(-1, 5)
    alld = np.asarray(alld, np.float32).reshape(-1, 5)
    ov = overlaps(top, alld) if ov is None else ov
    member = (ov >= thresh) if member is None else np.asarray(member, bool)
    a64 = alld.astype(np.float64)
    for n in range(len(top)):
        den, num, wsum, wden, voters = 0.0, [0.0, 0.0, 0.0, 0.0], 0.0, 0.0, 0
        for k in range(len(alld)):                       # ascending row index: the order of every sum
            if member[n, k]:
                s = float(a64[k, 4])
                voters += 1
                den = den + s
                for c in range(4):
                    num[c] = num[c] + s * float(a64[k, c])            # (the product of two float32 is exact in float64)
                wsum = wsum + float(ov[n, k]) * s
                wden = wden + float(ov[n, k])
        if voters == 0 or not den > 0:
            continue
        for c in range(4):
            top[n, c] = np.float32(num[c] / den)
        if method == 'AVG':
            top[n, 4] = np.float32(den / voters)
        elif method == 'IOU_AVG':
            top[n, 4] = np.float32(wsum / wden)
    return top


def box_vote_detectron(top, alld, thresh, method='ID'):
    """Detectron's box_utils.box_voting, its np.average / np.mean calls kept (pairwise float64 sums, not sequential ones)"""
    top = np.array(top, np.float32).reshape(-1, 5)
    alld = np.asarray(alld, np.float32).reshape(-1, 5)
    out = top.copy()
    ov = overlaps(top, alld)
    all_boxes, all_scores = alld[:, :4].astype(np.float64), alld[:, 4].astype(np.float64)
    for k in range(len(top)):
        inds = np.where(ov[k] >= thresh)[0]
        if len(inds) == 0 or not all_scores[inds].sum() > 0:
            continue
        boxes_to_vote, ws = all_boxes[inds, :], all_scores[inds]
        out[k, :4] = np.average(boxes_to_vote, axis=0, weights=ws)
        if method == 'AVG':
            out[k, 4] = ws.mean()
        elif method == 'IOU_AVG':
            out[k, 4] = np.average(ws, weights=ov[k, inds])
    return out


def ulp_distance(a, b):
    """largest distance in float32 ulps between two float32 arrays of non-negative finite values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def clustered(rs, centres=12, field=400.0, lo=20.0, hi=120.0, most=9, jitter=0.04, origin=0.0):
    """One problem's pre-NMS rows: `centres` objects in a field x field area, sides uniform in lo .. hi, 1 .. most boxes per object,
    each coordinate jittered by N(0, jitter * side), scores uniform in [0.01, 1], rows permuted.  -> (n, 5) float32"""
    rows = []
    for _ in range(centres):
        w, h = rs.uniform(lo, hi, 2)
        x, y = rs.uniform(0, field - w), rs.uniform(0, field - h)
        for _ in range(rs.randint(1, most + 1)):
            d = rs.normal(0.0, 1.0, 4) * jitter * np.array([w, h, w, h])
            rows.append([x + d[0], y + d[1], x + w + d[2], y + h + d[3], rs.uniform(0.01, 1.0)])
    rows = np.asarray(rows, np.float64)
    if origin == 0.0:
        rows[:, :4] = np.maximum(rows[:, :4], 0.0)          # the sets with non-negative coordinates
    else:
        rows[:, :4] += origin
    return np.ascontiguousarray(rows[rs.permutation(len(rows))], np.float32)


def keep_some(rs, alld, frac=0.5):
    """A stand-in for the NMS: a random subset of the rows in a random order, scores decayed (post-NMS scores differ from the
    pre-NMS ones, and the vote must use the latter).  -> (n_t, 5) float32"""
    n = len(alld)
    n_t = int(round(n * frac)) if n else 0
    idx = rs.permutation(n)[:n_t]
    top = alld[idx].copy()
    top[:, 4] *= rs.uniform(0.3, 1.0, n_t).astype(np.float32)
    return top


def sized(rs, n_a, n_t):
    """a clustered problem of exactly n_a pre-NMS rows, of which n_t are kept"""
    parts, have = [], 0
    while have < n_a:
        parts.append(clustered(rs))
        have += len(parts[-1])
    alld = np.concatenate(parts)[:n_a] if n_a else np.zeros((0, 5), np.float32)
    top = alld[rs.permutation(n_a)[:n_t]].copy()
    top[:, 4] *= rs.uniform(0.3, 1.0, n_t).astype(np.float32)
    return top, alld


def problem_sets(tile, chunk):
    """The edge set: {name: (top (n_t, 5), all (n_a, 5))}, sizes taken from the kernel's own limits"""
    rs = np.random.RandomState(20)
    z = np.zeros((0, 5), np.float32)
    sets = {'n_a = 0': (z, z)}
    one = np.array([[10, 20, 50, 80, 0.7]], np.float32)
    sets['n_a = 1'] = (one * np.array([1, 1, 1, 1, 0.5], np.float32), one)
    sets['n_t = 0'] = (z, clustered(rs))
    for n_t in (tile - 1, tile, tile + 1):
        sets['n_t = %d' % n_t] = sized(rs, n_t + 7, n_t)
    for n_a in (chunk - 1, chunk, chunk + 1):
        # the kept rows include the last pre-NMS rows and their cluster mates: a voter on each side of the chunk boundary
        top, alld = sized(rs, n_a, 9)
        alld[n_a - 3:] = alld[chunk - 6:chunk - 3] + np.float32(0.25) * np.array([1, -1, 1, -1, 0], np.float32)
        top[:3] = alld[n_a - 3:]
        sets['n_a = %d' % n_a] = (top, alld)
    # exact IoU: [0,0,9,9] (100 px) vs [0,0,9,4] (50 px) = 0.5, vs [0,0,9,3] (40 px) = 0.4
    exact = np.array([[0, 0, 9, 9, 0.9], [0, 0, 9, 4, 0.6], [0, 0, 9, 3, 0.8]], np.float32)
    sets['IoU exactly 0.5'] = (exact[:1].copy(), exact)
    dup = np.repeat(np.array([[30.5, 40.25, 90.75, 120.5, 0.5]], np.float32), 5, 0)
    dup[:, 4] = [0.9, 0.3, 0.3, 0.7, 0.01]
    sets['duplicates'] = (dup[[0, 3]].copy(), dup)
    deg = np.array([[50, 50, 40, 90, 0.8], [45, 55, 85, 95, 0.6], [46, 56, 86, 96, 0.5]], np.float32)      # row 0: x2 < x1 - 1
    sets['degenerate'] = (deg[[0, 1]].copy(), deg)
    top, alld = sized(rs, 30, 12)
    alld[:, 4] = 0
    top[:, 4] = 0
    sets['zero scores'] = (top, alld)
    neg = clustered(rs, origin=-250.0)
    sets['negative coordinates'] = (keep_some(rs, neg), neg)
    return sets


def golden_inputs():
    """The sets the golden file records: 20 clustered problems with non-negative coordinates and 4 that straddle the origin,
    each with a kept subset.  -> list of (top, all)"""
    rs = np.random.RandomState(35)
    out = []
    for k in range(24):
        alld = clustered(rs, origin=0.0 if k < 20 else -200.0)
        out.append((keep_some(rs, alld, 0.4 + 0.1 * (k % 4)), alld))
    return out


def ragged_batch(n=40, seed=7):
    """`n` clustered problems, every fifth one empty and some with nothing kept.  -> list of (top, all)"""
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n):
        if k % 5 == 3:
            out.append((np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32)))
            continue
        alld = clustered(rs, centres=int(rs.randint(1, 13)), origin=0.0 if k % 2 else -100.0)
        out.append((keep_some(rs, alld, 0.0 if k % 7 == 6 else 0.5), alld))
    return out


def stack(problems):
    """list of (top, all) -> (top_rows, top_counts, all_rows, sizes) in the stacked layout; the rows of `top_rows` past a
    problem's count hold a stale pattern that must come back untouched"""
    sizes = np.array([len(a) for _, a in problems], np.int64)
    counts = np.array([len(t) for t, _ in problems], np.int32)
    total = int(sizes.sum())
    all_rows = np.concatenate([a for _, a in problems]).astype(np.float32) if total else np.zeros((0, 5), np.float32)
    top_rows = np.full((total, 5), -12345.0, np.float32)
    off = np.concatenate(([0], np.cumsum(sizes)))
    for q, (t, _) in enumerate(problems):
        top_rows[off[q]:off[q] + len(t)] = t
    return top_rows, counts, all_rows, sizes
