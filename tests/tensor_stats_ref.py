"""The per-tensor statistics (sn_tensor_stats, include/sniper_hip.h) restated in numpy: the record of one tensor, the header, the whole
(1 + T, 8) output, the default value mx.mon.Monitor prints, and the dict Module.skip_report returns.  The two float sums are taken
chunk by chunk and the chunk sums added in chunk order, as the device does; INSIDE a chunk the device's order (thread, wave, block) is
not restated -- with integer data every order is exact, with random data the tests use the bound of fp64 summation."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
RECORD = 8
FIELDS = ('sumsq', 'sum', 'nonfinite', 'first_index', 'max_abs', 'zeros', 'numel', 'reserved')


def record(x, chunk):
    """one tensor (fp16 or fp32, any shape) -> its eight doubles"""
    f = np.asarray(x).ravel().astype(np.float32)
    n = f.size
    finite = np.abs(f) <= np.float32(FLT_MAX)          # (NaN compares false)
    d = np.where(finite, f, np.float32(0)).astype(np.float64)
    sumsq = sum_ = 0.0
    for c0 in range(0, n, chunk):
        sumsq += float(np.sum(d[c0:c0 + chunk] * d[c0:c0 + chunk]))
        sum_ += float(np.sum(d[c0:c0 + chunk]))
    bad = int(n - np.count_nonzero(finite))
    first = int(np.argmin(finite)) if bad else -1
    maxabs = float(np.max(np.abs(d))) if n else 0.0
    zeros = int(np.count_nonzero(f == 0))
    return np.array([sumsq, sum_, bad, first, maxabs, zeros, n, 0.0], np.float64)


def stats(arena, segs, chunk, step=0.0):
    """arena: 1-D array; segs: [(off, n), ...] -> the (1 + T, 8) output of one launch pair that wrote"""
    arena = np.asarray(arena)
    out = np.zeros((1 + len(segs), RECORD), np.float64)
    for t, (off, n) in enumerate(segs):
        out[1 + t] = record(arena[off:off + n], chunk)
    bad = np.flatnonzero(out[1:, 2] > 0)
    out[0] = [1.0, float(step), len(segs), bad.size, float(bad[0]) if bad.size else -1.0, 0.0, 0.0, 0.0]
    return out


def monitor_value(rec):
    """MXNet's default stat_func norm(x) / sqrt(x.size) from a record: nan for a tensor with a non-finite element (its norm), and for an
    empty one (0 / 0)"""
    if rec[2] > 0 or rec[6] == 0:
        return float('nan')
    return float(np.sqrt(rec[0]) / np.sqrt(rec[6]))


def report(out, names):
    """the (1 + T, 8) report buffer -> what Module.skip_report returns: None before the first skipped step"""
    out = np.asarray(out)
    if out[0, 0] != 1.0:
        return None
    tensors = []
    for name, r in zip(names, out[1:]):
        if r[2] > 0:
            tensors.append({'name': name, 'nonfinite': int(r[2]), 'first_index': int(r[3]), 'max_abs': float(r[4]),
                            'norm': float(np.sqrt(r[0])), 'zeros': int(r[5]), 'numel': int(r[6])})
    return {'step': int(out[0, 1]), 'tensors': tensors}
