"""``mx.mon.Monitor``: per-tensor statistics of a training run, every `interval`-th batch.

The fork's monitor source is not in the tree, so the semantics here are this project's, modelled on MXNet's (DESIGN.md "Per-tensor
statistics"):

* ``tic()`` starts a batch and arms every `interval`-th one (the first included); ``toc()`` on an armed batch returns
  ``[(step, name, str(value)), ...]`` and disarms, on any other batch ``[]``; ``toc_print()`` logs the rows as
  ``Batch: {:7d} {:30s} {:s}``.  `step` counts ``tic()`` calls, the first batch being 1, as in MXNet.
* Names: ``<param>`` (the fp32 master), ``<param>_grad``, ``<param>_mom``, ``<output>_output`` for the symbol's heads -- those the
  regular expression `pattern` matches at their start (``re.match``).  Order: the masters in arena order, then the gradients, then the
  momenta, then the heads; ``sort=True`` sorts by name.  Only trainable parameters have a gradient and a momentum, and only they are
  listed.
* ``stat_func=None``: the value is MXNet's default ``norm(x) / sqrt(x.size)``, from field 0 of the tensor's record
  (``sn_tensor_stats``): all matching tensors of an arena in ONE launch pair per arena, each head through a one-segment table, and the
  host waits only for the download of those records, only on armed batches.  A tensor with a non-finite element gives ``nan`` --
  which is what its norm is.  A batch that is not armed issues no launch at all.
* With a `stat_func` (a callable on an ``NDArray``) the slow path runs, as in MXNet: the function is called once per matching tensor on
  an ``NDArray`` view of it and whatever it returns is converted with ``asnumpy()`` -- hundreds of small launches and downloads on an
  armed batch of a large network.
* Gradients are the raw arena values: with a static or dynamic loss scale they are in scaled units, and one further row
  ``('loss_scale', ...)`` carries the scale so that a reader can divide.  While accumulating gradients a batch is a micro-batch and
  ``_grad`` is whatever the accumulation arena holds at that moment.
* Intermediate activations are not monitored: they live in a shared pool, are aliased across steps, and many never exist (folded
  BatchNorm, residual adds in convolution epilogues).  A pattern that names one simply matches nothing.
"""
import logging
import math
import re

import numpy as np


def check_monitor_options(interval, pattern):
    """ValueError unless these are an interval and a pattern Monitor takes"""
    if isinstance(interval, (bool, np.bool_)) or not isinstance(interval, (int, np.integer)) or int(interval) < 1:
        raise ValueError('monitor: interval must be an int >= 1, got %r' % (interval,))
    if not isinstance(pattern, str):
        raise ValueError('monitor: pattern must be a regular expression string, got %r' % (pattern,))
    try:
        re.compile(pattern)
    except re.error as e:
        raise ValueError('monitor: pattern %r is not a regular expression (%s)' % (pattern, e))
    return int(interval), pattern


def parse_monitor_env(text):
    """SNIPER_MONITOR=<interval>[:<regex>] -> (interval, pattern)"""
    head, sep, rest = text.strip().partition(':')
    try:
        interval = int(head)
    except ValueError:
        raise ValueError('SNIPER_MONITOR must be <interval>[:<regex>], got %r' % (text,))
    return check_monitor_options(interval, rest if sep else '.*')


def default_stat(rec):
    """norm(x) / sqrt(x.size) from a record of sn_tensor_stats; nan when the tensor holds a non-finite element or nothing"""
    if rec[2] > 0 or rec[6] == 0:
        return float('nan')
    return math.sqrt(rec[0]) / math.sqrt(rec[6])


class Monitor(object):
    def __init__(self, interval, stat_func=None, pattern='.*', sort=False):
        self.interval, self.pattern = check_monitor_options(interval, pattern)
        if stat_func is not None and not callable(stat_func):
            raise ValueError('monitor: stat_func must be None or a callable, got %r' % (stat_func,))
        self.stat_func = stat_func
        self.sort = bool(sort)
        self.re_prog = re.compile(self.pattern)
        self.exes = []
        self.extra_rows = []         # callables -> [(name, value)] appended to an armed batch's rows (Module: the loss scale)
        self.step = 0
        self.activated = False
        self.logger = logging

    def install(self, exe):
        """exe: an engine Executor (Module.install_monitor passes its own)"""
        if exe not in self.exes:
            self.exes.append(exe)

    def tic(self):
        if self.step % self.interval == 0:
            self.activated = True
        self.step += 1

    def _fast(self, exe):
        pending = []
        for which, suffix in (('weight', ''), ('grad', '_grad'), ('mom', '_mom')):
            out, names = exe.tensor_stats(which, self.pattern, suffix)
            if names and out is not None:
                pending.append(([n + suffix for n in names], out))
        heads = exe.output_stats(self.pattern)
        rows = []
        for names, out in pending:                       # (every launch is enqueued before the first download waits)
            rec = out.cpu().numpy()
            rows += [(n, default_stat(r)) for n, r in zip(names, rec[1:])]
        for name, out in heads:
            rows.append((name, default_stat(out.cpu().numpy()[1])))
        return rows

    def _slow(self, exe):
        from . import ndarray as nd
        rows = []
        for name, t in exe.stat_views(self.pattern):
            v = self.stat_func(nd.NDArray(t))
            rows.append((name, v))
        return rows

    @staticmethod
    def _text(v):
        if hasattr(v, 'asnumpy'):
            v = v.asnumpy()
        if isinstance(v, np.ndarray):
            return str(v.item()) if v.size == 1 else str(v)
        return str(v)

    def toc(self):
        if not self.activated:
            return []
        self.activated = False
        rows = []
        for exe in self.exes:
            rows += self._fast(exe) if self.stat_func is None else self._slow(exe)
        if self.sort:
            rows.sort(key=lambda r: r[0])
        for extra in self.extra_rows:
            rows += list(extra())
        return [(self.step, name, self._text(v)) for name, v in rows]

    def toc_print(self):
        rows = self.toc()
        for n, k, v in rows:
            self.logger.info('Batch: {:7d} {:30s} {:s}'.format(n, k, v))
        return rows
