"""Generate tests/golden/engine_call_trace_v1.json.gz: every C-ABI call the engine issues for the graphs below, in order, with every
argument -- what tests/test_engine_call_trace.py compares line by line (CPU only, needs the built library for the host-side queries).

An Executor lowers on torch.device('cpu'); hip.call / hip.stream / hip.Workspace / hip.wgrad_table are replaced by recorders, and set-up,
parameter refresh, one eager forward, backward and optimizer update run on CPU tensors.  Nothing is computed: the trace is WHICH entry
points the lowering chose, in which order, on which buffers, with which scalars (the library's answers to sn_conv_fwd_stats_blocks,
sn_conv_fwd_splitk_workspace_bytes, sn_conv_fwd_dual_ok ... are in it too, as buffer shapes, byte counts and the launch chosen).

When to regenerate: only in a change that MEANS to alter the lowering (a new fusion, another kernel for a layer, a kernel change that
moves a plan).  Such a change regenerates the file and the diff of the decompressed text is part of its review.  A refactor, a host-side
speed-up, anything that claims "same launches" must pass against the committed file untouched.

    python tests/golden/make_call_trace.py [OUT]
"""
import bisect
import gzip
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'engine_call_trace_v1.json.gz')

TEST_SHAPES = ((2, 512, 512), (2, 96, 128), (8, 480, 512))      # R101 test-time batches: (images, height, width)


def _networks():
    if os.path.join(ROOT, 'tests') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_frozen_bn_lowering import NETWORKS
    return NETWORKS


def case_names():
    names = ['%s/fix_bn=%d' % (n, f) for n in sorted(_networks()) for f in (0, 1)]
    return names + ['resnet_mx_101_e2e/wgrad_per_layer', 'resnet_mx_101_e2e/split_backward', 'resnet_mx_101_e2e/test']


class _Workspace(object):
    """hip.Workspace on the host"""

    def __init__(self):
        self.buf = None

    def get(self, nbytes):
        nbytes = int(nbytes)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 256), dtype=torch.uint8)
        return self.buf


class Recorder(object):
    """One trace: [[phase, [line, ...]], ...].  A tensor is written <owner>:<dtype>:<shape>; the owner is the bound value, parameter field
    or auxiliary state whose memory the address lies in (+ byte offset when it is not its start), `tmp` for step-private buffers and
    temporaries -- never an address, so two processes write the same text."""

    def __init__(self, mp):
        from sniper_amd import hip
        self.phases = []
        self.starts, self.owners = [], {}       # sorted start addresses; start -> (name, bytes)
        self._real_table = hip.wgrad_table
        mp.setattr(hip, 'call', self.call)
        mp.setattr(hip, 'stream', lambda: None)
        mp.setattr(hip, 'Workspace', _Workspace)
        mp.setattr(hip, 'wgrad_table', self.wgrad_table)

    def phase(self, name):
        self.phases.append([name, []])

    def note(self, text):
        self.phases[-1][1].append(text)

    def own(self, t, name):
        if t is None or t.numel() == 0 or t.data_ptr() in self.owners:
            return
        self.owners[t.data_ptr()] = (name, t.numel() * t.element_size())
        bisect.insort(self.starts, t.data_ptr())

    def name_tensors(self, ex):
        """(again after load_inputs: the input buffers are allocated there; names already given stay)"""
        for v in ex.vals.values():
            self.own(v.t, 'val.' + v.name)
        for n, p in ex.params.items():
            for f in ('master', 'grad', 'mom', 'w16', 'wT16'):
                self.own(getattr(p, f), 'par.%s.%s' % (n, f))
        for n, t in ex.aux.items():
            self.own(t, 'aux.' + n)

    def arg(self, a):
        if isinstance(a, torch.Tensor):
            ptr, who = a.data_ptr(), 'tmp'
            k = bisect.bisect_right(self.starts, ptr) - 1
            if k >= 0:
                name, nbytes = self.owners[self.starts[k]]
                if ptr < self.starts[k] + nbytes:
                    who = name if ptr == self.starts[k] else '%s+%d' % (name, ptr - self.starts[k])
            return '%s:%s:%s' % (who, str(a.dtype)[6:], tuple(a.shape))
        if isinstance(a, np.ndarray):
            return 'host%s' % (tuple(a.shape),)
        if isinstance(a, np.generic):
            a = a.item()
        if hasattr(a, '_type_') or hasattr(a, '_length_'):
            return 'ctypes'
        if isinstance(a, int) and not isinstance(a, bool) and abs(a) > (1 << 40):
            return 'hostptr'
        return repr(a)

    def call(self, name, *args):
        self.note('%s(%s)' % (name, ', '.join(self.arg(a) for a in args)))
        return 0

    def wgrad_table(self, problems):
        for pr in problems:
            self.note('  wgrad_desc(%s)' % ', '.join(self.arg(a) for a in pr))
        return self._real_table(problems)


def _zeros(shapes):
    return {k: np.zeros(v, np.float32) for k, v in shapes.items()}


def _train_case(rec, name, fix_bn=False, split=False):
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.train import fixed_param_names
    preset, shapes = _networks()[name]
    cfg = getattr(cfgmod, preset)(batch_images=2)
    cls = getattr(importlib.import_module('sniper_amd.symbols.faster.' + name), name)
    sym = cls(momentum=0.995, fix_bn=fix_bn).get_symbol_rcnn(cfg)
    rec.phase('setup')
    ex = Executor(sym, shapes, True, fixed_param_names(cfg, sym), device=torch.device('cpu'), split_backward=split)
    rec.name_tensors(ex)
    rec.phase('refresh')
    ex.refresh_compute_copies()
    rec.phase('forward')
    ex.is_train = True
    ex.load_inputs(_zeros(shapes))
    rec.name_tensors(ex)
    ex._forward_body()
    if split:
        rec.note('split_k = %d' % ex.split_k)
        for seg in ('a', 'b'):
            rec.phase('backward ' + seg)
            ex.backward(seg)
    else:
        rec.phase('backward')
        ex.backward()
    rec.phase('update')
    ex.update(0.01, 1e-4, 0.9, 1.0)


def _test_case(rec):
    """the R101 test-time graph at three batch shapes; the second and third share the first one's parameters (adopt_derived)"""
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.mx import symbol as symmod
    from sniper_amd.symbols.faster import resnet_mx_101_e2e as r101
    first = None
    for B, h, w in TEST_SHAPES:
        tag = '%dx%dx%d ' % (B, h, w)
        symmod._counter().clear()
        sym = r101.resnet_mx_101_e2e(test_nbatch=B).get_symbol_rcnn(cfgmod.res101_e2e(batch_images=B), is_train=False)
        shapes = dict(data=(B, 3, h, w), im_info=(B, 3), im_ids=(B,), chip_ids=(B,))
        rec.phase(tag + 'setup')
        ex = Executor(sym, shapes, False, [], device=torch.device('cpu'), share_params=first)
        rec.name_tensors(ex)
        rec.phase(tag + 'refresh')
        adopted = ex.adopt_derived() if first is not None else False
        rec.note('adopt_derived -> %r' % adopted)
        if not adopted:
            ex.refresh_compute_copies()
        rec.phase(tag + 'forward')
        ex.is_train = False
        ex.load_inputs(_zeros(shapes))
        rec.name_tensors(ex)
        ex._forward_body()
        first = first or ex


def trace(case, mp):
    """The trace of one case of case_names().  mp: a pytest MonkeyPatch (the recorders and the environment go back when it is undone)."""
    from sniper_amd.mx import symbol as symmod
    for k in [k for k in os.environ if k.startswith('SNIPER_')]:
        mp.delenv(k)
    symmod._counter().clear()
    rec = Recorder(mp)
    name, variant = case.split('/')
    if variant == 'test':
        _test_case(rec)
    elif variant == 'wgrad_per_layer':
        mp.setenv('SNIPER_WGRAD_DEFER', '0')
        _train_case(rec, name)
    elif variant == 'split_backward':
        _train_case(rec, name, split=True)
    else:
        _train_case(rec, name, fix_bn=variant == 'fix_bn=1')
    return rec.phases


def load():
    with gzip.open(OUT, 'rt') as fh:
        return json.load(fh)


def main():
    sys.path.insert(0, ROOT)
    out = {}
    for case in case_names():
        with pytest.MonkeyPatch.context() as mp:
            out[case] = trace(case, mp)
        print('%-45s %s' % (case, ', '.join('%s %d' % (p, len(lines)) for p, lines in out[case])))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, 'wb') as raw, gzip.GzipFile('', 'wb', fileobj=raw, mtime=0) as fh:      # (no file name, no time: same bytes anywhere)
        fh.write((json.dumps(out, sort_keys=True, indent=0, separators=(',', ':')) + '\n').encode())
    print('wrote', path, os.path.getsize(path), 'bytes,', sum(len(l) for c in out.values() for _, l in c), 'lines')


if __name__ == '__main__':
    main()
