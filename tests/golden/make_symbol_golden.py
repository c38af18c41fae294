"""Generate tests/golden/symbols_v1.json.gz from the REFERENCE's own symbol files (build container only): each network of
symbols/faster/ that sniper_amd mirrors, built over the mx shim for training and for test, and reduced to what
tests/test_symbols.py compares -- outputs, arguments, auxiliary states, inferred shapes and the operator nodes (op, name,
attributes without their defaults) in sorted order.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_symbol_golden.py
"""
import gzip
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'symbols_v1.json.gz')

B = 2
R_DEFAULTS = {'dilate': '(1, 1)', 'stride': '(1, 1)', 'pad': '(0, 0)'}
MNV2_DEFAULTS = dict(R_DEFAULTS, num_group='1')


def graph_signature(net, cfg, train, shapes, defaults, aux_shapes=True):
    """The graph `net.get_symbol_rcnn(cfg, is_train=train)` builds, as plain JSON data."""
    from sniper_amd.mx import symbol as _symmod
    _symmod._counter().clear()          # auto-names (blockgrad0, _plus0, pooling0 ...) count per graph build
    sym = net.get_symbol_rcnn(cfg, is_train=train)
    net.infer_shape(shapes)

    def norm(n):
        kv = [(k, str(tuple(v)) if isinstance(v, (list, tuple)) else str(v)) for k, v in n.attrs.items()
              if k not in ('workspace', 'cudnn_off')]
        return (n.op, n.name, sorted((k, v) for k, v in kv if defaults.get(k) != v))

    sig = {'outputs': sym.list_outputs(), 'arguments': sorted(sym.list_arguments()),
           'aux_states': sorted(sym.list_auxiliary_states()), 'arg_shapes': net.arg_shape_dict, 'out_shapes': net.out_shape_dict,
           'nodes': [norm(n) for n in sym._topo() if n.op]}
    if aux_shapes:
        sig['aux_shapes'] = net.aux_shape_dict
    sig = json.loads(json.dumps(sig))   # tuples -> lists, as the golden file stores them
    sig['nodes'] = sorted(sig['nodes'])
    return sig


def load():
    with gzip.open(OUT, 'rt') as fh:
        return json.load(fh)


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import sniper_amd.mx as mx
    from oracle.build import REF
    from sniper_amd import config as cfgmod
    from test_symbols import _cfg, _mask_shapes, _mnv2_shapes, _shapes
    mx.alias_as('mxnet')
    for p in (REF, os.path.join(REF, 'lib'), os.path.join(REF, 'symbols', 'faster')):
        if p not in sys.path:
            sys.path.insert(0, p)
    sys.dont_write_bytecode = True
    out = {}
    for name in ('resnet_mx_101_e2e', 'resnet_mx_50_e2e'):
        cls = getattr(importlib.import_module(name), name)
        for train in (True, False):
            out['%s_%s' % (name, 'train' if train else 'test')] = graph_signature(
                cls(n_proposals=400, momentum=0.995, test_nbatch=B), _cfg(B), train, _shapes(B, train=train), R_DEFAULTS)
    cls = importlib.import_module('mobilenetv2_e2e').mobilenetv2_e2e
    for train in (True, False):
        out['mobilenetv2_e2e_%s' % ('train' if train else 'test')] = graph_signature(
            cls(test_nbatch=B), cfgmod.mobilenetv2_e2e(batch_images=B), train, _mnv2_shapes(B, train), MNV2_DEFAULTS, aux_shapes=False)
    cls = importlib.import_module('resnet_mx_101_e2e_mask').resnet_mx_101_e2e_mask
    for autofocus in (False, True):
        for train in (True, False):
            cfg = _cfg(B)
            cfg.TRAIN.AUTO_FOCUS = cfg.TEST.AUTO_FOCUS = autofocus
            shp = _mask_shapes(B, train)
            if autofocus and train:
                shp['scale_label'] = (B, 1024)
            out['resnet_mx_101_e2e_mask%s_%s' % ('_autofocus' if autofocus else '', 'train' if train else 'test')] = graph_signature(
                cls(momentum=0.995, test_nbatch=B), cfg, train, shp, R_DEFAULTS, aux_shapes=False)
    with gzip.GzipFile(OUT, 'wb', mtime=0) as fh:
        fh.write((json.dumps(out, sort_keys=True, separators=(',', ':')) + '\n').encode())
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
