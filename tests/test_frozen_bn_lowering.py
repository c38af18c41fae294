"""CPU: lowering of fix_bn graphs (every BatchNorm of the trainable stages is a use_global_stats layer that still trains its
gamma / beta), and the pin that graphs WITHOUT fix_bn lower exactly as before (tests/golden/lowering_plans_fix_bn_false.json,
computed on the commit before moving-statistics layers could train)."""
import importlib
import json
import os

import torch

from sniper_amd import config as cfgmod
from sniper_amd.engine.executor import Executor
from sniper_amd.train import fixed_param_names

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lowering_plans_fix_bn_false.json')
B = 2
_R101_SHAPES = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, 21 * 32 * 32),
                    bbox_target=(B, 84, 32, 32), bbox_weight=(B, 84, 32, 32), gt_boxes=(B, 100, 5))
# name -> (symbol module / class, config preset, bound shapes): the graphs tests/test_engine_lowering.py lowers, plus R50
NETWORKS = {
    'resnet_mx_101_e2e': ('res101_e2e', _R101_SHAPES),
    'resnet_mx_50_e2e': ('res101_e2e', _R101_SHAPES),
    'resnet_mx_101_e2e_mask': ('res101_e2e', dict(_R101_SHAPES, gt_masks=(B, 100, 500))),
    'resnet_mx_101_e2e_rfcn': ('res101_e2e', _R101_SHAPES),
    'mobilenetv2_e2e': ('mobilenetv2_e2e', dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, 15 * 16 * 16),
                                                bbox_target=(B, 60, 16, 16), bbox_weight=(B, 60, 16, 16), gt_boxes=(B, 100, 5),
                                                crowd_boxes=(B, 10, 5))),
}


def _lower(name, fix_bn=False, more_fixed=()):
    preset, shapes = NETWORKS[name]
    cfg = getattr(cfgmod, preset)(batch_images=B)
    if more_fixed:
        cfg.network.FIXED_PARAMS = list(cfg.network.FIXED_PARAMS) + list(more_fixed)
    cls = getattr(importlib.import_module('sniper_amd.symbols.faster.' + name), name)
    sym = cls(momentum=0.995, fix_bn=fix_bn).get_symbol_rcnn(cfg)
    return Executor(sym, shapes, True, fixed_param_names(cfg, sym), device=torch.device('cpu'))


def lowering_plan(ex):
    """what the golden file holds per network: the trainable names, the step kinds in order, the folded BatchNorm layers"""
    return {'trainable': sorted(n for n, p in ex.params.items() if p.trainable),
            'n_trainable': int(ex.n_trainable),
            'steps': [type(s).__name__ for s in ex.steps],
            'folded': sorted(s.node.name for s in ex.steps if getattr(s, 'folded_into', None) is not None),
            'groups': [[list(g[0]), int(g[1]), int(g[2])] for g in ex.groups]}


def _bns(ex):
    return [s for s in ex.steps if type(s).__name__ == 'BatchNormStep']


def _in_stages_2_to_4(name):
    return name.startswith(('stage2_', 'stage3_', 'stage4_'))


def test_r101_fix_bn_layers_train_gamma_and_beta():
    ex = _lower('resnet_mx_101_e2e', fix_bn=True)
    ex0 = _lower('resnet_mx_101_e2e', fix_bn=False)
    bns = _bns(ex)
    assert len(bns) == 101 and all(s.global_stats for s in bns)
    late = [s for s in bns if _in_stages_2_to_4(s.node.name)]
    assert len(late) == 90
    for s in late:
        assert s.gamma.trainable and s.beta.trainable and s.folded_into is None, s.node.name
        assert s.y.needs_grad == (s.x.needs_grad or s.gamma.trainable or s.beta.trainable), s.node.name
        assert s.batched_refresh() and s.stats_from is None, s.node.name
    # 89 layers hand a gradient on; the first one reads the frozen stage-1 output and trains its parameters only
    assert [s.node.name for s in late if not s.x.needs_grad] == ['stage2_unit1_bn1']
    assert all(s.y.needs_grad for s in late)
    # bn_data, bn0 and stage 1: as without fix_bn
    early0 = {s.node.name: s for s in _bns(ex0) if not _in_stages_2_to_4(s.node.name)}
    early = {s.node.name: s for s in bns if not _in_stages_2_to_4(s.node.name)}
    assert sorted(early) == sorted(early0) and len(early) == 11
    for n, s in early.items():
        o = early0[n]
        assert s.global_stats and o.global_stats and not s.gamma.trainable and not s.beta.trainable and not s.y.needs_grad, n
        assert (s.folded_into is None) == (o.folded_into is None) and s.is_stem == o.is_stem and not s.batched_refresh(), n
    folded = sorted(s.node.name for s in bns if s.folded_into is not None)
    assert folded == sorted(s.node.name for s in _bns(ex0) if s.folded_into is not None) and len(folded) == 7
    assert sorted(n for n, p in ex.params.items() if p.trainable) == sorted(n for n, p in ex0.params.items() if p.trainable)
    assert ex.n_trainable == ex0.n_trainable == 73479464
    # no batch statistics anywhere: no convolution carries a statistics epilogue for a BatchNorm behind it
    assert not any(getattr(s, 'stats_buf', None) is not None for s in ex.steps)


def test_r101_fix_bn_with_gamma_beta_in_fixed_params():
    ex = _lower('resnet_mx_101_e2e', fix_bn=True, more_fixed=('gamma', 'beta'))
    assert not any(p.trainable for n, p in ex.params.items() if n.endswith(('_gamma', '_beta')))
    convs = [s for s in ex.steps if type(s).__name__ in ('ConvolutionStep', 'DeformableConvolutionStep') and _in_stages_2_to_4(s.node.name)]
    assert len(convs) == 30 * 3 + 3 + 3 and all(s.w.trainable for s in convs)        # bottleneck convs + shortcuts + offset convs
    late = [s for s in _bns(ex) if _in_stages_2_to_4(s.node.name)]
    assert len(late) == 90 and not any(s.batched_refresh() for s in late)
    # dx only: a gradient passes through every layer but the first, which has nothing left to compute
    assert [s.node.name for s in late if not s.y.needs_grad] == ['stage2_unit1_bn1']
    assert all(s.y.needs_grad == s.x.needs_grad for s in late)
    # frozen parameters behind TRAINABLE convolutions: nothing more is folded than without fix_bn
    assert len([s for s in _bns(ex) if s.folded_into is not None]) == 7


def test_graphs_without_fix_bn_lower_as_before():
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(golden) == sorted(NETWORKS)
    for name in sorted(NETWORKS):
        plan = json.loads(json.dumps(lowering_plan(_lower(name))))        # (tuples become lists, as in the file)
        for key in ('trainable', 'n_trainable', 'steps', 'folded', 'groups'):
            assert plan[key] == golden[name][key], (name, key)


def test_every_symbol_class_takes_fix_bn():
    for name in sorted(NETWORKS):
        n = len([s for s in _bns(_lower(name, fix_bn=True)) if s.global_stats])
        n0 = len([s for s in _bns(_lower(name, fix_bn=False)) if s.global_stats])
        if name == 'mobilenetv2_e2e':
            assert n == n0 == 0          # accepted and ignored, as the reference's class does
        else:
            assert n > n0 == 11 and n == len(_bns(_lower(name, fix_bn=True))), (name, n, n0)
