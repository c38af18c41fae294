"""GPU: sn_box_annotator_ohem against the float64 restatement of lib/operator_py/box_annotator_ohem.py (tests/ohem_util.py) --
EXACT equality: every case is tie-free at its selection boundary by a margin >= 100 x the fp32 error of the loss, which
tests/test_ohem_cases_cpu.py asserts -- the tie / NaN order, the refused arguments, the operator inside a graph (eager and
replayed as a hipGraph) and Trainer(ohem=k)."""
import numpy as np
import pytest
import torch

import ohem_util
from gpu_util import assert_close, dev

pytestmark = pytest.mark.gpu


def _run(ins, k, with_fg=True):
    """one call on NaN-poisoned outputs -> (labels_ohem, bbox_weights_ohem, fg_labels or None) device tensors"""
    from sniper_amd import hip
    score, pred, lab, tgt, wgt = [torch.from_numpy(np.array(a, np.float32)).to(dev()) for a in ins]
    B, R, C = score.shape
    poison = lambda t: torch.full_like(t, float('nan'))
    lo, wo = poison(lab), poison(wgt)
    fg = poison(lab) if with_fg else None
    hip.call('sn_box_annotator_ohem', score, pred, lab, tgt, wgt, lo, wo, fg, B, R, C, pred.shape[2], k, hip.stream())
    torch.cuda.synchronize()
    return lo, wo, fg


@pytest.mark.parametrize('name', sorted(ohem_util.CASES))
def test_kernel_equals_the_restatement(name):
    ins, k, want, _ = ohem_util.case(name)
    got = _run(ins, k)
    for g, w, what in zip(got, want, ('labels_ohem', 'bbox_weights_ohem', 'fg_labels')):
        g = g.cpu().numpy()
        assert not np.isnan(g).any(), '%s: %s has elements the call did not write' % (name, what)
        assert np.array_equal(g, w), '%s: %s differs at %s' % (name, what, np.argwhere(g != w)[:5].tolist())
    again = _run(ins, k)
    for a, b in zip(got, again):
        assert torch.equal(a, b), name + ': second call differs'
    lo, wo, fg = _run(ins, k, with_fg=False)                 # fg_labels = NULL: the other two outputs are the same
    assert fg is None and torch.equal(lo, got[0]) and torch.equal(wo, got[1])


def test_equal_losses_rank_by_index_and_nan_ranks_first():
    B, R, C, k = 2, 100, 7, 10
    rs = np.random.RandomState(3)
    score = np.full((B, R, C), 0.25, np.float32)
    pred = rs.standard_normal((B, R, 4)).astype(np.float32)
    tgt = pred.copy()
    lab = rs.choice(np.arange(-1, C), size=(B, R)).astype(np.float32)
    lab[0, 1] = C + 2                                         # a label beyond the classes: read as class C-1, written back as it is
    wgt = np.ones((B, R, 4), np.float32)
    ins = (score, pred, lab, tgt, wgt)
    lo, wo, fg = [t.cpu().numpy() for t in _run(ins, k)]
    for i in range(B):
        first = np.flatnonzero(lab[i] >= 0)[:k]               # every valid loss is log(C): the first k valid indices are kept
        want = np.full(R, -1, np.float32)
        want[first] = lab[i, first]
        assert np.array_equal(lo[i], want), i
        assert np.array_equal(wo[i], np.repeat((want >= 0).astype(np.float32)[:, None], 4, 1)), i
        assert np.array_equal(fg[i], np.where(want == 0, -1, want)), i
    assert lo[0, 1] == C + 2
    for a, b in zip((lo, wo, fg), ohem_util.ohem_reference(*ins, k)):
        assert np.array_equal(a, b)
    # one row of NaN scores, late in the image: it is the one RoI kept at k = 1, and the first of k = 3
    score = (rs.standard_normal((B, R, C)) * 2).astype(np.float32)
    lab = np.abs(lab) % C
    score[1, 77] = np.nan
    ins = (score, pred, lab, tgt, wgt)
    lo, wo, _ = [t.cpu().numpy() for t in _run(ins, 1)]
    assert np.flatnonzero(lo[1] >= 0).tolist() == [77] and np.flatnonzero(wo[1, :, 0]).tolist() == [77]
    assert int((lo[0] >= 0).sum()) == 1
    lo3 = _run(ins, 3)[0].cpu().numpy()
    assert lo3[1, 77] == lab[1, 77] and int((lo3[1] >= 0).sum()) == 3
    assert np.array_equal(lo3, ohem_util.ohem_reference(*ins, 3)[0])


@pytest.mark.parametrize('kw,words', [
    (dict(k=0), ('roi_per_img >= 1', 'roi_per_img = 0')),
    (dict(C=1), ('C >= 2', 'C = 1')),
    (dict(box_dim=0), ('box_dim >= 1', 'box_dim = 0')),
    (dict(B=0), ('B >= 1', 'B = 0')),
    (dict(R=0), ('R >= 1', 'R = 0')),
    (dict(R=16385), ('R <= 16384', 'LDS', 'R = 16385')),
    (dict(null=5), ('null pointer',)),
])
def test_refused_arguments_leave_the_outputs_alone(kw, words):
    from sniper_amd import hip
    from sniper_amd._lib import SniperHipError
    t = torch.zeros(64, device=dev())
    out = torch.full((64,), 7.0, device=dev())
    a = dict(B=1, R=4, C=3, box_dim=4, k=2, null=None)
    a.update(kw)
    args = [t, t, t, t, t, out, out, None]
    if a['null'] is not None:
        args[a['null']] = None
    with pytest.raises(SniperHipError) as e:
        hip.call('sn_box_annotator_ohem', *args, a['B'], a['R'], a['C'], a['box_dim'], a['k'], hip.stream())
    msg = str(e.value)
    assert 'sn_box_annotator_ohem' in msg and all(w in msg for w in words), msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the operator in a graph: the wiring of symbols/symbol.py::ohem on a small head ------------------------------------------
GB, GR, GD, GC, GK = 2, 24, 64, 5, 7


def _head_graph(mx):
    data = mx.sym.Variable('data')
    label, bt, bw = mx.sym.Variable('label'), mx.sym.Variable('bbox_target'), mx.sym.Variable('bbox_weight')
    cls_score = mx.sym.FullyConnected(name='cls_score', data=data, num_hidden=GC)
    bbox_pred = mx.sym.FullyConnected(name='bbox_pred', data=data, num_hidden=4)
    per_image = lambda x, name, *tail: mx.sym.Reshape(data=x, shape=(GB, -1) + tail, name=name)
    lo, wo = mx.contrib.sym.BoxAnnotatorOHEM(
        name='box_annotator_ohem', num_classes=GC, num_reg_classes=1, roi_per_img=GK, cls_score=per_image(cls_score, 'ohem_cls_score', GC),
        bbox_pred=per_image(bbox_pred, 'ohem_bbox_pred', 4), labels=per_image(label, 'ohem_label'),
        bbox_targets=per_image(bt, 'ohem_bbox_target', 4), bbox_weights=per_image(bw, 'ohem_bbox_weight', 4))
    lab_flat = mx.sym.Reshape(data=lo, shape=(-1,), name='label_reshape')
    w_flat = mx.sym.Reshape(data=wo, shape=(-1, 4), name='bbox_weight_reshape')
    cls_prob = mx.sym.SoftmaxOutput(name='cls_prob', data=cls_score, label=lab_flat, normalization='valid', use_ignore=True,
                                    ignore_label=-1, grad_scale=1.0)
    bbox_loss_ = w_flat * mx.sym.smooth_l1(name='bbox_loss_', scalar=1.0, data=(bbox_pred - bt))
    bbox_loss = mx.sym.MakeLoss(name='bbox_loss', data=bbox_loss_, grad_scale=1.0 / (GK * GB))
    return mx.sym.Group([cls_prob, bbox_loss, mx.sym.BlockGrad(lab_flat), mx.sym.BlockGrad(w_flat), mx.sym.BlockGrad(cls_score),
                         mx.sym.BlockGrad(bbox_pred)])


def _head_run(monkeypatch, graphs, steps):
    """`steps` forward + backward passes on one feed -> (outputs of the last pass, parameter gradients, executor, feed, parameters)"""
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', graphs)
    shapes = dict(data=(GB * GR, GD), label=(GB * GR,), bbox_target=(GB * GR, 4), bbox_weight=(GB * GR, 4))
    ex = Executor(_head_graph(mx), shapes, True, [])
    assert ex.use_graphs == (graphs == '1') and [type(s).__name__ for s in ex.steps].count('BoxAnnotatorOHEMStep') == 1
    rs = np.random.RandomState(0)
    P = {'cls_score_weight': (rs.standard_normal((GC, GD)) * 0.3).astype(np.float32), 'cls_score_bias': np.zeros(GC, np.float32),
         'bbox_pred_weight': (rs.standard_normal((4, GD)) * 0.1).astype(np.float32), 'bbox_pred_bias': np.zeros(4, np.float32)}
    ex.set_params(P, {})
    lab = rs.choice([-1, 0, 1, 2, 3, 4], size=(GB * GR,), p=[0.2, 0.4, 0.1, 0.1, 0.1, 0.1]).astype(np.float32)
    feed = dict(data=rs.standard_normal((GB * GR, GD)).astype(np.float32), label=lab,
                bbox_target=rs.standard_normal((GB * GR, 4)).astype(np.float32),
                bbox_weight=np.repeat((lab > 0).astype(np.float32)[:, None], 4, 1))
    for _ in range(steps):
        outs = ex.forward_backward(feed)
    torch.cuda.synchronize()
    return [o.clone() for o in outs], {k: p.grad.clone() for k, p in ex.params.items() if p.trainable}, ex, feed, P


def test_operator_in_a_graph_selects_and_trains_like_the_reference(monkeypatch):
    outs, grads, ex, feed, P = _head_run(monkeypatch, '0', 1)
    _, _, lab_o, w_o, score, pred = [o.cpu().numpy() for o in outs]
    three = lambda a, *tail: np.asarray(a).reshape((GB, GR) + tail)
    ins = (three(score, GC), three(pred, 4), three(feed['label']), three(feed['bbox_target'], 4), three(feed['bbox_weight'], 4))
    # the device's own fp32 scores: the selection is exact (and not decided by a tie: the condition of tests/ohem_util.py)
    assert ohem_util.gap_ok(ohem_util.losses(*ins), ins[2], GK)
    want_lab, want_w, _ = ohem_util.ohem_reference(*ins, GK)
    assert np.array_equal(three(lab_o), want_lab) and np.array_equal(three(w_o, 4), want_w)
    for i in range(GB):
        assert int((want_lab[i] >= 0).sum()) == min(GK, int((ins[2][i] >= 0).sum())) == GK
    # no gradient enters through the operator: the parameter gradients are those of the two losses with the selections held
    # constant (torch autograd on the fp16-rounded operands the device multiplies)
    from gpu_util import f16r
    xt = torch.from_numpy(f16r(feed['data']))
    wc = torch.from_numpy(f16r(P['cls_score_weight'])).requires_grad_(True)
    wb = torch.from_numpy(f16r(P['bbox_pred_weight'])).requires_grad_(True)
    sel = torch.from_numpy(lab_o.reshape(-1)).long()
    valid = sel >= 0
    logp = torch.log_softmax(xt @ wc.t(), 1)
    ce = -(logp[torch.arange(GB * GR), sel.clamp(min=0)] * valid).sum() / max(1, int(valid.sum()))
    d = xt @ wb.t() - torch.from_numpy(feed['bbox_target'])
    sl1 = (torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5) * torch.from_numpy(w_o.reshape(-1, 4))).sum() / (GK * GB)
    (ce + sl1).backward()
    for name, want in (('cls_score_weight', wc.grad.numpy()), ('bbox_pred_weight', wb.grad.numpy())):
        p = ex.params[name]
        assert_close(p.to_reference(grads[name].cpu().numpy()), want, 1e-2, 1e-2 * np.abs(want).max(), 'grad ' + name)


def test_operator_in_a_replayed_graph_is_bit_equal_to_eager(monkeypatch):
    outs_e, grads_e, _, _, _ = _head_run(monkeypatch, '0', 4)
    outs_g, grads_g, ex, _, _ = _head_run(monkeypatch, '1', 4)
    assert ex._graph_fb is not None, 'hipGraph capture did not happen'
    for a, b in zip(outs_e, outs_g):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert sorted(grads_e) == sorted(grads_g) and len(grads_e) == 4
    for k in grads_e:
        assert torch.equal(grads_e[k], grads_g[k]), k


def test_trainer_with_ohem_mines_inside_the_replayed_step():
    """Trainer(ohem=128), R101 at 2 chips: three steps (two eager, then the captured forward + backward and optimizer graphs).  In
    every chip the labels that reach the losses are min(128, labelled RoIs of MultiProposalTarget) many."""
    from sniper_amd.train import Trainer
    K = 128
    tr = Trainer(batch_images=2, n_images=8, ohem=K)
    assert tr.cfg.TRAIN.ENABLE_OHEM is True and tr.cfg.TRAIN.BATCH_ROIS_OHEM == K
    tr.mod.init_optimizer(optimizer='sgd', optimizer_params={'learning_rate': 2e-5, 'momentum': 0.9, 'wd': 1e-4})
    ex = tr.mod.exe
    target = [s for s in ex.steps if type(s).__name__ == 'MultiProposalTargetStep']
    ohem = [s for s in ex.steps if type(s).__name__ == 'BoxAnnotatorOHEMStep']
    assert len(target) == 1 and len(ohem) == 1 and ohem[0].k == K and ex.use_graphs
    for step in range(3):
        outs = tr.step()
        torch.cuda.synchronize()
        arrays = [o.asnumpy() for o in outs]
        assert all(np.isfinite(a).all() for a in arrays), step
        rcnn_label = arrays[4].reshape(2, -1)
        given = target[0].outs[1].t.cpu().numpy().reshape(2, -1)
        assert rcnn_label.shape == given.shape == (2, 300)
        for i in range(2):
            assert int((rcnn_label[i] >= 0).sum()) == min(K, int((given[i] >= 0).sum())), (step, i)
            kept = rcnn_label[i] >= 0
            assert np.array_equal(rcnn_label[i][kept], given[i][kept])
        assert int((given >= 0).sum()) > 2 * K            # the mining had something to drop
    assert ex._graph_fb is not None and ex._graph_up is not None, 'the OHEM step is not replayed'
