"""-m gpu: the Darknet backbone (backbones/darknet.py) on the dense conv path with the LeakyReLU passes of csrc/darknet.hip.

  fixture    tests/golden/darknet.npz (the reference's own Darknet in fp64, tools/gen_darknet.py): every case's outputs <= 2e-4
             max|level|, every parameter gradient of the fixture's linear functional through BackwardEngine._backward_backbone <= 2e-3
             rel-L2 on the norm and on the strided sample, and the gradient at the first stride-2 conv's image-side input; frozen
             parameters get none; the recorded forward has the forward-only bits
  batch      every output of a batch of 2 equals the single-image runs bit for bit; two runs agree, forward and backward
  locators   Darknet-53 + FPN under P2PHead (three levels) and CPRHead (one level) at 2 x 64 x 64: one train_step; loss.backward()
             through the autograd bridge bit-equal to the native trainer for frozen_stages -1 and 2; no ready point fires early
             (tests/ready_point_check.py); after a step the parameters moved and a second forward equals a freshly built model holding
             the stepped weights (the packs were refreshed)
  refusals   the bf16 compute mode names ``Darknet`` from set_compute_dtype, the forward, the trainers and the bridge; batch statistics
             name ``norm_eval`` from the forward, the trainer and the bridge"""
import warnings

import numpy as np
import pytest
import torch

from pointtinybenchmark_amd import synthetic
from tests import darknet_ref as DR
from tests.ready_point_check import run_checked_backward

pytestmark = pytest.mark.gpu
NECK_IN = [256, 512, 1024]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case_model(name):
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.backbones import Darknet
    DR.add_small_arch(Darknet)
    cfg = DR.CASES[name]
    m = P.build_backbone(dict(type='Darknet', **DR.constructor_kwargs(cfg))).cuda()
    m.load_state_dict(DR.case_state_dict(cfg), strict=True)
    m.train()
    return cfg, m


# ------------------------------------------------------------------------------------------------ forward against the fixture
@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = DR.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
        nhwc4 = m(torch.cat([img, torch.zeros_like(img[:, :1])], 1).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
        single = [m(img[n:n + 1].contiguous()) for n in range(img.shape[0])]
    torch.cuda.synchronize()
    stages = sorted(set(cfg['out_indices']))
    assert len(outs) == len(stages) and [o.shape[1] for o in outs] == [m.stage_widths[i] for i in stages]
    failed = []
    for l, o in enumerate(outs):
        assert o.permute(0, 2, 3, 1).is_contiguous()      # an NCHW view of the NHWC buffer
        e = DR.output_error(name, l, o)
        print('ERR forward %-10s output %d %-14s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[1:]), e), flush=True)
        if not e <= DR.BAR_OUT:
            failed.append((l, e))
        assert _same_bits(o, again[l]) and _same_bits(o, nhwc4[l])
        assert float(o.min()) < 0.0      # a leaky map: negative values survive
        for n in range(img.shape[0]):
            assert _same_bits(o[n:n + 1], single[n][l]), 'image %d of the batch differs from its single-image run' % n
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ backward against the fixture
def _engine_backward(m, cfg):
    """The recorded forward and BackwardEngine._backward_backbone on the fixture's linear functional
    -> (outs, {name: gradient}, the data gradient the first stride-2 conv hands down | None)."""
    from pointtinybenchmark_amd.training import BackwardEngine
    eng = BackwardEngine(m)
    eng._sink = {}
    seen = {}
    rule = eng._conv_bn_backward

    def wrapped(cache, conv, bn, *a, **kw):
        r = rule(cache, conv, bn, *a, **kw)
        if conv is m.conv_res_block1.conv.conv and r is not None:
            seen[DR.STEM_IN] = r.clone()
        return r
    eng._conv_bn_backward = wrapped
    tape = []
    outs = m(DR.case_input(cfg).cuda(), tape=tape)
    weights = [DR.functional_weight(cfg, l, o.shape) for l, o in enumerate(outs)]
    d_stage = {l: w.permute(0, 2, 3, 1).contiguous().cuda() for l, w in enumerate(weights)}
    eng._backward_backbone(m, tape, d_stage)
    if DR.STEM_IN in seen and 0 in cfg['out_indices']:
        # that map is output 0 as well: the reference's gradient at it holds the functional's own weight, which the walk adds below
        # the point the spy sees (one more fp32 rounding, far below the bar)
        seen[DR.STEM_IN] = seen[DR.STEM_IN] + d_stage[0]
    named = list(m.named_parameters())
    grads = {k: g for (k, _), g in zip(named, eng.collect([p for _, p in named])) if g is not None}
    torch.cuda.synchronize()
    return outs, grads, seen.get(DR.STEM_IN)


@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    cfg, m = _case_model(name)
    outs, grads, d_in = _engine_backward(m, cfg)
    with torch.no_grad():
        plain = m(DR.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert _same_bits(a, b), 'the recorded forward differs from the forward-only one'
    want = [k for k in DR.grad_names(name) if k != DR.STEM_IN]
    assert sorted(grads) == want
    assert sorted(grads) == sorted(k for k, p in m.named_parameters() if p.requires_grad)
    if cfg['frozen_stages'] == 2:
        assert not any(k.startswith(('conv1.', 'conv_res_block1.')) for k in grads) and d_in is None
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
        en, es = DR.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= DR.BAR_GRAD and es <= DR.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-10s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    if DR.STEM_IN in DR.grad_names(name):
        en, es = DR.grad_errors(name, DR.STEM_IN, d_in.permute(0, 3, 1, 2))
        print('ERR backward %-10s gradient at the first stride-2 conv\'s input: norm %.2e sample %.2e (bar 2e-3)' % (name, en, es), flush=True)
        if not (en <= DR.BAR_GRAD and es <= DR.BAR_GRAD):
            failed.append((DR.STEM_IN, en, es))
    assert not failed, failed[:8]


def test_gradients_are_repeatable():
    cfg, m = _case_model('small')
    _, ga, da = _engine_backward(m, cfg)
    _, gb, db = _engine_backward(m, cfg)
    assert sorted(ga) == sorted(gb) and all(_same_bits(ga[k], gb[k]) for k in ga) and _same_bits(da, db)


# ------------------------------------------------------------------------------------------------ locators
def _locator(head, seed=3, **bb_kw):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    n = 3 if head == 'p2p' else 1
    cfg = p2p_model_cfg(50, 1) if head == 'p2p' else model_cfg(50, 1, stride=8)
    cfg['backbone'] = dict(type='Darknet', depth=53, **bb_kw)
    cfg['neck'] = dict(cfg['neck'], in_channels=NECK_IN, num_outs=n, add_extra_convs=False)
    if head == 'p2p':
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[8 << k for k in range(n)])
    m = P.build_detector(cfg).cuda()
    sd = synthetic.darknet_state_dict(53, seed, prefix='backbone.')
    sd.update(synthetic.fpn_state_dict(NECK_IN, 256, 0, n, seed + 1))
    sd.update(synthetic.p2p_head_state_dict(1, seed=seed + 3, std=0.05) if head == 'p2p' else synthetic.cpr_head_state_dict(1, seed=seed + 2, std=0.3))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def _data(seed=4, hw=(64, 64)):
    batch = synthetic.synthetic_batch(2, hw[0], hw[1], 4, 1, seed=seed)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def _trainer(head):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return P2PTrainer if head == 'p2p' else CprTrainer


def _total(losses):
    return float(sum((sum(v) if isinstance(v, (list, tuple)) else v).sum() for k, v in losses.items() if 'loss' in k))


@pytest.mark.parametrize('head, fs', [('p2p', -1), ('p2p', 2), ('cpr', -1), ('cpr', 2)])
def test_bridge_is_bit_equal_to_the_trainer_and_no_ready_point_fires_early(head, fs):
    from pointtinybenchmark_amd import autograd_bridge
    data = _data()
    ma = _locator(head, frozen_stages=fs)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr, seen = run_checked_backward(_trainer(head), ma, data, lr=1e-3)      # NaN-filled buffer: every declared prefix is written
    assert {id(p) for p in tr.params} == {id(p) for p in ma.parameters() if p.requires_grad}
    first_bb = min(tr.offset[id(p)][0] for p in ma.backbone.parameters() if p.requires_grad)
    assert sum(1 for end in seen if end > first_bb) >= (46 if fs == 2 else 52), 'one ready point per trainable layer'
    type(tr).check = False
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    frozen = ('backbone.conv1.', 'backbone.conv_res_block1.')
    assert any(k.startswith(frozen) for k in want) == (fs == -1)
    for k in ('backbone.conv_res_block5.res3.conv2.conv.weight', 'backbone.conv_res_block2.conv.bn.bias') + \
            (('backbone.conv1.conv.weight', 'backbone.conv1.bn.weight') if fs == -1 else ()):
        assert float(want[k].abs().max()) > 0, k
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    assert np.isfinite(_total(la))
    for k, p in ma.named_parameters():
        if p.requires_grad:
            assert _same_bits(p.grad, want[k]), k      # equal run to run
    mb = _locator(head, frozen_stages=fs)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    assert abs(out['log_vars']['loss'] - _total(la)) <= 1e-6 * max(1.0, abs(_total(la)))
    n = 0
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and _same_bits(p.grad, want[k]), k
            n += 1
        else:
            assert p.grad is None, k
    assert n == len(want)


@pytest.mark.parametrize('head', ['p2p', 'cpr'])
def test_a_step_moves_the_parameters_and_refreshes_the_packs(head):
    data = _data()
    m = _locator(head)
    tr = _trainer(head)(m, lr=0.05)
    with torch.no_grad():
        m.eval()
        before = [o.clone() for o in m.backbone(data['img'])]      # builds the packs the step must not leave stale
        m.train()
    w0 = {k: p.detach().clone() for k, p in m.backbone.named_parameters()}
    out = tr.train_step(dict(data))
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in out['log_vars'].values()), out['log_vars']
    moved = [k for k, p in m.backbone.named_parameters() if not torch.equal(p.detach(), w0[k])]
    assert len(moved) == len(w0), sorted(set(w0) - set(moved))[:8]
    m.eval()
    fresh = _locator(head)
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    fresh.eval()
    with torch.no_grad():
        a, b = m.backbone(data['img']), fresh.backbone(data['img'])
        la, lb = m.extract_feat(data['img']), fresh.extract_feat(data['img'])
    torch.cuda.synchronize()
    assert not torch.equal(a[0], before[0])
    for x, y in zip(list(a) + list(la), list(b) + list(lb)):
        assert _same_bits(x, y), 'forward after the step differs from a fresh model in %d entries' % int((x != y).sum())


# ------------------------------------------------------------------------------------------------ refusals on the device
def test_bf16_and_batch_statistics_raise_from_forward_trainer_and_bridge():
    from pointtinybenchmark_amd import autograd_bridge
    data = _data()
    m = _locator('p2p')
    with pytest.raises(NotImplementedError, match='Darknet'):
        m.set_compute_dtype('bf16')
    m.backbone.compute_dtype = torch.bfloat16
    assert 'Darknet' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='Darknet'):
        m.backbone(data['img'])
    with pytest.raises(NotImplementedError, match='Darknet'):
        _trainer('p2p')(m)
    with pytest.raises(NotImplementedError, match='Darknet'), warnings.catch_warnings():
        warnings.simplefilter('ignore')      # (the bridge reports its reason once per process, then the forward-only path raises)
        m.train_step(dict(data))
    b = _locator('p2p', norm_eval=False)
    assert b.backbone.batch_stats_active()
    with pytest.raises(NotImplementedError, match='norm_eval'):
        b.backbone(data['img'])
    with pytest.raises(NotImplementedError, match='norm_eval'):
        _trainer('p2p')(b).forward_backward(**data)
    with pytest.raises(NotImplementedError, match='norm_eval'):
        _locator('p2p', norm_eval=False).train_step(dict(data))
    b.eval()
    with torch.no_grad():
        assert len(b.backbone(data['img'])) == 3      # the eval forward works
