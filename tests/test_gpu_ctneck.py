"""CTResNetNeck on the device (necks/ct_resnet_neck.py, training.BackwardEngine._backward_ctneck, the autograd bridge).

  fixtures     outputs within BAR_OUT = 2e-4 of max|output| and gradients within BAR_GRAD = 2e-3 rel-L2 per tensor of the reference class's
               fp64 run (tests/golden/ctneck.npz) -- the project's bars for backbone and neck fixtures (tests/hrnet_ref.py,
               tests/darknet_ref.py).  Every train-mode case runs in train mode (batch statistics); a 32-wide stage runs at the padded
               pitch 64 (CTResNetNeck.bn_pitch), which the tape shows
  buffers      running_mean / running_var after one training forward at rtol 1e-4, atol 1e-5 * max|want| -- the bar of
               tests/test_gpu_bn_batch_stats.py::_check_buffers for a network's buffers -- and num_batches_tracked exactly
  bit for bit  eval forward == forward_lazy; loss.backward() through the bridge == the native trainer; two identical steps
  end to end   R18 + CTResNetNeck(512, (256, 128, 64)) on a 2 x 3 x 64 x 96 batch under CPRHead and P2PHead (one / four points per cell),
               strides=[4]: a trainer step and a bridge step, every trainable gradient finite and non-zero
  refusals     the bf16 compute mode and a recorded forward through an eval() neck raise their named errors"""
import pytest
import torch

from pointtinybenchmark_amd import synthetic
from tests import ctneck_ref as CR
from tests.test_gpu_fpn_extra import GRID4, _data, _NeckOnly

pytestmark = pytest.mark.gpu
R18_NECK = dict(type='CTResNetNeck', in_channel=512, num_deconv_filters=(256, 128, 64), num_deconv_kernels=(4, 4, 4), use_dcn=False)
KINDS = ['cpr', 'p2p', 'p2p4']


def _neck(cfg):
    import pointtinybenchmark_amd as P
    neck = P.build_neck(dict(type='CTResNetNeck', **CR.constructor_kwargs(cfg)))
    neck.load_state_dict(CR.case_state_dict(cfg, torch.float32), strict=True)
    return neck.cuda().train(cfg['train'])


@pytest.mark.parametrize('name', CR.CASE_NAMES)
def test_neck_forward_vs_fixture_and_restatement(name):
    from pointtinybenchmark_amd import ops
    cfg = CR.CASES[name]
    x = CR.case_input(cfg, torch.float32).cuda()
    neck = _neck(cfg)
    sd0 = {k: v.clone() for k, v in neck.state_dict().items()}
    with torch.no_grad():
        out, = neck([x])
        lazy, = neck.forward_lazy([x]) if not cfg['train'] else [ops.from_nchw(out)]
    assert torch.is_tensor(lazy) and torch.equal(ops.as_nchw(lazy), out), 'the lazy form is the materialised map'
    err = CR.output_error(name, out)
    print('\nERR ctneck forward %-16s %s %.3e (bar %.0e)' % (name, 'train' if cfg['train'] else 'eval', err, CR.BAR_OUT), flush=True)
    assert err <= CR.BAR_OUT, (name, err)
    sd1 = neck.state_dict()
    if not cfg['train']:
        assert all(torch.equal(sd0[k], sd1[k]) for k in sd0), 'eval mode updates no buffer'
        return
    for key in CR.stat_names(name):
        ref = torch.from_numpy(CR.stat(name, key))
        if key.endswith('num_batches_tracked'):
            assert int(sd1[key]) == int(ref) == 1, key
        else:
            got = sd1[key].double().cpu()
            assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max())), (key, float((got - ref).abs().max()))


@pytest.mark.parametrize('name', CR.DEVICE_TRAIN)
def test_neck_backward_vs_reference_gradients(name):
    """The recorded forward + BackwardEngine._backward_neck on the fixture's linear functional (dz = w) against the reference class's
    fp64 autograd: rel-L2 <= BAR_GRAD per tensor, on the norm and on the strided sample."""
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg = CR.CASES[name]
    neck = _neck(cfg)
    x = CR.case_input(cfg, torch.float32).cuda()
    eng = BackwardEngine(_NeckOnly(neck))
    eng._sink = {}
    eng.begin_step()
    tape = []
    out, = neck.forward_lazy([x], tape=tape)
    assert [r['kind'] for r in tape] == ['ct_stage'] * len(cfg['filters']) and tape[0]['n_in'] == 1
    for r, f in zip(tape, cfg['filters']):      # a 32-wide stage's maps sit at pitch 64, pad channels exact zeros
        assert r['y1'].shape[-1] == r['o2'].shape[-1] == neck.bn_pitch(f) and not bool(r['o1'][..., f:].any()) and not bool(r['o2'][..., f:].any())
    assert out.shape[-1] == cfg['filters'][-1]
    dz = CR.functional_weight(cfg, (out.shape[0], out.shape[3], out.shape[1], out.shape[2]), torch.float32).permute(0, 2, 3, 1).contiguous().cuda()
    d_stage = eng._backward_neck(neck, tape, dz)
    params = dict(neck.named_parameters())
    grads = dict(zip(params, eng.collect(list(params.values()))))
    torch.cuda.synchronize()
    assert sorted(d_stage) == [0]
    grads[CR.INPUT] = d_stage[0].permute(0, 3, 1, 2)
    assert set(grads) == set(CR.grad_names(name))
    failed, worst = [], 0.0
    for k in sorted(grads):
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        en, es = CR.grad_errors(name, k, grads[k])
        worst = max(worst, en, es)
        print('ERR ctneck backward %-10s %-34s norm %.2e  sample rel-L2 %.2e (bar %.0e)' % (name, k, en, es, CR.BAR_GRAD), flush=True)
        if not (en <= CR.BAR_GRAD and es <= CR.BAR_GRAD):
            failed.append((k, en, es))
    assert not failed, failed
    print('ERR ctneck backward %s worst %.3e' % (name, worst), flush=True)


# ------------------------------------------------------------------------------------------------ the whole locator
def build_locator(kind, C=2, seed=3):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(18, C) if kind == 'cpr' else p2p_model_cfg(18, C)
    cfg['neck'] = dict(R18_NECK)
    cfg['bbox_head'] = dict(cfg['bbox_head'], in_channels=64, strides=[4], **(dict(point_anchor=list(GRID4)) if kind == 'p2p4' else {}))
    m = P.build_detector(cfg).cuda()
    kw = dict(head_std=0.3) if kind == 'cpr' else dict(head_std=0.05, num_points=4 if kind == 'p2p4' else 1)
    sd = synthetic.locator_state_dict(18, C, 0, 'cpr' if kind == 'cpr' else 'p2p', seed, **kw)
    sd = {k: (v[:, :64].contiguous() if k.endswith('_convs.0.conv.weight') else v) for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.ctneck_state_dict(512, (256, 128, 64), seed + 1))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def _trainer(kind):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return CprTrainer if kind == 'cpr' else P2PTrainer


def _small_data():
    return _data(seed=8, hw=(64, 96))[1]


@pytest.mark.parametrize('kind', KINDS)
def test_trainer_step_bridge_step_and_their_bits(kind):
    from pointtinybenchmark_amd import autograd_bridge
    data = _small_data()
    ma = build_locator(kind)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr = _trainer(kind)(ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    assert sum(k.startswith('neck.') for k in want) == 18
    for k, g in want.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, 'gradient of %s: finite and non-zero' % k
    assert all(int(v) == 1 for k, v in ma.state_dict().items() if k.startswith('neck.') and k.endswith('num_batches_tracked'))
    mb = build_locator(kind)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    la_total = float(sum((sum(v) if isinstance(v, (list, tuple)) else v) for k, v in la.items() if 'loss' in k))
    assert abs(out['log_vars']['loss'] - la_total) <= 1e-6 * max(1.0, abs(la_total))
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
    sa, sb = ma.state_dict(), mb.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa if k.startswith('neck.')), 'the same running statistics from either driver'
    # a second trainer on a third identical model: two optimisation steps, bit for bit
    mc = build_locator(kind)
    trc = _trainer(kind)(mc)
    trc.forward_backward(**data)
    assert torch.equal(tr.flat_g, trc.flat_g)
    for t in (tr, trc):
        t.step()
    for _ in range(2):
        for t in (tr, trc):
            t.forward_backward(**data)
            t.step()
        torch.cuda.synchronize()
        assert torch.equal(tr.flat_g, trc.flat_g)
    pa, pc = dict(ma.named_parameters()), dict(mc.named_parameters())
    for k in pa:
        assert torch.equal(pa[k], pc[k]), k
    assert bool(torch.isfinite(tr.flat_p).all())


def test_eval_forward_of_the_locator_is_forward_lazy_and_deterministic():
    from pointtinybenchmark_amd import ops
    m = build_locator('p2p').eval()
    data = _small_data()
    with torch.no_grad():
        feats = m.backbone(data['img'])
        out, = m.neck(feats)
        lazy, = m.neck.forward_lazy(feats)
        again, = m.neck(feats)
    assert tuple(out.shape) == (2, 64, 16, 24), 'stride 4, 64 channels from a stride-32 C5'
    assert torch.equal(ops.as_nchw(lazy), out) and torch.equal(out, again)
    want = CR.net({k[len('neck.'):]: v.double().cpu() for k, v in m.state_dict().items() if k.startswith('neck.')},
                  feats[-1].double().cpu(), 3, False)
    err = float((out.double().cpu() - want).abs().max() / want.abs().max())
    print('\nERR ctneck R18 eval forward %.3e (bar %.0e)' % (err, CR.BAR_OUT), flush=True)
    assert err <= CR.BAR_OUT


def test_bf16_and_eval_mode_with_a_tape_are_refused_by_name():
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer
    data = _small_data()
    m = build_locator('cpr')
    with pytest.raises(NotImplementedError, match='CTResNetNeck.*fp32 compute mode only'):
        m.set_compute_dtype('bf16')
    m.backbone.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match='CTResNetNeck.*fp32 compute mode only'):
        CprTrainer(m)
    assert 'CTResNetNeck' in autograd_bridge.unsupported_reason(m)
    m.backbone.compute_dtype = torch.float32
    with torch.no_grad(), pytest.raises(NotImplementedError, match='CTResNetNeck.*fp32 compute mode only'):
        m.neck([f.to(torch.bfloat16) for f in m.backbone(data['img'])])
    tr = CprTrainer(m)
    m.neck.eval()
    with pytest.raises(NotImplementedError, match='CTResNetNeck in eval'):
        tr.forward_backward(**data)
    assert 'CTResNetNeck in eval() mode' in autograd_bridge.unsupported_reason(m, data['gt_bboxes'], data['gt_labels'])
