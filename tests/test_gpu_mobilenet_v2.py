"""-m gpu: the MobileNetV2 backbone (backbones/mobilenet_v2.py) on the depthwise kernels (csrc/mbv2.hip), the dense 1x1 path at padded
pitches and the 3x3 stem.

  fixture    tests/golden/mobilenet_v2.npz (the reference's own MobileNetV2 in fp64, tools/gen_mobilenet_v2.py): stage outputs <= 2e-4
             max|level|, parameter gradients of the fixture's linear functional through BackwardEngine._backward_backbone <= 2e-3
             rel-L2; the recorded forward has the forward-only bits; pad channels of every stage output buffer and of every gradient
             handed down are bit-zero
  per block  'base' replayed block by block in fp64 autograd of tests/mobilenet_v2_ref's restatement from the recorded input and output
             gradient with the kernels' own clamp patterns, within 1e-4 (the bar and method of the sibling per-block tests)
  neck       FPN(num_outs=5, add_extra_convs='on_input') on the padded 24- / 32-channel outputs read in place, against fp64 autograd of
             tests/fpn_extra_ref.fpn_forward on the compact outputs
  locator    P2PTrainer / CprTrainer with frozen_stages=-1 at 70 x 90: gradients bit-equal to loss.backward() through the autograd
             bridge; after one optimizer step a fresh model holding the stepped weights gives the same forward bit for bit (the packs,
             depthwise ones included, were rebuilt); the bf16 compute mode raises, naming ``MobileNetV2``"""
import pytest
import torch
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic
from tests import fpn_extra_ref as FR
from tests import mobilenet_v2_ref as MB

pytestmark = pytest.mark.gpu
NECK_IN = [24, 32, 96, 1280]


def _rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _bit_zero(t):
    return t.numel() == 0 or int(torch.count_nonzero(t.contiguous().view(torch.int32))) == 0


def _case_model(name):
    import pointtinybenchmark_amd as P
    cfg = MB.CASES[name]
    m = P.build_backbone(dict(type='MobileNetV2', **MB.mobilenet_kwargs(cfg))).cuda()
    m.load_state_dict(MB.case_state_dict(cfg), strict=True)
    m.train()
    return cfg, m


def _pads_are_zero(m, outs):
    """Every stage output: the reference's shape; a padded stage's view carries its buffer, whose pad channels are bit-zero."""
    from pointtinybenchmark_amd import ops
    stages = sorted(set(m.out_indices))
    assert len(outs) == len(stages)
    for i, o in zip(stages, outs):
        C = m.stage_widths[i]
        assert o.shape[1] == C
        buf = ops.padded_buffer(o)
        assert (buf is not None) == (C % 32 != 0), (i, C)
        if buf is not None:
            assert buf.shape[-1] == ops.pad32(C) and _bit_zero(buf[..., C:]) and torch.equal(buf[..., :C].permute(0, 3, 1, 2), o)


@pytest.mark.parametrize('name', MB.CASE_NAMES)
def test_stage_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = MB.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
        nhwc4 = m(img.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))      # the other input layout of the stem: the same bits
    torch.cuda.synchronize()
    _pads_are_zero(m, outs)
    failed = []
    for l, o in enumerate(outs):
        e = MB.output_error(name, l, o)
        print('ERR forward %-6s output %d %-14s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[1:]), e), flush=True)
        if not e <= MB.BAR_OUT:
            failed.append((l, e))
        assert torch.equal(o, again[l]) and torch.equal(o, nhwc4[l])
    assert not failed, failed
    if 7 in cfg['out_indices']:
        assert float(outs[-1].max()) == 6.0 and float(outs[-1].min()) == 0.0      # conv2's map leaves clamped
    assert len(nhwc4) == len(outs)


def _engine_backward(m, cfg, spy=None):
    """The recorded forward and BackwardEngine._backward_backbone on the fixture's linear functional -> (outs, tape, {name: gradient})."""
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.training import BackwardEngine
    eng = BackwardEngine(m)
    eng._sink = {}
    if spy is not None:
        spy(eng)
    tape = []
    outs = m(MB.case_input(cfg).cuda(), tape=tape)
    d_stage = {}
    for l, (stage, o) in enumerate(zip(sorted(set(m.out_indices)), outs)):
        if stage == 7 or stage + 1 > cfg['frozen_stages']:
            w = MB.functional_weight(cfg, l, o.shape).permute(0, 2, 3, 1)
            d = torch.zeros(tuple(w.shape[:3]) + (ops.pad32(w.shape[3]),))
            d[..., :w.shape[3]] = w
            d_stage[l] = d.cuda()
    eng._backward_backbone(m, tape, d_stage)
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    grads = {k: g for (k, _), g in zip(named, eng.collect([p for _, p in named])) if g is not None}
    torch.cuda.synchronize()
    return outs, tape, grads


@pytest.mark.parametrize('name', MB.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    """Against the reference class's fp64 autograd: rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample.  The gradient every
    block hands down keeps bit-zero pad channels; the recorded forward has the forward-only bits."""
    from pointtinybenchmark_amd import ops
    cfg, m = _case_model(name)
    handed = []

    def spy(eng):
        rule = eng._block_backward

        def wrapped(cache, blk, rec, dout, need_dx, **kw):
            dx = rule(cache, blk, rec, dout, need_dx, **kw)
            if dx is not None:
                handed.append((rec['x'].shape[-1], blk.in_channels if blk.kind == 'mbv2' else blk.conv.in_channels,
                               dx[0] if isinstance(dx, tuple) else dx))
            return dx
        eng._block_backward = wrapped
    outs, tape, grads = _engine_backward(m, cfg, spy)
    with torch.no_grad():
        plain = m(MB.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    _pads_are_zero(m, outs)
    assert list(grads) == MB.grad_names(name)
    assert handed and (tape[0].get('stem') is True) == (cfg['frozen_stages'] < 0)
    for Cp, C, dx in handed:
        assert dx.shape[-1] == Cp == ops.pad32(C) and _bit_zero(dx[..., C:]), (C, tuple(dx.shape))
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
        en, es = MB.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= MB.BAR_GRAD and es <= MB.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-6s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    assert not failed, failed[:8]


def _conv_bn64(mod, P, x, stride=1, padding=0, groups=1):
    bn = mod.bn
    y = F.conv2d(x, P[id(mod.conv.weight)], None, stride, padding, 1, groups)
    return F.batch_norm(y, bn.running_mean.double().cpu(), bn.running_var.double().cpu(), P[id(bn.weight)], P[id(bn.bias)], False, 0.0, bn.eps)


def _act_as_recorded(v, m):
    """ReLU6 with the kernel's own pattern: 6 where the recorded map clamped (>= 6), v where it is inside (0, 6), 0 where it is 0."""
    return torch.where(m >= 6, torch.full_like(v, 6.0), torch.where(m > 0, v, torch.zeros_like(v)))


def test_backward_vs_fp64_autograd_per_block():
    """'base' (everything trains): every recorded block and conv2 replayed in fp64 autograd from the block input and the output gradient
    the engine saw: forward, parameter gradients and input gradient within 1e-4."""
    cfg, m = _case_model('base')
    seen = {}

    def spy(eng):
        rule = eng._mbv2_block_backward

        def wrapped(cache, blk, rec, dout, need_dx):
            seen[id(rec)] = dout.clone()
            r = rule(cache, blk, rec, dout, need_dx)
            seen[id(rec), 'dx'] = None if r is None else (r[0] if isinstance(r, tuple) else r).clone()
            return r
        eng._mbv2_block_backward = wrapped
    outs, tape, grads = _engine_backward(m, cfg, spy)
    recs = [r for r in tape if not r.get('stem')]
    assert len(recs) == 18 and all(id(r) in seen for r in recs)
    names = {id(p): k for k, p in m.named_parameters()}
    torch.set_num_threads(min(torch.get_num_threads(), 16))

    def nchw64(t):
        return t.detach().double().cpu().permute(0, 3, 1, 2)
    bad, worst = [], 0.0
    for bi, rec in enumerate(recs):
        blk = rec['block']
        P = {id(p): p.detach().double().cpu().clone().requires_grad_(True) for p in blk.parameters()}
        Cin = blk.in_channels if blk.kind == 'mbv2' else blk.conv.in_channels
        Cout = blk.out_channels if blk.kind == 'mbv2' else blk.conv.out_channels
        x = nchw64(rec['x'])[:, :Cin].clone().requires_grad_(True)
        if blk.kind == 'mbv2_conv2':
            out = _act_as_recorded(_conv_bn64(blk, P, x), nchw64(rec['out']))
        else:
            M = blk.mid_channels
            o = x
            if blk.with_expand_conv:
                o = _act_as_recorded(_conv_bn64(blk.expand_conv, P, o), nchw64(rec['o1'])[:, :M])
            else:
                o = o.clamp(max=6.0)      # layer1.0 reads the stem's ReLU(v) map
            o = _act_as_recorded(_conv_bn64(blk.depthwise_conv, P, o, blk.stride, 1, M), nchw64(rec['o2'])[:, :M])
            out = _conv_bn64(blk.linear_conv, P, o)
            if blk.with_res_shortcut:
                out = out + x
        errs = [('forward', _rel_l2(nchw64(rec['out'])[:, :Cout], out))]
        (out * nchw64(seen[id(rec)])[:, :Cout]).sum().backward()
        errs += [(n, _rel_l2(grads[names[id(p)]], P[id(p)].grad)) for n, p in blk.named_parameters()]
        if seen[id(rec), 'dx'] is not None:
            want = x.grad
            if blk.kind == 'mbv2' and not blk.with_expand_conv:      # the rule's g1 is already taken through the stem's ReLU
                want = want * (x.detach() > 0)
            errs.append(('dx', _rel_l2(nchw64(seen[id(rec), 'dx'])[:, :Cin], want)))
        worst = max([worst] + [e for _, e in errs])
        bad += [(e, rec['stage'], bi, n) for n, e in errs if e > 1e-4]
    print('ERR backward base per block: worst rel-L2 %.2e (bar 1e-4)' % worst, flush=True)
    assert not bad, 'block mismatch (rel L2, stage, block, what): %s' % sorted(bad, reverse=True)[:8]


# ------------------------------------------------------------------------------------------------ the neck on padded maps
class _BackboneNeck(torch.nn.Module):
    def __init__(self, backbone, neck):
        super().__init__()
        self.backbone, self.neck, self.bbox_head = backbone, neck, None


def test_fpn_reads_the_padded_maps_in_place_vs_fp64_autograd(monkeypatch):
    """The 24- and 32-channel maps (24 sits at pitch 32): FPN with an 'on_input' extra level on the backbone's own views.  Reference:
    fp64 autograd of fpn_extra_ref.fpn_forward on the compact (contiguous, fp64) copies of the same stage outputs."""
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg, bb = _case_model('base')
    neck = P.build_neck(dict(type='FPN', in_channels=NECK_IN, out_channels=64, num_outs=5, add_extra_convs='on_input',
                             norm_cfg=dict(type='GN', num_groups=32))).cuda()
    sd = synthetic.fpn_state_dict(NECK_IN, 64, 0, 5, 11, prefix='', add_extra_convs='on_input')
    neck.load_state_dict(sd, strict=True)
    copies, n_copied = [], ops.NECK_INPUT_COPIES[0]
    real = ops.nchw_to_nhwc
    monkeypatch.setattr(ops, 'nchw_to_nhwc', lambda x: copies.append(tuple(x.shape)) or real(x))
    with torch.no_grad():
        feats = bb(MB.case_input(cfg).cuda())
    assert ops.padded_buffer(feats[0]) is not None and ops.padded_buffer(feats[1]) is None
    eng = BackwardEngine(_BackboneNeck(bb, neck))
    eng._sink = {}
    eng.begin_step()
    tape = []
    lazy = neck.forward_lazy(feats, tape=tape)
    assert not copies and ops.NECK_INPUT_COPIES[0] == n_copied, copies   # no map took the copying route
    with torch.no_grad():
        outs = neck(feats)
    assert len(outs) == len(lazy) == 5
    for l, (raw, (a, b)) in enumerate(lazy):
        assert torch.equal(ops.as_nchw(ops.gn_apply(raw, a, b)), outs[l])
    ws = [FR.functional_weight(dict(seed=cfg['seed']), l, o.shape) for l, o in enumerate(outs)]
    dzs = [w.float().permute(0, 2, 3, 1).contiguous().cuda() for w in ws]
    d_stage = eng._backward_neck(neck, tape, dzs)
    params = dict(neck.named_parameters())
    grads = dict(zip(params, eng.collect(list(params.values()))))
    torch.cuda.synchronize()
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = [f.detach().double().cpu().contiguous().requires_grad_(True) for f in feats]
    ref = FR.fpn_forward(sd64, x64, 5, add_extra_convs='on_input')
    sum((w * o).sum() for w, o in zip(ws, ref)).backward()
    failed = []
    for l, o in enumerate(outs):
        e = float((o.double().cpu() - ref[l].detach()).abs().max() / ref[l].detach().abs().max())
        print('ERR neck forward level %d %-10s max|diff|/max|level| %.2e (bar 2e-4)' % (l, tuple(o.shape[2:]), e), flush=True)
        if not e <= MB.BAR_OUT:
            failed.append(('out%d' % l, e))
    for k in sorted(grads):
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        e = _rel_l2(grads[k], sd64[k].grad)
        if not e <= MB.BAR_GRAD:
            failed.append((k, e))
    assert tuple(grads['lateral_convs.0.conv.weight'].shape) == (64, 24, 1, 1)
    # the gradients handed to the stages arrive padded, pad channels bit-zero, real channels as autograd's
    assert sorted(d_stage) == [0, 1, 2, 3]
    for i in range(4):
        C = NECK_IN[i]
        assert d_stage[i].shape[-1] == ops.pad32(C) and _bit_zero(d_stage[i][..., C:])
        e = _rel_l2(d_stage[i][..., :C].permute(0, 3, 1, 2), x64[i].grad)
        print('ERR neck backward input %d (%d channels) rel-L2 %.2e (bar 2e-3)' % (i, C, e), flush=True)
        if not e <= MB.BAR_GRAD:
            failed.append(('in%d' % i, e))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ locator
def _locator(head, seed=3):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(type='MobileNetV2', out_indices=(1, 2, 4, 7), frozen_stages=-1, norm_eval=True)
    cfg['neck'] = dict(cfg['neck'], in_channels=NECK_IN)
    m = P.build_detector(cfg).cuda()
    m.load_state_dict(synthetic.locator_state_dict(num_classes=1, head=head, seed=seed, head_std=0.3, arch='mobilenet_v2'), strict=True)
    m.train()
    return m


def _data():
    batch = synthetic.synthetic_batch(2, 70, 90, 5, 1, seed=3, ragged=True)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def _trainer(head):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return CprTrainer if head == 'cpr' else P2PTrainer


@pytest.mark.parametrize('head', ['p2p', 'cpr'])
def test_bridge_is_bit_equal_to_the_trainer(head):
    data = _data()
    ma = _locator(head)
    tr = _trainer(head)(ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    for k, shape in (('backbone.conv1.conv.weight', (32, 3, 3, 3)), ('backbone.layer2.1.depthwise_conv.conv.weight', (144, 1, 3, 3)),
                     ('backbone.layer1.0.linear_conv.conv.weight', (16, 32, 1, 1)), ('backbone.conv2.conv.weight', (1280, 320, 1, 1)),
                     ('neck.lateral_convs.0.conv.weight', (256, 24, 1, 1))):
        assert tuple(want[k].shape) == shape and float(want[k].abs().max()) > 0 and bool(torch.isfinite(want[k]).all()), k
    assert 'backbone.conv1.bn.weight' in want and 'backbone.conv1.bn.bias' in want
    mb = _locator(head)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad
    out['loss'].backward()
    torch.cuda.synchronize()
    n = 0
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
            n += 1
        else:
            assert p.grad is None, k
    assert n == len(want) and n > 0
    for v in la.values():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            assert bool(torch.isfinite(t).all())


def test_optimizer_step_refreshes_the_packs_depthwise_ones_included():
    data = _data()
    m = _locator('p2p')
    tr = _trainer('p2p')(m, lr=0.05)
    with torch.no_grad():
        m.eval()
        before = [o.clone() for o in m.backbone(data['img'])]     # builds the packs the step must not leave stale
        m.train()
    out = tr.train_step(dict(data))
    torch.cuda.synchronize()
    assert all(v == v and abs(v) < float('inf') for v in out['log_vars'].values()), out['log_vars']
    assert any(k[0] == 'dw' for k in m.backbone._cache._d) and any(k[0] == 'dw_dgrad' for k in m.backbone._cache._d)
    out2 = tr.train_step(dict(data))                              # a second step on the stepped weights
    torch.cuda.synchronize()
    assert all(v == v and abs(v) < float('inf') for v in out2['log_vars'].values()), out2['log_vars']
    m.eval()
    fresh = _locator('p2p')
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    fresh.eval()
    with torch.no_grad():
        a, b = m.backbone(data['img']), fresh.backbone(data['img'])
        la, lb = m.extract_feat(data['img']), fresh.extract_feat(data['img'])
    torch.cuda.synchronize()
    assert not torch.equal(a[0], before[0])                       # frozen_stages=-1: everything moved
    for x, y in zip(list(a) + list(la), list(b) + list(lb)):
        assert torch.equal(x, y), 'forward after the step differs from a fresh model in %d entries' % int((x != y).sum())


def test_second_step_equals_a_fresh_model_built_from_the_updated_parameters():
    """One optimizer step, then the gradients of a second forward_backward against those of a fresh model (fresh packs and folds) that
    holds the stepped weights: bit-equal."""
    data = _data()
    m = _locator('p2p')
    tr = _trainer('p2p')(m, lr=0.05)
    tr.train_step(dict(data))
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    got = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}
    fresh = _locator('p2p')
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    trf = _trainer('p2p')(fresh, lr=0.05)
    trf.forward_backward(**data)
    torch.cuda.synchronize()
    for k, p in fresh.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, got[k]), k


def test_bf16_mode_raises_naming_the_backbone():
    from pointtinybenchmark_amd import autograd_bridge
    m = _locator('p2p')
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        m.set_compute_dtype('bf16')
    m.backbone.compute_dtype = torch.bfloat16
    assert 'MobileNetV2' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        m.backbone(torch.zeros((1, 3, 64, 64), device='cuda'))
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        _trainer('p2p')(m)
