"""-m gpu: dilated ResNet / ResNetV1d / ResNeXt stages (``dilations`` at stride 1) on the dilated HIP kernels.

  fixture    tests/golden/dilated.npz (the reference's own classes in fp64, tools/gen_dilated.py; B = 2, eval BatchNorm): stage outputs
             <= 2e-4 of max|level|; every trainable gradient of the fixture's linear functional <= 2e-3 rel-L2 with norm agreement.  The
             gradients are taken by the backward walk writing into ``p.grad`` as the native trainers do and by the same walk handing
             fresh tensors to the autograd bridge (``_sink``): bit-equal.  The third way, ``loss.backward()`` through the bridge, is
             the locator tests below (bit-equal to the trainers).
  batch statistics   R18, norm_eval=False, trainable dilated stages: every recorded block replayed in fp64 autograd with the kernel's
             own ReLU patterns (the method and the 1e-4 bar of tests/test_gpu_bn_batch_stats.py)
  neck       a dilated net hands the FPN adjacent levels of EQUAL size: gn_apply(up=) and upsample_add_bwd at scale 1 against fp64
             F.interpolate(size=) + add and its adjoint -- forward exact to one rounded add, backward exact
  locator    P2P with the dc5_18 backbone and a 4-level FPN, CPR with it at num_outs=1: trainer and loss.backward() bit-equal and
             finite; two steps from the same state bit-equal; a fresh model holding the stepped weights gives the same forward (the
             in-place pack refresh reaches the dilated layers)
  dispatch   the dilated layers reach the dilated entries and never a Winograd one; an undilated net never reaches a dilated entry
  bf16       the four refusals"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic
from tests import dilated_ref as DR

pytestmark = pytest.mark.gpu


def _rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _case_model(name):
    cfg = DR.CASES[name]
    m = DR.build(cfg).cuda()
    m.load_state_dict(DR.state_dict(cfg), strict=True)
    m.train()
    return cfg, m


@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_stage_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = DR.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
    torch.cuda.synchronize()
    assert len(outs) == 4
    failed = []
    for l, o in enumerate(outs):
        e = DR.output_error(name, l, o)
        print('ERR forward %-12s stage %d %-10s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[2:]), e), flush=True)
        if not e <= DR.BAR_OUT:
            failed.append((l, e))
        assert torch.equal(o, again[l])
    assert not failed, failed


def _walk(name, sink):
    """Recorded forward + BackwardEngine._backward_backbone on the fixture's functional.  sink: True hands fresh tensors out (the
    autograd bridge's mode), False writes into p.grad (the native trainers' mode)."""
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg, m = _case_model(name)
    eng = BackwardEngine(m)
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    if sink:
        eng._sink = {}
    else:
        for _, p in named:
            p.grad = torch.zeros_like(p)
    tape = []
    outs = m(DR.case_input(cfg).cuda(), tape=tape)
    with torch.no_grad():       # the forward-only path (fused projection shortcut) gives the recorded one's bits
        plain = m(DR.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    d_stage = {l: DR.functional_weight(cfg, l, o.shape).permute(0, 2, 3, 1).contiguous().cuda() for l, o in enumerate(outs)
               if l + 1 > cfg['frozen_stages']}
    eng._backward_backbone(m, tape, d_stage)
    assert [k for k, _ in named] == DR.grad_names(name)
    if sink:
        grads = dict(zip([k for k, _ in named], eng.collect([p for _, p in named])))
    else:
        if eng.side is not None:
            torch.cuda.current_stream().wait_stream(eng.side)
        grads = {k: p.grad for k, p in named}
    torch.cuda.synchronize()
    return grads


@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    grads = _walk(name, sink=False)
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        en, es = DR.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= DR.BAR_GRAD and es <= DR.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-12s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    assert not failed, failed[:8]
    bridge = _walk(name, sink=True)
    assert list(bridge) == list(grads)
    for k in grads:
        assert torch.equal(bridge[k], grads[k]), k


# ------------------------------------------------------------------------------------------------ dispatch
def test_dilated_layers_reach_the_dilated_entries_and_nothing_else_does(monkeypatch):
    from pointtinybenchmark_amd import _lib
    from pointtinybenchmark_amd.training import BackwardEngine
    real = _lib.call

    def run(cfg, hw):
        m = DR.build(cfg).cuda()
        m.load_state_dict(DR.state_dict(cfg), strict=True)
        m.train()
        eng = BackwardEngine(m)
        eng._sink = {}
        calls = []

        def spy(name, *args, **kw):
            calls.append(name)
            return real(name, *args, **kw)
        monkeypatch.setattr(_lib, 'call', spy)
        tape = []
        outs = m(torch.randn((2, 3) + hw, generator=torch.Generator().manual_seed(1)).cuda(), tape=tape)
        d_stage = {l: torch.ones(tuple(o.shape), device='cuda').permute(0, 2, 3, 1).contiguous() for l, o in enumerate(outs) if l > 0}
        eng._backward_backbone(m, tape, d_stage)
        eng.collect([p for p in m.parameters() if p.requires_grad])
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, 'call', real)
        return m, calls
    # 640 x 640 would put layer3 on 40 x 40 maps; 320 x 336 gives 20 x 21 at stride 16: layer3 (d = 2) and layer4 (d = 4) of the
    # OS8 net at a size where an UNDILATED 3x3 of layer2 (40 x 42) is Winograd-eligible
    m, calls = run(dict(DR.CASES['os8_50']), (320, 336))
    n3x3 = len(m.layer3) + len(m.layer4)
    assert calls.count('cpr_conv2d_fwd_dil') == 2 * n3x3            # forward + data gradient of every dilated conv2
    assert calls.count('cpr_conv2d_wgrad_dil') == n3x3
    assert any('wino' in c for c in calls)                          # the undilated layer2 keeps its Winograd route
    x, calls = run(dict(DR.CASES['dc5_x50']), (128, 160))
    assert calls.count('cpr_conv_group_fwd_dil') == 2 * len(x.layer4) and calls.count('cpr_conv_group_wgrad_dil') == len(x.layer4)
    assert 'cpr_conv2d_fwd_dil' not in calls
    plain = dict(DR.CASES['os8_50'], strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1))
    _, calls = run(plain, (128, 160))
    assert calls and not [c for c in calls if c.endswith('_dil')]


# ------------------------------------------------------------------------------------------------ batch statistics
def _block_fp64(blk, x, P, masks):
    """fp64 torch autograd of one block with training-mode BatchNorm; the ReLUs take their 0/1 pattern from the kernel's recorded
    outputs (tests/test_gpu_bn_batch_stats.py, with each conv's own padding and dilation)."""
    def bn(t, mod):
        return F.batch_norm(t, None, None, P[id(mod.weight)], P[id(mod.bias)], True, 0.1, mod.eps)

    def conv(t, c):
        return F.conv2d(t, P[id(c.weight)], None, c.stride, c.padding, c.dilation, c.groups)

    def relu(t, mk):
        return t * (mk > 0).to(t.dtype)
    o = relu(bn(conv(x, blk.conv1), blk.bn1), masks[0])
    if blk.kind == 'bottleneck':
        o = relu(bn(conv(o, blk.conv2), blk.bn2), masks[1])
        o = bn(conv(o, blk.conv3), blk.bn3)
    else:
        o = bn(conv(o, blk.conv2), blk.bn2)
    idn = x
    if blk.downsample is not None:
        idn = bn(conv(idn, blk.ds_conv), blk.ds_bn)
    return relu(o + idn, masks[2])


def test_batch_statistics_backward_vs_fp64_autograd_per_block():
    """R18 OS8 (layer3 d = 2, layer4 d = 4), norm_eval=False, frozen_stages=1, 2 x 3 x 93 x 131: every recorded block replayed in fp64
    autograd from the block input and output gradient the engine saw: forward, parameter gradients and input gradient within 1e-4."""
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    from pointtinybenchmark_amd.training import BackwardEngine
    m = ResNet(depth=18, frozen_stages=1, norm_eval=False, **DR.OS8).cuda()
    m.load_state_dict(synthetic.resnet_state_dict(18, 3, prefix=''), strict=True)
    m.train()
    assert m.batch_stats_active()
    eng = BackwardEngine(m)
    eng._sink = {}
    g = torch.Generator().manual_seed(3)
    img = torch.randn((2, 3, 93, 131), generator=g)
    tape = []
    outs = m(img.cuda(), tape=tape)
    assert [tuple(o.shape[2:]) for o in outs] == [(24, 33), (12, 17), (12, 17), (12, 17)]
    d_stage = {i: torch.randn(tuple(o.shape), generator=g).permute(0, 2, 3, 1).contiguous().cuda() for i, o in enumerate(outs) if i > 0}
    seen = {}
    rule = eng._block_backward_batch_stats

    def spy(cache, blk, rec, dout, need_dx):
        seen[id(rec)] = (dout[0] if isinstance(dout, tuple) else dout).clone()
        r = rule(cache, blk, rec, dout, need_dx)
        seen[id(rec), 'dx'] = None if r is None else r.clone()
        return r
    eng._block_backward_batch_stats = spy
    eng._backward_backbone(m, tape, d_stage)
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    got = dict(zip([id(p) for _, p in named], eng.collect([p for _, p in named])))
    torch.cuda.synchronize()
    assert len(tape) == 6 and all(id(r) in seen for r in tape)

    def nchw64(t):
        return t.detach().double().cpu().permute(0, 3, 1, 2)
    bad, worst, dilated = [], 0.0, 0
    for rec in tape:
        blk = rec['block']
        dilated += blk.conv1.dilation[0] > 1
        P = {id(p): p.detach().double().cpu().clone().requires_grad_(True) for p in blk.parameters()}
        x = nchw64(rec['x']).clone().requires_grad_(True)
        masks = [nchw64(rec['o1']), None, nchw64(rec['out'])]
        out = _block_fp64(blk, x, P, masks)
        errs = [('forward', _rel_l2(nchw64(rec['out']), out))]
        (out * nchw64(seen[id(rec)])).sum().backward()
        errs += [(n, _rel_l2(got[id(p)], P[id(p)].grad)) for n, p in blk.named_parameters()]
        if seen[id(rec), 'dx'] is not None:
            errs.append(('dx', _rel_l2(nchw64(seen[id(rec), 'dx']), x.grad)))
        worst = max([worst] + [e for _, e in errs])
        bad += [(e, rec['stage'], n) for n, e in errs if e > 1e-4]
    assert dilated == 4
    print('ERR batch statistics r18 os8 per block: worst rel-L2 %.2e (bar 1e-4)' % worst, flush=True)
    assert not bad, 'block mismatch (rel L2, stage, what): %s' % sorted(bad, reverse=True)[:8]


# ------------------------------------------------------------------------------------------------ neck at scale 1
def test_top_down_add_between_levels_of_equal_size():
    """Two 9 x 12 x 256 levels: fine = x * a + b + up(coarse) with a nearest scale of 1 is the plain sum -- exact to the one rounded
    add per element (the affine is the kernel's own fma, taken from a run without ``up``); its adjoint copies each cell."""
    from pointtinybenchmark_amd import ops
    N, H, W, C = 2, 9, 12, 256
    g = torch.Generator().manual_seed(21)
    x, coarse, dfine = (torch.randn((N, H, W, C), generator=g) for _ in range(3))
    a, b = torch.rand((N, C), generator=g) + 0.5, torch.randn((N, C), generator=g)
    xd, cd = x.cuda(), coarse.cuda()
    base = ops.gn_apply(xd, a.cuda(), b.cuda())
    got = ops.gn_apply(xd, a.cuda(), b.cuda(), up=cd)
    up64 = F.interpolate(coarse.double().permute(0, 3, 1, 2), size=(H, W), mode='nearest').permute(0, 2, 3, 1)
    assert torch.equal(up64, coarse.double())
    want = (base.cpu().double() + up64).float()          # one rounded add
    assert torch.equal(got.cpu(), want)
    ref = x.double() * a.double()[:, None, None, :] + b.double()[:, None, None, :] + up64
    assert float((got.cpu().double() - ref).abs().max()) <= 2.0 ** -22 * float(ref.abs().max())
    # adjoint: d coarse = sum over the children = the one cell itself
    c64 = coarse.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    (F.interpolate(c64, size=(H, W), mode='nearest') * dfine.double().permute(0, 3, 1, 2)).sum().backward()
    ref_b = c64.grad.permute(0, 2, 3, 1)
    assert torch.equal(ops.upsample_add_bwd(dfine.cuda(), (N, H, W, C)).cpu().double(), ref_b)
    acc = coarse.cuda().clone()
    ops.upsample_add_bwd(dfine.cuda(), acc)
    assert torch.equal(acc.cpu(), coarse + dfine)


# ------------------------------------------------------------------------------------------------ locators
def _locator(head, seed=3, depth=18):
    """BasicLocator on the dc5_18 backbone (R18; depth=50: the same on R50, strides (1, 2, 2, 1), dilations (1, 1, 1, 2): levels of 1/4, 1/8, 1/16, 1/16): P2P with
    a 4-level FPN, CPR with num_outs=1."""
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(depth, 1) if head == 'cpr' else p2p_model_cfg(depth, 2)
    cfg['backbone'] = dict(cfg['backbone'], **DR.DC5)
    C, npts = 1, 1
    if head == 'p2p':
        C, npts = 2, 4
        cfg['neck'] = dict(cfg['neck'], num_outs=4)
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16, 16], point_anchor=[(-.25, -.25), (.25, -.25), (-.25, .25), (.25, .25)])
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, C, 0, head, seed, head_std=0.05, num_points=npts)
    if head == 'p2p':
        sd.update(synthetic.fpn_state_dict(synthetic.backbone_out_channels(depth), 256, 0, 4, seed + 1))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def _data(head, seed=4):
    batch = synthetic.synthetic_batch(2, 128, 160, 6, 1 if head == 'cpr' else 2, seed=seed)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def _trainer(head, m, **kw):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return (CprTrainer if head == 'cpr' else P2PTrainer)(m, **kw)


@pytest.mark.parametrize('head', ['p2p', 'cpr'])
def test_bridge_is_bit_equal_to_the_trainer_and_steps_repeat(head):
    from pointtinybenchmark_amd import autograd_bridge
    data = _data(head)
    ma = _locator(head)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    with torch.no_grad():
        feats = ma.backbone(data['img'])
    assert [tuple(f.shape[2:]) for f in feats] == [(32, 40), (16, 20), (8, 10), (8, 10)]       # the two deepest levels: equal size
    tr = _trainer(head, ma, lr=0.01)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    k4 = 'backbone.layer4.1.conv1.weight'
    assert ma.backbone.layer4[1].conv1.dilation == (2, 2) and float(want[k4].abs().max()) > 0
    for v in la.values():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            assert bool(torch.isfinite(t).all())
    mb = _locator(head)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad
    out['loss'].backward()
    torch.cuda.synchronize()
    n = 0
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]) and bool(torch.isfinite(p.grad).all()), k
            n += 1
        else:
            assert p.grad is None, k
    assert n == len(want) and n > 0
    # two optimizer steps from the same state, twice: the packs of the dilated layers are refreshed in place after each update
    mc = _locator(head)
    trc = _trainer(head, mc, lr=0.01)
    for _ in range(2):
        tr.forward_backward(**data)
        tr.step()
        trc.forward_backward(**data)
        trc.step()
        torch.cuda.synchronize()
        assert torch.equal(tr.flat_g, trc.flat_g)
    pa, pc = dict(ma.named_parameters()), dict(mc.named_parameters())
    for k in pa:
        assert torch.equal(pa[k], pc[k]), k
    assert not torch.equal(pa[k4], dict(mb.named_parameters())[k4])         # the dilated layer moved
    # ... and a fresh model holding the stepped weights computes the same forward as the stepped model's refreshed packs
    fresh = _locator(head)
    fresh.load_state_dict({k: v.detach().clone() for k, v in ma.state_dict().items()}, strict=True)
    ma.eval(), fresh.eval()
    with torch.no_grad():
        a, b = ma.backbone(data['img']), fresh.backbone(data['img'])
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), 'forward after the steps differs from a fresh model in %d entries' % int((x != y).sum())


# ------------------------------------------------------------------------------------------------ bf16
def test_bf16_mode_raises_naming_dilations():
    from pointtinybenchmark_amd import autograd_bridge, ops
    m = _locator('cpr')
    with pytest.raises(NotImplementedError, match='dilations'):
        m.set_compute_dtype('bf16')
    m.backbone.compute_dtype = torch.bfloat16
    assert 'dilations' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='dilations'):
        _trainer('cpr', m)
    with pytest.raises(NotImplementedError, match='dilations'):
        m.backbone(torch.zeros((1, 3, 64, 64), device='cuda'))
    w = torch.zeros((64, 64, 3, 3), device='cuda')
    with pytest.raises(NotImplementedError, match='dilation'):
        ops.PackedConv(w, 1, 2, torch.bfloat16, dilation=2)
    with pytest.raises(NotImplementedError, match='dilation'):
        ops.dgrad_pack(w, 1, 2, dtype=torch.bfloat16, dilation=2)
