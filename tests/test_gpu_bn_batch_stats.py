"""-m gpu: training-mode BatchNorm (ResNet norm_eval=False; T/mmdet/models/backbones/resnet.py:647-657, torch.nn.BatchNorm2d in
training mode) -- the kernels of csrc/bn_train.hip against fp64 torch, the backbone forward / training step against the CPU oracle
with its BatchNorm switched to batch statistics for the non-frozen stages (monkeypatched here; the oracle file is unchanged), the
autograd bridge, the eval-after-train refold, determinism, the multi-stream guard and the bf16 refusal."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import cpr_oracle as O
from oracle.gen_golden import CPR_CASES
from pointtinybenchmark_amd import ops, synthetic
from tests.test_gpu_cpr_parity import build_hip_locator, to_cuda

pytestmark = pytest.mark.gpu


def _rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ------------------------------------------------------------------------------------------------ kernels vs fp64 torch
def _ref_bn(y, gamma, beta, rm, rv, momentum, dout=None, relu=True, eps=1e-5):
    """fp64 torch: F.batch_norm in training mode on the NCHW view, (+ReLU), autograd for the gradients."""
    x = y.double().permute(0, 3, 1, 2).detach().requires_grad_(True)
    g = gamma.double().detach().requires_grad_(True)
    b = beta.double().detach().requires_grad_(True)
    rm, rv = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(x, rm, rv, g, b, True, momentum, eps)
    if relu:
        z = F.relu(z)
    out = dict(z=z.detach().permute(0, 2, 3, 1), rm=rm, rv=rv)
    if dout is not None:
        (z * dout.double().permute(0, 3, 1, 2)).sum().backward()
        out.update(dy=x.grad.permute(0, 2, 3, 1), dgamma=g.grad, dbeta=b.grad)
    return out


SHAPES = [(2, 40, 40, 256), (3, 7, 9, 64), (64, 20, 20, 2048), (4, 160, 160, 128)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('offset', [0.0, 1e3])
def test_kernels_match_fp64_torch(shape, offset):
    torch.manual_seed(sum(shape))
    C = shape[-1]
    dev = 'cuda'
    std = 1.0 + torch.rand(C, device=dev)
    y = (torch.randn(shape, device=dev) * std + offset * std + 0.3 * torch.randn(C, device=dev)).contiguous()
    gamma = 1.0 + 0.5 * torch.randn(C, device=dev)
    beta = 0.5 * torch.randn(C, device=dev)
    rm, rv = 0.1 * torch.randn(C, device=dev), 1.0 + torch.rand(C, device=dev)
    nbt = torch.zeros((), device=dev, dtype=torch.int64)
    dout = torch.randn(shape, device=dev)
    ref = _ref_bn(y, gamma, beta, rm, rv, 0.1, dout)
    rm_k, rv_k = rm.clone(), rv.clone()
    st = ops.bn_batch_stats(y, gamma, beta, rm_k, rv_k, nbt, 0.1, 1e-5)
    mean, rstd, scale, shift = st.mean, st.rstd, st.scale, st.shift
    z = ops.bn_apply(y, scale, st.cshift, center=st.center, relu=True)
    torch.cuda.synchronize()
    yd = y.double().reshape(-1, C)
    mu_ref, var_ref = yd.mean(0), yd.var(0, unbiased=False)
    sd_ref = var_ref.sqrt()
    # the mean is returned in fp32: beyond 1e-6 std, it can only be as close as its own rounding (half an ulp of |mean|)
    assert ((mean.double() - mu_ref).abs() <= 1e-6 * sd_ref + 2.0 ** -24 * mu_ref.abs()).all()
    var_k = 1.0 / rstd.double() ** 2 - 1e-5
    assert ((var_k - var_ref).abs() <= 1e-5 * var_ref).all()
    assert torch.allclose(scale.double(), gamma.double() * rstd.double(), rtol=1e-6, atol=0)
    assert torch.allclose(shift.double(), beta.double() - mean.double() * scale.double(), rtol=1e-5, atol=1e-5 * float(beta.abs().max()))
    assert float((z.double() - ref['z']).abs().max()) <= 1e-5 * float(ref['z'].abs().max())
    assert ((rm_k.double() - ref['rm']).abs() <= 1e-5 * ref['rm'].abs() + 1e-7).all()
    assert ((rv_k.double() - ref['rv']).abs() <= 1e-5 * ref['rv'].abs()).all()
    assert int(nbt) == 1
    dy, dg, db = ops.bn_train_bwd(dout, y, st.cmean, rstd, gamma, mask=z, center=st.center)
    torch.cuda.synchronize()
    assert _rel_l2(dy, ref['dy']) <= 1e-5
    assert _rel_l2(dg, ref['dgamma']) <= 1e-5
    assert _rel_l2(db, ref['dbeta']) <= 1e-5


def test_dual_apply_and_residual():
    torch.manual_seed(1)
    y, y2, r = (torch.randn(2, 20, 24, 128, device='cuda') for _ in range(3))
    s, b, s2, b2, c, c2 = (torch.randn(128, device='cuda') for _ in range(6))
    out = ops.bn_apply(y, s, b, center=c, y2=y2, scale2=s2, shift2=b2, center2=c2, relu=True)
    want = F.relu((y.double() - c.double()) * s.double() + b.double() + (y2.double() - c2.double()) * s2.double() + b2.double())
    assert float((out.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    out = ops.bn_apply(y, s, b, residual=r, relu=False)
    want = y.double() * s.double() + b.double() + r.double()
    assert float((out.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_momentum_none_and_single_row_refusal():
    torch.manual_seed(2)
    C = 64
    y = torch.randn(2, 5, 6, C, device='cuda')
    gamma, beta = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    rm, rv = torch.randn(C, device='cuda'), torch.rand(C, device='cuda') + 1
    bn = torch.nn.BatchNorm2d(C, momentum=None).cuda().double()
    bn.running_mean.copy_(rm)
    bn.running_var.copy_(rv)
    bn.num_batches_tracked.fill_(3)
    nbt = torch.full((), 3, device='cuda', dtype=torch.int64)
    rm_k, rv_k = rm.clone(), rv.clone()
    ops.bn_batch_stats(y, gamma, beta, rm_k, rv_k, nbt, None, 1e-5)
    bn.train()
    bn(y.double().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert int(nbt) == 4 and int(bn.num_batches_tracked) == 4
    assert torch.allclose(rm_k.double(), bn.running_mean, rtol=1e-5, atol=1e-7)
    assert torch.allclose(rv_k.double(), bn.running_var, rtol=1e-5, atol=0)
    with pytest.raises(ValueError):
        ops.bn_batch_stats(torch.randn(1, 1, 1, C, device='cuda'), gamma, beta, rm_k, rv_k, nbt, 0.1, 1e-5)


# ------------------------------------------------------------------------------------------------ oracle with batch statistics
def _stage_of(prefix):
    p = prefix[len('backbone.'):]
    return 0 if p.startswith('bn1') else int(p.split('.')[0][len('layer'):])


def _patch_oracle(monkeypatch, frozen_stages, momentum=0.1):
    """O._bn_eval -> training-mode F.batch_norm on cloned running buffers for the stages the reference's train() puts in training
    mode (stem: frozen_stages < 0; layer i: i > frozen_stages).  Returns prefix -> [running_mean, running_var] as updated."""
    bufs = {}
    orig = O._bn_eval

    def bn(x, sd, p, eps=1e-5):
        if _stage_of(p) <= frozen_stages:
            return orig(x, sd, p, eps)
        if p not in bufs:
            bufs[p] = [sd[p + '.running_mean'].detach().clone(), sd[p + '.running_var'].detach().clone()]
        return F.batch_norm(x, bufs[p][0], bufs[p][1], sd[p + '.weight'], sd[p + '.bias'], True, momentum, eps)
    monkeypatch.setattr(O, '_bn_eval', bn)
    return bufs


def _check_buffers(model, sd0, bufs, frozen_stages, prefix='backbone.'):
    sd = model.state_dict()
    n = 0
    for k, v in sd.items():
        if not k.startswith(prefix) or not k.endswith('num_batches_tracked'):
            continue
        p = k[:-len('.num_batches_tracked')]
        trained = _stage_of(p) > frozen_stages
        assert int(v) == int(sd0.get(k, torch.tensor(0))) + int(trained), k
        if trained:
            n += 1
            for i, name in enumerate(('running_mean', 'running_var')):
                got, want = sd[p + '.' + name].cpu().double(), bufs[p][i].double()
                assert torch.allclose(got, want, rtol=1e-4, atol=1e-5 * float(want.abs().max())), (p, name, _rel_l2(got, want))
        else:
            for name in ('running_mean', 'running_var'):
                assert torch.equal(sd[p + '.' + name].cpu(), sd0[p + '.' + name]), (p, name)
    assert n == len(bufs) and n > 0


@pytest.mark.parametrize('depth', [18, 50])
@pytest.mark.parametrize('frozen_stages', [1, -1])
def test_backbone_forward_matches_patched_oracle(monkeypatch, depth, frozen_stages):
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    sd = {k: v for k, v in synthetic.locator_state_dict(depth, 1, 0, 'cpr', 3, 0.3).items() if k.startswith('backbone.')}
    m = ResNet(depth, frozen_stages=frozen_stages, norm_eval=False).cuda()
    m.load_state_dict({k[len('backbone.'):]: v for k, v in sd.items()}, strict=True)
    m.train()
    torch.manual_seed(0)
    img = torch.randn(2, 3, 96, 128)
    outs = m(img.cuda())
    torch.cuda.synchronize()
    bufs = _patch_oracle(monkeypatch, frozen_stages)
    with torch.no_grad():
        ref = O.resnet_forward(sd, img, depth)
    for i, (a, b) in enumerate(zip(outs, ref)):
        assert _rel_l2(a, b) <= 1e-4, (i, _rel_l2(a, b))
    full = {'backbone.' + k: v for k, v in m.state_dict().items()}

    class _Wrap:
        def state_dict(self):
            return full
    _check_buffers(_Wrap(), sd, bufs, frozen_stages)


def _block_fp64(blk, x, P, masks):
    """fp64 torch autograd of one ResNet block with training-mode BatchNorm.  masks: the kernel's recorded ReLU outputs (o1, o2, out)
    -- the fp64 ReLUs take their 0/1 pattern from them, so a pre-activation within rounding of 0 (which fp32 and fp64 put on
    different sides) cannot move a whole channel of the batch-coupled BatchNorm backward."""
    def bn(t, m):
        return F.batch_norm(t, None, None, P[id(m.weight)], P[id(m.bias)], True, 0.1, m.eps)

    def conv(t, c):
        return F.conv2d(t, P[id(c.weight)], None, c.stride, c.padding)

    def relu(t, mk):
        return t * (mk > 0).to(t.dtype)
    o = relu(bn(conv(x, blk.conv1), blk.bn1), masks[0])
    if blk.kind == 'bottleneck':
        o = relu(bn(conv(o, blk.conv2), blk.bn2), masks[1])
        o = bn(conv(o, blk.conv3), blk.bn3)
    else:
        o = bn(conv(o, blk.conv2), blk.bn2)
    idn = bn(conv(x, blk.downsample[0]), blk.downsample[1]) if blk.downsample is not None else x
    return relu(o + idn, masks[2])


@pytest.mark.parametrize('depth', [18, 50])
@pytest.mark.parametrize('frozen_stages', [1, 2])
def test_backbone_backward_matches_fp64_autograd_per_block(depth, frozen_stages):
    """The batch-statistics backward rules of the backbone with no head or neck in the loop: the recorded forward and
    BackwardEngine._backward_backbone under fixed random upstream gradients on the stage outputs; every recorded block is then
    replayed in fp64 torch autograd from the block input and output gradient the engine saw, with the kernel's own ReLU patterns.
    The block's forward, its parameter gradients and its input gradient must agree to 1e-4 (measured ~2e-6)."""
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    from pointtinybenchmark_amd.training import BackwardEngine
    sd = {k[len('backbone.'):]: v for k, v in synthetic.locator_state_dict(depth, 1, 0, 'cpr', 3, 0.3).items()
          if k.startswith('backbone.')}
    m = ResNet(depth, frozen_stages=frozen_stages, norm_eval=False).cuda()
    m.load_state_dict(sd, strict=True)
    m.train()
    eng = BackwardEngine(m)
    eng._sink = {}
    g = torch.Generator().manual_seed(3)
    img = torch.randn((2, 3, 160, 192), generator=g)
    tape = []
    outs = m(img.cuda(), tape=tape)
    d_stage = {i: torch.randn(tuple(o.shape), generator=g).permute(0, 2, 3, 1).contiguous().cuda()
               for i, o in enumerate(outs) if i > frozen_stages - 1}
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
    assert len(tape) == sum(len(getattr(m, 'layer%d' % i)) for i in range(frozen_stages + 1, 5)) and all(id(r) in seen for r in tape)

    def nchw64(t):
        return t.detach().double().cpu().permute(0, 3, 1, 2)
    bad = []
    for rec in tape:
        blk = rec['block']
        P = {id(p): p.detach().double().cpu().clone().requires_grad_(True) for p in blk.parameters()}
        x = nchw64(rec['x']).clone().requires_grad_(True)
        masks = [nchw64(rec['o1']), nchw64(rec['o2']) if rec['o2'] is not None else None, nchw64(rec['out'])]
        out = _block_fp64(blk, x, P, masks)
        errs = [('forward', _rel_l2(nchw64(rec['out']), out))]
        (out * nchw64(seen[id(rec)])).sum().backward()
        errs += [(n, _rel_l2(got[id(p)], P[id(p)].grad)) for n, p in blk.named_parameters()]
        if seen[id(rec), 'dx'] is not None:
            errs.append(('dx', _rel_l2(nchw64(seen[id(rec), 'dx']), x.grad)))
        bad += [(e, rec['stage'], n) for n, e in errs if e > 1e-4]
    assert not bad, 'block mismatch (rel L2, stage, what): %s' % sorted(bad, reverse=True)[:8]


def _bs_locator(cfg, frozen_stages=1):
    m, sd = build_hip_locator(cfg)          # frozen_stages=1, norm_eval=True as built; the switches are plain attributes
    m.backbone.norm_eval = False
    m.backbone.frozen_stages = frozen_stages
    m.train()
    return m, sd


def _batch(cfg, seed=None):
    b = synthetic.synthetic_batch(cfg['batch'], cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'],
                                  cfg['seed'] if seed is None else seed, cfg.get('ragged', False))
    cb = to_cuda(b)
    return b, dict(img=cb['img'], img_metas=cb['img_metas'], gt_bboxes=cb['gt_bboxes'], gt_labels=cb['gt_labels'])


@pytest.mark.parametrize('name,frozen_stages', [('cpr_r18_c3_128', 1), ('cpr_r50_c1_160_spread', 1), ('cpr_r18_c3_128', 2)])
def test_train_step_matches_patched_oracle_autograd(monkeypatch, name, frozen_stages):
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES[name]
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    m, sd = _bs_locator(cfg, frozen_stages)
    batch, data = _batch(cfg)
    tr = CprTrainer(m)
    trainable = [k for k, p in m.named_parameters() if p.requires_grad]
    losses = tr.forward_backward(**data)
    torch.cuda.synchronize()
    got = {k: float(v) for k, v in losses.items()}
    bufs = _patch_oracle(monkeypatch, frozen_stages)
    osd = {k: v.clone() for k, v in sd.items()}
    for k in trainable:
        osd[k].requires_grad_(True)
    olosses, _, _ = O.locator_forward_train(osd, batch, cfg['depth'], cfg['start_level'], cfg['stride'], cfg['radius'],
                                            cfg['num_classes'])
    sum(v for k, v in olosses.items() if 'loss' in k).backward()
    for k, v in olosses.items():
        assert abs(got[k] - float(v)) <= 1e-4 * max(1.0, abs(float(v))), (k, got[k], float(v))
    params = dict(m.named_parameters())
    worst = sorted(((_rel_l2(params[k].grad, osd[k].grad), k, float(osd[k].grad.abs().max())) for k in trainable), reverse=True)
    # The per-tensor 2e-3 bar of the eval-BN step cannot hold here for ANY fp32 implementation: with batch statistics one ReLU
    # whose pre-activation sits within rounding of 0 (fp32 and fp64 put it on different sides) moves the BatchNorm backward of its
    # whole channel, and such elements exist in most blocks.  Measured on the same weights: the torch fp32 oracle itself is
    # 1.4e-2 (median) / 1.6e-2 (worst) rel-L2 off the fp64 oracle on these R50 backbone gradients (tools/bn_fp32_conditioning.py,
    # profiles/bn_fp32_conditioning.txt).  The backward rules are held to 1e-4 per block, ReLU patterns pinned, by
    # test_backbone_backward_matches_fp64_autograd_per_block; here: the direction of the whole gradient and a loose per-tensor bound.
    live = [k for _, k, mx in worst if mx > 1e-6 * max(w[2] for w in worst)]
    a = torch.cat([params[k].grad.detach().double().cpu().flatten() for k in live])
    b = torch.cat([osd[k].grad.detach().double().flatten() for k in live])
    cos = float(a @ b / (a.norm() * b.norm()))
    assert cos >= 0.999, cos
    bad = [w for w in worst if w[1] in live and w[0] > 5e-2]
    assert not bad, 'gradient mismatch (rel L2, key, ref max): %s' % bad[:6]
    _check_buffers(m, sd, bufs, frozen_stages)


def test_bridge_is_bit_equal_to_the_trainer_cpr():
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES['cpr_r18_c3_128']
    _, data = _batch(cfg)
    ma, _ = _bs_locator(cfg)
    tr = CprTrainer(ma)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb, _ = _bs_locator(cfg)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad
    out['loss'].backward()
    torch.cuda.synchronize()
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
    # the forward ran once per step: every running buffer equals the trainer's
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        if 'running' in k or 'num_batches' in k:
            assert torch.equal(sa[k], sb[k]), k


def test_bridge_is_bit_equal_to_the_trainer_p2p():
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd.training import P2PTrainer

    def build():
        cfg = p2p_model_cfg(18)
        cfg['backbone']['norm_eval'] = False
        m = P.build_detector(cfg).cuda()
        m.load_state_dict(synthetic.locator_state_dict(18, 1, 0, 'p2p', 3, head_std=0.05), strict=True)
        m.train()
        return m
    cb = to_cuda(synthetic.synthetic_batch(2, 128, 160, 6, 1, seed=8))
    data = dict(img=cb['img'], img_metas=cb['img_metas'], gt_bboxes=cb['gt_bboxes'], gt_labels=cb['gt_labels'])
    ma = build()
    assert ma.backbone.batch_stats_active()
    P2PTrainer(ma).forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb = build()
    out = mb.train_step(dict(data))
    out['loss'].backward()
    torch.cuda.synchronize()
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k


def test_eval_after_train_uses_the_updated_buffers(monkeypatch):
    """A folded eval-mode BatchNorm built before a training-mode forward must not survive it (the stale-fold check)."""
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES['cpr_r18_c3_128']
    m, _ = _bs_locator(cfg)
    _, data = _batch(cfg)
    m.eval()
    with torch.no_grad():
        before = [o.clone() for o in m.backbone(data['img'])]        # folds built from the initial buffers
    m.train()
    CprTrainer(m).forward_backward(**data)                           # training-mode forward: running buffers move
    m.eval()
    with torch.no_grad():
        after = m.backbone(data['img'])
    torch.cuda.synchronize()
    sd = {'backbone.' + k: v.detach().cpu() for k, v in m.backbone.state_dict().items()}
    ref = O.resnet_forward(sd, data['img'].cpu(), cfg['depth'])
    for a, b, r in zip(after, before, ref):
        assert _rel_l2(a, r) <= 1e-4
    assert any(not torch.equal(a, b) for a, b in zip(after, before))


def test_repeated_step_is_bit_repeatable_and_streams_do_not_split_the_batch():
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES['cpr_r18_c3_128']
    _, data = _batch(cfg)
    res = []
    for _ in range(2):
        m, _ = _bs_locator(cfg)
        tr = CprTrainer(m)
        tr.forward_backward(**data)
        torch.cuda.synchronize()
        res.append((tr.flat_g.clone(), {k: v.clone() for k, v in m.state_dict().items() if 'running' in k}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    m, _ = _bs_locator(cfg)
    with torch.no_grad():
        m.num_streams = 1
        l1 = m.forward_train(**data)
        m.num_streams = 2
        l2 = m.forward_train(**data)
    for k in l1:
        a, b = l1[k], l2[k]
        a = torch.stack(a) if isinstance(a, list) else a
        b = torch.stack(b) if isinstance(b, list) else b
        assert torch.equal(a, b), k


def test_bf16_with_batch_statistics_is_refused():
    from pointtinybenchmark_amd import autograd_bridge
    cfg = CPR_CASES['cpr_r18_c3_128']
    m, _ = _bs_locator(cfg)
    m.set_compute_dtype('bf16')
    _, data = _batch(cfg)
    assert 'norm_eval' in autograd_bridge.unsupported_reason(m)
    with torch.no_grad(), pytest.raises(NotImplementedError, match='norm_eval'):
        m.forward_train(**data)
    with pytest.warns(UserWarning), pytest.raises(NotImplementedError, match='norm_eval'):
        m.forward_train(**data)
