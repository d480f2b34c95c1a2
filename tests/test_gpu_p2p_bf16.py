"""-m gpu: P2PNet (P2PHead) in the bf16 compute mode.  The head's 3x3 output convs read the raw bf16 last tower layer with its
GroupNorm affine and ReLU on load (csrc/p2p_out_bf16.hip: forward, data gradient, weight + bias gradient, J <= 8); larger J take the
bf16 matrix-core conv.  Kernels against fp64 torch, the bf16 locator against the fp32 oracle, the mixed-precision P2PTrainer step
against the fp32 step, and the autograd bridge against the trainer."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpr_oracle as O
from pointtinybenchmark_amd import synthetic
from tests.test_gpu_cpr_parity import to_cuda

pytestmark = pytest.mark.gpu

MAPS = [(2, 160, 160, 256), (2, 40, 48, 256), (1, 25, 19, 256)]


def _operands(shape, J, seed):
    g = torch.Generator().manual_seed(seed)
    N, H, W, Cin = shape
    x = (torch.randn(shape, generator=g) * 2).bfloat16()
    a = (torch.rand((N, Cin), generator=g) + 0.25) * torch.where(torch.rand((N, Cin), generator=g) < 0.2, -1.0, 1.0)
    b = torch.randn((N, Cin), generator=g) * 0.5
    w = torch.randn((J, Cin, 3, 3), generator=g) * 0.02
    bias = torch.randn((J,), generator=g)
    return x, a, b, w, bias


def _act64(x, a, b):
    """relu(a*x + b) in fp64 from the widened bf16 map, NCHW."""
    xd = x.double()
    return torch.relu(xd * a.double()[:, None, None, :] + b.double()[:, None, None, :]).permute(0, 3, 1, 2)


@pytest.mark.parametrize('J', [1, 2, 3, 8])
@pytest.mark.parametrize('shape', MAPS, ids=lambda s: '%dx%dx%dx%d' % s)
def test_forward_kernel_vs_fp64_and_the_fp32_tap_projection(shape, J):
    from pointtinybenchmark_amd import ops
    x, a, b, w, bias = _operands(shape, J, sum(shape) + J)
    ref = F.conv2d(_act64(x, a, b), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    xc, ac, bc, wc, biasc = (t.cuda().contiguous() for t in (x, a, b, w, bias))
    with torch.no_grad():
        out = ops.p2p_out_bf16(xc, (ac, bc), wc, biasc)
        # the fp32 mode's forward-only form on the widened map: 1x1 projection to 9 J tap responses + the tap sum
        pc1 = ops.PackedConv(wc.permute(2, 3, 0, 1).reshape(9 * J, -1)[:, :, None, None].contiguous(), 1, 0)
        R = ops.conv2d(ops.gn_apply(xc.float(), ac, bc, relu=True), pc1)
        tap = ops.tap_sum3x3(R, biasc, J)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == shape[:3] + (J,)
    bar = 1e-5 * max(float(ref.abs().max()), 1.0)
    err = float((out.cpu().double() - ref).abs().max())
    assert err <= bar, 'forward vs fp64: %.3e (bar %.3e)' % (err, bar)
    err_t = float((out - tap).abs().max())
    assert err_t <= bar, 'forward vs the fp32 tap projection: %.3e (bar %.3e)' % (err_t, bar)


@pytest.mark.parametrize('J', [1, 2, 3, 8])
@pytest.mark.parametrize('shape', MAPS, ids=lambda s: '%dx%dx%dx%d' % s)
def test_backward_kernels_vs_fp64_autograd(shape, J):
    from pointtinybenchmark_amd import ops
    x, a, b, w, bias = _operands(shape, J, 7 * sum(shape) + J)
    N, H, W, Cin = shape
    Jd = max(4, J)          # a channel-padded gradient map as the loss backward writes it: the pad channels must be ignored
    g = torch.Generator().manual_seed(J)
    dout = torch.randn((N, H, W, Jd), generator=g)
    act = _act64(x, a, b).requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    F.conv2d(act, wd, bd, padding=1).backward(dout[..., :J].double().permute(0, 3, 1, 2))
    ref_dx, ref_gw, ref_gb = act.grad.permute(0, 2, 3, 1), wd.grad, bd.grad
    xc, ac, bc, wc, dc = (t.cuda().contiguous() for t in (x, a, b, w, dout))
    with torch.no_grad():
        dx = ops.p2p_out_bf16_dgrad(dc, wc, tuple(xc.shape))
        dx16 = ops.p2p_out_bf16_dgrad(dc, wc, tuple(xc.shape), torch.bfloat16)
        gw = torch.full((J, Cin, 3, 3), float('nan'), device='cuda')
        gb = torch.full((J,), float('nan'), device='cuda')
        r = ops.p2p_out_bf16_wgrad(dc, xc, (ac, bc), (J, Cin, 3, 3), out_w=gw, out_b=gb)
        assert r[0] is gw and r[1] is gb
        gw2, gb2 = ops.p2p_out_bf16_wgrad(dc, xc, (ac, bc), (J, Cin, 3, 3))
    torch.cuda.synchronize()
    for name, got, ref in (('dx', dx, ref_dx), ('gw', gw, ref_gw), ('gb', gb, ref_gb)):
        assert got.dtype == torch.float32
        bar = 1e-5 * max(float(ref.abs().max()), 1e-30)
        err = float((got.cpu().double() - ref).abs().max())
        assert err <= bar, '%s vs fp64: %.3e (bar %.3e)' % (name, err, bar)
    assert dx16.dtype == torch.bfloat16 and torch.equal(dx16, dx.to(torch.bfloat16)), 'bf16 dx is not the RNE rounding of fp32 dx'
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2), 'weight gradient is not bit-repeatable'


def test_support_predicate():
    from pointtinybenchmark_amd import ops
    assert ops.p2p_out_bf16_supported((2, 25, 19, 256), 8) and ops.p2p_out_bf16_supported((1, 8, 8, 64), 1)
    assert not ops.p2p_out_bf16_supported((2, 25, 19, 256), 9)
    assert not ops.p2p_out_bf16_supported((2, 25, 19, 320), 2) and not ops.p2p_out_bf16_supported((2, 25, 19, 96), 2)
    x = torch.zeros((1, 8, 8, 256), dtype=torch.bfloat16, device='cuda')
    ab = (torch.ones((1, 256), device='cuda'), torch.zeros((1, 256), device='cuda'))
    assert ops.p2p_out_bf16(x, ab, torch.zeros((15, 256, 3, 3), device='cuda'), torch.zeros(15, device='cuda')) is None


# ------------------------------------------------------------------------------------------------ the locator
def _build(depth, C, seed, bf16=True):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    m = P.build_detector(p2p_model_cfg(depth, C)).cuda()
    sd = synthetic.locator_state_dict(depth, C, 0, 'p2p', seed, head_std=0.05)
    m.load_state_dict(sd, strict=True)
    m.train()
    if bf16:
        m.set_compute_dtype('bf16')
    return m, sd


# the loss bars hold only where the bf16 maps give the oracle's Hungarian assignment: the small case's seed is one on which they do
LOCATOR_CASES = {
    'r50_c1_640_b1': dict(depth=50, C=1, batch=1, h=640, w=640, gts=32, seed=61),     # BASELINE configs[3] shape
    'r18_c1_128x160_b2': dict(depth=18, C=1, batch=2, h=128, w=160, gts=6, seed=16),
    'r18_c15_128x160_b2': dict(depth=18, C=15, batch=2, h=128, w=160, gts=6, seed=9),  # J = 15 > 8: the matrix-core fallback
}


@pytest.mark.parametrize('name', list(LOCATOR_CASES))
def test_bf16_p2p_locator_vs_fp32_oracle(name):
    c = LOCATOR_CASES[name]
    m, sd = _build(c['depth'], c['C'], c['seed'])
    batch = synthetic.synthetic_batch(c['batch'], c['h'], c['w'], c['gts'], c['C'], seed=c['seed'])
    cb = to_cuda(batch)
    head = m.bbox_head
    with torch.no_grad():
        feats = m.neck(m.backbone(cb['img']))
        assert feats[0].dtype == torch.bfloat16
        cls_outs, pts_outs = head(feats)
        losses = head.loss(cls_outs, pts_outs, cb['gt_bboxes'], cb['gt_labels'], cb['img_metas'])
        fused = m.forward_train(cb['img'], cb['img_metas'], cb['gt_bboxes'], cb['gt_labels'])
        torch.cuda.synchronize()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        ofeats = O.fpn_forward(sd, O.resnet_forward(sd, batch['img'], c['depth']), 0, 1)
        rc, rp = O.p2p_head_forward(sd, ofeats)
        ref_losses, _ = O.p2p_loss(rc[0], rp[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'][0]['img_shape'])
    for got, ref in ((cls_outs[0], rc[0]), (pts_outs[0], rp[0])):
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        scale = max(1.0, float(ref.abs().max()))
        err = (got.float().cpu() - ref).abs()
        assert float(err.max()) <= 8e-2 * scale and float(err.mean()) <= 1e-2 * scale, \
            'bf16 map: max %.3e mean %.3e (scale %.2e)' % (float(err.max()), float(err.mean()), scale)
    for k in ('loss_cls', 'loss_pts'):
        a = sum(float(v) for v in losses[k])
        b = sum(float(v) for v in ref_losses[k])
        assert abs(a - b) <= 3e-2 * max(abs(b), 1e-3), (k, a, b)
        assert abs(sum(float(v) for v in fused[k]) - a) <= 1e-5 * max(abs(a), 1e-6)


def test_bf16_simple_test_equals_oracle_postprocessing_of_the_same_maps():
    m, _ = _build(18, 1, 8)
    m.eval()
    batch = synthetic.synthetic_batch(2, 256, 256, 12, 1, seed=12)
    cb = to_cuda(batch)
    head = m.bbox_head
    with torch.no_grad():
        res = m.simple_test(cb['img'], cb['img_metas'])
        cls_outs, pts_outs = head(m.extract_feat(cb['img']))
        _, pred, _, cls = head.get_pred_points(cls_outs, pts_outs, cb['img_metas'])
        torch.cuda.synchronize()
    shape = batch['img_metas'][0]['img_shape']
    for b in range(2):
        dets, labels, _, _ = O.p2p_get_points_single(cls[b].cpu(), pred[b, :, :2].cpu(), None, shape)
        got_d, got_l = res[b][0].cpu(), res[b][1].cpu()
        ref = torch.cat([dets[:, :2] - 8, dets[:, :2] + 8, dets[:, 2:]], dim=1)
        assert got_d.shape == ref.shape and got_d.shape[0] > 0, (got_d.shape, ref.shape)
        assert np.array_equal(got_d.numpy()[:, 4], ref.numpy()[:, 4]), 'scores must agree index for index'
        assert torch.equal(got_l, labels.to(got_l.dtype))
        np.testing.assert_allclose(got_d.numpy(), ref.numpy(), rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------ mixed-precision training
def _train_data(seed=4):
    batch = synthetic.synthetic_batch(2, 128, 160, 6, 1, seed=seed)
    cb = to_cuda(batch)
    return dict(img=cb['img'], img_metas=cb['img_metas'], gt_bboxes=cb['gt_bboxes'], gt_labels=cb['gt_labels'])


def _record_assignments(head):
    rec = []
    orig = head.assign_batch

    def assign_batch(*a, **k):
        out = orig(*a, **k)
        rec.append(out.clone())
        return out
    head.assign_batch = assign_batch
    return rec


def _worst_rel(tr, ga, gb, gmax):
    worst, off = 0.0, 0
    for p_ in tr.params:
        n = p_.numel()
        a, b = ga[off:off + n].double(), gb[off:off + n].double()
        off += n
        if float(b.norm()) >= 1e-2 * gmax:
            worst = max(worst, float((a - b).norm() / b.norm()))
    return worst


def test_mixed_precision_p2p_step_tracks_the_fp32_step():
    from pointtinybenchmark_amd import training
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = _build(18, 1, 3, bf16=False)
    data = _train_data(seed=14)     # (a batch on which the bf16 and fp32 forwards make the same Hungarian assignment)
    rec = _record_assignments(m.bbox_head)
    tr = P2PTrainer(m, lr=1e-3)
    l32 = tr.forward_backward(**data)
    torch.cuda.synchronize()
    g32, inds32 = tr.flat_g.clone(), rec[-1]
    m.set_compute_dtype('bf16')
    l16 = tr.forward_backward(**data)
    torch.cuda.synchronize()
    g16, inds16 = tr.flat_g.clone(), rec[-1]
    assert torch.equal(inds16, inds32), 'the fixture must give both steps the same Hungarian assignment (%d differ)' % \
        int((inds16 != inds32).sum())
    assert torch.isfinite(g16).all()
    for k in ('loss_cls', 'loss_pts'):
        a, b = sum(float(v) for v in l16[k]), sum(float(v) for v in l32[k])
        assert abs(a - b) <= 5e-2 * max(1.0, abs(b)), (k, a, b)
    cos = float(torch.dot(g16.double(), g32.double()) / (g16.double().norm() * g32.double().norm()))
    assert cos >= 0.99, 'mixed-precision gradient direction: cosine %.4f' % cos
    gmax = max(float(p.grad.norm()) for p in m.parameters() if p.requires_grad)
    worst = _worst_rel(tr, g16, g32, gmax)
    assert worst <= 0.25, 'mixed-precision gradient, worst relative L2 over the large tensors: %.3f' % worst
    # the bf16 output-conv / tower kernels against the fp32 kernels behind the same bf16 forward
    training.MIXED_BF16.update(wgrad=False, dgrad=False)
    try:
        tr.forward_backward(**data)
        torch.cuda.synchronize()
    finally:
        training.MIXED_BF16.update(wgrad=True, dgrad=True)
    gB = tr.flat_g.clone()
    assert torch.equal(rec[-1], inds16)
    worst_k = _worst_rel(tr, g16, gB, gmax)
    assert worst_k <= 0.02, 'bf16 gradient kernels against fp32 ones behind the same bf16 forward: %.4f' % worst_k
    tr.forward_backward(**data)
    tr.step()
    torch.cuda.synchronize()
    for k, p_ in m.named_parameters():
        assert p_.dtype == torch.float32 and torch.isfinite(p_).all(), k


def test_mixed_precision_p2p_steps_lower_the_loss():
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = _build(18, 1, 3)
    data = _train_data()
    tr = P2PTrainer(m, lr=2e-4, momentum=0.9, weight_decay=1e-4, max_norm=35.0)
    w0 = m.bbox_head.reg_out.weight.detach().clone()
    totals = []
    for _ in range(4):
        out = tr.train_step(dict(data))
        assert np.isfinite(out['log_vars']['loss'])
        totals.append(out['log_vars']['loss'])
    assert totals[1] < totals[0], totals
    assert float((m.bbox_head.reg_out.weight - w0).abs().max()) > 0


def test_mixed_precision_p2p_bridge_and_repeatability():
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import P2PTrainer
    data = _train_data(seed=8)
    ma, _ = _build(18, 1, 3)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr = P2PTrainer(ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb, _ = _build(18, 1, 3)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    la_total = float(sum(sum(v) for k, v in la.items() if 'loss' in k))
    assert abs(out['log_vars']['loss'] - la_total) <= 1e-6 * max(1.0, abs(la_total))
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and p.grad.dtype == torch.float32 and torch.equal(p.grad, want[k]), k
    # two mixed steps from the same state: the same bits
    mc, _ = _build(18, 1, 3)
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
