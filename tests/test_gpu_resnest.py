"""-m gpu: the ResNeSt backbone on the split-attention kernels (csrc/splat.hip) and the block-diagonal dense conv2, forward and training.

  fixture    tests/golden/resnest.npz (the reference's own ResNeSt in fp64, tools/gen_resnest.py): stage outputs <= 2e-4 max|level| for
             every case (s50, odd maps, layer1.0 training, style='caffe' without a pooled block, reduction_factor=2, depth 101); a second
             forward is bit-equal, the recorded forward equals the forward-only one bit for bit; parameter gradients of the fixture's
             linear functional through BackwardEngine._backward_backbone <= 2e-3 rel-L2 on norm and sample, named_parameters order the
             fixture's
  per block  s50_fs0 replayed block by block in fp64 autograd of tests/resnest_ref's restatement from the recorded input and output
             gradient with the kernel's own ReLU patterns, within 1e-4 (the bar and method of the Res2Net per-block test): pooled blocks
             (layer2-4.0), unpooled ones, and layer1.0 with a shortcut conv and no pool
  isolation  changing input channels [w/2, w) of o1 leaves output channels [0, w) of u bit-equal (and the other way round), on a
             Winograd-sized and on a small map: the off-diagonal blocks of the dense weight are exact zeros
  locator    a small CPR and a small P2P locator with the ResNeSt backbone: forward_train's losses are finite, repeat bit for bit and the
             backbone's maps match the restatement (fp64, CPU) within the fixture's output bar
  training   a CPR and a P2P locator (frozen_stages=1): loss.backward() through the bridge is bit-equal to the native trainer; after one
             optimizer step a fresh model holding the stepped weights gives the same forward bit for bit (the lapsing packs rebuilt)
  refusals   the bf16 compute mode names ``radix``, batch statistics ``norm_eval`` -- on the device"""
import pytest
import torch
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic
from tests import resnest_ref as RS

pytestmark = pytest.mark.gpu


def _case_model(name, **kw):
    import pointtinybenchmark_amd as P
    cfg = RS.CASES[name]
    m = P.build_backbone(dict(type='ResNeSt', **dict(RS.resnest_kwargs(cfg), **kw))).cuda()
    m.load_state_dict(RS.case_state_dict(cfg), strict=True)
    m.train()
    return cfg, m


@pytest.mark.parametrize('name', RS.CASE_NAMES)
def test_stage_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = RS.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
    torch.cuda.synchronize()
    assert len(outs) == 4
    failed = []
    for l, o in enumerate(outs):
        e = RS.output_error(name, l, o)
        print('ERR forward %-10s stage %d %-10s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[2:]), e), flush=True)
        if not e <= RS.BAR_OUT:
            failed.append((l, e))
        assert torch.equal(o, again[l])
    assert not failed, failed


def _rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _engine_backward(m, cfg, spy=None):
    """The recorded forward and BackwardEngine._backward_backbone on the fixture's linear functional -> (outs, tape, {name: grad})."""
    from pointtinybenchmark_amd.training import BackwardEngine
    eng = BackwardEngine(m)
    eng._sink = {}
    if spy is not None:
        spy(eng)
    tape = []
    outs = m(RS.case_input(cfg).cuda(), tape=tape)
    d_stage = {l: RS.functional_weight(cfg, l, o.shape).permute(0, 2, 3, 1).contiguous().cuda() for l, o in enumerate(outs)
               if l + 1 > cfg['frozen_stages']}
    eng._backward_backbone(m, tape, d_stage)
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    grads = dict(zip([k for k, _ in named], eng.collect([p for _, p in named])))
    torch.cuda.synchronize()
    return outs, tape, grads


@pytest.mark.parametrize('name', RS.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    """rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample, against the reference class's fp64 autograd; the recorded
    forward gives the forward-only one's bits."""
    cfg, m = _case_model(name)
    outs, tape, grads = _engine_backward(m, cfg)
    with torch.no_grad():
        plain = m(RS.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    assert list(grads) == RS.grad_names(name)
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        en, es = RS.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= RS.BAR_GRAD and es <= RS.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-10s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    assert not failed, failed[:8]


def _block_fp64(blk, x, P, rec):
    """fp64 torch autograd of one ResNeSt block with eval-mode BatchNorm (tests/resnest_ref's restatement on the block's own
    parameters); the ReLUs take their 0/1 pattern from the kernel's recorded maps."""
    def bn(t, mod):
        return F.batch_norm(t, mod.running_mean.double().cpu(), mod.running_var.double().cpu(), P[id(mod.weight)], P[id(mod.bias)], False,
                            0.0, mod.eps)

    def nchw64(t):
        return t.detach().double().cpu().permute(0, 3, 1, 2)

    def relu(t, mk):
        return t * (mk > 0).to(t.dtype)
    sa = blk.conv2
    o1 = relu(bn(F.conv2d(x, P[id(blk.conv1.weight)], None, blk.conv1.stride), blk.bn1), nchw64(rec['o1']))
    u = relu(bn(F.conv2d(o1, P[id(sa.conv.weight)], None, 1, 1, groups=2), sa.bn0), nchw64(rec['u']))
    g = RS.splat_gap(u)
    h = F.linear(g, P[id(sa.fc1.weight)].flatten(1), P[id(sa.fc1.bias)])
    hn = (h - sa.bn1.running_mean.double().cpu()) / torch.sqrt(sa.bn1.running_var.double().cpu() + sa.bn1.eps) * P[id(sa.bn1.weight)] + \
        P[id(sa.bn1.bias)]
    z = relu(hn, rec['z'].detach().double().cpu())
    a = F.linear(z, P[id(sa.fc2.weight)].flatten(1), P[id(sa.fc2.bias)])
    att = torch.softmax(a.view(a.shape[0], 2, -1), dim=1)
    o = RS.splat_apply(u, att, blk.pool)
    o = bn(F.conv2d(o, P[id(blk.conv3.weight)]), blk.bn3)
    idn = x
    if blk.downsample is not None:
        if blk.stride > 1:
            idn = F.avg_pool2d(idn, blk.stride, blk.stride, ceil_mode=True, count_include_pad=False)
        idn = bn(F.conv2d(idn, P[id(blk.ds_conv.weight)]), blk.ds_bn)
    return relu(o + idn, nchw64(rec['out']))


def test_backward_vs_fp64_autograd_per_block():
    """s50_fs0 (layer1.0 -- stride 1, a shortcut conv, no pool -- trains): every recorded block replayed in fp64 autograd from the block
    input and the output gradient the engine saw: forward, parameter gradients and input gradient within 1e-4."""
    cfg, m = _case_model('s50_fs0')
    seen = {}

    def spy(eng):
        rule = eng._resnest_block_backward

        def wrapped(cache, blk, rec, dout, need_dx):
            seen[id(rec)] = dout.clone()
            r = rule(cache, blk, rec, dout, need_dx)
            seen[id(rec), 'dx'] = None if r is None else r.clone()
            return r
        eng._resnest_block_backward = wrapped
    outs, tape, grads = _engine_backward(m, cfg, spy)
    assert len(tape) == 16 and all(id(r) in seen for r in tape)
    kinds = {(r['block'].pool, r['block'].downsample is not None) for r in tape}
    assert kinds == {(True, True), (False, True), (False, False)}      # pooled, unpooled with a shortcut conv (layer1.0), plain
    names = {id(p): k for k, p in m.named_parameters()}
    torch.set_num_threads(min(torch.get_num_threads(), 16))

    def nchw64(t):
        return t.detach().double().cpu().permute(0, 3, 1, 2)
    bad, worst = [], 0.0
    for bi, rec in enumerate(tape):
        blk = rec['block']
        P = {id(p): p.detach().double().cpu().clone().requires_grad_(True) for p in blk.parameters()}
        x = nchw64(rec['x']).clone().requires_grad_(True)
        out = _block_fp64(blk, x, P, rec)
        errs = [('forward', _rel_l2(nchw64(rec['out']), out))]
        (out * nchw64(seen[id(rec)])).sum().backward()
        errs += [(n, _rel_l2(grads[names[id(p)]], P[id(p)].grad)) for n, p in blk.named_parameters()]
        if seen[id(rec), 'dx'] is not None:
            errs.append(('dx', _rel_l2(nchw64(seen[id(rec), 'dx']), x.grad)))
        worst = max([worst] + [e for _, e in errs])
        bad += [(e, rec['stage'], bi, n) for n, e in errs if e > 1e-4]
    print('ERR backward s50_fs0 per block: worst rel-L2 %.2e (bar 1e-4)' % worst, flush=True)
    assert not bad, 'block mismatch (rel L2, stage, block, what): %s' % sorted(bad, reverse=True)[:8]


@pytest.mark.parametrize('hw', [(18, 23), (50, 44)], ids=['18x23', '50x44'])
def test_conv2_groups_are_isolated(hw):
    """The dense block-diagonal conv2: output channels [0, w) of u read input channels [0, w/2) alone, [w, 2w) read [w/2, w) alone."""
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.layers import folded_bn
    cfg, m = _case_model('s50')
    blk = m.layer2[1]
    w = blk.width
    pc = blk.conv2_pack(m._cache)
    s0, b0 = folded_bn(m._cache, blk.conv2.bn0)
    g = torch.Generator().manual_seed(5)
    o1 = torch.randn((2,) + hw + (w,), generator=g).cuda()
    other = torch.randn((2,) + hw + (w,), generator=g).cuda()
    hi, lo = o1.clone(), o1.clone()
    hi[..., w // 2:] = other[..., w // 2:]
    lo[..., :w // 2] = other[..., :w // 2]
    u, u_hi, u_lo = (ops.conv2d(t.contiguous(), pc, scale=s0, bias=b0, relu=True) for t in (o1, hi, lo))
    torch.cuda.synchronize()
    assert tuple(u.shape) == (2,) + hw + (2 * w,)
    assert torch.equal(u[..., :w], u_hi[..., :w]) and not torch.equal(u[..., w:], u_hi[..., w:])
    assert torch.equal(u[..., w:], u_lo[..., w:]) and not torch.equal(u[..., :w], u_lo[..., :w])
    ref = F.relu(F.batch_norm(F.conv2d(o1.double().cpu().permute(0, 3, 1, 2), blk.conv2.conv.weight.detach().double().cpu(), None, 1, 1, groups=2),
                              blk.conv2.bn0.running_mean.double().cpu(), blk.conv2.bn0.running_var.double().cpu(),
                              blk.conv2.bn0.weight.detach().double().cpu(), blk.conv2.bn0.bias.detach().double().cpu(), False, 0.0, 1e-5))
    assert float((u.double().cpu().permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max()) <= RS.BAR_OUT


def _torch_forward(m, img):
    """The backbone restated in plain torch (tests/resnest_ref.restated_forward) on the CPU in fp64, from the model's state dict."""
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()}
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    with torch.no_grad():
        return RS.restated_forward(sd, dict(depth=m.depth, style=m.style), img.detach().cpu().double())


def _locator(head, seed=0, frozen_stages=4):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(cfg['backbone'], type='ResNeSt', frozen_stages=frozen_stages)
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(50, 1, head=head, seed=seed, head_std=0.3)
    sd = {k: v for k, v in sd.items() if not k.startswith('backbone.')}
    sd.update(synthetic.resnest_state_dict(50, seed))
    m.load_state_dict(sd, strict=True)
    return m.train()


def _batch(seed=11):
    b = synthetic.synthetic_batch(2, 128, 160, 5, 1, seed)
    return b['img'].cuda(), b['img_metas'], [t.cuda() for t in b['gt_bboxes']], [t.cuda() for t in b['gt_labels']]


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_locator_runs_with_the_resnest_backbone(head):
    m = _locator(head)
    img, metas, boxes, labels = _batch()
    with torch.no_grad():
        a = m.forward_train(img, metas, boxes, labels)
        b = m.forward_train(img, metas, boxes, labels)
        feats = m.backbone(img)
    torch.cuda.synchronize()

    def flat(d):      # (a loss entry is a tensor or a list of tensors)
        return [(k, t) for k, v in d.items() for t in (v if isinstance(v, (list, tuple)) else [v])]
    assert a and all(bool(torch.isfinite(t).all()) for _, t in flat(a))
    for (k, t), (_, u) in zip(flat(a), flat(b)):
        assert torch.equal(t, u), k
    for l, (o, r) in enumerate(zip(feats, _torch_forward(m.backbone, img))):
        assert float((o.double().cpu() - r).abs().max() / r.abs().max()) <= RS.BAR_OUT, l


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_bridge_is_bit_equal_to_the_trainer(head):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    img, metas, boxes, labels = _batch()
    data = dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels)
    ma = _locator(head, frozen_stages=1)
    assert autograd_bridge.unsupported_reason(ma, boxes, labels) is None
    tr = (CprTrainer if head == 'cpr' else P2PTrainer)(ma)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    for k in ('backbone.layer2.0.conv2.conv.weight', 'backbone.layer4.2.conv2.fc1.bias', 'backbone.layer3.1.conv2.bn1.weight',
              'backbone.layer2.0.conv2.fc2.weight', 'backbone.layer3.1.conv1.weight'):
        assert k in want and bool(torch.isfinite(want[k]).all()) and float(want[k].abs().max()) > 0, k
    mb = _locator(head, frozen_stages=1)
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


def test_optimizer_step_then_fresh_model_gives_the_same_forward():
    """One native optimizer step (parameters change through raw pointers, the weight epoch is bumped): the block-diagonal packs lapse
    and rebuild, the folds refresh -- a fresh model holding the stepped weights gives the same forward bit for bit."""
    from pointtinybenchmark_amd.training import CprTrainer
    img, metas, boxes, labels = _batch()
    data = dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels)
    m = _locator('cpr', frozen_stages=1)
    tr = CprTrainer(m, lr=0.05)
    with torch.no_grad():
        m.eval()
        before = [o.clone() for o in m.backbone(img)]      # builds the packs the step must refresh or drop
        m.train()
    out = tr.train_step(dict(data))
    torch.cuda.synchronize()
    assert all(v == v and abs(v) < float('inf') for v in out['log_vars'].values()), out['log_vars']
    m.eval()
    fresh = _locator('cpr', frozen_stages=1)
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    fresh.eval()
    with torch.no_grad():
        a, b = m.backbone(img), fresh.backbone(img)
        la, lb = m.extract_feat(img), fresh.extract_feat(img)
    torch.cuda.synchronize()
    assert torch.equal(a[0], before[0])                    # the frozen stage did not move
    assert not torch.equal(a[1], before[1])                # the trained ones did
    for x, y in zip(list(a) + list(la), list(b) + list(lb)):
        assert torch.equal(x, y), 'forward after the step differs from a fresh model in %d entries' % int((x != y).sum())


def test_refusals_on_the_device():
    cfg, m = _case_model('s50')
    img = RS.case_input(cfg).cuda()
    m.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match='radix=2'):
        m(img)
    m.compute_dtype = torch.float32
    _, bs = _case_model('s50', norm_eval=False)
    with pytest.raises(NotImplementedError, match='norm_eval'):
        bs(img)
    with torch.no_grad():
        assert len(bs.eval()(img)) == 4
