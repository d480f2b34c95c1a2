"""-m gpu: the Res2Net backbone on the slice kernels (csrc/res2net.hip), forward and training.

  fixture    tests/golden/res2net.npz (the reference's own Res2Net in fp64, tools/gen_res2net.py): stage outputs <= 2e-4 max|level| for
             every case (26w4s, 14w8s on odd maps, 48w2s with its empty loop and no pad channels, 101 / 26w4s); a second forward is
             bit-equal
             ... and the recorded forward equals the forward-only one bit for bit; parameter gradients of the fixture's linear functional
             through BackwardEngine._backward_backbone <= 2e-3 rel-L2 on norm and sample, named_parameters order the fixture's
  per block  one case replayed block by block in fp64 autograd from the recorded input and output gradient with the kernel's own ReLU
             patterns, within 1e-4 (the method of the ResNeXt batch-statistics test)
  pad        the pad channels of the block's two internal maps hold exact zeros in every block
  locator    a small CPR and a small P2P locator with the Res2Net backbone: forward_train's losses are finite, repeat bit for bit and
             the backbone's maps match its plain-torch restatement (fp64, CPU) within the fixture's output bar
  training   a CPR and a P2P locator (frozen_stages=1): loss.backward() through the bridge is bit-equal to the native trainer; the same
             over a frozen Res2Net (frozen_stages=4); after one optimizer step a fresh model holding the stepped weights gives the same
             forward bit for bit
  packs      after the parameters are stepped in place and the weight epoch is bumped, the model gives the same forward bit for bit as a
             fresh model holding the stepped weights (a stale padded pack would show)
  refusals   the bf16 compute mode names ``scales``, batch statistics ``norm_eval`` -- on the device"""
import pytest
import torch
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic
from tests import res2net_ref as R2

pytestmark = pytest.mark.gpu


def _case_model(name, **kw):
    import pointtinybenchmark_amd as P
    cfg = R2.CASES[name]
    m = P.build_backbone(dict(type='Res2Net', **dict(R2.res2net_kwargs(cfg), **kw))).cuda()
    m.load_state_dict(R2.case_state_dict(cfg), strict=True)
    m.train()
    return cfg, m


@pytest.mark.parametrize('name', R2.CASE_NAMES)
def test_stage_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = R2.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
    torch.cuda.synchronize()
    assert len(outs) == 4
    failed = []
    for l, o in enumerate(outs):
        e = R2.output_error(name, l, o)
        print('ERR forward %-14s stage %d %-10s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[2:]), e), flush=True)
        if not e <= R2.BAR_OUT:
            failed.append((l, e))
        assert torch.equal(o, again[l])
    assert not failed, failed


def test_pad_channels_hold_exact_zeros_in_every_block(monkeypatch):
    """26w4s: the internal maps of layer1 / layer2 are 128 / 224 channels wide for 104 / 208 real ones."""
    from pointtinybenchmark_amd import ops
    cfg, m = _case_model('r50_26w4s')
    img = R2.case_input(cfg).cuda()
    seen = []
    real_pool = ops.res2_pool

    def spy_pool(x, x_off, out, out_off, width, stride):
        r = real_pool(x, x_off, out, out_off, width, stride)
        seen.append((x, out, x_off + width))
        return r
    monkeypatch.setattr(ops, 'res2_pool', spy_pool)
    with torch.no_grad():
        outs = m(img)
    monkeypatch.setattr(ops, 'res2_pool', real_pool)
    assert len(seen) == 16
    padded = 0
    for o1, cat, Wd in seen:
        assert o1.shape[-1] % 32 == 0 and cat.shape[-1] == o1.shape[-1] and o1.shape[-1] - Wd < 32
        if o1.shape[-1] > Wd:
            padded += 1
            assert int(torch.count_nonzero(o1[..., Wd:])) == 0 and int(torch.count_nonzero(cat[..., Wd:])) == 0
        assert bool(torch.isfinite(cat).all())
    assert padded == 7          # layer1 (104 -> 128) and layer2 (208 -> 224); 416 and 832 need no padding
    assert all(bool(torch.isfinite(o).all()) for o in outs)


def _torch_forward(m, img):
    """The backbone restated in plain torch (tests/res2net_ref.restated_forward) on the CPU in fp64, from the model's state dict."""
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()}
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    with torch.no_grad():
        return R2.restated_forward(sd, dict(depth=m.depth, scales=m.scales), img.detach().cpu().double())


@pytest.mark.parametrize('setting', [(26, 6), (26, 8)], ids=['26w6s', '26w8s'])
def test_other_published_settings_run(setting):
    """26w6s / 26w8s (156 / 208 .. channels: pitches 160, 224, ...) have no fixture case: against the restatement in fp64 on the CPU
    (held to the fixture at 1e-9 by tests/test_res2net_host.py), at the fixture's output bar."""
    import pointtinybenchmark_amd as P
    bw, s = setting
    m = P.build_backbone(dict(type='Res2Net', depth=50, scales=s, base_width=bw, frozen_stages=4)).cuda()
    m.load_state_dict(synthetic.res2net_state_dict(50, s, bw, 7, prefix=''), strict=True)
    m.eval()
    img = torch.randn((2, 3, 67, 93), generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        outs = m(img)
    for l, (o, r) in enumerate(zip(outs, _torch_forward(m, img))):
        e = float((o.double().cpu() - r).abs().max() / r.abs().max())
        print('ERR forward %dw%ds stage %d max|diff|/max|level| %.2e (bar 2e-4)' % (bw, s, l, e), flush=True)
        assert e <= R2.BAR_OUT


def _locator(head, seed=0, frozen_stages=4):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(cfg['backbone'], type='Res2Net', scales=4, base_width=26, frozen_stages=frozen_stages)
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(50, 1, head=head, seed=seed, head_std=0.3)
    sd = {k: v for k, v in sd.items() if not k.startswith('backbone.')}
    sd.update(synthetic.res2net_state_dict(50, 4, 26, seed))
    m.load_state_dict(sd, strict=True)
    return m.train()


def _batch(seed=11):
    b = synthetic.synthetic_batch(2, 128, 160, 5, 1, seed)
    return b['img'].cuda(), b['img_metas'], [t.cuda() for t in b['gt_bboxes']], [t.cuda() for t in b['gt_labels']]


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_locator_runs_with_the_res2net_backbone(head):
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
        assert float((o.double().cpu() - r).abs().max() / r.abs().max()) <= R2.BAR_OUT, l


def test_frozen_backbone_trains_neck_and_head_bridge_bit_equal_to_the_trainer():
    """frozen_stages=4: the Res2Net forward under the native trainer and under loss.backward() through the autograd bridge -- the same
    bits for every neck and head gradient, none for the backbone; then one optimizer step runs."""
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer
    img, metas, boxes, labels = _batch()
    data = dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels)
    ma = _locator('cpr')
    assert autograd_bridge.unsupported_reason(ma, boxes, labels) is None
    tr = CprTrainer(ma)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    assert want and not any(k.startswith('backbone.') for k in want)
    assert all(bool(torch.isfinite(g).all()) for g in want.values()) and float(want['neck.lateral_convs.0.conv.weight'].abs().max()) > 0
    mb = _locator('cpr')
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad
    out['loss'].backward()
    torch.cuda.synchronize()
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
        else:
            assert p.grad is None, k
    step = tr.train_step(dict(data))
    torch.cuda.synchronize()
    assert all(v == v and abs(v) < float('inf') for v in step['log_vars'].values()), step['log_vars']


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
    outs = m(R2.case_input(cfg).cuda(), tape=tape)
    d_stage = {l: R2.functional_weight(cfg, l, o.shape).permute(0, 2, 3, 1).contiguous().cuda() for l, o in enumerate(outs)
               if l + 1 > cfg['frozen_stages']}
    eng._backward_backbone(m, tape, d_stage)
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    grads = dict(zip([k for k, _ in named], eng.collect([p for _, p in named])))
    torch.cuda.synchronize()
    return outs, tape, grads


@pytest.mark.parametrize('name', R2.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    """rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample, against the reference class's fp64 autograd; the recorded
    forward gives the forward-only one's bits."""
    cfg, m = _case_model(name)
    outs, tape, grads = _engine_backward(m, cfg)
    with torch.no_grad():
        plain = m(R2.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    assert list(grads) == R2.grad_names(name)
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        en, es = R2.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= R2.BAR_GRAD and es <= R2.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-14s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    assert not failed, failed[:8]


def _block_fp64(blk, x, P, rec):
    """fp64 torch autograd of one Bottle2neck with eval-mode BatchNorm; the ReLUs take their 0/1 pattern from the kernel's recorded maps."""
    def bn(t, mod):
        return F.batch_norm(t, mod.running_mean.double().cpu(), mod.running_var.double().cpu(), P[id(mod.weight)], P[id(mod.bias)], False,
                            0.0, mod.eps)

    def nchw64(t):
        return t.detach().double().cpu().permute(0, 3, 1, 2)

    def relu(t, mk):
        return t * (mk > 0).to(t.dtype)
    s, w = blk.scales, blk.width
    o1, cat = nchw64(rec['o1'])[:, :s * w], nchw64(rec['cat'])[:, :s * w]
    o = relu(bn(F.conv2d(x, P[id(blk.conv1.weight)]), blk.bn1), o1)
    spx = [o[:, i * w:(i + 1) * w] for i in range(s)]
    ys = []
    for i in range(s - 1):
        inp = spx[i] if (i == 0 or blk.stage_type == 'stage') else ys[-1] + spx[i]
        ys.append(relu(bn(F.conv2d(inp, P[id(blk.convs[i].weight)], None, blk.stride, 1), blk.bns[i]), cat[:, i * w:(i + 1) * w]))
    last = spx[s - 1]
    if blk.stage_type == 'stage' and blk.stride == 2:
        last = F.avg_pool2d(last, 3, 2, 1)
    o = bn(F.conv2d(torch.cat(ys + [last], 1), P[id(blk.conv3.weight)]), blk.bn3)
    idn = x
    if blk.downsample is not None:
        if blk.stride > 1:
            idn = F.avg_pool2d(idn, blk.stride, blk.stride, ceil_mode=True, count_include_pad=False)
        idn = bn(F.conv2d(idn, P[id(blk.ds_conv.weight)]), blk.ds_bn)
    return relu(o + idn, nchw64(rec['out']))


def test_backward_vs_fp64_autograd_per_block():
    """r50_26w4s_fs0 (layer1.0, a stage block at stride 1, trains): every recorded block replayed in fp64 autograd from the block input
    and the output gradient the engine saw: forward, parameter gradients and input gradient within 1e-4."""
    cfg, m = _case_model('r50_26w4s_fs0')
    seen = {}

    def spy(eng):
        rule = eng._bottle2neck_backward

        def wrapped(cache, blk, rec, dout, need_dx):
            seen[id(rec)] = dout.clone()
            r = rule(cache, blk, rec, dout, need_dx)
            seen[id(rec), 'dx'] = None if r is None else r.clone()
            return r
        eng._bottle2neck_backward = wrapped
    outs, tape, grads = _engine_backward(m, cfg, spy)
    assert len(tape) == 16 and all(id(r) in seen for r in tape)
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
    print('ERR backward r50_26w4s_fs0 per block: worst rel-L2 %.2e (bar 1e-4)' % worst, flush=True)
    assert not bad, 'block mismatch (rel L2, stage, block, what): %s' % sorted(bad, reverse=True)[:8]


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
    for k in ('backbone.layer2.0.convs.1.weight', 'backbone.layer4.2.bns.0.weight', 'backbone.layer3.1.conv1.weight'):
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
    """One native optimizer step (parameters change through raw pointers, the weight epoch is bumped): the padded packs, the slice packs
    and the folds are rebuilt or refreshed -- a fresh model holding the stepped weights gives the same forward bit for bit."""
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
    cfg, m = _case_model('r50_26w4s')
    img = R2.case_input(cfg).cuda()
    m.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match='scales=4'):
        m(img)
    m.compute_dtype = torch.float32
    _, bs = _case_model('r50_26w4s', norm_eval=False)
    with pytest.raises(NotImplementedError, match='norm_eval'):
        bs(img)
    with torch.no_grad():
        assert len(bs.eval()(img)) == 4
