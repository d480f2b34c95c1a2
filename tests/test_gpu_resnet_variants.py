"""-m gpu: the ResNet variants -- style='caffe', avg_down, deep_stem, ResNetV1d.

  kernels    average pool forward / backward (csrc/stem_deep.hip) against fp64 torch on even, odd x even and odd x odd maps; the
             deep stem against an fp64 chain of the same folded layers, planar and NHWC4 inputs, the bf16 mode against the fp32 mode
  fixture    tests/golden/resnet_variants.npz (the reference's own classes in fp64, tools/gen_resnet_variants.py): stage outputs
             <= 2e-4 max|level|, parameter gradients of the fixture's linear functional through BackwardEngine <= 2e-3 rel-L2
  bridge     loss.backward() through the autograd bridge is bit-equal to the native trainer
  batch statistics (fp32)  forward and running buffers against an fp64 restatement, the backward per block replayed in fp64 autograd
             (the method and the 1e-4 bar of tests/test_gpu_bn_batch_stats.py); bf16 + batch statistics still raises
  mixed precision          the bf16 backward kernels against fp32 ones behind the same bf16 forward (<= 0.03 per tensor), the whole
             gradient against the fp32 step (cosine >= 0.995): the bars of bench.py's training parity gate
  trainers   one full CprTrainer / P2PTrainer step with ResNetV1d: finite, bit-repeatable, eval after train reads refreshed packs"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic
from tests import resnet_variants_ref as RV

pytestmark = pytest.mark.gpu


def _rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


# ------------------------------------------------------------------------------------------------ average pool
MAPS = [(8, 12), (7, 12), (8, 11), (7, 9), (1, 1), (1, 2), (3, 1), (17, 24)]


@pytest.mark.parametrize('C', [64, 256, 1024])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_avgpool_forward_and_backward_vs_fp64_torch(dtype, C):
    """fp32: <= 1e-6 relative per element; bf16 maps: <= 2^-8 relative (one bf16 rounding of the fp32 result) against fp64 on the
    same bf16 inputs.  The forward is held to the per-element bar on non-negative maps -- what the pool reads in the network, a
    ReLU output: a window sum does not cancel there, so three fp32 roundings (<= 1.8e-7) and the bf16 one are all there is; on signed
    maps a window may cancel to any fraction of its terms, so the same bars are taken relative to the window's largest |term| (the
    bound of any fp32 sum).  The backward is one division (+ one addition): per element on signed gradients; the sum relative to
    itself (its one output rounding) or, where it cancels, to the larger of its two terms (the fp32 addition).  Run twice -> equal
    bits."""
    from pointtinybenchmark_amd import ops
    bar = 1e-6 if dtype == torch.float32 else 2.0 ** -8
    for i, (H, W) in enumerate(MAPS):
        for s, signed in ((2, False), (2, True), (3, False)):
            x = _rand((2, H, W, C), 10 + i, dtype)
            x = x if signed else x.abs()
            got = ops.avgpool(x, s)
            xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
            want = F.avg_pool2d(xr, s, s, ceil_mode=True, count_include_pad=False)
            torch.cuda.synchronize()
            assert got.shape == (2, -(-H // s), -(-W // s), C) and got.dtype == dtype and got.is_contiguous()
            w = want.detach().permute(0, 2, 3, 1)
            tol = bar * w.abs()
            if signed:
                tol = bar * F.max_pool2d(x.double().abs().permute(0, 3, 1, 2), s, s, ceil_mode=True).permute(0, 2, 3, 1)
            assert bool(((got.double() - w).abs() <= tol).all()), (H, W, s, signed, float(((got.double() - w).abs() / w.abs()).max()))
            assert torch.equal(got, ops.avgpool(x, s))
            g = _rand(tuple(got.shape), 40 + i, dtype)
            want.backward(g.double().permute(0, 3, 1, 2))
            dx = ops.avgpool_bwd(g, (H, W), s)
            torch.cuda.synchronize()
            assert dx.shape == x.shape and dx.dtype == dtype
            wg = xr.grad.permute(0, 2, 3, 1)
            assert bool(((dx.double() - wg).abs() <= bar * wg.abs()).all()), (H, W, s)
            assert torch.equal(dx, ops.avgpool_bwd(g, (H, W), s))
            add = _rand(tuple(x.shape), 70 + i, dtype)
            dxa = ops.avgpool_bwd(g, (H, W), s, add=add)
            torch.cuda.synchronize()
            wa = wg + add.double()
            assert bool(((dxa.double() - wa).abs() <= bar * torch.maximum(wa.abs(), torch.maximum(wg.abs(), add.double().abs()))).all()), (H, W, s)
            if dtype == torch.float32:      # the add form = pool-backward + axpby, bit for bit
                assert torch.equal(dxa, ops.axpby(ops.avgpool_bwd(g, (H, W), s), add, 1.0, 1.0))
            assert torch.equal(dxa, ops.avgpool_bwd(g, (H, W), s, add=add))


def test_avgpool_refuses_what_it_cannot_run():
    from pointtinybenchmark_amd import ops
    x = _rand((1, 4, 4, 64), 1)
    with pytest.raises(AssertionError):
        ops.avgpool(x, 1)
    with pytest.raises(AssertionError):
        ops.avgpool(_rand((1, 4, 4, 6), 1), 2)
    with pytest.raises(AssertionError):
        ops.avgpool_bwd(x, (9, 8), 2)


# ------------------------------------------------------------------------------------------------ deep stem
def _v1d(depth=18, seed=5, **kw):
    from pointtinybenchmark_amd.backbones.resnet import ResNetV1d
    m = ResNetV1d(depth=depth, frozen_stages=kw.pop('frozen_stages', 1), **kw).cuda()
    m.load_state_dict(synthetic.resnet_state_dict(depth, seed, prefix='', deep_stem=True, avg_down=True), strict=True)
    m.train()
    return m


def _deep_stem64(m, img):
    """fp64 torch: the three convs with their BatchNorms folded to (scale, shift) in fp64, ReLU after each, then the max-pool."""
    x = img.double().cpu()
    for i in (0, 3, 6):
        conv, bn = m.stem[i], m.stem[i + 1]
        scale = bn.weight.double().cpu() / torch.sqrt(bn.running_var.double().cpu() + bn.eps)
        shift = bn.bias.double().cpu() - bn.running_mean.double().cpu() * scale
        x = F.relu(F.conv2d(x, conv.weight.double().cpu(), None, conv.stride, conv.padding) * scale[None, :, None, None]
                   + shift[None, :, None, None])
    return F.max_pool2d(x, 3, 2, 1)


@pytest.mark.parametrize('hw', [(70, 90), (128, 160), (67, 93), (33, 65), (5, 3)])
def test_deep_stem_vs_fp64_chain(hw):
    """<= 2e-4 max|out| (the a3 bar); planar and NHWC4 inputs give equal bits; the bf16 mode against the fp32 mode within the bars of
    tests/test_gpu_bf16.py (max <= 8 % of the scale, mean <= 1 %)."""
    from pointtinybenchmark_amd import ops
    m = _v1d()
    img = _rand((2, 3) + hw, 3) * 1.2
    with torch.no_grad():
        out = m.run_stem(img)
        x4 = ops.nchw_to_nhwc(img)
        out4 = m.run_stem(ops.as_nchw(x4))                       # the 4-channel channels-last view the image pipeline emits
        torch.cuda.synchronize()
        ref = _deep_stem64(m, img).permute(0, 2, 3, 1)
        assert out.shape == tuple(ref.shape) and out.dtype == torch.float32
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print('ERR deep stem %s max|diff|/max|out| %.2e (bar 2e-4)' % (hw, err), flush=True)
        assert err <= 2e-4
        assert torch.equal(out, out4), 'planar and NHWC4 inputs differ in %d entries' % int((out != out4).sum())
        assert torch.equal(out, m.run_stem(img))
        m.compute_dtype = torch.bfloat16
        o16 = m.run_stem(img)
        o16b = m.run_stem(ops.as_nchw(x4))
        torch.cuda.synchronize()
    assert o16.dtype == torch.bfloat16 and o16.shape == out.shape and torch.equal(o16, o16b)
    # the bf16 mode differs only in the last store: the rounding of the fp32 mode's output, bit for bit
    assert torch.equal(o16.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), \
        'the bf16 output is not the rounding of the fp32 output in %d entries' % int((o16 != out.to(torch.bfloat16)).sum())
    scale = max(1.0, float(out.abs().max()))
    e = (o16.float() - out).abs()
    assert float(e.max()) <= 8e-2 * scale and float(e.mean()) <= 1e-2 * scale, (float(e.max()), float(e.mean()), scale)


def test_deep_stem_forward_only_with_a_trainable_stem_runs_and_a_tape_raises():
    m = _v1d(frozen_stages=-1)
    img = _rand((1, 3, 64, 64), 2)
    with torch.no_grad():
        outs = m(img)
    torch.cuda.synchronize()
    assert len(outs) == 4 and all(bool(torch.isfinite(o).all()) for o in outs)
    with pytest.raises(NotImplementedError, match='deep_stem'):
        m(img, tape=[])


# ------------------------------------------------------------------------------------------------ the fixture cases
def _case_model(name):
    import pointtinybenchmark_amd as P
    cfg = RV.CASES[name]
    kw = RV.resnet_kwargs(cfg)
    typ = 'ResNet'
    if kw['deep_stem'] and kw['avg_down']:
        kw.pop('deep_stem'), kw.pop('avg_down')
        typ = 'ResNetV1d'
    m = P.build_backbone(dict(type=typ, **kw)).cuda()
    m.load_state_dict(RV.case_state_dict(cfg), strict=True)
    m.train()
    return cfg, m


@pytest.mark.parametrize('name', RV.CASE_NAMES)
def test_stage_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = RV.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
    torch.cuda.synchronize()
    assert len(outs) == 4
    failed = []
    for l, o in enumerate(outs):
        e = RV.output_error(name, l, o)
        print('ERR forward %-12s stage %d %-10s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[2:]), e), flush=True)
        if not e <= RV.BAR_OUT:
            failed.append((l, e))
        assert torch.equal(o, again[l])
    assert not failed, failed


@pytest.mark.parametrize('name', RV.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    """The recorded forward + BackwardEngine._backward_backbone on the fixture's linear functional (the gradient of stage l's output
    = w_l) against the reference classes' fp64 autograd: rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample."""
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg, m = _case_model(name)
    eng = BackwardEngine(m)
    eng._sink = {}
    tape = []
    outs = m(RV.case_input(cfg).cuda(), tape=tape)
    # the forward-only path fuses the projection shortcut into conv3's launch; the recorded one must give the same bits
    with torch.no_grad():
        plain = m(RV.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    d_stage = {l: RV.functional_weight(cfg, l, o.shape).permute(0, 2, 3, 1).contiguous().cuda() for l, o in enumerate(outs)
               if l + 1 > cfg['frozen_stages']}
    eng._backward_backbone(m, tape, d_stage)
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    assert [k for k, _ in named] == RV.grad_names(name)
    grads = dict(zip([k for k, _ in named], eng.collect([p for _, p in named])))
    torch.cuda.synchronize()
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        en, es = RV.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= RV.BAR_GRAD and es <= RV.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-12s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    assert not failed, failed[:8]


# ------------------------------------------------------------------------------------------------ locators
def _locator(head, variant, depth, frozen_stages=1, norm_eval=True, seed=3):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(depth, 1) if head == 'cpr' else p2p_model_cfg(depth, 1)
    deep, avg = variant in ('v1d', 'deepstem'), variant in ('v1d', 'avgdown')
    bb = dict(cfg['backbone'], frozen_stages=frozen_stages, norm_eval=norm_eval)
    if variant == 'v1d':
        bb['type'] = 'ResNetV1d'
    else:
        bb.update(deep_stem=deep, avg_down=avg, style='caffe' if variant == 'caffe' else 'pytorch')
    cfg['backbone'] = bb
    m = P.build_detector(cfg).cuda()
    m.load_state_dict(synthetic.locator_state_dict(depth, 1, 0, head, seed, head_std=0.05, deep_stem=deep, avg_down=avg), strict=True)
    m.train()
    return m


def _data(hw=(96, 128), seed=4, n=2):
    batch = synthetic.synthetic_batch(n, hw[0], hw[1], 6, 1, seed=seed)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def _trainer(head, m, **kw):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return (CprTrainer if head == 'cpr' else P2PTrainer)(m, **kw)


@pytest.mark.parametrize('head,variant,depth,fs', [('cpr', 'v1d', 18, 1), ('cpr', 'v1d', 50, 0), ('cpr', 'caffe', 50, 1),
                                                   ('cpr', 'avgdown', 50, 1), ('p2p', 'v1d', 50, 1), ('p2p', 'caffe', 18, 1)])
def test_bridge_is_bit_equal_to_the_trainer(head, variant, depth, fs):
    data = _data((70, 90))
    ma = _locator(head, variant, depth, fs)
    tr = _trainer(head, ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb = _locator(head, variant, depth, fs)
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


# ------------------------------------------------------------------------------------------------ batch statistics
def _variant_backbone(variant, depth, frozen_stages, norm_eval=False, seed=3):
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    deep, avg = variant in ('v1d', 'deepstem'), variant in ('v1d', 'avgdown')
    m = ResNet(depth, frozen_stages=frozen_stages, norm_eval=norm_eval, deep_stem=deep, avg_down=avg,
               style='caffe' if variant == 'caffe' else 'pytorch').cuda()
    m.load_state_dict(synthetic.resnet_state_dict(depth, seed, prefix='', deep_stem=deep, avg_down=avg), strict=True)
    m.train()
    return m


def _backbone64(m, img, sd, momentum=0.1, stage_inputs=None):
    """fp64 torch restatement of the backbone forward as the reference's modules run it in train(): eval-mode BatchNorm on the
    frozen stages (and the stem), batch statistics on the others, running buffers updated on clones.  -> (stage outputs, buffers).
    stage_inputs (optional, NCHW): stage i >= 1 reads stage_inputs[i] instead of the restatement's own stage i - 1 output."""
    bufs = {}

    def bn(x, prefix, mod):
        w, b = sd[prefix + '.weight'].double(), sd[prefix + '.bias'].double()
        if not mod.training:
            return F.batch_norm(x, sd[prefix + '.running_mean'].double(), sd[prefix + '.running_var'].double(), w, b, False, 0.0, mod.eps)
        bufs[prefix] = [sd[prefix + '.running_mean'].double().clone(), sd[prefix + '.running_var'].double().clone()]
        return F.batch_norm(x, bufs[prefix][0], bufs[prefix][1], w, b, True, momentum, mod.eps)

    def conv(x, prefix, mod):
        return F.conv2d(x, sd[prefix + '.weight'].double(), None, mod.stride, mod.padding)
    x = img.double()
    if m.deep_stem:
        for i in (0, 3, 6):
            x = F.relu(bn(conv(x, 'stem.%d' % i, m.stem[i]), 'stem.%d' % (i + 1), m.stem[i + 1]))
    else:
        x = F.relu(bn(conv(x, 'conv1', m.conv1), 'bn1', m.bn1))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    for si, name in enumerate(m.res_layers):
        if stage_inputs is not None and si >= 1:
            x = stage_inputs[si].double()
        for bi, blk in enumerate(getattr(m, name)):
            p = '%s.%d.' % (name, bi)
            o = F.relu(bn(conv(x, p + 'conv1', blk.conv1), p + 'bn1', blk.bn1))
            if blk.kind == 'bottleneck':
                o = F.relu(bn(conv(o, p + 'conv2', blk.conv2), p + 'bn2', blk.bn2))
                o = bn(conv(o, p + 'conv3', blk.conv3), p + 'bn3', blk.bn3)
            else:
                o = bn(conv(o, p + 'conv2', blk.conv2), p + 'bn2', blk.bn2)
            idn = x
            if blk.downsample is not None:
                ds = blk.downsample
                j = 0
                if isinstance(ds[0], nn.AvgPool2d):
                    idn = F.avg_pool2d(idn, ds[0].kernel_size, ds[0].stride, ceil_mode=True, count_include_pad=False)
                    j = 1
                idn = bn(conv(idn, p + 'downsample.%d' % j, ds[j]), p + 'downsample.%d' % (j + 1), ds[j + 1])
            x = F.relu(o + idn)
        outs.append(x)
    return outs, bufs


BS_CASES = [('avgdown', 18, 1), ('avgdown', 50, 1), ('avgdown', 50, 2), ('caffe', 50, 1), ('caffe', 50, 2), ('caffe', 18, 2),
            ('v1d', 50, 1), ('v1d', 18, 2)]


@pytest.mark.parametrize('variant,depth,frozen_stages', BS_CASES)
def test_batch_statistics_forward_and_buffers_vs_fp64(variant, depth, frozen_stages):
    """Every stage against the fp64 restatement of that stage on the input the kernels gave it (stage 0: on the image), rel-L2 <= 1e-4,
    and the running buffers it updates.  Stage by stage because a chained comparison has no room under this bar on an R50: with
    these weights torch itself in fp32 is 4.5e-5 .. 9.4e-5 off its fp64 run at stage 3 of the three R50 frozen_stages=1 variants
    (x 3 .. 5 per batch-statistics stage, the same on 93 x 131, 96 x 128 and 189 x 259 images and on three image seeds), while one
    stage alone is <= 7e-6 (restatement run in fp32, CPU) -- the same isolation the per-block backward test below uses."""
    m = _variant_backbone(variant, depth, frozen_stages)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    img = torch.randn((2, 3, 93, 131), generator=torch.Generator().manual_seed(0))      # odd maps: 24x33 -> 12x17 -> 6x9 -> 3x5
    assert m.batch_stats_active()
    outs = m(img.cuda())
    torch.cuda.synchronize()
    with torch.no_grad():
        ref, bufs = _backbone64(m, img, sd0, stage_inputs=[None] + [o.detach().cpu() for o in outs[:-1]])
    for i, (a, b) in enumerate(zip(outs, ref)):
        print('ERR batch statistics %s R%d fs%d stage %d rel-L2 %.2e (bar 1e-4)' % (variant, depth, frozen_stages, i, _rel_l2(a, b)),
              flush=True)
        assert _rel_l2(a, b) <= 1e-4, (i, _rel_l2(a, b))
    sd = m.state_dict()
    assert bufs and all(int(p.split('.')[0][len('layer'):]) > frozen_stages for p in bufs)
    for k, v in sd.items():
        if not k.endswith('num_batches_tracked'):
            continue
        p = k[:-len('.num_batches_tracked')]
        assert int(v) == int(p in bufs), k
        for j, nm in enumerate(('running_mean', 'running_var')):
            got = sd[p + '.' + nm].cpu().double()
            if p in bufs:
                assert torch.allclose(got, bufs[p][j], rtol=1e-4, atol=1e-5 * float(bufs[p][j].abs().max())), (p, nm)
            else:
                assert torch.equal(sd[p + '.' + nm].cpu(), sd0[p + '.' + nm]), (p, nm)


def _block_fp64(blk, x, P, masks):
    """fp64 torch autograd of one block with training-mode BatchNorm (tests/test_gpu_bn_batch_stats.py, with the avg_down shortcut):
    the ReLUs take their 0/1 pattern from the kernel's recorded outputs."""
    def bn(t, mod):
        return F.batch_norm(t, None, None, P[id(mod.weight)], P[id(mod.bias)], True, 0.1, mod.eps)

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
    idn = x
    if blk.downsample is not None:
        if isinstance(blk.downsample[0], nn.AvgPool2d):
            pool = blk.downsample[0]
            idn = F.avg_pool2d(idn, pool.kernel_size, pool.stride, ceil_mode=True, count_include_pad=False)
        idn = bn(conv(idn, blk.ds_conv), blk.ds_bn)
    return relu(o + idn, masks[2])


@pytest.mark.parametrize('variant,depth,frozen_stages', BS_CASES)
def test_batch_statistics_backward_vs_fp64_autograd_per_block(variant, depth, frozen_stages):
    """Every recorded block replayed in fp64 autograd from the block input and output gradient the engine saw, with the kernel's own
    ReLU patterns: forward, parameter gradients and input gradient within 1e-4."""
    from pointtinybenchmark_amd.training import BackwardEngine
    m = _variant_backbone(variant, depth, frozen_stages)
    eng = BackwardEngine(m)
    eng._sink = {}
    g = torch.Generator().manual_seed(3)
    img = torch.randn((2, 3, 93, 131), generator=g)
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
    pooled = 0
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
        if blk.ds_pool:
            pooled += 1
            assert rec['xp'].shape[1] == -(-rec['x'].shape[1] // 2)
        bad += [(e, rec['stage'], n) for n, e in errs if e > 1e-4]
    assert (pooled > 0) == (variant in ('v1d', 'avgdown'))
    assert not bad, 'block mismatch (rel L2, stage, what): %s' % sorted(bad, reverse=True)[:8]


@pytest.mark.parametrize('variant', ['v1d', 'caffe', 'avgdown'])
def test_bf16_with_batch_statistics_still_raises(variant):
    m = _variant_backbone(variant, 18, 1)
    m.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m(_rand((1, 3, 64, 64), 1))


# ------------------------------------------------------------------------------------------------ mixed precision
@pytest.mark.parametrize('variant', ['v1d', 'caffe'])
def test_mixed_precision_step(variant):
    """R50-shaped, eval BatchNorm.  The bars and the skip rule of bench.py's training parity gate: the product step against the same
    bf16 forward with fp32 weight / data gradients <= 0.03 per tensor (tensors below 1e-3 of the largest norm skipped); the whole
    gradient against the fp32 step: cosine >= 0.995."""
    from pointtinybenchmark_amd import training
    m = _locator('cpr', variant, 50)
    data = _data((160, 192), n=2)
    tr = _trainer('cpr', m, lr=1e-3)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    g32 = tr.flat_g.clone()
    m.set_compute_dtype('bf16')
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    g16 = tr.flat_g.clone()
    assert bool(torch.isfinite(g16).all())
    # the recorded shortcut input of an avg_down block is the pooled bf16 map
    training.MIXED_BF16.update(wgrad=False, dgrad=False)
    try:
        tr.forward_backward(**data)
        torch.cuda.synchronize()
    finally:
        training.MIXED_BF16.update(wgrad=True, dgrad=True)
    gB = tr.flat_g.clone()
    names = {id(p): k for k, p in m.named_parameters()}
    norms, off = [], 0
    for p_ in tr.params:
        n = p_.numel()
        norms.append((names[id(p_)], off, n, float(gB[off:off + n].double().norm())))
        off += n
    gmax = max(x[3] for x in norms)
    worst = max(((float((g16[o:o + n].double() - gB[o:o + n].double()).norm()) / nb, k) for k, o, n, nb in norms if nb > 1e-3 * gmax))
    cos = float(torch.dot(g16.double(), g32.double()) / (g16.double().norm() * g32.double().norm()))
    print('ERR mixed %-6s backward kernels worst per tensor %.4f at %s (bar 0.03); cosine to the fp32 step %.5f (bar 0.995)'
          % (variant, worst[0], worst[1], cos), flush=True)
    assert worst[0] <= 0.03, worst
    assert cos >= 0.995, cos


# ------------------------------------------------------------------------------------------------ trainers
@pytest.mark.parametrize('head', ['cpr', 'p2p'])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_full_step_with_resnetv1d(head, mode):
    """One full optimisation step: finite losses; a second identical step from the same state is bit-equal; eval after the step
    reads the refreshed packs (compared with a fresh model holding the stepped weights)."""
    data = _data((96, 128))
    runs = []
    for _ in range(2):
        m = _locator(head, 'v1d', 50)
        m.set_compute_dtype(mode)
        tr = _trainer(head, m, lr=0.05)
        with torch.no_grad():
            m.eval()
            before = [o.clone() for o in m.backbone(data['img'])]     # builds the eval packs the step must refresh
            m.train()
        out = tr.train_step(dict(data))
        torch.cuda.synchronize()
        assert all(v == v and abs(v) < float('inf') for v in out['log_vars'].values()), out['log_vars']
        runs.append((out['log_vars'], tr.flat_p.clone(), m, before))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]), 'parameters differ in %d entries' % int((runs[0][1] != runs[1][1]).sum())
    m, before = runs[0][2], runs[0][3]
    # layer2.0's avg_down shortcut conv and conv1 sit right behind the frozen layer1: they trained
    assert m.backbone.layer2[0].downsample[1].weight.requires_grad
    m.eval()
    fresh = _locator(head, 'v1d', 50)
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    fresh.set_compute_dtype(mode)
    fresh.eval()
    with torch.no_grad():
        a, b = m.backbone(data['img']), fresh.backbone(data['img'])
    torch.cuda.synchronize()
    assert torch.equal(a[0], before[0])                           # the frozen stage did not move
    assert not torch.equal(a[1], before[1])                       # the trained ones did
    for x, y in zip(a, b):
        assert torch.equal(x, y), 'eval after train differs from a fresh model in %d entries' % int((x != y).sum())
