"""-m gpu: the HRNet backbone (backbones/hrnet.py) and its exchange kernels (csrc/hrnet.hip).

  hrnet_fuse      bit-equal to tests/hrnet_ref.fuse_ref on every (shape, term table), guard-filled outputs, bit-repeatable; CPR_ERR_ARG on
                  an indivisible size and on five terms
  hrnet_fuse_bwd  g and the pools bit-equal to the ordered fp32 reference (y == 0 elements and a -0.0 in dy included); pools within
                  (4^k - 1) * 2^-24 * sum|terms| of fp64 per element, the reduced column sums within (n - 1) * 2^-24 * sum|g| per channel;
                  bit-repeatable; image 0 of an N = 2 launch equals the N = 1 launch on it
  backbone        tests/golden/hrnet.npz (the reference's own HRNet in fp64, tools/gen_hrnet.py): branch outputs <= 2e-4 max|level|,
                  parameter gradients through BackwardEngine._backward_backbone <= 2e-3 rel-L2 on the norm and on the strided sample;
                  a frozen group (the stem; one fuse conv) gets no gradient and leaves every other gradient unchanged to the bit
  locators        P2P (strides [4, 8, 16]) and CPR (one level) behind HRFPN, P2P behind FPN: one train_step, loss.backward() through the
                  bridge bit-equal to the native trainer, finite losses equal run to run; bf16 and norm_eval=False raise from forward,
                  trainer and bridge; the shipped W32 net loads strictly and takes one P2PTrainer step; conv1 alone against fp64"""
import warnings

import numpy as np
import pytest
import torch

from pointtinybenchmark_amd import synthetic
from tests import hrnet_ref as HR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8, 32), (2, 16, 24, 32), (2, 8, 24, 64), (1, 2, 3, 256), (3, 40, 8, 128)]
TABLES = [(0, 1), (0, 1, 2, 3), (0, 0, 1, 2), (0, 0, 0, 0), (0, 0)]


def _fits(shape, k):
    return shape[1] % (1 << k) == 0 and shape[2] % (1 << k) == 0


FUSE_CASES = [(s, t) for s in SHAPES for t in TABLES if _fits(s, max(t))]
BWD_CASES = [(s, K) for s in SHAPES for K in (0, 1, 2, 3) if _fits(s, K)]
assert len(FUSE_CASES) == 4 * 5 + 2 and len(BWD_CASES) == 4 * 4 + 1      # (1, 2, 3, 256) takes the k = 0 tables and K = 0 only


def _terms(shape, ks):
    rng = np.random.default_rng(sum(shape) * 131 + sum((i + 1) * (k + 1) for i, k in enumerate(ks)))
    N, H, W, C = shape
    terms = []
    for k in ks:
        m = rng.standard_normal((N, H >> k, W >> k, C)).astype(np.float32)
        m *= (10.0 ** rng.integers(-2, 3, m.shape)).astype(np.float32)      # mixed magnitudes: the order of the sum shows in the bits
        terms.append((m, k))
    return terms


# ------------------------------------------------------------------------------------------------ hrnet_fuse
@pytest.mark.parametrize('shape, ks', FUSE_CASES)
def test_fuse_is_bit_equal_to_the_reference(shape, ks):
    from pointtinybenchmark_amd import ops
    terms = _terms(shape, ks)
    want = HR.fuse_ref(terms)
    dev = [(torch.from_numpy(m).cuda(), k) for m, k in terms]
    out = torch.full(shape, float('nan'), device='cuda')
    ops.hrnet_fuse(dev, shape[1:3], out=out)
    again = ops.hrnet_fuse(dev, shape[1:3])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), 'differs in %d elements' % int((got != want).sum())
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    assert float(out.min()) == 0.0 and (got == 0).any() and (got > 0).any()


def test_fuse_argument_checks():
    import ctypes
    from pointtinybenchmark_amd import _lib, ops
    x = torch.zeros((1, 6, 8, 32), device='cuda')
    with pytest.raises(_lib.CprHipError, match='invalid argument'):      # 6 % 4 != 0
        ops.hrnet_fuse([(x, 0), (torch.zeros((1, 1, 2, 32), device='cuda'), 2)], (6, 8))
    with pytest.raises(_lib.CprHipError, match='invalid argument'):      # five terms
        ops.hrnet_fuse([(x, 0)] * 5, (6, 8))
    t = (ops._HrnetTerm * 5)()
    for e in t:
        e.p, e.k = x.data_ptr(), 0
    out = torch.zeros_like(x)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cpr_hrnet_fuse(t, 5, out.data_ptr(), 1, 6, 8, 32, stream) == -1001
    assert lib.cpr_hrnet_fuse(t, 0, out.data_ptr(), 1, 6, 8, 32, stream) == -1001
    t[1].k = 2
    assert lib.cpr_hrnet_fuse(t, 2, out.data_ptr(), 1, 6, 8, 32, stream) == -1001
    t[1].k = 4
    assert lib.cpr_hrnet_fuse(t, 2, out.data_ptr(), 1, 16, 16, 32, stream) == -1001
    t[1].k = 1
    assert lib.cpr_hrnet_fuse(t, 2, out.data_ptr(), 1, 6, 8, 30, stream) == -1001      # C % 4
    assert lib.cpr_hrnet_fuse_bwd_blocks(1, 6, 8, 32, 2) == -1001
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0      # a refused call launches nothing


def test_fuse_and_its_adjoint_propagate_nan_as_torch_does():
    from pointtinybenchmark_amd import ops
    t = torch.tensor([float('nan'), -1.0, 2.0, -0.0] * 8, device='cuda').reshape(1, 1, 1, 32)
    out = ops.hrnet_fuse([(t, 0), (torch.zeros_like(t), 0)], (1, 1))
    want = torch.relu(t + 0)
    g, _, _ = ops.hrnet_fuse_bwd(torch.ones_like(t), out, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[..., 0::4]).all()) and torch.equal(out[..., 1:4], want[..., 1:4]) and not bool(torch.signbit(out[..., 3]).any())
    assert g.flatten()[:4].tolist() == [1.0, 0.0, 1.0, 0.0]      # threshold_backward: the gradient passes where y is NaN


# ------------------------------------------------------------------------------------------------ hrnet_fuse_bwd
def _bwd_inputs(shape, K):
    rng = np.random.default_rng(sum(shape) * 17 + K)
    dy = rng.standard_normal(shape).astype(np.float32)
    dy *= (10.0 ** rng.integers(-2, 3, shape)).astype(np.float32)
    y = np.maximum(rng.standard_normal(shape), 0).astype(np.float32)      # about half the elements are exactly 0
    dy.reshape(-1)[::7] = -0.0
    y.reshape(-1)[0], y.reshape(-1)[7] = 1.0, 0.0      # a -0.0 that passes and one that is masked
    return dy, y


def _run_bwd(dy, y, K, guard=True):
    from pointtinybenchmark_amd import _lib, ops
    N, H, W, C = dy.shape
    d, m = torch.from_numpy(dy).cuda(), torch.from_numpy(y).cuda()
    if not guard:
        return ops.hrnet_fuse_bwd(d, m, K)
    tiles = _lib.call('cpr_hrnet_fuse_bwd_blocks', N, H, W, C, K, positive=True)
    out = (torch.full(dy.shape, float('nan'), device='cuda'),
           [torch.full((N, H >> k, W >> k, C), float('nan'), device='cuda') for k in range(1, K + 1)],
           torch.full((tiles, C, 2), float('nan'), device='cuda'))
    return ops.hrnet_fuse_bwd(d, m, K, out=out)


@pytest.mark.parametrize('shape, K', BWD_CASES)
def test_fuse_bwd_maps_pools_and_column_sums(shape, K):
    dy, y = _bwd_inputs(shape, K)
    g32, pools32, _ = HR.fuse_bwd_ref(dy, y, K)
    g64, pools64, cs64 = HR.fuse_bwd_ref64(dy, y, K)
    g, pools, part = _run_bwd(dy, y, K)
    g2, pools2, part2 = _run_bwd(dy, y, K, guard=False)
    cs = part.reduce()
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), g32.view(np.uint32))
    assert np.signbit(got.reshape(-1)[0]) and not np.signbit(got.reshape(-1)[7]) and (got == 0).any()
    assert len(pools) == K
    for k, (p, p32, p64, mag) in enumerate(zip(pools, pools32, pools64, HR.pool_abs_sums(g64, K)), 1):
        pn = p.cpu().numpy()
        assert pn.shape == (shape[0], shape[1] >> k, shape[2] >> k, shape[3])
        assert np.array_equal(pn.view(np.uint32), p32.view(np.uint32)), (k, int((pn != p32).sum()))
        assert np.all(np.abs(pn.astype(np.float64) - p64) <= (4 ** k - 1) * HR.U * mag), k
    n = shape[0] * shape[1] * shape[2]
    bound = (n - 1) * HR.U * np.abs(g64).reshape(-1, shape[3]).sum(0)
    err = np.abs(cs.cpu().numpy().astype(np.float64) - cs64)
    print('ERR fuse_bwd %s K=%d column sums worst err / bound %.3f' % (shape, K, float((err / np.maximum(bound, 1e-300)).max())), flush=True)
    assert np.all(err <= bound)
    assert torch.equal(part.part[..., 1], torch.zeros_like(part.part[..., 1])) and bool(torch.isfinite(part.part).all())
    # bit-repeatable
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32)) and torch.equal(part.part.view(torch.int32), part2.part.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(pools, pools2))


@pytest.mark.parametrize('shape, K', [(s, K) for s, K in BWD_CASES if s[0] == 2])
def test_fuse_bwd_image_does_not_depend_on_its_batch(shape, K):
    from pointtinybenchmark_amd import ops
    dy, y = _bwd_inputs(shape, K)
    g, pools, _ = _run_bwd(dy, y, K)
    g1, pools1, _ = _run_bwd(dy[:1].copy(), y[:1].copy(), K)
    terms = _terms(shape, (0,) + tuple(range(1, K + 1)))
    full = ops.hrnet_fuse([(torch.from_numpy(m).cuda(), k) for m, k in terms], shape[1:3])
    one = ops.hrnet_fuse([(torch.from_numpy(m[:1].copy()).cuda(), k) for m, k in terms], shape[1:3])
    torch.cuda.synchronize()
    assert torch.equal(g[:1].view(torch.int32), g1.view(torch.int32)) and torch.equal(full[:1].view(torch.int32), one.view(torch.int32))
    for a, b in zip(pools, pools1):
        assert torch.equal(a[:1].view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ backbone against the fixture
def _case_model(name):
    import pointtinybenchmark_amd as P
    cfg = HR.CASES[name]
    m = P.build_backbone(dict(type='HRNet', extra=cfg['extra'])).cuda()
    m.load_state_dict(HR.case_state_dict(cfg), strict=True)
    m.train()
    return cfg, m


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_branch_outputs_vs_reference(name):
    cfg, m = _case_model(name)
    img = HR.case_input(cfg).cuda()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
        nhwc4 = m(torch.cat([img, torch.zeros_like(img[:, :1])], 1).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert len(outs) == 4 and [o.shape[1] for o in outs] == m.out_channels
    failed = []
    for l, o in enumerate(outs):
        assert o.permute(0, 2, 3, 1).is_contiguous()      # an NCHW view of the NHWC buffer
        e = HR.output_error(name, l, o)
        print('ERR forward %-18s output %d %-14s max|diff|/max|level| %.2e (bar 2e-4)' % (name, l, tuple(o.shape[1:]), e), flush=True)
        if not e <= HR.BAR_OUT:
            failed.append((l, e))
        assert torch.equal(o, again[l]) and torch.equal(o, nhwc4[l])
        assert float(o.min()) == 0.0
    assert not failed, failed


def test_conv1_on_the_generic_kernels_vs_fp64():
    """The stem's conv1 (3 -> 64, 3x3 / 2) on its own: the dense kernel's Cin == 4 mode with bn1 + ReLU in the epilogue, and the generic weight
    gradient over the NHWC4 image with the zero fourth column dropped, against fp64 F.conv2d / autograd at an odd size (two blocks of
    output rows, a ragged right edge)."""
    import torch.nn.functional as F
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.layers import folded_bn, packed_conv
    cfg, m = _case_model('n1')
    g = torch.Generator().manual_seed(9)
    img = torch.randn((2, 3, 37, 70), generator=g)
    x4 = ops.nchw_to_nhwc(img.cuda())
    assert x4.shape[-1] == 4 and float(x4[..., 3].abs().max()) == 0.0
    s1, b1 = folded_bn(m._cache, m.bn1)
    o1 = ops.conv2d(x4, packed_conv(m._cache, m.conv1), scale=s1, bias=b1, relu=True)
    w64 = m.conv1.weight.detach().double().cpu().requires_grad_(True)
    bn = m.bn1
    y64 = F.batch_norm(F.conv2d(img.double(), w64, None, 2, 1), bn.running_mean.double().cpu(), bn.running_var.double().cpu(),
                       bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), False, 0.0, bn.eps)
    raw = F.conv2d(img.double(), w64, None, 2, 1)
    e = float((o1.permute(0, 3, 1, 2).double().cpu() - torch.relu(y64).detach()).abs().max() / y64.detach().abs().max())
    dy = torch.randn(raw.shape, generator=g)
    (raw * dy.double()).sum().backward()
    full = ops.conv2d_wgrad(dy.permute(0, 2, 3, 1).contiguous().cuda(), x4, (64, 4, 3, 3), 2, 1)
    torch.cuda.synchronize()
    ew = float((full[:, :3].double().cpu() - w64.grad).norm() / w64.grad.norm())
    print('ERR conv1 forward max|diff|/max %.2e (bar 2e-4), weight gradient rel-L2 %.2e (bar 2e-3)' % (e, ew), flush=True)
    assert tuple(o1.shape) == (2, 19, 35, 64) and e <= HR.BAR_OUT and ew <= HR.BAR_GRAD
    assert float(full[:, 3].abs().max()) == 0.0      # the zero column's gradient is zero: dropping it loses nothing


def _engine_backward(m, cfg, spy=None):
    """The recorded forward and BackwardEngine._backward_backbone on the fixture's linear functional -> (outs, {name: gradient})."""
    from pointtinybenchmark_amd.training import BackwardEngine
    eng = BackwardEngine(m)
    eng._sink = {}
    if spy is not None:
        spy(eng)
    tape = []
    outs = m(HR.case_input(cfg).cuda(), tape=tape)
    d_stage = {l: HR.functional_weight(cfg, l, o.shape).permute(0, 2, 3, 1).contiguous().cuda() for l, o in enumerate(outs)}
    eng._backward_backbone(m, tape, d_stage)
    named = list(m.named_parameters())
    grads = {k: g for (k, _), g in zip(named, eng.collect([p for _, p in named])) if g is not None}
    torch.cuda.synchronize()
    return outs, tape, grads


_FULL_GRADS = {}


def _full_grads(name):
    """Everything trains: computed once per case and shared (left unchanged) by the tests that compare against it."""
    if name not in _FULL_GRADS:
        cfg, m = _case_model(name)
        seen = {}

        def spy(eng):
            rule = eng._conv_bn_backward

            def wrapped(cache, conv, bn, *a, **kw):
                r = rule(cache, conv, bn, *a, **kw)
                if conv is m.conv2:
                    seen['g1'] = r[0].clone()
                return r
            eng._conv_bn_backward = wrapped
        outs, tape, grads = _engine_backward(m, cfg, spy)
        _FULL_GRADS[name] = (outs, tape, grads, seen['g1'])
    return _FULL_GRADS[name]


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_parameter_gradients_vs_reference(name):
    """Against the reference class's fp64 autograd: rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample; the gradient at
    conv2's image-side input, taken through conv1's ReLU by the data gradient's epilogue, against the fixture's under the recorded mask.
    The recorded forward has the forward-only bits."""
    from oracle.gen_golden import grad_sample_index
    cfg, m = _case_model(name)
    outs, tape, grads, g1 = _full_grads(name)
    with torch.no_grad():
        plain = m(HR.case_input(cfg).cuda())
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    assert sorted(grads) == sorted(k for k in HR.grad_names(name) if k != 'conv2_in')
    assert len(grads) == len(list(m.parameters()))
    failed, worst = [], 0.0
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
        en, es = HR.grad_errors(name, k, g)
        worst = max(worst, en, es)
        if not (en <= HR.BAR_GRAD and es <= HR.BAR_GRAD):
            failed.append((k, en, es))
    print('ERR backward %-18s %d tensors, worst of norm / sample rel-L2 %.2e (bar 2e-3)' % (name, len(grads), worst), flush=True)
    assert not failed, failed[:8]
    o1 = tape[0]['stem']['o1'].permute(0, 3, 1, 2).contiguous().flatten().cpu()
    idx = torch.from_numpy(grad_sample_index(o1.numel(), HR.GRAD_K))
    ref = torch.from_numpy(HR.archive()['%s:sample:conv2_in' % name]) * (o1[idx] > 0)
    got = g1.permute(0, 3, 1, 2).contiguous().flatten().cpu()[idx].double()
    e = float((got - ref).norm() / ref.norm())
    print('ERR backward %-18s conv2 input gradient (masked sample) rel-L2 %.2e (bar 2e-3)' % (name, e), flush=True)
    assert e <= HR.BAR_GRAD


def _freeze_stem(m):
    return [m.conv1, m.bn1, m.conv2, m.bn2]


def _freeze_fuse_conv(m):
    fl = m.stage3[0].fuse_layers[0][1]
    return [fl[0], fl[1]]


@pytest.mark.parametrize('group', [_freeze_stem, _freeze_fuse_conv], ids=['stem', 'fuse_conv'])
@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_a_frozen_group_gets_no_gradient_and_changes_no_other(name, group):
    cfg, m = _case_model(name)
    frozen = set()
    for mod in group(m):
        for p in mod.parameters():
            p.requires_grad = False
            frozen.add(id(p))
    names = {id(p): k for k, p in m.named_parameters()}
    _, _, grads = _engine_backward(m, cfg)
    _, _, full, _ = _full_grads(name)
    assert frozen and all(names[i] not in grads for i in frozen)
    assert sorted(grads) == sorted(k for k in full if k not in {names[i] for i in frozen})
    for k, g in grads.items():
        assert torch.equal(g.view(torch.int32), full[k].view(torch.int32)), k


# ------------------------------------------------------------------------------------------------ locators
LOCATORS = {'p2p_hrfpn': ('p2p', 'HRFPN', 3), 'cpr_hrfpn': ('cpr', 'HRFPN', 1), 'p2p_fpn': ('p2p', 'FPN', 3), 'cpr_fpn': ('cpr', 'FPN', 1)}
WIDTHS = [32, 64, 128, 256]


def build_locator(kind, seed=3, **bb_kw):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    head, neck, n = LOCATORS[kind]
    cfg = p2p_model_cfg(50, 1) if head == 'p2p' else model_cfg(50, 1)
    extra = HR.CASES['w32_tiny']['extra']
    cfg['backbone'] = dict(type='HRNet', extra=extra, **bb_kw)
    if neck == 'HRFPN':
        cfg['neck'] = dict(type='HRFPN', in_channels=WIDTHS, out_channels=256, num_outs=n)
    else:
        cfg['neck'] = dict(cfg['neck'], in_channels=WIDTHS, num_outs=n, add_extra_convs=False)
    if head == 'p2p':
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4 << k for k in range(n)])
    m = P.build_detector(cfg).cuda()
    sd = synthetic.hrnet_state_dict(extra, seed, prefix='backbone.')
    sd.update(synthetic.hrfpn_state_dict(WIDTHS, 256, n, seed + 1) if neck == 'HRFPN' else synthetic.fpn_state_dict(WIDTHS, 256, 0, n, seed + 1))
    sd.update(synthetic.p2p_head_state_dict(1, seed=seed + 3, std=0.05) if head == 'p2p' else synthetic.cpr_head_state_dict(1, seed=seed + 2, std=0.3))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def _data(seed=4, hw=(128, 160)):
    batch = synthetic.synthetic_batch(2, hw[0], hw[1], 6, 1, seed=seed)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def _trainer(kind):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return P2PTrainer if LOCATORS[kind][0] == 'p2p' else CprTrainer


def _total(losses):
    return float(sum((sum(v) if isinstance(v, (list, tuple)) else v).sum() for k, v in losses.items() if 'loss' in k))


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_bridge_is_bit_equal_to_the_trainer_and_a_step_runs(kind):
    from pointtinybenchmark_amd import autograd_bridge
    data = _data()
    ma = build_locator(kind)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr = _trainer(kind)(ma, lr=1e-3)
    tr.check_bindings()
    assert {id(p) for p in tr.params} == {id(p) for p in ma.parameters() if p.requires_grad}
    tr.flat_g.fill_(float('nan'))
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.flat_g).all()), 'a trainable parameter was left without a gradient'
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    for k in ('backbone.conv1.weight', 'backbone.bn1.bias', 'backbone.transition3.3.0.0.weight', 'backbone.stage3.1.fuse_layers.2.0.1.0.weight',
              'backbone.stage4.0.fuse_layers.0.3.1.weight', 'backbone.layer1.0.downsample.0.weight'):
        assert float(want[k].abs().max()) > 0, k
    lb = tr.forward_backward(**data)
    torch.cuda.synchronize()
    assert _total(la) == _total(lb) and np.isfinite(_total(la))      # equal run to run
    for k, p in ma.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, want[k]), k
    mb = build_locator(kind)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    assert abs(out['log_vars']['loss'] - _total(la)) <= 1e-6 * max(1.0, abs(_total(la)))
    n = 0
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
            n += 1
    assert n == len(want)
    step = tr.train_step(dict(data))      # optimizer step included; the refreshed packs serve a second forward
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in step['log_vars'].values()), step['log_vars']
    after = tr.forward_backward(**data)
    torch.cuda.synchronize()
    assert np.isfinite(_total(after)) and _total(after) != _total(la)


def test_bridge_with_a_frozen_group_is_bit_equal_to_the_trainer():
    data = _data()

    def frozen(m):
        for mod in _freeze_stem(m.backbone) + _freeze_fuse_conv(m.backbone):
            for p in mod.parameters():
                p.requires_grad = False
        return m
    ma = frozen(build_locator('p2p_hrfpn'))
    tr = _trainer('p2p_hrfpn')(ma)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    assert 'backbone.conv1.weight' not in want and 'backbone.stage3.0.fuse_layers.0.1.0.weight' not in want
    mb = frozen(build_locator('p2p_hrfpn'))
    mb.train_step(dict(data))['loss'].backward()
    torch.cuda.synchronize()
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, want[k]), k
        else:
            assert p.grad is None, k


def test_a_pair_frozen_in_part_after_the_engine_was_built_is_refused_in_the_walk():
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg, m = _case_model('n1')
    eng = BackwardEngine(m)
    eng._sink = {}
    tape = []
    outs = m(HR.case_input(cfg).cuda(), tape=tape)
    m.stage2[0].fuse_layers[1][0][0][0].weight.requires_grad = False      # the conv alone: its norm would be left without a gradient
    with pytest.raises(NotImplementedError, match=r'stage2\.0\.fuse_layers\.1\.0\.0\.0\.weight'):
        eng._backward_backbone(m, tape, {l: torch.zeros_like(o.permute(0, 2, 3, 1)).contiguous() for l, o in enumerate(outs)})


def test_the_shipped_w32_net_loads_strictly_and_takes_a_p2p_step_behind_hrfpn():
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    cfg = p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(type='HRNet', extra=HR.W32_EXTRA)
    cfg['neck'] = dict(type='HRFPN', in_channels=WIDTHS, out_channels=256, num_outs=3)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16])
    m = P.build_detector(cfg).cuda()
    sd = synthetic.hrnet_state_dict(HR.W32_EXTRA, 3, prefix='backbone.')
    sd.update(synthetic.hrfpn_state_dict(WIDTHS, 256, 3, 4))
    sd.update(synthetic.p2p_head_state_dict(1, seed=6, std=0.05))
    m.load_state_dict(sd, strict=True)
    m.train()
    tr = _trainer('p2p_hrfpn')(m, lr=1e-3)
    tr.flat_g.fill_(float('nan'))
    out = tr.train_step(_data(hw=(64, 96)))
    torch.cuda.synchronize()
    assert len(tr.params) == 951 and all(np.isfinite(v) for v in out['log_vars'].values()), out['log_vars']
    assert bool(torch.isfinite(tr.flat_g).all()) and bool(torch.isfinite(tr.flat_p).all())


def test_bf16_and_batch_statistics_raise_from_forward_trainer_and_bridge():
    from pointtinybenchmark_amd import autograd_bridge
    data = _data()
    m = build_locator('p2p_hrfpn')
    with pytest.raises(NotImplementedError, match='extra'):
        m.set_compute_dtype('bf16')
    m.backbone.compute_dtype = torch.bfloat16
    assert 'extra' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='extra'):
        m.backbone(data['img'])
    with pytest.raises(NotImplementedError, match='extra'):
        _trainer('p2p_hrfpn')(m)
    with pytest.raises(NotImplementedError, match='extra'), warnings.catch_warnings():
        warnings.simplefilter('ignore')      # (the bridge reports its reason once per process, then the forward-only path raises)
        m.train_step(dict(data))
    b = build_locator('p2p_hrfpn', norm_eval=False)
    assert b.backbone.batch_stats_active()
    with pytest.raises(NotImplementedError, match='norm_eval'):
        b.backbone(data['img'])
    with pytest.raises(NotImplementedError, match='norm_eval'):
        _trainer('p2p_hrfpn')(b).forward_backward(**data)
    with pytest.raises(NotImplementedError, match='norm_eval'):
        build_locator('p2p_hrfpn', norm_eval=False).train_step(dict(data))
