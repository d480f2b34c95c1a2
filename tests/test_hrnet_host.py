"""CPU: the HRNet backbone's interface (backbones/hrnet.py) against the reference class's key list in tests/golden/hrnet.npz, its
refusals, and the numpy references of the exchange kernels (tests/hrnet_ref.py) against torch fp64 -- with deliberately wrong variants
of those references, each refuted by a named case."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic
from tests import hrnet_ref as HR


def _build(extra=None, **kw):
    import pointtinybenchmark_amd as P
    return P.build_backbone(dict(type='HRNet', extra=HR.W32_EXTRA if extra is None else extra, **kw))


def _with(stage, **kw):
    extra = {k: dict(v) for k, v in HR.W32_EXTRA.items()}
    extra[stage].update(kw)
    return extra


# ------------------------------------------------------------------------------------------------ construction, keys, modes
def test_registered_and_exported():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.backbones import HRNet
    assert P.BACKBONES.get('HRNet') is HRNet
    m = _build()
    assert m.out_channels == [32, 64, 128, 256] and m.norm_eval is True and m.hrnet
    assert len(m.stage2) == 1 and len(m.stage3) == 4 and len(m.stage4) == 3
    assert [len(b) for b in m.stage4[0].branches] == [4, 4, 4, 4]


def test_constructor_keys_are_the_references():
    import inspect
    from pointtinybenchmark_amd.backbones import HRNet
    sig = inspect.signature(HRNet.__init__)
    assert list(sig.parameters)[1:] == ['extra', 'in_channels', 'conv_cfg', 'norm_cfg', 'norm_eval', 'with_cp', 'zero_init_residual',
                                        'pretrained', 'init_cfg']
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d['in_channels'], d['conv_cfg'], d['norm_cfg'], d['norm_eval'], d['with_cp'], d['zero_init_residual'], d['pretrained'],
            d['init_cfg']) == (3, None, dict(type='BN'), True, False, False, None, None)


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_state_dict_keys_order_and_shapes_equal_the_references(name):
    cfg = HR.CASES[name]
    m = _build(cfg['extra'])
    want = HR.archive_keys(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want
    sd = HR.case_state_dict(cfg)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want      # synthetic.hrnet_layout walks the same layout on its own
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.stage4[0].fuse_layers[3][0][2][0].weight, sd['stage4.0.fuse_layers.3.0.2.0.weight'])
    # None entries leave gaps, as in the reference
    assert m.stage4[0].fuse_layers[1][1] is None and not any(k.startswith('stage4.0.fuse_layers.1.1.') for k, _ in got)
    assert any(k.startswith('stage4.0.fuse_layers.1.0.0.0.') for k, _ in got) and any(k.startswith('stage4.0.fuse_layers.1.2.0.') for k, _ in got)


def test_w32_layout_of_the_shipped_config():
    m = _build()
    lay = synthetic.hrnet_layout(HR.W32_EXTRA)
    keys = [k for k, _ in m.state_dict().items()]
    assert keys[:7] == ['conv1.weight', 'bn1.weight', 'bn1.bias', 'bn1.running_mean', 'bn1.running_var', 'bn1.num_batches_tracked', 'conv2.weight']
    assert len(keys) == 6 * len(lay) and keys[0] == 'conv1.weight' and keys[1] == 'bn1.weight'
    for key, shape, norm in lay:
        assert tuple(m.state_dict()[key].shape) == shape and tuple(m.state_dict()[norm + '.running_var'].shape) == (shape[0],)
    assert 'transition1.0.0.weight' in keys and 'transition1.1.0.0.weight' in keys and 'transition3.3.0.0.weight' in keys
    assert not any(k.startswith('transition2.0') or k.startswith('transition2.1') for k in keys)
    m.load_state_dict(synthetic.hrnet_state_dict(HR.W32_EXTRA, 5), strict=True)      # a reference-layout state dict of the shipped W32 net
    assert float(m.stage4[2].fuse_layers[3][0][2][1].running_var.min()) >= 0.5


def test_train_modes_follow_norm_eval():
    m = _build(HR.CASES['n1']['extra'])
    bns = [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
    assert m.train() is m and m.training and not any(b.training for b in bns) and not m.batch_stats_active()
    m.eval()
    assert not m.training and not any(b.training for b in bns)
    m2 = _build(HR.CASES['n1']['extra'], norm_eval=False)
    m2.train()
    assert all(b.training for b in m2.modules() if isinstance(b, nn.BatchNorm2d)) and m2.batch_stats_active()
    m2.eval()
    assert not m2.batch_stats_active()
    sync = _build(HR.CASES['n1']['extra'], norm_cfg=dict(type='SyncBN'))
    assert isinstance(sync.bn1, nn.SyncBatchNorm) and list(sync.state_dict()) == list(m.state_dict())


def test_init_weights_and_zero_init_residual():
    from pointtinybenchmark_amd.backbones.resnet import _Block
    m = _build(HR.CASES['n1']['extra'])
    assert all(float(b.weight.min()) == 1.0 == float(b.weight.max()) and float(b.bias.abs().max()) == 0.0
               for b in m.modules() if isinstance(b, nn.BatchNorm2d))
    w = m.stage3[0].branches[1][0].conv1.weight
    assert abs(float(w.std()) - (2.0 / (w.shape[0] * 9)) ** 0.5) < 0.1 * (2.0 / (w.shape[0] * 9)) ** 0.5      # Kaiming, fan_out
    z = _build(HR.CASES['n1']['extra'], zero_init_residual=True)
    blocks = [b for b in z.modules() if isinstance(b, _Block)]
    assert blocks and all(float((b.bn3 if b.kind == 'bottleneck' else b.bn2).weight.abs().max()) == 0.0 for b in blocks)
    assert float(z.bn1.weight.min()) == 1.0 and float(z.stage2[0].fuse_layers[0][1][1].weight.min()) == 1.0


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('kw, key', [
    (dict(extra=_with('stage2', num_channels=(18, 36))), r"extra\['stage2'\]\['num_channels'\]"),                      # W18
    (dict(extra=_with('stage4', num_channels=(40, 80, 160, 320))), r"extra\['stage4'\]\['num_channels'\].*W32"),      # W40
    (dict(extra=_with('stage3', num_channels=(48, 96, 192))), r"extra\['stage3'\]\['num_channels'\]"),                # W48
    (dict(extra=_with('stage4', num_branches=5, num_blocks=(1,) * 5, num_channels=(32, 64, 128, 256, 512))), 'num_branches'),
    (dict(with_cp=True), 'with_cp'),
    (dict(conv_cfg=dict(type='DCN')), 'conv_cfg'),
    (dict(norm_cfg=dict(type='GN', num_groups=32)), 'norm_cfg'),
    (dict(extra=HR.WIDEN_BRANCH0['extra']), r"extra\['stage3'\]\['num_channels'\].*other than the last"),
    (dict(in_channels=1), 'in_channels'),
    (dict(in_channels=4), 'in_channels'),
])
def test_refusals_name_their_key(kw, key):
    with pytest.raises(NotImplementedError, match=key):
        _build(**kw)


def test_only_the_last_existing_branch_may_widen_as_in_the_reference():
    """The fixture tool recorded the reference's own error on hrnet_ref.WIDEN_BRANCH0 (transition2[0] is fed the last branch); widening
    the last branch is what the reference runs, and the 'widen' case holds it: transition2[1] and transition3[2] are same-resolution
    3x3 convs on an existing branch."""
    msg = str(HR.archive()['raises:widen_branch0'])
    assert 'weight of size [64, 32, 3, 3]' in msg and '64 channels' in msg
    m = _build(HR.CASES['widen']['extra'])
    assert m.transition2[0] is None and tuple(m.transition2[1][0].weight.shape) == (128, 64, 3, 3) and m.transition2[1][0].stride == (1, 1)
    assert m.transition3[1] is None and tuple(m.transition3[2][0].weight.shape) == (256, 128, 3, 3) and m.transition3[2][0].stride == (1, 1)
    assert tuple(m.transition3[3][0][0].weight.shape) == (256, 128, 3, 3) and m.transition3[3][0][0].stride == (2, 2)
    assert m.out_channels == [32, 128, 256, 256]


def test_archive_stays_below_the_committed_file_limit():
    import os
    assert os.path.getsize(HR.GOLDEN) < 1 << 20
    a = HR.archive()
    for name in HR.CASE_NAMES:
        worst_out, worst_grad = a[name + ':fp32:worst']
        assert worst_out <= HR.BAR_OUT / 4 and worst_grad <= HR.BAR_GRAD / 4      # the admission rule the tool applied


def test_partly_frozen_conv_bn_pairs_are_refused_naming_the_pair():
    """A conv and its BatchNorm get their gradients from one pass: conv-only and gamma-only freezes are refused by name -- by the backbone's
    own query, by the trainers' constructor and by the bridge -- while a whole pair, or a frozen norm under a trainable conv, is served."""
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import BackwardEngine, P2PBackwardEngine
    cfg = p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(type='HRNet', extra=HR.CASES['n1']['extra'])
    cfg['neck'] = dict(type='HRFPN', in_channels=[32, 64, 128, 256], out_channels=256, num_outs=1)
    m = P.build_detector(cfg)
    bb = m.backbone
    fl = bb.stage3[0].fuse_layers[0][1]
    assert bb.freeze_reason() is None and autograd_bridge.unsupported_reason(m) is None
    for p, key in ((fl[0].weight, r'stage3\.0\.fuse_layers\.0\.1\.0\.weight.*False, True, True'), (fl[1].weight, r'fuse_layers\.0\.1\.1\.weight.*True, False, True'),
                   (bb.bn1.bias, r'conv1\.weight, bn1\.weight and bn1\.bias.*True, True, False')):
        p.requires_grad = False
        import re
        assert re.search(key, bb.freeze_reason()), bb.freeze_reason()
        assert autograd_bridge.unsupported_reason(m) == bb.freeze_reason()
        for eng in (BackwardEngine, P2PBackwardEngine):
            with pytest.raises(NotImplementedError, match=key):
                eng(m, two_streams=False)
        p.requires_grad = True
    for p in list(fl[0].parameters()) + list(fl[1].parameters()):      # the whole pair
        p.requires_grad = False
    assert bb.freeze_reason() is None
    for b in bb.modules():      # norm_cfg requires_grad=False: every norm frozen under trainable convs
        if isinstance(b, nn.BatchNorm2d):
            b.weight.requires_grad = b.bias.requires_grad = False
    assert bb.freeze_reason() is None and autograd_bridge.unsupported_reason(m) is None
    assert _build(HR.CASES['n1']['extra'], norm_cfg=dict(type='BN', requires_grad=False)).freeze_reason() is None


def test_relu_of_the_references_propagates_nan_as_torch_does():
    t = np.array([np.nan, -1.0, 2.0, -0.0], dtype=np.float32).reshape(1, 1, 1, 4)
    got = HR.fuse_ref([(t, 0), (np.zeros_like(t), 0)]).reshape(-1)
    want = torch.relu(torch.from_numpy(t) + 0).numpy().reshape(-1)
    assert np.isnan(got[0]) and np.isnan(want[0]) and np.array_equal(got[1:], want[1:]) and not np.signbit(got[3])
    x = torch.tensor([float('nan'), 0.0, 3.0], requires_grad=True)
    torch.relu(x).backward(torch.ones(3))
    g = HR.fuse_bwd_ref(np.ones((1, 1, 1, 3), np.float32), torch.relu(x).detach().numpy().reshape(1, 1, 1, 3), 0)[0].reshape(-1)
    assert np.array_equal(g, x.grad.numpy())


def test_batch_statistics_and_bf16_are_refused_in_the_run_path():
    m = _build(HR.CASES['n1']['extra'], norm_eval=False)
    m.train()
    x = torch.zeros((1, 3, 64, 64))
    for entry in (m, m.run, m.run_stem):
        with pytest.raises(NotImplementedError, match='norm_eval'):
            entry(x)
    m.eval()
    m.compute_dtype = torch.bfloat16
    for entry in (m, m.run, m.run_stem):
        with pytest.raises(NotImplementedError, match='extra'):
            entry(x)
    assert 'fp32 compute mode only' in m.fp32_only


def test_locator_refuses_the_bf16_mode_naming_extra():
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    cfg = p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(type='HRNet', extra=HR.CASES['n1']['extra'])
    cfg['neck'] = dict(type='HRFPN', in_channels=[32, 64, 128, 256], out_channels=256, num_outs=1)
    m = P.build_detector(cfg)
    with pytest.raises(NotImplementedError, match='extra'):
        m.set_compute_dtype('bf16')


def test_input_sizes_are_checked_up_front():
    from pointtinybenchmark_amd.backbones.hrnet import branch_sizes
    m = _build(HR.CASES['n1']['extra'])
    m.eval()
    assert branch_sizes(64, 96, 4) == [(16, 24), (8, 12), (4, 6), (2, 3)]
    for H, W in ((32, 32), (64, 96), (640, 640), (96, 32)):
        m.check_size(H, W)
    with pytest.raises(ValueError, match=r'72 x 64.*branch 0.*branch 2'):
        m.check_size(72, 64)      # 18, 9, 5: 5 * 4 != 18
    with pytest.raises(ValueError, match='72 x 64'):
        m(torch.zeros((1, 3, 72, 64)))
    # what the reference does there: its exchange adds maps of different sizes
    x = torch.zeros((1, 8, 18, 16))
    with pytest.raises(RuntimeError):
        x + F.interpolate(torch.zeros((1, 8, 5, 4)), scale_factor=4, mode='nearest')


# ------------------------------------------------------------------------------------------------ the numpy references
def _terms(rng, shape, ks):
    N, H, W, C = shape
    return [(rng.standard_normal((N, H >> k, W >> k, C)).astype(np.float32), k) for k in ks]


@pytest.mark.parametrize('shape, ks', [((2, 16, 24, 8), (0, 1, 2, 3)), ((1, 8, 8, 4), (0, 0, 1, 2)), ((2, 4, 6, 8), (0, 1)),
                                        ((1, 2, 3, 4), (0, 0))])
def test_fuse_ref_against_torch_fp64(shape, ks):
    """F.interpolate(mode='nearest') is the [y >> k, x >> k] rule; the fp32 left-to-right sum stays within (T - 1) ulps of fp64."""
    rng = np.random.default_rng(7)
    terms = _terms(rng, shape, ks)
    got = HR.fuse_ref(terms)
    acc = 0
    for m, k in terms:
        t = torch.from_numpy(m).double().permute(0, 3, 1, 2)
        acc = acc + (F.interpolate(t, scale_factor=2 ** k, mode='nearest') if k else t)
    want = torch.relu(acc).permute(0, 2, 3, 1).numpy()
    mag = sum(np.abs(HR.upsample_nearest(m, k)).astype(np.float64) for m, k in terms)
    assert got.dtype == np.float32 and got.shape == shape
    assert np.all(np.abs(got - want) <= (len(terms) - 1) * HR.U * mag * (1 + 1e-6))
    assert np.array_equal(got == 0, want <= 0) or np.all(np.abs(want[(got == 0) != (want <= 0)]) <= len(terms) * HR.U * mag[(got == 0) != (want <= 0)])


def test_fuse_ref_term_order_changes_bits():
    """Case 'order': fp32 addition is not associative -- summing the terms in another order gives other bits on some elements, which
    is why the kernel's order is pinned to the reference's (source branch ascending)."""
    rng = np.random.default_rng(11)
    terms = _terms(rng, (2, 16, 24, 8), (0, 1, 2, 3))
    right, wrong = HR.fuse_ref(terms), HR.fuse_ref(terms, order=(3, 2, 1, 0))
    assert not np.array_equal(right, wrong) and np.allclose(right, wrong, atol=1e-5)
    assert np.array_equal(HR.fuse_ref(terms, order=(0, 1, 2, 3)), right)


@pytest.mark.parametrize('K', [0, 1, 2, 3])
def test_fuse_bwd_ref_against_torch_autograd_fp64(K):
    """The adjoint of ReLU(x + sum_k up_k(t_k)) wrt x is g, wrt t_k the 2^k x 2^k block SUM of g."""
    rng = np.random.default_rng(3 + K)
    N, H, W, C = 2, 8, 16, 4
    x = torch.from_numpy(rng.standard_normal((N, C, H, W))).requires_grad_(True)
    ts = [torch.from_numpy(rng.standard_normal((N, C, H >> k, W >> k))).requires_grad_(True) for k in range(1, K + 1)]
    y = x
    for k, t in enumerate(ts, 1):
        y = y + F.interpolate(t, scale_factor=2 ** k, mode='nearest')
    y = torch.relu(y)
    dy = rng.standard_normal((N, H, W, C)).astype(np.float32)
    y.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    y_nhwc = y.detach().permute(0, 2, 3, 1).numpy().astype(np.float32)
    y_nhwc[(y.detach().permute(0, 2, 3, 1).numpy() > 0) & (y_nhwc == 0)] = np.float32(1e-30)      # (a positive value that rounded to 0)
    g64, pools64, cs64 = HR.fuse_bwd_ref64(dy, y_nhwc, K)
    assert np.array_equal(g64, x.grad.permute(0, 2, 3, 1).numpy())
    for p, t in zip(pools64, ts):
        assert np.allclose(p, t.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-13, atol=1e-13)
    g32, pools32, cs32 = HR.fuse_bwd_ref(dy, y_nhwc, K)
    assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g64)
    for k, (p32, p64, mag) in enumerate(zip(pools32, pools64, HR.pool_abs_sums(g64, K)), 1):
        assert np.all(np.abs(p32 - p64) <= (4 ** k - 1) * HR.U * mag)
    assert np.allclose(cs32, cs64, rtol=1e-4, atol=1e-4) and np.allclose(cs64, g64.reshape(-1, C).sum(0))
    if K:      # the column sums of a pooled map are those of g
        assert np.allclose(pools64[-1].reshape(-1, C).sum(0), cs64, rtol=1e-12, atol=1e-12)


def test_wrong_pool_variant_average_is_refuted():
    """Case 'average': an average over the block is the adjoint of nothing here -- it is 4^-k of torch's gradient."""
    rng = np.random.default_rng(5)
    dy = rng.standard_normal((1, 4, 4, 4)).astype(np.float32)
    y = np.ones_like(dy)
    t = torch.zeros((1, 4, 2, 2), dtype=torch.float64, requires_grad=True)
    (F.interpolate(t, scale_factor=2, mode='nearest') * torch.from_numpy(dy).double().permute(0, 3, 1, 2)).sum().backward()
    want = t.grad.permute(0, 2, 3, 1).numpy()
    assert np.allclose(HR.fuse_bwd_ref64(dy, y, 1)[1][0], want)
    wrong = HR.fuse_bwd_ref(dy, y, 1, dtype=np.float64, average=True)[1][0]
    assert not np.allclose(wrong, want) and np.allclose(wrong * 4, want)


def test_wrong_mask_variant_ge_is_refuted():
    """Case 'ge_mask': ReLU's gradient at an output of exactly 0 is 0 (torch's threshold_backward: grad where y > 0) -- a ``>=`` mask
    lets the gradient through at every clamped element."""
    x = torch.tensor([[-1.0, 0.0, 2.0, -0.0]], dtype=torch.float64, requires_grad=True)
    y = torch.relu(x)
    y.backward(torch.ones_like(y))
    dy = np.ones((1, 1, 1, 4), dtype=np.float32)
    y4 = y.detach().numpy().astype(np.float32).reshape(1, 1, 1, 4)
    assert np.array_equal(HR.fuse_bwd_ref(dy, y4, 0)[0].reshape(-1), x.grad.numpy().reshape(-1))
    assert not np.array_equal(HR.fuse_bwd_ref(dy, y4, 0, ge_mask=True)[0].reshape(-1), x.grad.numpy().reshape(-1))


def test_masked_elements_are_positive_zero_and_negative_zero_passes():
    dy = np.array([-0.0, -0.0, 3.0, -2.0], dtype=np.float32).reshape(1, 1, 1, 4)
    y = np.array([1.0, 0.0, 0.0, 5.0], dtype=np.float32).reshape(1, 1, 1, 4)
    g = HR.fuse_bwd_ref(dy, y, 0)[0].reshape(-1)
    assert np.signbit(g[0]) and not np.signbit(g[1]) and g[2] == 0 and not np.signbit(g[2]) and g[3] == -2.0


def test_pool_order_is_hierarchical_not_flat():
    """Case 'flat order': summing the 4x4 block row by row gives other bits than 2x2 blocks of 2x2 blocks on some elements; the
    reference follows the kernel's documented order."""
    rng = np.random.default_rng(13)
    g = (rng.standard_normal((4, 32, 32, 8)) * 10.0 ** rng.integers(-3, 4, (4, 32, 32, 8))).astype(np.float32)
    hier = HR.fuse_bwd_ref(g, np.ones_like(g), 2)[1][1]
    flat = np.zeros_like(hier)
    for yy in range(4):
        for xx in range(4):
            flat = (flat + g[:, yy::4, xx::4]).astype(np.float32)
    assert not np.array_equal(hier, flat) and np.allclose(hier, flat, rtol=1e-4, atol=1e-4)


def test_ops_and_library_entries_exist():
    from pointtinybenchmark_amd import _lib, build, ops
    assert 'hrnet.hip' in build.SOURCES
    assert {'cpr_hrnet_fuse', 'cpr_hrnet_fuse_bwd', 'cpr_hrnet_fuse_bwd_blocks'} <= set(_lib.SIGNATURES)
    assert callable(ops.hrnet_fuse) and callable(ops.hrnet_fuse_bwd) and ops.HRNET_MAX_TERMS == 4 and ops.HRNET_MAX_K == 3
    build.build(verbose=False)
    lib = _lib.load()
    # the argument checks answer without a device: the partial count query, an indivisible size, K beyond 3
    assert lib.cpr_hrnet_fuse_bwd_blocks(2, 16, 24, 32, 3) == 2 and lib.cpr_hrnet_fuse_bwd_blocks(2, 16, 24, 32, 0) == 2 * 1
    assert lib.cpr_hrnet_fuse_bwd_blocks(1, 12, 24, 32, 3) == -1001 and lib.cpr_hrnet_fuse_bwd_blocks(1, 16, 16, 32, 4) == -1001


def test_backward_order_lists_every_parameter_once():
    """CprTrainer._backward_order's HRNet branch names every backbone parameter exactly once (host: no device needed)."""
    from types import SimpleNamespace
    from pointtinybenchmark_amd.training import CprTrainer
    bb = _build(HR.CASES['w32_tiny']['extra'])
    neck = SimpleNamespace(lateral_convs=[], fpn_convs=[], num_outs=0)
    tr = SimpleNamespace(model=SimpleNamespace(bbox_head=None, neck=neck, backbone=bb), _head_units=lambda head: [],
                         _neck_units=CprTrainer._neck_units, _backbone_units=CprTrainer._backbone_units)
    order = CprTrainer._backward_order(tr)
    assert len(order) == len(list(bb.parameters())) and {id(p) for p in order} == {id(p) for p in bb.parameters()}
    names = {id(p): k for k, p in bb.named_parameters()}
    assert names[id(order[0])].startswith('stage4.0.fuse_layers.1.0.') and names[id(order[-1])] == 'bn1.bias'
    bb.conv1.weight.requires_grad = False
    assert len(CprTrainer._backward_order(tr)) == len(order) - 1
