"""CPU: the ResNeSt backbone -- what runs without a GPU.

  registry   build_backbone(dict(type='ResNeSt', ...)); a shipped CPR and a shipped P2P config build with the backbone dict switched
  layout     state-dict keys, their order and shapes equal the reference class's (recorded per depth and per case in
             tests/golden/resnest.npz by tools/gen_resnest.py) and load strictly; named_parameters order; no bn2, no avd parameters;
             style='caffe' puts the stride on conv1 and no block pools
  refusals   radix, groups, avg_down_stride, dilations, the bf16 compute mode (``radix``) -- in set_compute_dtype, the backbone,
             autograd_bridge.unsupported_reason and the trainers' constructors -- batch statistics (``norm_eval``), and ResNet's own
  fixture    the conditioning entries are within a quarter of the bars; the fp64 restatement (tests/resnest_ref.py) matches the fixture's
             stage outputs at 1e-9; the synthetic generators' other draws are unchanged
  dense      the block-diagonal dense weight equals F.conv2d(groups=2) in fp64 and its off-diagonal blocks are bit-zero
  kernels    the inputs of tests/test_gpu_splat.py: the fp32 torch restatement alone stays within a quarter of its 1e-5 bar
  walk       the trainers' flat order, and the backward rule's launch order with torch stand-ins"""
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import resnest_ref as RS
from tests import splat_ref as SR

CPR_CFG = 'configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_1x_TinyPersonV2_640.py'
P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'


def _build(**kw):
    import pointtinybenchmark_amd as P
    return P.build_backbone(dict(kw))


def test_registry_builds_resnest():
    from pointtinybenchmark_amd import backbones
    from pointtinybenchmark_amd.backbones.resnest import ResNeSt, inter_channels
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    from pointtinybenchmark_amd.registry import BACKBONES
    assert BACKBONES.get('ResNeSt') is ResNeSt and backbones.ResNeSt is ResNeSt and issubclass(ResNeSt, ResNet)
    m = _build(type='ResNeSt', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
               norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch')
    assert type(m) is ResNeSt and m.radix == 2 and m.reduction_factor == 4 and m.feat_dim == 2048
    assert m.deep_stem and m.avg_down and m.style == 'pytorch'
    for i, name in enumerate(m.res_layers):
        w = 64 * 2 ** i
        for bi, blk in enumerate(getattr(m, name)):
            sa = blk.conv2
            assert blk.kind == 'resnest' and not hasattr(blk, 'bn2') and blk.width == w
            assert blk.pool == (bi == 0 and i > 0) and (blk.downsample is not None) == (bi == 0)
            assert blk.conv1.stride == (1, 1)
            assert tuple(sa.conv.weight.shape) == (2 * w, w // 2, 3, 3) and sa.conv.stride == (1, 1) and sa.conv.groups == 2
            inter = inter_channels(w)
            assert inter == max(w // 2, 32)
            assert tuple(sa.fc1.weight.shape) == (inter, w, 1, 1) and tuple(sa.fc1.bias.shape) == (inter,)
            assert tuple(sa.fc2.weight.shape) == (2 * w, inter, 1, 1) and tuple(sa.fc2.bias.shape) == (2 * w,)
            assert sa.bn0.num_features == 2 * w and sa.bn1.num_features == inter
    assert not any('avd' in k for k in m.state_dict())


@pytest.mark.parametrize('depth', RS.DEPTHS)
def test_state_dict_layout_is_the_reference_classes(depth):
    from pointtinybenchmark_amd import synthetic
    m = _build(type='ResNeSt', depth=depth)
    want = RS.depth_keys(depth)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]          # keys, their order, shapes
    sd = synthetic.resnest_state_dict(depth, 3, prefix='')
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want                     # the synthetic generator keeps that order too
    m.load_state_dict(sd, strict=True)
    assert not any('.bn2.' in k or k.endswith('conv2.weight') for k in sd) and 'stem.0.weight' in sd
    assert [len(getattr(m, n)) for n in m.res_layers] == list(RS.BLOCKS[depth])


@pytest.mark.parametrize('name', RS.CASE_NAMES)
def test_fixture_case_has_the_reference_state_dict_layout(name):
    cfg = RS.CASES[name]
    m = _build(type='ResNeSt', **RS.resnest_kwargs(cfg))
    want = RS.keys(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]
    sd = RS.case_state_dict(cfg)
    assert list(sd) == [k for k, _ in want]
    m.load_state_dict(sd, strict=True)
    m.train()
    assert [n for n, p in m.named_parameters() if p.requires_grad] == RS.grad_names(name)
    assert not any(mod.training for mod in m.modules() if isinstance(mod, nn.BatchNorm2d))


def test_case_names_are_the_fixtures_and_the_cases_are_admitted():
    f = RS.fixture()
    assert json.loads(str(f['cases'])) == json.loads(json.dumps(RS.CASES))
    for name in RS.CASE_NAMES:      # admission: the reference alone in fp32, and its fp64 gradients under a one-ulp perturbation
        assert float(f[name + ':fp32:out'].max()) <= RS.BAR_OUT / 4 and float(f[name + ':fp32:grad'].max()) <= RS.BAR_GRAD / 4
        assert float(f[name + ':perturbed:grad'].max()) <= RS.BAR_GRAD / 4
    assert os.path.getsize(RS.GOLDEN) < (1 << 20)


def test_options_style_out_indices_zero_init_and_frozen_stages():
    caffe = _build(type='ResNeSt', depth=50, style='caffe')
    assert caffe.layer2[0].conv1.stride == (2, 2) and not any(blk.pool for n in caffe.res_layers for blk in getattr(caffe, n))
    assert [k for k in caffe.state_dict()] == [k for k in _build(type='ResNeSt', depth=50).state_dict()]
    caffe_no_avd = _build(type='ResNeSt', depth=50, style='caffe', avg_down_stride=False)     # the stride is on conv1 either way
    assert caffe_no_avd.layer3[0].conv1.stride == (2, 2)
    assert _build(type='ResNeSt', depth=50, out_indices=(1, 3)).out_indices == (1, 3)
    z = _build(type='ResNeSt', depth=50, zero_init_residual=True)
    assert float(z.layer3[2].bn3.weight.detach().abs().max()) == 0 and float(z.layer3[2].conv2.bn1.weight.detach().min()) == 1
    nz = _build(type='ResNeSt', depth=50, zero_init_residual=False)
    assert float(nz.layer3[2].bn3.weight.detach().min()) == 1
    for fs in range(5):
        m = _build(type='ResNeSt', depth=50, frozen_stages=fs).train()
        assert not any(p.requires_grad for p in m.stem.parameters())
        for i, n in enumerate(m.res_layers):
            assert all(p.requires_grad == (i + 1 > fs) for p in getattr(m, n).parameters()), (fs, n)
    for norm in ('BN', 'SyncBN'):
        m = _build(type='ResNeSt', depth=50, norm_cfg=dict(type=norm, requires_grad=True), norm_eval=True).train()
        cls = nn.SyncBatchNorm if norm == 'SyncBN' else nn.BatchNorm2d
        assert isinstance(m.layer1[0].conv2.bn0, cls) and isinstance(m.layer1[0].conv2.bn1, cls)
        assert not any(mod.training for mod in m.modules() if isinstance(mod, nn.modules.batchnorm._BatchNorm))


def test_refusals_name_the_option():
    from pointtinybenchmark_amd.backbones import resnest
    for kw, key in ((dict(radix=1), 'radix'), (dict(radix=4), 'radix'), (dict(groups=2), 'groups'), (dict(groups=32), 'groups'),
                    (dict(avg_down_stride=False), 'avg_down_stride'), (dict(dilations=(1, 1, 1, 2), strides=(1, 2, 2, 1)), 'dilations'),
                    (dict(dilations=(1, 1, 2, 4)), 'dilations')):
        with pytest.raises(NotImplementedError, match=key):
            _build(type='ResNeSt', depth=50, **kw)
    assert resnest.unsupported_reason() is None and 'radix' in resnest.unsupported_reason(radix=3)
    for depth in (18, 34):
        with pytest.raises(KeyError, match='invalid depth %d' % depth):
            _build(type='ResNeSt', depth=depth)
    # what ResNet refuses stays refused
    for bad in (dict(dcn=dict(type='DCN')), dict(plugins=[dict()]), dict(with_cp=True)):
        with pytest.raises(AssertionError):
            _build(type='ResNeSt', depth=50, **bad)
    for sc in (32, 128):          # (the published S-101 config's stem_channels=128)
        with pytest.raises(NotImplementedError, match='stem_channels'):
            _build(type='ResNeSt', depth=101, stem_channels=sc)
    assert _build(type='ResNeSt', depth=101, stem_channels=64).depth == 101
    m = _build(type='ResNeSt', depth=50, frozen_stages=-1)
    assert 'deep_stem' in m.stem_train_reason()


def test_batch_statistics_are_refused_naming_norm_eval():
    m = _build(type='ResNeSt', depth=50, norm_eval=False, frozen_stages=1)
    m.train()
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m.layer2[0].run(None, torch.zeros(1, 8, 8, 256))
    m.eval()              # eval mode: running statistics everywhere, nothing to refuse
    m._check_mode()
    frozen = _build(type='ResNeSt', depth=50, norm_eval=False, frozen_stages=4)
    frozen.train()
    assert not any(blk.batch_stats() for n in frozen.res_layers for blk in getattr(frozen, n))


def _locator(head, **bb):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(cfg['backbone'], type='ResNeSt', **bb)
    return P.build_detector(cfg)


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_bf16_mode_is_refused_with_the_reason(head):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    m = _locator(head, frozen_stages=4)
    assert autograd_bridge.unsupported_reason(m) is None
    with pytest.raises(NotImplementedError, match='radix=2'):
        m.set_compute_dtype('bf16')
    assert m.backbone.compute_dtype == torch.float32 and m.set_compute_dtype('fp32') is m
    # a mode set behind the detector's back: the bridge reports it, the trainers' constructors and the backbone refuse it
    m.backbone.compute_dtype = torch.bfloat16
    assert 'radix=2' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='radix=2'):
        (CprTrainer if head == 'cpr' else P2PTrainer)(m, two_streams=False)
    with pytest.raises(NotImplementedError, match='radix=2'):
        m.backbone(torch.zeros(1, 3, 32, 32))


def _shipped(golden_dir, rel):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[rel])))
    assert cfg.model.backbone.type == 'ResNet' and list(cfg.model.neck.in_channels) == [256, 512, 1024, 2048]
    cfg.merge_from_dict({'model.backbone.type': 'ResNeSt'})
    return P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


@pytest.mark.parametrize('rel', [CPR_CFG, P2P_CFG], ids=['cpr', 'p2p'])
def test_shipped_configs_build_with_the_backbone_dict_switched(golden_dir, rel):
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.backbones.resnest import ResNeSt
    m = _shipped(golden_dir, rel)
    assert type(m.backbone) is ResNeSt and m.backbone.depth == 50 and m.backbone.frozen_stages == 1
    assert tuple(m.backbone.layer1[0].conv2.conv.weight.shape) == (128, 32, 3, 3)
    assert tuple(m.backbone.layer4[2].conv2.fc2.weight.shape) == (1024, 256, 1, 1)
    want = synthetic.resnest_state_dict(50, 0)
    got = {k: v for k, v in m.state_dict().items() if k.startswith('backbone.')}
    assert [(k, tuple(v.shape)) for k, v in got.items()] == [(k, tuple(v.shape)) for k, v in want.items()]


@pytest.mark.parametrize('name', ['s50', 's50_odd', 's50_caffe', 's50_rf2'])
def test_fp64_restatement_matches_the_fixture(name):
    """The semantics restated in plain torch (tests/resnest_ref.restated_forward), in fp64 on the case's weights and image, against the
    reference class's fp64 outputs."""
    cfg = RS.CASES[name]
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    with torch.no_grad():
        outs = RS.restated_forward(RS.case_state_dict(cfg, torch.float64), cfg, RS.case_input(cfg, torch.float64))
    assert len(outs) == 4
    for l, o in enumerate(outs):
        assert RS.output_error(name, l, o) <= 1e-9


def test_synthetic_defaults_draw_what_they_drew():
    from pointtinybenchmark_amd import synthetic
    before = synthetic.resnet_state_dict(50, 3)
    synthetic.resnest_state_dict(50, 3)
    after = synthetic.resnet_state_dict(50, 3)
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    a, b = synthetic.resnest_state_dict(50, 5, prefix=''), synthetic.resnest_state_dict(50, 5, prefix='')
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert tuple(a['layer3.0.conv2.conv.weight'].shape) == (512, 128, 3, 3) and tuple(a['layer3.0.conv2.fc1.weight'].shape) == (128, 256, 1, 1)
    rf2 = synthetic.resnest_state_dict(50, 5, reduction_factor=2, prefix='')
    assert tuple(rf2['layer3.0.conv2.fc1.weight'].shape) == (256, 256, 1, 1)


@pytest.mark.parametrize('w', [64, 96])
def test_dense_block_diagonal_weight_equals_the_grouped_conv(w):
    from pointtinybenchmark_amd import ops
    g = torch.Generator().manual_seed(w)
    weight = torch.randn((2 * w, w // 2, 3, 3), generator=g)
    dense = ops.splat_dense_weight(weight)
    assert tuple(dense.shape) == (2 * w, w, 3, 3) and dense.dtype == torch.float32
    assert int(torch.count_nonzero(dense[:w, w // 2:])) == 0 and int(torch.count_nonzero(dense[w:, :w // 2])) == 0
    assert not bool(torch.signbit(dense[:w, w // 2:]).any()) and not bool(torch.signbit(dense[w:, :w // 2]).any())      # +0 bits
    assert torch.equal(dense[:w, :w // 2], weight[:w]) and torch.equal(dense[w:, w // 2:], weight[w:])
    x = torch.randn((2, w, 7, 9), generator=g, dtype=torch.float64)
    a = F.conv2d(x, dense.double(), None, 1, 1)
    b = F.conv2d(x, weight.double(), None, 1, 1, groups=2)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize('shape', SR.SHAPES, ids=SR.IDS)
def test_kernel_test_inputs_are_well_conditioned_in_fp32(shape):
    """Admission of tests/test_gpu_splat.py's inputs: the restatement in fp32 torch against itself in fp64 stays within a quarter of
    the kernels' bar on every output the kernels are held to."""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    d = SR.inputs(shape)
    worst = 0.0
    att_in = torch.softmax(torch.randn(d['datt'].shape, generator=torch.Generator().manual_seed(3)).double(), 1)
    for pool in (False, True):
        f64, f32 = SR.forward(d, torch.float64, pool), SR.forward(d, torch.float32, pool)
        errs = [SR.rel_l2(f32[k], f64[k]) for k in ('g', 'att', 'z', 'out')]
        b64, b32 = SR.map_backward(d, att_in, torch.float64, pool), SR.map_backward(d, att_in, torch.float32, pool)
        errs += [SR.rel_l2(a, b) for a, b in zip(b32, b64)]
        worst = max([worst] + errs)
    _, z64 = SR.attention_from(d, torch.float64)
    a64, a32 = SR.attn_backward(d, z64, torch.float64), SR.attn_backward(d, z64, torch.float32)
    worst = max([worst] + [SR.rel_l2(a32[k], a64[k]) for k in a64])
    print('fp32 restatement vs fp64 %s: worst rel-L2 %.2e (admit %.1e)' % (shape, worst, SR.BAR / 4))
    assert worst <= SR.BAR / 4


@pytest.mark.parametrize('frozen', [1, 4])
@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_trainers_build_and_order_every_trainable_parameter(head, frozen):
    """The bridge has no objection, the trainers build, and the flat order holds each trainable parameter once: per block conv3 / bn3,
    the attention MLP (fc2, fc1, bn1), conv2.conv / bn0, conv1 / bn1, the shortcut (the order their gradients complete in)."""
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    m = _locator(head, frozen_stages=frozen).train()
    assert autograd_bridge.unsupported_reason(m) is None
    tr = (CprTrainer if head == 'cpr' else P2PTrainer)(m, two_streams=False)
    names = {id(p): k for k, p in m.named_parameters()}
    order = [names[id(p)] for p in tr._backward_order()]
    assert sorted(order) == sorted(k for k, p in m.named_parameters() if p.requires_grad) and len(set(order)) == len(order)
    bb = [k for k in order if k.startswith('backbone.')]
    assert bool(bb) == (frozen == 1)
    if bb:
        blk = [k[len('backbone.layer4.0.'):] for k in bb if k.startswith('backbone.layer4.0.')]
        assert blk == ['conv3.weight', 'bn3.weight', 'bn3.bias', 'conv2.fc2.weight', 'conv2.fc2.bias', 'conv2.fc1.weight', 'conv2.fc1.bias',
                       'conv2.bn1.weight', 'conv2.bn1.bias', 'conv2.conv.weight', 'conv2.bn0.weight', 'conv2.bn0.bias', 'conv1.weight',
                       'bn1.weight', 'bn1.bias', 'downsample.1.weight', 'downsample.2.weight', 'downsample.2.bias']
        assert bb[0] == 'backbone.layer4.2.conv3.weight'


def test_backward_walk_order_with_torch_stand_ins(monkeypatch):
    """_resnest_block_backward on a CPU block with every op replaced by a recorder: the launches come in the rule's order -- conv3's
    data gradient, splat_attn_grad, splat_attn_bwd, splat_apply_bwd, conv2's dense weight gradient and data gradient, conv1's ReLU
    backward -- the pooled block passes pool=True, and the dense weight gradient's diagonal blocks land in the parameter's gradient."""
    from pointtinybenchmark_amd import layers, ops, training
    m = _build(type='ResNeSt', depth=50, frozen_stages=1).train()
    blk = m.layer2[0]
    w = blk.width
    calls = []
    N, H, W = 1, 6, 8
    OH, OW = 3, 4
    dense_gw = torch.arange(2 * w * w * 9, dtype=torch.float32).reshape(2 * w, w, 3, 3)

    def rec(name, ret):
        def f(*a, **k):
            calls.append((name, k.get('pool')))
            return ret(*a, **k) if callable(ret) else ret
        return f
    monkeypatch.setattr(ops, 'relu_bwd_colsum', rec('relu_bwd_colsum', lambda dy, y=None, **k: (dy, torch.zeros(dy.shape[-1]))))
    monkeypatch.setattr(ops, 'splat_attn_grad', rec('splat_attn_grad', torch.zeros(N, 2, w)))
    monkeypatch.setattr(ops, 'splat_attn_bwd', rec('splat_attn_bwd', torch.zeros(N, w)))
    monkeypatch.setattr(ops, 'splat_apply_bwd', rec('splat_apply_bwd', (torch.zeros(N, H, W, 2 * w), torch.zeros(2 * w))))
    monkeypatch.setattr(ops, 'conv2d_wgrad', rec('conv2d_wgrad', lambda g, x, shape, s, p, **k: dense_gw.clone()))
    monkeypatch.setattr(ops, 'dgrad_pack', rec('dgrad_pack', 'PACK'))
    monkeypatch.setattr(ops, 'conv2d_dgrad', rec('conv2d_dgrad', lambda g, pt, hw, s, **k: torch.zeros((N,) + tuple(hw) + (w,))))
    monkeypatch.setattr(ops, 'bn_fold_bwd', rec('bn_fold_bwd', None))
    monkeypatch.setattr(training, 'folded_bn', lambda cache, bn: (torch.ones(bn.num_features), torch.zeros(bn.num_features)))
    monkeypatch.setattr(training, 'bn_inv_sigma', lambda cache, bn: torch.ones(bn.num_features))
    eng = training.BackwardEngine.__new__(training.BackwardEngine)
    eng._sink, eng._redirect, eng.side, eng._mixed = {}, None, None, False
    inner = []
    monkeypatch.setattr(eng, '_conv_bn_backward', lambda cache, conv, bn, g, cs, x, need_dx, **k:
                        inner.append(conv) or (torch.zeros(tuple(x.shape)) if need_dx else None), raising=False)
    monkeypatch.setattr(ops, 'avgpool_bwd', rec('avgpool_bwd', lambda dxp, hw, pool, add=None: add))
    rcd = dict(x=torch.zeros(N, H, W, 256), xp=torch.zeros(N, OH, OW, 256), o1=torch.zeros(N, H, W, w), u=torch.zeros(N, H, W, 2 * w),
               g=torch.zeros(N, w), z=torch.zeros(N, blk.conv2.inter), att=torch.zeros(N, 2, w), o=torch.zeros(N, OH, OW, w),
               out=torch.zeros(N, OH, OW, 4 * w))
    cache = layers._PackCache()
    monkeypatch.setattr(cache, 'get', lambda key, tensors, make, refresh=None: make())
    dx = eng._resnest_block_backward(cache, blk, rcd, torch.zeros(N, OH, OW, 4 * w), True)
    assert tuple(dx.shape) == (N, H, W, 256)
    assert [c[0] for c in calls] == ['relu_bwd_colsum', 'splat_attn_grad', 'splat_attn_bwd', 'splat_apply_bwd', 'conv2d_wgrad', 'bn_fold_bwd',
                                     'dgrad_pack', 'conv2d_dgrad', 'relu_bwd_colsum', 'avgpool_bwd']
    assert [c[1] for c in calls if c[0] in ('splat_attn_grad', 'splat_apply_bwd')] == [True, True]
    assert inner == [blk.conv3, blk.conv1, blk.ds_conv]
    gw = eng._sink[id(blk.conv2.conv.weight)]
    assert torch.equal(gw[:w], dense_gw[:w, :w // 2]) and torch.equal(gw[w:], dense_gw[w:, w // 2:])
