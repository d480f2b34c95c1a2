"""CPU: the ResNet variants -- style='caffe', avg_down, deep_stem, ResNetV1d -- what runs without a GPU.

  module     the four variants and ResNetV1d build from config dicts; state-dict keys and shapes equal the reference classes'
             (recorded in tests/golden/resnet_variants.npz by tools/gen_resnet_variants.py) and a strict load succeeds; train()
             flags and requires_grad follow resnet.py:612-657 for frozen_stages x norm_eval, ``stem.eval()`` included; a caffe
             BasicBlock net has the strides of the pytorch one
  refusals   a trainable deep stem and deep_stem with stem_channels != 64 name the option
  synthetic  resnet_state_dict()'s defaults are the tensors they were before the keywords existed
  configs    a shipped CPR and a shipped P2P config with the backbone overridden to ResNetV1d build"""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests import resnet_variants_ref as RV

CPR_CFG = 'configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_1x_TinyPersonV2_640.py'
P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'


def _build(**kw):
    import pointtinybenchmark_amd as P
    return P.build_backbone(dict(kw))


def _case_cfg(cfg):
    kw = RV.resnet_kwargs(cfg)
    if kw['deep_stem'] and kw['avg_down']:
        kw.pop('deep_stem'), kw.pop('avg_down')
        return dict(type='ResNetV1d', **kw)
    return dict(type='ResNet', **kw)


@pytest.mark.parametrize('kw', [dict(type='ResNet', depth=50, style='caffe'), dict(type='ResNet', depth=50, avg_down=True),
                                dict(type='ResNet', depth=18, deep_stem=True), dict(type='ResNet', depth=50, deep_stem=True, avg_down=True),
                                dict(type='ResNetV1d', depth=50), dict(type='ResNetV1d', depth=18, frozen_stages=1)],
                         ids=['caffe', 'avg_down', 'deep_stem', 'both', 'v1d50', 'v1d18'])
def test_variants_build_from_config_dicts(kw):
    from pointtinybenchmark_amd.backbones.resnet import ResNet, ResNetV1d
    m = _build(**kw)
    assert isinstance(m, ResNet) and (kw['type'] != 'ResNetV1d' or (type(m) is ResNetV1d and m.deep_stem and m.avg_down))
    if m.deep_stem:
        assert isinstance(m.stem, nn.Sequential) and not hasattr(m, 'conv1') and not hasattr(m, 'bn1')
        assert [tuple(m.stem[i].weight.shape) for i in (0, 3, 6)] == [(32, 3, 3, 3), (32, 32, 3, 3), (64, 32, 3, 3)]
        assert [m.stem[i].stride for i in (0, 3, 6)] == [(2, 2), (1, 1), (1, 1)] and all(m.stem[i].bias is None for i in (0, 3, 6))
    if m.avg_down:
        for i, name in enumerate(m.res_layers):
            ds = getattr(m, name)[0].downsample
            if ds is None:
                continue
            stride = 1 if i == 0 else 2
            pool = ds[0]
            assert isinstance(pool, nn.AvgPool2d) and pool.kernel_size == stride and pool.stride == stride
            assert pool.ceil_mode and not pool.count_include_pad
            assert ds[1].stride == (1, 1) and isinstance(ds[2], nn.BatchNorm2d)
            assert getattr(m, name)[0].ds_pool == (0 if stride == 1 else 2)      # the stride-1 pool is the identity: no launch


@pytest.mark.parametrize('name', RV.CASE_NAMES)
def test_fixture_case_has_the_reference_state_dict_layout(name):
    cfg = RV.CASES[name]
    m = _build(**_case_cfg(cfg))
    want = RV.keys(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    sd = RV.case_state_dict(cfg)
    assert sorted(sd) == sorted(k for k, _ in want)
    m.load_state_dict(sd, strict=True)
    if cfg.get('deep_stem'):
        assert {'stem.0.weight', 'stem.1.running_var', 'stem.3.weight', 'stem.4.bias', 'stem.6.weight', 'stem.7.weight'} <= set(sd)
        assert not any(k.startswith(('conv1.', 'bn1.')) for k in sd)
    if cfg.get('avg_down'):
        assert 'layer2.0.downsample.1.weight' in sd and 'layer2.0.downsample.2.running_mean' in sd
        assert not any('.downsample.0.' in k for k in sd)
        if cfg['depth'] >= 50:
            assert 'layer1.0.downsample.1.weight' in sd        # the stride-1 pool still shifts the keys
    # the trainable set is the fixture's gradient list
    m.train()
    assert [n for n, p in m.named_parameters() if p.requires_grad] == RV.grad_names(name)


def test_case_names_are_the_fixtures():
    assert sorted(RV.CASE_NAMES) == sorted(json.loads(str(RV.fixture()['cases'])))
    assert json.loads(str(RV.fixture()['cases'])) == json.loads(json.dumps(RV.CASES))
    f = RV.fixture()
    for name in RV.CASE_NAMES:      # admission: the reference alone in fp32 within a quarter of the bars
        assert float(f[name + ':fp32:out'].max()) <= RV.BAR_OUT / 4 and float(f[name + ':fp32:grad'].max()) <= RV.BAR_GRAD / 4
        assert float(f[name + ':perturbed:grad'].max()) <= RV.BAR_GRAD / 4


@pytest.mark.parametrize('norm_eval', [True, False])
@pytest.mark.parametrize('frozen_stages', [-1, 0, 1, 2])
@pytest.mark.parametrize('kw', [dict(type='ResNetV1d', depth=50), dict(type='ResNet', depth=18, deep_stem=True),
                                dict(type='ResNet', depth=50, avg_down=True, style='caffe')], ids=['v1d50', 'deepstem18', 'caffe_avgdown50'])
def test_train_flags_follow_the_reference(kw, frozen_stages, norm_eval):
    """resnet.py:612-657: frozen_stages >= 0 puts the whole stem in eval mode with requires_grad False (deep stem: ``stem.eval()``),
    stages 1..frozen_stages likewise; norm_eval puts every BatchNorm in eval mode while the other modules train."""
    m = _build(frozen_stages=frozen_stages, norm_eval=norm_eval, **kw)
    assert all(p.requires_grad == (frozen_stages < 0) for p in m.stem_parameters())      # the constructor freezes already
    m.train()
    for _ in range(2):      # (train() twice: it must not drift)
        stem = [m.stem] if m.deep_stem else [m.conv1, m.bn1]
        for mod in stem:
            assert all(p.requires_grad == (frozen_stages < 0) for p in mod.parameters())
        if m.deep_stem and m.training:
            assert m.stem.training == (frozen_stages < 0)
            assert all(sub.training == (frozen_stages < 0) for sub in m.stem if not isinstance(sub, nn.BatchNorm2d))
        for i, name in enumerate(m.res_layers):
            layer = getattr(m, name)
            frozen = i + 1 <= frozen_stages
            assert all(p.requires_grad != frozen for p in layer.parameters())
            if m.training:
                assert layer.training != frozen
                for sub in layer.modules():
                    if isinstance(sub, nn.BatchNorm2d):
                        assert sub.training == (not frozen and not norm_eval)
        if m.training:
            for bn in m.stem_norms():
                assert bn.training == (frozen_stages < 0 and not norm_eval)
            assert m.batch_stats_active() == (not norm_eval and frozen_stages < 4)
        m.train()
    m.eval()
    assert not any(sub.training for sub in m.modules()) and not m.batch_stats_active()


def test_caffe18_has_the_strides_of_pytorch18():
    a, b = _build(type='ResNet', depth=18, style='caffe'), _build(type='ResNet', depth=18, style='pytorch')
    sa = [(n, mod.stride) for n, mod in a.named_modules() if isinstance(mod, nn.Conv2d)]
    sb = [(n, mod.stride) for n, mod in b.named_modules() if isinstance(mod, nn.Conv2d)]
    assert sa == sb
    # and a bottleneck moves the stride from the 3x3 to the first 1x1
    c, p = _build(type='ResNet', depth=50, style='caffe'), _build(type='ResNet', depth=50)
    for i in (2, 3, 4):
        bc, bp = getattr(c, 'layer%d' % i)[0], getattr(p, 'layer%d' % i)[0]
        assert (bc.conv1.stride, bc.conv2.stride) == ((2, 2), (1, 1)) and (bp.conv1.stride, bp.conv2.stride) == ((1, 1), (2, 2))
        assert bc.conv1.kernel_size == (1, 1) and bc.conv2.kernel_size == (3, 3) and bc.conv2.padding == (1, 1)
        assert getattr(c, 'layer%d' % i)[1].conv1.stride == (1, 1)
    assert c.layer1[0].conv1.stride == (1, 1)


def test_refusals_name_the_option():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import autograd_bridge, synthetic
    from bench import p2p_model_cfg
    with pytest.raises(NotImplementedError, match='stem_channels=32'):
        _build(type='ResNet', depth=50, deep_stem=True, stem_channels=32)
    with pytest.raises(NotImplementedError, match='stem_channels=128'):
        _build(type='ResNetV1d', depth=50, stem_channels=128)
    assert _build(type='ResNetV1d', depth=18, stem_channels=64).deep_stem
    m = _build(type='ResNetV1d', depth=18, frozen_stages=-1)
    assert 'deep_stem' in m.stem_train_reason()
    # a recorded forward (tape) through a trainable deep stem raises that reason before any kernel runs
    with pytest.raises(NotImplementedError, match='deep_stem'):
        m.run_stem(torch.zeros(1, 3, 32, 32), tape=[])
    # the bridge says the same, and admits the frozen one
    cfg = p2p_model_cfg(18, 1)
    cfg['backbone'] = dict(type='ResNetV1d', depth=18, frozen_stages=-1, norm_eval=True)
    assert 'deep_stem' in autograd_bridge.unsupported_reason(P.build_detector(cfg))
    cfg['backbone']['frozen_stages'] = 1
    assert autograd_bridge.unsupported_reason(P.build_detector(cfg)) is None
    # what stays refused
    for bad in (dict(dilations=(1, 1, 2, 4)), dict(dcn=dict(type='DCN')), dict(plugins=[dict()]), dict(with_cp=True), dict(style='tf')):
        with pytest.raises(AssertionError):
            _build(type='ResNet', depth=50, **bad)


def test_trainer_refuses_a_trainable_deep_stem_with_the_reason():
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd.training import P2PTrainer
    cfg = p2p_model_cfg(18, 1)
    cfg['backbone'] = dict(type='ResNetV1d', depth=18, frozen_stages=-1, norm_eval=True)
    m = P.build_detector(cfg)
    with pytest.raises(AssertionError, match='deep_stem'):
        P2PTrainer(m, two_streams=False)


def _old_resnet_state_dict(depth, seed, prefix):
    """synthetic.resnet_state_dict as it was before the deep_stem / avg_down keywords, restated."""
    from pointtinybenchmark_amd.synthetic import ARCH, _bn, _kaiming
    g = torch.Generator().manual_seed(seed)
    kind, blocks = ARCH[depth]
    sd = {prefix + 'conv1.weight': _kaiming((64, 3, 7, 7), g)}
    _bn(sd, prefix + 'bn1', 64, g)
    inplanes = 64
    for li, nb in enumerate(blocks):
        planes, stride, exp = 64 * 2 ** li, (1 if li == 0 else 2), (4 if kind == 'bottleneck' else 1)
        for bi in range(nb):
            p = '%slayer%d.%d.' % (prefix, li + 1, bi)
            shapes = [(planes, inplanes, 1, 1), (planes, planes, 3, 3), (planes * 4, planes, 1, 1)] if kind == 'bottleneck' else \
                [(planes, inplanes, 3, 3), (planes, planes, 3, 3)]
            for j, shp in enumerate(shapes):
                sd['%sconv%d.weight' % (p, j + 1)] = _kaiming(shp, g)
                _bn(sd, '%sbn%d' % (p, j + 1), shp[0], g)
            if bi == 0 and (stride != 1 or inplanes != planes * exp):
                sd[p + 'downsample.0.weight'] = _kaiming((planes * exp, inplanes, 1, 1), g)
                _bn(sd, p + 'downsample.1', planes * exp, g)
            inplanes = planes * exp
    return sd


@pytest.mark.parametrize('depth', [18, 50])
def test_synthetic_defaults_are_unchanged(depth):
    from pointtinybenchmark_amd import synthetic
    want = _old_resnet_state_dict(depth, 0, 'backbone.')
    for got in (synthetic.resnet_state_dict(depth), synthetic.resnet_state_dict(depth, deep_stem=False, avg_down=False)):
        assert list(got) == list(want)
        assert all(torch.equal(got[k], want[k]) for k in want)
    loc = synthetic.locator_state_dict(depth)
    assert all(torch.equal(loc[k], want[k]) for k in want)
    # the new layouts: same count of tensors per module, the keys moved
    v = synthetic.resnet_state_dict(depth, deep_stem=True, avg_down=True)
    assert 'backbone.stem.6.weight' in v and 'backbone.layer2.0.downsample.2.weight' in v and 'backbone.conv1.weight' not in v


def _shipped(golden_dir, rel, backbone):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[rel])))
    assert cfg.model.backbone.type == 'ResNet' and cfg.model.backbone.style == 'pytorch'
    cfg.merge_from_dict({'model.backbone.type': 'ResNetV1d'} if backbone == 'v1d' else {'model.backbone.style': 'caffe'})
    return P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


@pytest.mark.parametrize('rel', [CPR_CFG, P2P_CFG], ids=['cpr', 'p2p'])
def test_shipped_configs_build_with_the_backbone_overridden(golden_dir, rel):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.backbones.resnet import ResNetV1d
    m = _shipped(golden_dir, rel, 'v1d')
    assert type(m.backbone) is ResNetV1d and m.backbone.depth == 50 and m.backbone.frozen_stages == 1
    keys = set(m.state_dict())
    assert 'backbone.stem.6.weight' in keys and 'backbone.layer1.0.downsample.1.weight' in keys and 'backbone.conv1.weight' not in keys
    assert autograd_bridge.unsupported_reason(m) is None
    m = _shipped(golden_dir, rel, 'caffe')
    assert m.backbone.layer3[0].conv1.stride == (2, 2) and autograd_bridge.unsupported_reason(m) is None
