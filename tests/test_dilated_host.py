"""CPU: dilated ResNet / ResNetV1d / ResNeXt stages (``dilations``) -- what runs without a GPU.

  layout     for every case of tests/golden/dilated.npz (tools/gen_dilated.py): state-dict keys, order and shapes equal the reference
             class's; every conv's stride / padding / dilation / groups equal the recorded list; the synthetic weights load strictly;
             the trainable parameters are the reference's; train() keeps eval BatchNorm with norm_eval=True
  refusals   a dilated stage with a stride names strides and dilations; Res2Net names dilations (also at stride 1); RegNet keeps its
             NotImplementedError; the bf16 compute mode names dilations -- in set_compute_dtype, in autograd_bridge.unsupported_reason,
             in the trainers' constructors and in the backbone; PackedConv(dilation > 1, bf16) names dilation
  geometry   PackedConv.out_hw and the data-gradient padding at d = 2, 3, 4; wino_eligible is False for a dilated pack
  configs    a shipped CPR and a shipped P2P config build unmodified and with the two DC5 keys changed"""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests import dilated_ref as DR

CPR_CFG = 'configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_1x_TinyPersonV2_640.py'
P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'


def _build(**kw):
    import pointtinybenchmark_amd as P
    return P.build_backbone(dict(kw))


def _case_kwargs(cfg):
    kw = DR.kwargs(cfg)
    if DR.case_class(cfg) == 'ResNetV1d':
        kw.pop('deep_stem'), kw.pop('avg_down')
    return dict(kw, type=DR.case_class(cfg))


@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_fixture_case_has_the_reference_layout(name):
    cfg = DR.CASES[name]
    m = _build(**_case_kwargs(cfg))
    assert type(m).__name__ == DR.case_class(cfg) and m.dilations == tuple(cfg['dilations']) and m.strides == tuple(cfg['strides'])
    want = DR.keys(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want, sorted(set(got) ^ set(want))          # keys, ORDER and shapes
    assert DR.conv_settings(m) == DR.convs(name), [(a, b) for a, b in zip(DR.conv_settings(m), DR.convs(name)) if a != b]
    sd = DR.state_dict(cfg)
    assert sorted(sd) == sorted(k for k, _ in want)
    m.load_state_dict(sd, strict=True)
    # the same keys and shapes as the undilated net of that class: dilation changes no parameter
    kw = _case_kwargs(cfg)
    kw.pop('strides'), kw.pop('dilations')
    assert [(k, tuple(v.shape)) for k, v in _build(**kw).state_dict().items()] == got
    m.train()
    assert [n for n, p in m.named_parameters() if p.requires_grad] == DR.grad_names(name)
    assert not any(mod.training for mod in m.modules() if isinstance(mod, nn.BatchNorm2d))      # norm_eval=True
    m2 = _build(**dict(_case_kwargs(cfg), norm_eval=False)).train()
    first_live = cfg['frozen_stages'] + 1
    for i, lname in enumerate(m2.res_layers, 1):
        assert all(mod.training == (i >= first_live) for mod in getattr(m2, lname).modules() if isinstance(mod, nn.BatchNorm2d))


def test_every_block_of_a_dilated_stage_is_dilated():
    m = _build(type='ResNet', depth=50, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4))
    for name, d in zip(m.res_layers, (1, 1, 2, 4)):
        for blk in getattr(m, name):
            assert blk.conv2.dilation == (d, d) and blk.conv2.padding == (d, d) and blk.conv2.stride == ((2, 2) if (name == 'layer2' and blk is m.layer2[0]) else (1, 1))
            assert blk.conv1.dilation == (1, 1) and blk.conv3.dilation == (1, 1)
    b = _build(type='ResNet', depth=18, strides=(1, 2, 2, 1), dilations=(1, 1, 1, 3))
    for blk in b.layer4:      # BasicBlock: conv1 carries the dilation, conv2 stays padding 1 / dilation 1
        assert blk.conv1.dilation == (3, 3) and blk.conv1.padding == (3, 3) and blk.conv2.dilation == (1, 1) and blk.conv2.padding == (1, 1)
    for blk in b.layer3:
        assert blk.conv1.dilation == (1, 1) and blk.conv1.padding == (1, 1)
    x = _build(type='ResNeXt', depth=50, groups=32, base_width=4, **DR.DC5)
    assert all(blk.conv2.dilation == (2, 2) and blk.conv2.groups == 32 and blk.conv2.padding == (2, 2) for blk in x.layer4)
    assert all(p == 1 for p in _build(type='ResNet', depth=50).dilations)


def test_case_names_are_the_fixtures_and_the_cases_are_admitted():
    f = DR.fixture()
    assert json.loads(str(f['cases'])) == json.loads(json.dumps(DR.CASES))
    for name in DR.CASE_NAMES:      # admission: the reference alone in fp32, and its fp64 gradients under a one-ulp perturbation
        assert float(f[name + ':fp32:out'].max()) <= DR.BAR_OUT / 4 and float(f[name + ':fp32:grad'].max()) <= DR.BAR_GRAD / 4
        assert float(f[name + ':perturbed:grad'].max()) <= DR.BAR_GRAD / 4
        assert any(c[3] > 1 for c in DR.convs(name))
    assert os.path.getsize(DR.GOLDEN) < (1 << 20)


def test_refusals_name_their_key():
    for cls, kw in (('ResNet', dict(depth=50)), ('ResNet', dict(depth=18)), ('ResNetV1d', dict(depth=50)),
                    ('ResNeXt', dict(depth=50, groups=32, base_width=4))):
        # a dilated stage with a stride: at the default strides, and with one strided dilated stage among stride-1 ones
        for bad in (dict(dilations=(1, 1, 2, 4)), dict(strides=(1, 2, 2, 1), dilations=(1, 1, 2, 2)), dict(dilations=(1, 2, 1, 1))):
            with pytest.raises(AssertionError, match=r'(?s)dilations.*strides|strides.*dilations'):
                _build(type=cls, **kw, **bad)
        with pytest.raises(AssertionError):
            _build(type=cls, **kw, strides=(1, 2, 2, 1), dilations=(1, 1, 1, 0))
    # Res2Net: no dilated slice kernels, at stride 1 either
    for bad in (dict(strides=(1, 2, 2, 1), dilations=(1, 1, 1, 2)), dict(dilations=(1, 1, 2, 4))):
        with pytest.raises(AssertionError, match='dilations'):
            _build(type='Res2Net', depth=50, **bad)
    with pytest.raises(NotImplementedError, match='dilations'):
        _build(type='RegNet', arch='regnetx_800mf', strides=(2, 2, 2, 1), dilations=(1, 1, 1, 2))
    with pytest.raises(NotImplementedError, match='dilations'):
        _build(type='RegNet', arch='regnetx_800mf', dilations=(1, 1, 2, 4))


def test_packed_conv_geometry_and_refusals():
    from pointtinybenchmark_amd import ops
    w = torch.randn(64, 32, 3, 3)
    for d in (2, 3, 4):
        pc = ops.PackedConv(w, 1, d, dilation=d)
        assert pc.dilation == d and pc.padding == d and pc.Kpad == 9 * 32 and tuple(pc.w.shape) == (64, 288)
        for H, W in ((3, 3), (9, 12), (13, 11), (40, 40)):
            assert pc.out_hw(H, W) == (H, W)
            want = torch.nn.functional.conv2d(torch.zeros(1, 32, H, W), w, padding=d, dilation=d).shape[2:]
            assert pc.out_hw(H, W) == tuple(want)
        # the data gradient: the same dilated conv over dy, padding d (k - 1) - p = d
        assert ops.PackedConv.dgrad_padding(3, d, d) == d
        assert not ops.wino_eligible(pc, 40, 40)
        # the pack image is the undilated one
        assert torch.equal(pc.w, ops.PackedConv(w, 1, 1).w)
    assert ops.PackedConv.dgrad_padding(3, 1) == 1 and ops.PackedConv.dgrad_padding(1, 0) == 0 and ops.PackedConv.dgrad_padding(7, 3) == 3
    pc1 = ops.PackedConv(torch.randn(64, 64, 3, 3), 1, 1)
    assert pc1.dilation == 1 and pc1.out_hw(17, 23) == (17, 23) and ops.PackedConv(w, 2, 1).out_hw(17, 23) == (9, 12)
    assert ops.wino_eligible(pc1, 40, 40)
    with pytest.raises(NotImplementedError, match='dilation'):
        ops.PackedConv(torch.randn(64, 64, 3, 3), 1, 2, dtype=torch.bfloat16, dilation=2)
    for bad in (dict(stride=2, padding=2), dict(stride=1, padding=1)):       # a stride, or padding != dilation
        with pytest.raises(AssertionError, match='dilation'):
            ops.PackedConv(w, dilation=2, **bad)
    with pytest.raises(AssertionError, match='dilation'):
        ops.PackedConv(torch.randn(64, 32, 1, 1), 1, 2, dilation=2)
    with pytest.raises(AssertionError, match='dilation'):
        ops.dgrad_pack(w, 2, 2, dilation=2)
    with pytest.raises(NotImplementedError, match='dilation'):
        ops.dgrad_pack(w, 1, 2, dtype=torch.bfloat16, dilation=2)


def _locator(head, **bb):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(cfg['backbone'], **bb)
    return P.build_detector(cfg)


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_bf16_mode_is_refused_with_the_reason(head):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    m = _locator(head, **DR.DC5)
    assert autograd_bridge.unsupported_reason(m) is None
    with pytest.raises(NotImplementedError, match='dilations'):
        m.set_compute_dtype('bf16')
    assert m.backbone.compute_dtype == torch.float32 and m.set_compute_dtype('fp32') is m
    # a mode set behind the detector's back: the bridge reports it, the trainers' constructors and the backbone refuse it
    m.backbone.compute_dtype = torch.bfloat16
    assert 'dilations' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='dilations'):
        (CprTrainer if head == 'cpr' else P2PTrainer)(m, two_streams=False)
    with pytest.raises(NotImplementedError, match='dilations'):
        m.backbone(torch.zeros(1, 3, 32, 32))
    # dilations of 1 at other strides: the bf16 mode stays open
    assert _locator(head, strides=(1, 2, 2, 1)).set_compute_dtype('bf16').backbone.compute_dtype == torch.bfloat16


def _shipped(golden_dir, rel, merge=None):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[rel])))
    assert cfg.model.backbone.type == 'ResNet'
    if merge:
        cfg.merge_from_dict(merge)
    return P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


@pytest.mark.parametrize('rel', [CPR_CFG, P2P_CFG], ids=['cpr', 'p2p'])
def test_shipped_configs_build_unmodified_and_as_dc5(golden_dir, rel):
    from pointtinybenchmark_amd import autograd_bridge, synthetic
    m = _shipped(golden_dir, rel)
    assert m.backbone.dilations == (1, 1, 1, 1) and m.backbone.strides == (1, 2, 2, 2)
    assert all(c.dilation == (1, 1) for c in m.backbone.modules() if isinstance(c, nn.Conv2d))
    d = _shipped(golden_dir, rel, {'model.backbone.strides': (1, 2, 2, 1), 'model.backbone.dilations': (1, 1, 1, 2)})
    assert d.backbone.dilations == (1, 1, 1, 2) and all(b.conv2.dilation == (2, 2) for b in d.backbone.layer4)
    assert autograd_bridge.unsupported_reason(d) is None
    want = synthetic.resnet_state_dict(50, 0)
    got = {k: v for k, v in d.state_dict().items() if k.startswith('backbone.')}
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
