"""CPU: the Res2Net backbone -- what runs without a GPU.

  registry   build_backbone(dict(type='Res2Net', ...)); a shipped CPR and a shipped P2P config build with the backbone keys changed
  layout     state-dict keys, their order and shapes equal the reference class's (recorded in tests/golden/res2net.npz by
             tools/gen_res2net.py) for every fixture case and load strictly; named_parameters order; slice widths per stage;
             style='caffe' / deep_stem=False are overridden as the reference overrides them
  refusals   settings outside the slice kernels' rule name scales and base_width; depth 18 is ResNet's KeyError; the bf16 compute mode
             names ``scales`` -- in set_compute_dtype, the backbone, autograd_bridge.unsupported_reason and the trainers' constructors;
             batch statistics name ``norm_eval``; the deep stem's and ResNet's refusals stay
  fixture    the conditioning entries are within a quarter of the bars; an fp64 restatement of the block in plain torch matches the
             fixture's stage outputs at 1e-9; the synthetic generators' other draws are unchanged"""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests import res2net_ref as R2

CPR_CFG = 'configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_1x_TinyPersonV2_640.py'
P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'
PUBLISHED = [(26, 4), (26, 6), (26, 8), (14, 8), (48, 2)]


def _build(**kw):
    import pointtinybenchmark_amd as P
    return P.build_backbone(dict(kw))


def test_registry_builds_res2net():
    from pointtinybenchmark_amd import backbones
    from pointtinybenchmark_amd.backbones.res2net import Res2Net
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    from pointtinybenchmark_amd.registry import BACKBONES
    assert BACKBONES.get('Res2Net') is Res2Net and backbones.Res2Net is Res2Net and issubclass(Res2Net, ResNet)
    m = _build(type='Res2Net', depth=50, scales=4, base_width=26, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
               norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch')
    assert type(m) is Res2Net and m.scales == 4 and m.base_width == 26 and m.feat_dim == 2048
    assert m.deep_stem and m.avg_down and m.style == 'pytorch'
    for name in m.res_layers:
        for bi, blk in enumerate(getattr(m, name)):
            assert blk.stage_type == ('stage' if bi == 0 else 'normal')
            assert not hasattr(blk, 'conv2') and not hasattr(blk, 'bn2')
            assert len(blk.convs) == len(blk.bns) == 3
            assert (blk.downsample is not None) == (bi == 0)


@pytest.mark.parametrize('base_width,scales', PUBLISHED, ids=['%dw%ds' % p for p in PUBLISHED])
@pytest.mark.parametrize('depth', [50, 101, 152])
def test_published_settings_build_with_their_widths(depth, base_width, scales):
    from pointtinybenchmark_amd.backbones.res2net import slice_width
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    m = _build(type='Res2Net', depth=depth, scales=scales, base_width=base_width)
    assert [len(getattr(m, n)) for n in m.res_layers] == list(ResNet.arch_settings[depth][1])
    inplanes = 64
    for i, name in enumerate(m.res_layers):
        planes = 64 * 2 ** i
        w = base_width * 2 ** i
        assert slice_width(planes, base_width) == w
        for bi, blk in enumerate(getattr(m, name)):
            stride = 2 if (bi == 0 and i > 0) else 1
            assert tuple(blk.conv1.weight.shape) == (w * scales, inplanes, 1, 1) and blk.bn1.num_features == w * scales
            assert blk.conv1.stride == (1, 1)
            assert tuple(blk.conv3.weight.shape) == (4 * planes, w * scales, 1, 1) and blk.bn3.num_features == 4 * planes
            assert len(blk.convs) == scales - 1
            for conv, bn in zip(blk.convs, blk.bns):
                assert tuple(conv.weight.shape) == (w, w, 3, 3) and conv.stride == (stride, stride) and conv.padding == (1, 1)
                assert conv.bias is None and bn.num_features == w
            inplanes = 4 * planes


@pytest.mark.parametrize('name', R2.CASE_NAMES)
def test_fixture_case_has_the_reference_state_dict_layout(name):
    cfg = R2.CASES[name]
    m = _build(type='Res2Net', **R2.res2net_kwargs(cfg))
    want = R2.keys(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]          # keys, their order, shapes
    if name in R2.STATE_DICT_KEYS:
        assert len(got) == R2.STATE_DICT_KEYS[name]
    sd = R2.case_state_dict(cfg)
    assert list(sd) == [k for k, _ in want]                                         # the synthetic generator keeps that order too
    m.load_state_dict(sd, strict=True)
    assert not any(k.endswith(('conv2.weight', 'bn2.weight')) for k in sd) and 'stem.0.weight' in sd
    m.train()
    assert [n for n, p in m.named_parameters() if p.requires_grad] == R2.grad_names(name)
    assert not any(mod.training for mod in m.modules() if isinstance(mod, nn.BatchNorm2d))


def test_case_names_are_the_fixtures_and_the_cases_are_admitted():
    f = R2.fixture()
    assert json.loads(str(f['cases'])) == json.loads(json.dumps(R2.CASES))
    for name in R2.CASE_NAMES:      # admission: the reference alone in fp32, and its fp64 gradients under a one-ulp perturbation
        assert float(f[name + ':fp32:out'].max()) <= R2.BAR_OUT / 4 and float(f[name + ':fp32:grad'].max()) <= R2.BAR_GRAD / 4
        assert float(f[name + ':perturbed:grad'].max()) <= R2.BAR_GRAD / 4
    assert os.path.getsize(R2.GOLDEN) < (1 << 20)


def test_style_and_stem_arguments_are_overridden_as_the_reference_overrides_them():
    a = _build(type='Res2Net', depth=50, style='caffe', deep_stem=False, avg_down=False)
    b = _build(type='Res2Net', depth=50)
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    assert a.style == 'pytorch' and a.deep_stem and a.avg_down
    assert a.layer2[0].conv1.stride == (1, 1) and a.layer2[0].convs[0].stride == (2, 2)
    assert isinstance(a.layer2[0].downsample[0], nn.AvgPool2d) and isinstance(a.layer1[0].downsample[0], nn.AvgPool2d)


def test_refusals_name_the_option():
    from pointtinybenchmark_amd.backbones import res2net
    for scales, bw in ((4, 13), (4, 27), (9, 26), (1, 26), (4, 66)):
        # 13 / 27: odd slices at stage 1; 9, 1: scales outside 2 .. 8; 66: 528-channel slices at stage 4
        with pytest.raises(NotImplementedError, match=r'scales=%d.*base_width=%d' % (scales, bw)):
            _build(type='Res2Net', depth=50, scales=scales, base_width=bw)
        assert res2net.unsupported_reason(scales, bw) is not None
    for bw, scales in PUBLISHED:
        assert res2net.unsupported_reason(scales, bw) is None
    for depth in (18, 34):
        with pytest.raises(KeyError, match='invalid depth %d' % depth):
            _build(type='Res2Net', depth=depth)
    # what ResNet refuses stays refused
    for bad in (dict(dilations=(1, 1, 2, 4)), dict(dcn=dict(type='DCN')), dict(plugins=[dict()]), dict(with_cp=True)):
        with pytest.raises(AssertionError):
            _build(type='Res2Net', depth=50, **bad)
    with pytest.raises(NotImplementedError, match='stem_channels'):
        _build(type='Res2Net', depth=50, stem_channels=32)
    m = _build(type='Res2Net', depth=50, frozen_stages=-1)
    assert 'deep_stem' in m.stem_train_reason()


def test_batch_statistics_are_refused_naming_norm_eval():
    m = _build(type='Res2Net', depth=50, norm_eval=False, frozen_stages=1)
    m.train()
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m.layer2[0].run(None, torch.zeros(1, 8, 8, 256))
    m.eval()              # eval mode: running statistics everywhere, nothing to refuse
    m._check_mode()
    frozen = _build(type='Res2Net', depth=50, norm_eval=False, frozen_stages=4)
    frozen.train()
    assert not any(blk.batch_stats() for n in frozen.res_layers for blk in getattr(frozen, n))


def _locator(head, **bb):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(cfg['backbone'], type='Res2Net', scales=4, base_width=26, **bb)
    return P.build_detector(cfg)


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_bf16_mode_is_refused_with_the_reason(head):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    m = _locator(head, frozen_stages=4)
    assert autograd_bridge.unsupported_reason(m) is None
    with pytest.raises(NotImplementedError, match='scales=4'):
        m.set_compute_dtype('bf16')
    assert m.backbone.compute_dtype == torch.float32 and m.set_compute_dtype('fp32') is m
    # a mode set behind the detector's back: the bridge reports it, the trainers' constructors and the backbone refuse it
    m.backbone.compute_dtype = torch.bfloat16
    assert 'scales=4' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='scales=4'):
        (CprTrainer if head == 'cpr' else P2PTrainer)(m, two_streams=False)
    with pytest.raises(NotImplementedError, match='scales=4'):
        m.backbone(torch.zeros(1, 3, 32, 32))


def _shipped(golden_dir, rel):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[rel])))
    assert cfg.model.backbone.type == 'ResNet' and list(cfg.model.neck.in_channels) == [256, 512, 1024, 2048]
    cfg.merge_from_dict({'model.backbone.type': 'Res2Net', 'model.backbone.scales': 4, 'model.backbone.base_width': 26})
    return P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


@pytest.mark.parametrize('rel', [CPR_CFG, P2P_CFG], ids=['cpr', 'p2p'])
def test_shipped_configs_build_with_the_backbone_keys_changed(golden_dir, rel):
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.backbones.res2net import Res2Net
    m = _shipped(golden_dir, rel)
    assert type(m.backbone) is Res2Net and m.backbone.depth == 50 and m.backbone.frozen_stages == 1
    assert tuple(m.backbone.layer1[0].convs[0].weight.shape) == (26, 26, 3, 3)
    assert tuple(m.backbone.layer4[2].convs[2].weight.shape) == (208, 208, 3, 3)
    want = synthetic.res2net_state_dict(50, 4, 26, 0)
    got = {k: v for k, v in m.state_dict().items() if k.startswith('backbone.')}
    assert [(k, tuple(v.shape)) for k, v in got.items()] == [(k, tuple(v.shape)) for k, v in want.items()]


@pytest.mark.parametrize('name', ['r50_26w4s', 'r50_14w8s', 'r50_48w2s'])
def test_fp64_restatement_matches_the_fixture(name):
    """The semantics restated in plain torch (tests/res2net_ref.restated_forward), in fp64 on the case's weights and image, against the
    reference class's fp64 outputs."""
    cfg = R2.CASES[name]
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    with torch.no_grad():
        outs = R2.restated_forward(R2.case_state_dict(cfg, torch.float64), cfg, R2.case_input(cfg, torch.float64))
    assert len(outs) == 4
    for l, o in enumerate(outs):
        assert R2.output_error(name, l, o) <= 1e-9


def test_synthetic_defaults_draw_what_they_drew():
    from pointtinybenchmark_amd import synthetic
    before = synthetic.resnet_state_dict(50, 3)
    synthetic.res2net_state_dict(50, 4, 26, 3)
    after = synthetic.resnet_state_dict(50, 3)
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    a, b = synthetic.res2net_state_dict(50, 4, 26, 5, prefix=''), synthetic.res2net_state_dict(50, 4, 26, 5, prefix='')
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert tuple(a['layer3.0.convs.1.weight'].shape) == (104, 104, 3, 3) and tuple(a['layer3.0.conv3.weight'].shape) == (1024, 416, 1, 1)


@pytest.mark.parametrize('frozen', [1, 4])
@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_trainers_build_and_order_every_trainable_parameter(head, frozen):
    """The bridge has no objection, the trainers build, and the flat order holds each trainable parameter once: per block conv3 / bn3,
    the slice convs last first, conv1 / bn1, the shortcut (the order their gradients complete in)."""
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
        blk = [k[len('backbone.layer4.2.'):] for k in bb if k.startswith('backbone.layer4.2.')]
        assert blk == ['conv3.weight', 'bn3.weight', 'bn3.bias', 'convs.2.weight', 'bns.2.weight', 'bns.2.bias', 'convs.1.weight',
                       'bns.1.weight', 'bns.1.bias', 'convs.0.weight', 'bns.0.weight', 'bns.0.bias', 'conv1.weight', 'bn1.weight', 'bn1.bias']
        assert bb[0] == 'backbone.layer4.2.conv3.weight'
