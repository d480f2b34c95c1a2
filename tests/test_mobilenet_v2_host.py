"""CPU: the MobileNetV2 backbone -- what runs without a GPU.

  registry   build_backbone(dict(type='MobileNetV2')); a CPR and a P2P config build with the backbone dict switched
  layout     state-dict keys, their order and shapes equal the reference class's (recorded in tests/golden/mobilenet_v2.npz by
             tools/gen_mobilenet_v2.py) and load strictly; make_divisible and arch_settings restated; train() / _freeze_stages
  refusals   widen_factor, act_cfg, conv_cfg, norm_cfg, with_cp, the bf16 compute mode (``MobileNetV2``) -- in set_compute_dtype, the
             backbone, autograd_bridge.unsupported_reason and the trainers' constructors --, batch statistics (``norm_eval``); the
             reference's ValueErrors for out_indices / frozen_stages
  fixture    the conditioning entries are within a quarter of the bars; the fp64 restatement (tests/mobilenet_v2_ref.py) matches the
             fixture's stage outputs at 1e-9; every ReLU6 map of every case has >= 1 % of its elements on either clamp; the kernel tests'
             mask sources have <= 0.5 % threshold elements
  walk       the trainers' flat order, and the block rule's launch order with torch stand-ins"""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests import mobilenet_v2_ref as MB

NECK_IN = [24, 32, 96, 1280]


def _build(**kw):
    import pointtinybenchmark_amd as P
    return P.build_backbone(dict(type='MobileNetV2', **kw))


def test_registry_builds_mobilenet_v2():
    from pointtinybenchmark_amd import backbones
    from pointtinybenchmark_amd.backbones.mobilenet_v2 import MobileNetV2, make_divisible
    from pointtinybenchmark_amd.registry import BACKBONES
    assert BACKBONES.get('MobileNetV2') is MobileNetV2 and backbones.MobileNetV2 is MobileNetV2
    m = _build()
    assert m.out_indices == (1, 2, 4, 7) and m.frozen_stages == -1 and m.norm_eval is False and m.widen_factor == 1.0
    assert m.arch_settings == MB.ARCH and m.layers == ['layer%d' % i for i in range(1, 8)] + ['conv2']
    assert m.stage_widths == MB.STAGE_CHANNELS and m.out_channel == 1280 and m.feat_dim == 1280
    got = [(b.in_channels, b.mid_channels, b.out_channels, b.stride, b.with_expand_conv)
           for i in range(7) for b in m.stage_blocks(i)]
    assert got == [b[1:] for b in MB.blocks()]
    assert not hasattr(m.layer1[0], 'expand_conv') and m.layer1[0].kind == 'mbv2' and m.conv2.kind == 'mbv2_conv2'
    assert [b.with_res_shortcut for b in m.layer2] == [False, True] and [b.with_res_shortcut for b in m.layer5] == [False, True, True]
    assert tuple(m.layer2[1].depthwise_conv.conv.weight.shape) == (144, 1, 3, 3) and m.layer2[1].depthwise_conv.conv.groups == 144
    # make_divisible as the reference computes it
    assert [make_divisible(v, 8) for v in (32, 16, 24, 12, 20, 35.2, 8.0, 3)] == [32, 16, 24, 16, 24, 32, 8, 8]
    assert make_divisible(10, 8) == 16 and make_divisible(17, 8, min_ratio=0.5) == 16 and make_divisible(4, 8, min_value=16) == 16


def test_state_dict_layout_is_the_reference_classes():
    from pointtinybenchmark_amd import synthetic
    m = _build()
    want = MB.class_keys()
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]          # keys, their order, shapes
    sd = synthetic.mobilenet_v2_state_dict(3, prefix='')
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want                     # the synthetic generator keeps that order too
    m.load_state_dict(sd, strict=True)
    assert 'layer1.0.expand_conv.conv.weight' not in sd and tuple(sd['layer1.0.depthwise_conv.conv.weight'].shape) == (32, 1, 3, 3)
    assert tuple(sd['conv2.conv.weight'].shape) == (1280, 320, 1, 1) and tuple(sd['conv1.conv.weight'].shape) == (32, 3, 3, 3)
    a, b = synthetic.mobilenet_v2_state_dict(5), synthetic.mobilenet_v2_state_dict(5)
    assert all(k.startswith('backbone.') for k in a) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('name', MB.CASE_NAMES)
def test_fixture_case_has_the_reference_state_dict_layout(name):
    cfg = MB.CASES[name]
    m = _build(**MB.mobilenet_kwargs(cfg))
    want = MB.keys(name)
    assert want == MB.class_keys()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    sd = MB.case_state_dict(cfg)
    assert list(sd) == [k for k, _ in want]
    m.load_state_dict(sd, strict=True)
    m.train()
    # the fixture lists the parameters a gradient reaches: trainable, and not behind the last output
    reached = tuple('%s.' % n for n in m.layers[:m.last_stage() + 1]) + ('conv1.',)
    assert [n for n, p in m.named_parameters() if p.requires_grad and n.startswith(reached)] == MB.grad_names(name)
    assert not any(mod.training for mod in m.modules() if isinstance(mod, nn.BatchNorm2d))


def test_case_names_are_the_fixtures_and_the_cases_are_admitted():
    f = MB.fixture()
    assert json.loads(str(f['cases'])) == json.loads(json.dumps(MB.CASES))
    for name in MB.CASE_NAMES:      # admission: the reference alone in fp32, and its fp64 gradients under a one-ulp perturbation
        assert float(f[name + ':fp32:out'].max()) <= MB.BAR_OUT / 4 and float(f[name + ':fp32:grad'].max()) <= MB.BAR_GRAD / 4
        assert float(f[name + ':perturbed:grad'].max()) <= MB.BAR_GRAD / 4
    assert os.path.getsize(MB.GOLDEN) < (1 << 20)
    assert all(c['hw'] == (64, 64) for n, c in MB.CASES.items() if n != 'odd') and MB.CASES['odd']['hw'] == (72, 104)
    assert MB.BATCH == 2


def test_freeze_stages_and_train_follow_the_reference():
    for fs in range(-1, 8):
        m = _build(frozen_stages=fs, norm_eval=True)
        assert all(p.requires_grad for p in m.parameters())        # the reference freezes in train(), not in its constructor
        m.train()
        assert all(p.requires_grad == (fs < 0) for p in m.conv1.parameters())
        for i in range(1, 8):
            layer = getattr(m, 'layer%d' % i)
            assert all(p.requires_grad == (i > fs) for p in layer.parameters()), (fs, i)
            assert layer.training == (i > fs)
        assert all(p.requires_grad for p in m.conv2.parameters())      # conv2 is never frozen
        assert not any(mod.training for mod in m.modules() if isinstance(mod, nn.modules.batchnorm._BatchNorm))
    m = _build(frozen_stages=2, norm_eval=False).train()
    assert m.layer3[0].depthwise_conv.bn.training and not m.layer2[0].depthwise_conv.bn.training and m.conv1.bn.training
    for norm in ('BN', 'SyncBN'):
        m = _build(norm_cfg=dict(type=norm, momentum=0.05))
        assert isinstance(m.conv1.bn, nn.SyncBatchNorm if norm == 'SyncBN' else nn.BatchNorm2d) and m.conv2.bn.momentum == 0.05


def test_refusals_name_their_key_and_value_errors_are_the_references():
    from pointtinybenchmark_amd.backbones import mobilenet_v2
    for kw, key in ((dict(widen_factor=0.5), 'widen_factor'), (dict(widen_factor=1.4), 'widen_factor'),
                    (dict(act_cfg=dict(type='ReLU')), 'act_cfg'), (dict(act_cfg=None), 'act_cfg'),
                    (dict(conv_cfg=dict(type='DCN')), 'conv_cfg'), (dict(norm_cfg=dict(type='GN', num_groups=8)), 'norm_cfg'),
                    (dict(with_cp=True), 'with_cp')):
        with pytest.raises(NotImplementedError, match=key):
            _build(**kw)
        assert key in mobilenet_v2.unsupported_reason(**kw)
    assert mobilenet_v2.unsupported_reason() is None and _build(conv_cfg=dict(type='Conv2d')).conv_cfg == dict(type='Conv2d')
    with pytest.raises(ValueError, match=r'out_indices must be a subset of range\(0, 8\)'):
        _build(out_indices=(1, 8))
    for fs in (-2, 8):
        with pytest.raises(ValueError, match=r'frozen_stages must be in range\(-1, 8\)'):
            _build(frozen_stages=fs)
    with pytest.raises(TypeError, match='pretrained must be a str or None'):
        _build(pretrained=3)
    assert _build(out_indices=(0, 7), frozen_stages=7).out_indices == (0, 7)


def test_batch_statistics_are_refused_naming_norm_eval():
    m = _build(norm_eval=False, frozen_stages=1)
    m.train()
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m.layer2[0].run(None, torch.zeros(1, 8, 8, 32))
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m.conv2.run(None, torch.zeros(1, 2, 2, 320))
    m.eval()              # eval mode: running statistics everywhere, nothing to refuse
    m._check_mode()
    assert not m.batch_stats_active()
    ok = _build(norm_eval=True).train()
    ok._check_mode()


def _locator(head, **bb):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cfg = model_cfg(50, 1) if head == 'cpr' else p2p_model_cfg(50, 1)
    cfg['backbone'] = dict(dict(type='MobileNetV2', norm_eval=True), **bb)
    cfg['neck'] = dict(cfg['neck'], in_channels=NECK_IN)
    return P.build_detector(cfg)


@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_bf16_mode_is_refused_with_the_reason(head):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    m = _locator(head, frozen_stages=7).train()
    assert autograd_bridge.unsupported_reason(m) is None
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        m.set_compute_dtype('bf16')
    assert m.backbone.compute_dtype == torch.float32 and m.set_compute_dtype('fp32') is m
    m.backbone.compute_dtype = torch.bfloat16
    assert 'MobileNetV2' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        (CprTrainer if head == 'cpr' else P2PTrainer)(m, two_streams=False)
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        m.backbone(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='MobileNetV2'):
        m.backbone.run_stage(3, torch.zeros(1, 4, 4, 32))


@pytest.mark.parametrize('rel', ['configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_1x_TinyPersonV2_640.py',
                                 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'], ids=['cpr', 'p2p'])
def test_shipped_configs_build_with_the_backbone_dict_switched(golden_dir, rel):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.backbones.mobilenet_v2 import MobileNetV2
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[rel])))
    assert cfg.model.backbone.type == 'ResNet'
    cfg.model['backbone'] = _wrap(dict(type='MobileNetV2', out_indices=(1, 2, 4, 7), frozen_stages=-1, norm_eval=True))
    cfg.model['neck']['in_channels'] = NECK_IN
    m = P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    assert type(m.backbone) is MobileNetV2 and list(m.neck.in_channels) == NECK_IN
    want = synthetic.mobilenet_v2_state_dict(0)
    got = {k: v for k, v in m.state_dict().items() if k.startswith('backbone.')}
    assert [(k, tuple(v.shape)) for k, v in got.items()] == [(k, tuple(v.shape)) for k, v in want.items()]


@pytest.mark.parametrize('name', MB.CASE_NAMES)
def test_fp64_restatement_matches_the_fixture_and_the_clamps_are_exercised(name):
    """The semantics restated in plain torch (tests/mobilenet_v2_ref.restated_forward), in fp64 on the case's weights and image, against
    the reference class's fp64 outputs; and the condition that makes the fixture a test of the clamp: every ReLU6 map of the case has at
    least 1 % of its elements at 6 and at least 1 % at 0."""
    cfg = MB.CASES[name]
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    maps = []
    with torch.no_grad():
        outs = MB.restated_forward(MB.case_state_dict(cfg, torch.float64), cfg, MB.case_input(cfg, torch.float64), maps)
    assert len(outs) == len(cfg['out_indices'])
    for l, o in enumerate(outs):
        assert MB.output_error(name, l, o) <= 1e-9
    assert len(maps) == 1 + 17 * 2 - 1 + 1          # the stem, expand (but layer1.0) and depthwise of 17 blocks, conv2
    for key, t in maps:
        at6, at0 = float((t == 6).double().mean()), float((t == 0).double().mean())
        assert at6 >= 0.01 and at0 >= 0.01, (name, key, at6, at0)


@pytest.mark.parametrize('shape', MB.SHAPES, ids=[MB.shape_id(s) for s in MB.SHAPES])
def test_kernel_test_inputs_have_few_threshold_elements(shape):
    """tests/test_gpu_mbv2_kernels.py: at most 0.5 % of the elements of a mask source or a clamped input lie within their own fp32
    rounding of 0 or 6 (there either branch would be admitted); the maps exercise both clamps where they have enough elements."""
    c = MB.make_case(shape, seed=5)
    for k in ('x', 'm'):
        assert MB.threshold_fraction(c[k]) <= 0.005
        if c[k].numel() >= 1024:
            assert float((c[k] > 6).double().mean()) >= 0.01 and float((c[k] == 0).double().mean()) >= 0.01
    assert abs(float(c['dy'].mean())) < 0.2      # zero-mean output gradients (tests/wgrad_fp64_ref.py says why)


@pytest.mark.parametrize('frozen', [-1, 3, 7])
@pytest.mark.parametrize('head', ['cpr', 'p2p'])
def test_trainers_build_and_order_every_trainable_parameter(head, frozen):
    """The bridge has no objection, the trainers build, and the flat order holds each trainable parameter once: conv2, then per block
    linear, depthwise, expand conv (the order their gradients complete in), the stem last."""
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    m = _locator(head, frozen_stages=frozen).train()
    assert autograd_bridge.unsupported_reason(m) is None
    tr = (CprTrainer if head == 'cpr' else P2PTrainer)(m, two_streams=False)
    names = {id(p): k for k, p in m.named_parameters()}
    order = [names[id(p)] for p in tr._backward_order()]
    assert sorted(order) == sorted(k for k, p in m.named_parameters() if p.requires_grad) and len(set(order)) == len(order)
    bb = [k for k in order if k.startswith('backbone.')]
    assert bb[:3] == ['backbone.conv2.conv.weight', 'backbone.conv2.bn.weight', 'backbone.conv2.bn.bias']
    if frozen == 7:
        assert len(bb) == 3
    else:
        assert bb[3] == 'backbone.layer7.0.linear_conv.conv.weight'
        blk = [k[len('backbone.layer6.1.'):] for k in bb if k.startswith('backbone.layer6.1.')]
        assert blk == ['%s.%s' % (mod, p) for mod in ('linear_conv', 'depthwise_conv', 'expand_conv')
                       for p in ('conv.weight', 'bn.weight', 'bn.bias')]
    if frozen == -1:
        assert bb[-6:] == ['backbone.layer1.0.depthwise_conv.conv.weight', 'backbone.layer1.0.depthwise_conv.bn.weight',
                           'backbone.layer1.0.depthwise_conv.bn.bias', 'backbone.conv1.conv.weight', 'backbone.conv1.bn.weight',
                           'backbone.conv1.bn.bias']
    else:
        assert not any(k.startswith('backbone.conv1.') for k in bb)


@pytest.mark.parametrize('which', ['shortcut', 'stride2', 'layer1'])
def test_backward_walk_order_with_torch_stand_ins(monkeypatch, which):
    """_mbv2_block_backward on a CPU block with every op replaced by a recorder: the launches come in the rule's order, the depthwise
    calls carry in_clamp6 / mask6 / colsum, the shortcut block adds dout to the expand conv's data gradient, and layer1.0 returns the
    pair (g1, column sums) for the stem."""
    from pointtinybenchmark_amd import layers, ops, training
    from pointtinybenchmark_amd.backbones import mobilenet_v2
    m = _build(norm_eval=True).train()
    blk = {'shortcut': m.layer2[1], 'stride2': m.layer3[0], 'layer1': m.layer1[0]}[which]
    I, M, O, s = blk.in_channels, blk.mid_channels, blk.out_channels, blk.stride
    Ip, Mp, Op = (ops.pad32(c) for c in (I, M, O))
    N, H, W = 1, 6, 8
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    calls = []

    def rec(name, ret):
        def f(*a, **k):
            calls.append((name, {key: (v is not None and v is not False) for key, v in k.items()
                                 if key in ('in_clamp6', 'mask6', 'colsum', 'add')}))
            return ret(*a, **k) if callable(ret) else ret
        return f
    monkeypatch.setattr(ops, 'relu6_bwd_colsum', rec('relu6_bwd_colsum', lambda dy, y=None, **k: (dy, torch.zeros(dy.shape[-1]))))
    monkeypatch.setattr(ops, 'dw_wgrad', rec('dw_wgrad', lambda g, x, C, stride, **k: k['out'].zero_()))
    monkeypatch.setattr(ops, 'dw_dgrad', rec('dw_dgrad', lambda g, pack, hw, stride, **k: (torch.zeros((N,) + tuple(hw) + (Mp,)), torch.ones(M))))
    monkeypatch.setattr(ops, 'bn_fold_bwd', rec('bn_fold_bwd', None))
    monkeypatch.setattr(mobilenet_v2, 'dw_dgrad_pack', lambda cache, conv, bn: 'PACK')
    monkeypatch.setattr(training, 'folded_bn', lambda cache, bn: (torch.ones(bn.num_features), torch.zeros(bn.num_features)))
    monkeypatch.setattr(training, 'bn_inv_sigma', lambda cache, bn: torch.ones(bn.num_features))
    eng = training.BackwardEngine.__new__(training.BackwardEngine)
    eng._sink, eng._redirect, eng.side, eng._mixed = {}, None, None, False
    inner = []
    monkeypatch.setattr(eng, '_padded_conv_bn_backward', lambda cache, conv, bn, g, cs, x, need_dx, add=None, **k:
                        inner.append((conv, tuple(cs.shape), add is not None)) or (torch.zeros(tuple(x.shape)) if need_dx else None),
                        raising=False)
    rcd = dict(x=torch.zeros(N, H, W, Ip), o1=torch.zeros(N, H, W, Mp), o2=torch.zeros(N, OH, OW, Mp), out=torch.zeros(N, OH, OW, Op))
    dx = eng._mbv2_block_backward(layers._PackCache(), blk, rcd, torch.zeros(N, OH, OW, Op), True)
    assert [c[0] for c in calls] == ['relu6_bwd_colsum', 'relu6_bwd_colsum', 'dw_wgrad', 'bn_fold_bwd', 'dw_dgrad']
    assert calls[2][1] == dict(in_clamp6=True) and calls[4][1] == dict(mask6=True, colsum=True)
    assert tuple(eng._sink[id(blk.depthwise_conv.conv.weight)].shape) == (M, 1, 3, 3)
    if which == 'layer1':
        assert isinstance(dx, tuple) and tuple(dx[0].shape) == (N, H, W, Mp) and tuple(dx[1].shape) == (M,)
        assert inner == [(blk.linear_conv.conv, (O,), False)]
    else:
        assert tuple(dx.shape) == (N, H, W, Ip)
        assert inner == [(blk.linear_conv.conv, (O,), False), (blk.expand_conv.conv, (M,), which == 'shortcut')]
    # a block whose input gradient nobody reads (the lowest trainable one): layer1.0 then skips its depthwise data gradient
    calls.clear()
    assert eng._mbv2_block_backward(layers._PackCache(), blk, rcd, torch.zeros(N, OH, OW, Op), False) is None
    assert ('dw_dgrad' in [c[0] for c in calls]) == (which != 'layer1')


def test_flag_values_agree_in_header_kernel_file_and_wrappers():
    """CPR_DW_IN_CLAMP6 / CPR_DW_RELU6: include/cpr_hip.h, their restatement in csrc/mbv2.hip (the kernels do not include the public
    header) and ops.DW_* hold the same values."""
    import re
    from pointtinybenchmark_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    found = []
    for rel in ('include/cpr_hip.h', 'pointtinybenchmark_amd/csrc/mbv2.hip'):
        with open(os.path.join(root, rel)) as f:
            found.append(dict(re.findall(r'^#define (CPR_DW_\w+) (\d+)', f.read(), flags=re.M)))
    assert found[0] == found[1] == dict(CPR_DW_IN_CLAMP6=str(ops.DW_IN_CLAMP6), CPR_DW_RELU6=str(ops.DW_RELU6))
