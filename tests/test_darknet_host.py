"""Host: the Darknet backbone's layout, flags, refusals and parameter order, and the restatement of tests/darknet_ref.py against
tests/golden/darknet.npz (the reference's own class in fp64, tools/gen_darknet.py).  No device needed.

The flat parameter order of the new backward rule (CprTrainer._backward_order through BackwardEngine._darknet_units) is compared, for
three configurations, with the order written out here from the rule's statement: stages last first; per stage its ResBlocks last first,
each conv2 then conv1, then the stride-2 conv; conv1 of the net last; (conv.weight, bn.weight, bn.bias) per layer.  Whether a ready
point fires early under that order needs the device: the NaN-prefix check of tests/ready_point_check.py runs in
tests/test_gpu_darknet.py."""
import json

import pytest
import torch

from tests import darknet_ref as DR


def _darknet():
    from pointtinybenchmark_amd.backbones import Darknet
    return DR.add_small_arch(Darknet)


def _build(cfg, **kw):
    import pointtinybenchmark_amd as P
    _darknet()
    return P.build_backbone(dict(type='Darknet', **dict(DR.constructor_kwargs(cfg), **kw)))


def test_registered_and_exported():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import backbones
    from pointtinybenchmark_amd.registry import BACKBONES
    assert BACKBONES.get('Darknet') is backbones.Darknet
    assert 'Darknet' in P.__doc__
    m = P.build_backbone(dict(type='Darknet'))
    assert m.depth == 53 and m.out_indices == (3, 4, 5) and m.frozen_stages == -1 and m.norm_eval is True
    assert m.act_cfg == dict(type='LeakyReLU', negative_slope=0.1) and m.negative_slope == 0.1
    assert [m.stage_widths[i] for i in m.out_indices] == [256, 512, 1024]


@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_state_dict_keys_order_and_shapes_are_the_references(name):
    cfg = DR.CASES[name]
    m = _build(cfg)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == DR.archive_keys(name)
    sd = DR.case_state_dict(cfg)
    assert list(sd) == [k for k, _ in got]
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_archive_holds_the_cases_and_the_synthetic_layout_is_the_references():
    from pointtinybenchmark_amd import synthetic
    _darknet()
    a = DR.archive()
    assert json.loads(str(a['cases'])) == json.loads(json.dumps(DR.CASES))
    for name in DR.CASE_NAMES:
        worst = a[name + ':fp32:worst']
        assert worst[0] <= 2e-4 / 4 and worst[1] <= 2e-3 / 4      # the admission rule of tools/gen_darknet.py
        convs = [(k[:-len('.conv.weight')], s) for k, s in DR.archive_keys(name) if k.endswith('.conv.weight')]
        assert convs == synthetic.darknet_layout(DR.CASES[name]['depth'])


@pytest.mark.parametrize('fs', DR.FLAG_STAGES)
def test_train_and_freeze_flags_equal_the_recorded_ones(fs):
    m = _build(DR.CASES['small'], frozen_stages=fs)
    m.train()
    params, norms = json.loads(str(DR.archive()['flags:%d' % fs]))
    assert [[n, bool(p.requires_grad)] for n, p in m.named_parameters()] == params
    assert [[n, bool(b.training)] for n, b in m.named_modules() if isinstance(b, torch.nn.BatchNorm2d)] == norms
    frozen = [getattr(m, n) for n in m.cr_blocks[:max(fs, 0)]]
    assert all(not mod.training for mod in frozen) and len(frozen) == max(fs, 0)
    assert m.training and all(getattr(m, n).training for n in m.cr_blocks[max(fs, 0):])
    m.eval()
    assert not any(mod.training for mod in m.modules())


def test_norm_eval_false_leaves_the_trainable_norms_in_train_mode():
    m = _build(DR.CASES['small'], frozen_stages=2, norm_eval=False)
    m.train()
    assert not m.conv1.bn.training and not m.conv_res_block1.conv.bn.training and m.conv_res_block2.conv.bn.training
    assert m.batch_stats_active()
    m.eval()
    assert not m.batch_stats_active()


def test_init_weights_kaiming_convs_and_unit_norms():
    torch.manual_seed(0)
    m = _build(DR.CASES['small'])
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert bool((mod.weight == 1).all()) and bool((mod.bias == 0).all())
    w = m.conv_res_block5.conv.conv.weight      # (256, 128, 3, 3): fan_out = 256 * 9
    assert w.numel() > 1e5 and abs(float(w.detach().std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02


def test_unknown_depth_raises_the_references_key_error():
    with pytest.raises(KeyError) as e:
        _darknet()(depth=7)
    assert e.value.args[0] == str(DR.archive()['raises:depth']) == 'invalid depth 7 for darknet'


def test_arch_settings_extension_builds_and_bad_entries_are_refused():
    D = _darknet()
    m = D(depth=DR.SMALL_DEPTH, out_indices=(0, 2, 5))
    assert m.layers == DR.SMALL_ARCH[0] and m.stage_widths == [32, 64, 64, 128, 128, 256]
    bad = {91: ((1, 1), ((32, 64), (128, 128))),            # the chain is broken
           92: ((1, 1), ((16, 64), (64, 128))),             # does not start at 32
           93: ((1, 1), ((32, 96), (96, 128))),             # a width that is no multiple of 64
           94: ((1, 1, 1), ((32, 64), (64, 128)))}          # counts and pairs differ
    try:
        for depth, entry in bad.items():
            D.arch_settings[depth] = entry
            with pytest.raises(NotImplementedError, match='arch_settings'):
                D(depth=depth)
    finally:
        for depth in bad:
            D.arch_settings.pop(depth, None)


@pytest.mark.parametrize('kw, key', [
    (dict(act_cfg=dict(type='ReLU')), 'act_cfg'),
    (dict(act_cfg=None), 'act_cfg'),
    (dict(act_cfg=dict(type='LeakyReLU', negative_slope=1.0)), 'act_cfg'),
    (dict(act_cfg=dict(type='LeakyReLU', negative_slope=-0.1)), 'act_cfg'),
    (dict(conv_cfg=dict(type='ConvWS')), 'conv_cfg'),
    (dict(norm_cfg=dict(type='GN', num_groups=32)), 'norm_cfg'),
    (dict(norm_cfg=None), 'norm_cfg'),
])
def test_constructor_refusals_name_their_key(kw, key):
    with pytest.raises(NotImplementedError, match=key):
        _darknet()(depth=DR.SMALL_DEPTH, **kw)


def test_accepted_settings_build():
    D = _darknet()
    assert D(depth=DR.SMALL_DEPTH, act_cfg=dict(type='LeakyReLU', negative_slope=0.0)).negative_slope == 0.0
    assert isinstance(D(depth=DR.SMALL_DEPTH, norm_cfg=dict(type='SyncBN')).conv1.bn, torch.nn.SyncBatchNorm)
    assert D(depth=DR.SMALL_DEPTH, conv_cfg=dict(type='Conv2d')).conv_cfg == dict(type='Conv2d')
    m = D(depth=DR.SMALL_DEPTH, norm_cfg=dict(type='BN', requires_grad=False))
    assert not any(p.requires_grad for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d) for p in b.parameters())
    assert D(depth=DR.SMALL_DEPTH, norm_eval=False) is not None      # construction works; the refusal is the forward's


def _locator(head='p2p', num_outs=3, **bb_kw):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    _darknet()
    cfg = p2p_model_cfg(50, 1) if head == 'p2p' else model_cfg(50, 1, stride=8)
    cfg['backbone'] = dict(type='Darknet', **bb_kw)
    cfg['neck'] = dict(cfg['neck'], in_channels=[256, 512, 1024], num_outs=num_outs, add_extra_convs=False)
    if head == 'p2p':
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[8 << k for k in range(num_outs)])
    m = P.build_detector(cfg)
    m.train()
    return m


def test_bf16_is_refused_in_all_four_places_naming_darknet():
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import BackwardEngine, CprTrainer, P2PTrainer
    m = _locator('p2p')
    with pytest.raises(NotImplementedError, match='Darknet'):
        m.set_compute_dtype('bf16')
    assert m.backbone.compute_dtype == torch.float32
    m.backbone.compute_dtype = torch.bfloat16
    assert 'Darknet' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='Darknet'):
        m.backbone._check_mode()
    with pytest.raises(NotImplementedError, match='Darknet'):
        m.backbone.run(torch.zeros(1, 3, 32, 32))
    for cls in (BackwardEngine, P2PTrainer):
        with pytest.raises(NotImplementedError, match='Darknet'):
            cls(m)
    c = _locator('cpr', 1)
    c.backbone.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match='Darknet'):
        CprTrainer(c)


def test_batch_statistics_are_refused_naming_norm_eval():
    m = _build(DR.CASES['small'], norm_eval=False)
    m.train()
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='norm_eval'):
        m.run(torch.zeros(1, 3, 32, 32))


# ------------------------------------------------------------------------------------------------ the flat parameter order
def _expected_backbone_order(bb):
    """The rule's statement written out over parameter names (see the module docstring); frozen parameters left out."""
    names = []

    def layer(prefix):
        names.extend([prefix + '.conv.weight', prefix + '.bn.weight', prefix + '.bn.bias'])
    for i in range(max(bb.out_indices), 0, -1):
        for j in range(bb.layers[i - 1] - 1, -1, -1):
            layer('conv_res_block%d.res%d.conv2' % (i, j))
            layer('conv_res_block%d.res%d.conv1' % (i, j))
        layer('conv_res_block%d.conv' % i)
    layer('conv1')
    trainable = {k for k, p in bb.named_parameters() if p.requires_grad}
    return ['backbone.' + k for k in names if k in trainable]


@pytest.mark.parametrize('head, num_outs, bb_kw', [
    ('p2p', 3, dict(depth=53)),
    ('p2p', 3, dict(depth=53, frozen_stages=2)),
    ('cpr', 1, dict(depth=DR.SMALL_DEPTH, out_indices=(2, 5), frozen_stages=-1, norm_cfg=dict(type='BN', requires_grad=False))),
], ids=['d53_fs-1', 'd53_fs2', 'small_out25_frozen_norms'])
def test_flat_order_of_the_darknet_rule(head, num_outs, bb_kw):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    if bb_kw['depth'] == 53:
        m = _locator(head, num_outs, **bb_kw)
    else:
        _darknet()
        cfg = model_cfg(50, 1, stride=4)
        cfg['backbone'] = dict(type='Darknet', **bb_kw)
        cfg['neck'] = dict(cfg['neck'], in_channels=[64, 256], num_outs=1, add_extra_convs=False)
        m = P.build_detector(cfg)
        m.train()
    names = {id(p): k for k, p in m.named_parameters()}
    shell = object.__new__(P2PTrainer if head == 'p2p' else CprTrainer)
    shell.model = m
    order = [names[id(p)] for p in shell._backward_order()]
    trainable = [k for k, p in m.named_parameters() if p.requires_grad]
    assert len(set(order)) == len(order) and sorted(order) == sorted(trainable)
    bb_order = [k for k in order if k.startswith('backbone.')]
    assert bb_order == _expected_backbone_order(m.backbone)
    assert order[-len(bb_order):] == bb_order      # the backbone completes last, conv1 of the net at the very end
    if bb_kw.get('frozen_stages', -1) == 2:
        assert not any(k.startswith(('backbone.conv1.', 'backbone.conv_res_block1.')) for k in order)
    elif bb_kw['depth'] == 53:
        assert order[-3:] == ['backbone.conv1.conv.weight', 'backbone.conv1.bn.weight', 'backbone.conv1.bn.bias']
    else:      # frozen norms: the convs alone
        assert order[-1] == 'backbone.conv1.conv.weight' and not any('.bn.' in k for k in bb_order) and len(bb_order) == 18


# ------------------------------------------------------------------------------------------------ the restatement against the archive
@pytest.mark.parametrize('name', DR.CASE_NAMES)
def test_restatement_equals_the_fixture(name):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg = DR.CASES[name]
    outs, grads = DR.restated_case(cfg)
    assert len(outs) == len(cfg['out_indices'])
    for l, o in enumerate(outs):
        assert DR.output_error(name, l, o) <= 1e-12, (name, l)
    assert sorted(grads) == DR.grad_names(name)
    for k, g in grads.items():
        en, es = DR.grad_errors(name, k, g)
        assert en <= 1e-12 and es <= 1e-12, (name, k, en, es)
    frozen = DR.frozen_keys(cfg['depth'], cfg['frozen_stages'])
    assert (DR.STEM_IN in grads) == (cfg['frozen_stages'] < 1)
    assert not any(k.startswith(frozen) for k in grads) if frozen else len(grads) == 1 + sum(
        1 for k, _ in DR.archive_keys(name) if k.endswith(('.weight', '.bias')))
