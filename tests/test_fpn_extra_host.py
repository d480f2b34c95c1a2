"""CPU: FPN extra pyramid levels (num_outs > laterals) -- what runs without a GPU.

  module     every fixture case builds; state-dict keys and shapes equal the reference class's (recorded in the fixture by
             tools/gen_fpn_extra_levels.py); the deprecated ``add_extra_convs=True`` forms resolve as the reference does;
             ``relu_before_extra_convs`` is kept; ``end_level`` with extras is refused
  config     the shipped P2P config with the multi-level values its comments name builds through config.Config and the
             autograd bridge admits it; a CPRHead on extras stays refused
  trainer    ``_backward_order`` lists every trainable parameter once, the extras' convs before the regular output convs
  fixture    tests/golden/fpn_extra_levels.npz covers every parameter and every input of every case
  reference  tests/fpn_extra_ref.fpn_forward (the fp64 restatement the whole-network GPU tests differentiate) against the fixture,
             outputs and gradients"""
import json
import os
import warnings

import pytest
import torch

from tests import fpn_extra_ref as FR

P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'


def _build(cfg):
    import pointtinybenchmark_amd as P
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        return P.build_neck(dict(type='FPN', **FR.fpn_kwargs(cfg)))


@pytest.mark.parametrize('name', FR.CASE_NAMES)
def test_fixture_case_builds_with_the_reference_state_dict_layout(name):
    cfg = FR.cases()[name]
    neck = _build(cfg)
    want = [(k, tuple(s)) for k, s in json.loads(str(FR.fixture()['keys:' + name]))]
    got = [(k, tuple(v.shape)) for k, v in neck.state_dict().items()]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    # strict loading in both directions: the synthetic weights are laid out as the reference class's
    sd = FR.case_state_dict(cfg, torch.float32)
    assert sorted(sd) == sorted(k for k, _ in want)
    neck.load_state_dict(sd, strict=True)
    L = len(cfg['in_channels']) - cfg.get('start_level', 0)
    assert neck.extra_levels == cfg['num_outs'] - L
    assert len(neck.fpn_convs) == (cfg['num_outs'] if cfg.get('add_extra_convs', False) else L)
    for cm in list(neck.fpn_convs)[L:]:
        assert cm.conv.stride == (2, 2) and cm.conv.padding == (1, 1) and cm.conv.bias is None and not cm.with_activation


def test_case_names_are_the_fixtures():
    assert sorted(FR.CASE_NAMES) == sorted(FR.cases())


def test_deprecated_true_forms_resolve_as_the_reference_does():
    import pointtinybenchmark_amd as P
    kw = dict(type='FPN', in_channels=[8, 16], out_channels=32, num_outs=3, norm_cfg=dict(type='GN', num_groups=4))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        n = P.build_neck(dict(kw, add_extra_convs=True))
    assert n.add_extra_convs == 'on_input' and n.fpn_convs[2].conv.in_channels == 16
    assert any(issubclass(x.category, DeprecationWarning) and 'extra_convs_on_inputs' in str(x.message) for x in w)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        n = P.build_neck(dict(kw, add_extra_convs=True, extra_convs_on_inputs=False))
    assert n.add_extra_convs == 'on_output' and n.fpn_convs[2].conv.in_channels == 32 and not w
    n = P.build_neck(dict(kw, add_extra_convs=False))
    assert n.add_extra_convs is False and len(n.fpn_convs) == 2 and n.extra_levels == 1
    with pytest.raises(AssertionError):
        P.build_neck(dict(kw, add_extra_convs='on_top'))


def test_relu_before_extra_convs_is_kept_and_end_level_with_extras_refused():
    import pointtinybenchmark_amd as P
    kw = dict(type='FPN', in_channels=[8, 16, 32], out_channels=32, norm_cfg=dict(type='GN', num_groups=4))
    assert P.build_neck(dict(kw, num_outs=5, add_extra_convs='on_output', relu_before_extra_convs=True)).relu_before_extra_convs is True
    assert P.build_neck(dict(kw, num_outs=5, add_extra_convs='on_output')).relu_before_extra_convs is False
    with pytest.raises(AssertionError):
        P.build_neck(dict(kw, num_outs=3, end_level=2, add_extra_convs='on_input'))
    assert len(P.build_neck(dict(kw, num_outs=2, end_level=2)).fpn_convs) == 2      # without extras end_level keeps working
    # what stays refused: non-GN laterals, no_norm_on_lateral, activated convs, a fixed upsampling scale
    for bad in (dict(norm_cfg=None), dict(no_norm_on_lateral=True), dict(act_cfg=dict(type='ReLU')),
                dict(upsample_cfg=dict(mode='nearest', scale_factor=2))):
        with pytest.raises(AssertionError):
            P.build_neck(dict(kw, num_outs=4, add_extra_convs='on_input', **bad))


def _shipped_p2p(golden_dir, **neck):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[P2P_CFG])))
    assert cfg.model.neck.add_extra_convs == 'on_input' and cfg.model.neck.num_outs == 1
    cfg.merge_from_dict({'model.neck.start_level': 1, 'model.neck.num_outs': 5, 'model.bbox_head.strides': [8, 16, 32, 64, 128]})
    cfg.merge_from_dict({'model.neck.' + k: v for k, v in neck.items()})
    return P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))


def test_shipped_p2p_config_with_its_multilevel_values_builds_and_trains_through_the_bridge(golden_dir):
    """start_level=1, num_outs=5, strides [8, 16, 32, 64, 128]: the variant the shipped config names in its comments."""
    from pointtinybenchmark_amd import autograd_bridge
    m = _shipped_p2p(golden_dir)
    assert m.neck.add_extra_convs == 'on_input' and m.neck.extra_levels == 2 and len(m.neck.fpn_convs) == 5
    assert tuple(m.neck.fpn_convs[3].conv.weight.shape) == (256, 2048, 3, 3)
    assert tuple(m.neck.fpn_convs[4].conv.weight.shape) == (256, 256, 3, 3)
    assert autograd_bridge.unsupported_reason(m) is None
    # max-pool extras: outputs are counted, not fpn_convs
    m = _shipped_p2p(golden_dir, add_extra_convs=False)
    assert len(m.neck.fpn_convs) == 3 and autograd_bridge.unsupported_reason(m) is None
    m.bbox_head.strides = [8, 16, 32]
    assert 'one FPN output per stride' in autograd_bridge.unsupported_reason(m)


def test_cpr_head_on_extra_levels_stays_refused():
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import autograd_bridge
    for extra in ('on_input', False):
        cfg = model_cfg(18, 1)
        cfg['neck'] = dict(cfg['neck'], num_outs=5, add_extra_convs=extra)
        assert 'num_outs == 1' in autograd_bridge.unsupported_reason(P.build_detector(cfg))


@pytest.mark.parametrize('extra', ['on_input', 'on_lateral', 'on_output', False])
def test_backward_order_lists_every_parameter_once_extras_before_the_output_convs(extra):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd.training import P2PTrainer
    cfg = p2p_model_cfg(18, 2)
    cfg['neck'] = dict(cfg['neck'], num_outs=6, add_extra_convs=extra)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16, 32, 64, 128])
    m = P.build_detector(cfg)
    shell = P2PTrainer.__new__(P2PTrainer)
    shell.model = m
    order = shell._backward_order()
    ids = [id(p) for p in order]
    assert len(set(ids)) == len(ids)
    assert set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
    pos = {i: n for n, i in enumerate(ids)}
    fpn = list(m.neck.fpn_convs)
    assert len(fpn) == (6 if extra else 4)
    head_last = max(pos[id(p)] for p in m.bbox_head.parameters())
    reg_first = min(pos[id(p)] for cm in fpn[:4] for p in cm.parameters())
    lat_first = min(pos[id(p)] for cm in m.neck.lateral_convs for p in cm.parameters())
    if extra:
        e5 = [pos[id(p)] for p in fpn[5].parameters()]
        e4 = [pos[id(p)] for p in fpn[4].parameters()]
        assert head_last < min(e5) and max(e5) < min(e4) and max(e4) < reg_first, 'head -> extras (last first) -> output convs'
    assert head_last < reg_first < lat_first
    for cm in fpn:      # each module's weight completes last (the rule calls _done on it)
        assert pos[id(cm.conv.weight)] > pos[id(cm.gn.weight)] and pos[id(cm.conv.weight)] > pos[id(cm.gn.bias)]


def test_fixture_covers_every_parameter_and_every_input_of_every_case():
    fx = FR.fixture()
    for name, cfg in FR.cases().items():
        neck = _build(cfg)
        s = cfg.get('start_level', 0)
        want = {n for n, _ in neck.named_parameters()} | {'in%d' % i for i in range(s, len(cfg['in_channels']))}
        assert set(FR.grad_names(name)) == want, (name, sorted(set(FR.grad_names(name)) ^ want))
        for k in want:
            assert float(fx['%s:norm:%s' % (name, k)]) > 0.5, (name, k)       # a linear functional: no degenerate gradients
            assert float(fx['%s:fp32:%s' % (name, k)]) <= 2e-3 / 4, (name, k)   # the conditioning the generator admitted
        shapes = FR.out_shapes(name)
        assert len(shapes) == cfg['num_outs'] and [sh[2:] for sh in shapes[-2:]] == ([(2, 3), (1, 2)] if cfg['num_outs'] - (4 - s) == 2
                                                                                     else [(4, 6), (2, 3)])
        for l in range(cfg['num_outs']):
            assert float(fx['%s:fp32:out%d' % (name, l)]) <= 2e-4 / 4, (name, l)
            if l >= 4 - s:
                assert '%s:out%d' % (name, l) in fx, 'every extra level is stored in full'


@pytest.mark.parametrize('name', FR.CASE_NAMES)
def test_fp64_restatement_matches_the_reference_class(name):
    """tests/fpn_extra_ref.fpn_forward in fp64 against the reference's own FPN class in fp64 (the fixture): the same formulas on
    both sides, bar 1e-9 relative on every output level and every gradient (norm and strided sample).
    Measured maximum over the eight cases: outputs 0 (bit-equal), gradient samples 6.7e-16, gradient norms 1.5e-16."""
    cfg = FR.cases()[name]
    sd = {k: v.requires_grad_(True) for k, v in FR.case_state_dict(cfg).items()}
    xs = [x.requires_grad_(True) for x in FR.case_inputs(cfg)]
    kw = {k: cfg[k] for k in FR.FPN_KEYS if k in cfg}
    outs = FR.fpn_forward(sd, xs, groups=cfg['groups'], **kw)
    assert [tuple(o.shape) for o in outs] == FR.out_shapes(name)
    worst_o = max(FR.output_error(name, l, o) for l, o in enumerate(outs))
    total = sum((FR.functional_weight(cfg, l, o.shape) * o).sum() for l, o in enumerate(outs))
    total.backward()
    got = dict(sd)
    got.update({'in%d' % i: x for i, x in enumerate(xs)})
    worst_n = worst_s = 0.0
    for k in FR.grad_names(name):
        en, es = FR.grad_errors(name, k, got[k].grad)
        worst_n, worst_s = max(worst_n, en), max(worst_s, es)
    print('ERR restatement %-18s outputs %.2e  grad norms %.2e  grad samples %.2e (bar 1e-9)' % (name, worst_o, worst_n, worst_s))
    assert worst_o <= 1e-9 and worst_n <= 1e-9 and worst_s <= 1e-9, (worst_o, worst_n, worst_s)
    for i in range(cfg.get('start_level', 0)):
        assert xs[i].grad is None
