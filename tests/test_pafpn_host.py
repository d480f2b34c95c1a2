"""CPU: the PAFPN neck (FPN + bottom-up path aggregation) -- what runs without a GPU.

  registry   ``dict(type='PAFPN', ...)`` resolves through the registry; the shipped P2P config with ``neck.type`` switched to 'PAFPN'
             builds through config.Config / build_detector and the autograd bridge admits it
  module     every fixture case builds; state-dict keys and shapes equal the reference class's (recorded in the fixture by
             tools/gen_pafpn.py); strict loading both ways
  refusals   everything FPN refuses; ``num_outs`` below the level count (the reference cannot run it); a CPRHead on several PAFPN
             levels (unsupported_reason and CprTrainer, naming the level count); a single-level PAFPN has empty module lists
  trainer    ``_backward_order`` lists every trainable parameter once, in the order _backward_pafpn finishes them
  reference  tests/pafpn_ref.pafpn_forward (the fp64 restatement the whole-network GPU tests differentiate) against the fixture
  walk       PAFPN's own forward / forward_lazy / taped forward with torch stand-ins for the HIP ops: the tape's kinds and levels, and
             the walk's outputs against the fixture"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import pafpn_ref as PR

P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'


def _build(cfg):
    import pointtinybenchmark_amd as P
    return P.build_neck(dict(type='PAFPN', **PR.neck_kwargs(cfg)))


def test_registry_knows_pafpn_and_exports_it():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.necks import FPN, PAFPN
    assert P.PAFPN is PAFPN and issubclass(PAFPN, FPN)
    n = P.build_neck(dict(type='PAFPN', in_channels=[8, 16, 32], out_channels=32, num_outs=3, norm_cfg=dict(type='GN', num_groups=4)))
    assert type(n) is PAFPN and len(n.downsample_convs) == len(n.pafpn_convs) == 2 and len(n.fpn_convs) == 3


def test_shipped_p2p_config_with_a_pafpn_neck_builds_and_the_bridge_admits_it(golden_dir):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[P2P_CFG])))
    cfg.merge_from_dict({'model.neck.type': 'PAFPN', 'model.neck.start_level': 1, 'model.neck.num_outs': 5,
                         'model.bbox_head.strides': [8, 16, 32, 64, 128]})
    m = P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    assert type(m.neck).__name__ == 'PAFPN' and m.neck.extra_levels == 2 and len(m.neck.fpn_convs) == 5
    assert len(m.neck.downsample_convs) == len(m.neck.pafpn_convs) == 2
    assert tuple(m.neck.downsample_convs[0].conv.weight.shape) == (256, 256, 3, 3) and m.neck.downsample_convs[0].conv.stride == (2, 2)
    assert autograd_bridge.unsupported_reason(m) is None
    m.bbox_head.strides = [8, 16, 32]
    assert 'one FPN output per stride' in autograd_bridge.unsupported_reason(m)


def test_case_names_are_the_fixtures():
    assert sorted(PR.CASE_NAMES) == sorted(PR.cases())


@pytest.mark.parametrize('name', PR.CASE_NAMES)
def test_fixture_case_builds_with_the_reference_state_dict_layout(name):
    cfg = PR.cases()[name]
    neck = _build(cfg)
    want = [(k, tuple(s)) for k, s in json.loads(str(PR.fixture()['keys:' + name]))]
    got = [(k, tuple(v.shape)) for k, v in neck.state_dict().items()]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    sd = PR.case_state_dict(cfg, torch.float32)
    assert sorted(sd) == sorted(k for k, _ in want)
    neck.load_state_dict(sd, strict=True)                       # reference layout -> the class
    assert sorted(neck.state_dict()) == sorted(sd)              # and back
    L = len(cfg['in_channels']) - cfg.get('start_level', 0)
    assert len(neck.downsample_convs) == len(neck.pafpn_convs) == L - 1 and neck.extra_levels == cfg['num_outs'] - L
    for cm in neck.downsample_convs:
        assert cm.conv.stride == (2, 2) and cm.conv.padding == (1, 1) and cm.conv.bias is None and not cm.with_activation
    for cm in neck.pafpn_convs:
        assert cm.conv.stride == (1, 1) and cm.conv.padding == (1, 1) and cm.conv.bias is None and not cm.with_activation


def test_fixture_covers_every_parameter_and_every_input_of_every_case():
    fx = PR.fixture()
    for name, cfg in PR.cases().items():
        neck = _build(cfg)
        s = cfg.get('start_level', 0)
        want = {n for n, _ in neck.named_parameters()} | {'in%d' % i for i in range(s, len(cfg['in_channels']))}
        assert set(PR.grad_names(name)) == want, (name, sorted(set(PR.grad_names(name)) ^ want))
        for k in want:
            assert float(fx['%s:norm:%s' % (name, k)]) > 0.5, (name, k)
            assert float(fx['%s:fp32:%s' % (name, k)]) <= 2e-3 / 4, (name, k)   # the conditioning the generator admitted
        for l in range(cfg['num_outs']):
            assert float(fx['%s:fp32:out%d' % (name, l)]) <= 2e-4 / 4, (name, l)


def test_xavier_init_covers_the_bottom_up_convs():
    torch.manual_seed(0)
    n = _build(PR.cases()['pa4'])
    for cm in list(n.downsample_convs) + list(n.pafpn_convs):
        w = cm.conv.weight
        bound = (6.0 / (w.shape[1] * 9 + w.shape[0] * 9)) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
        assert bool((cm.gn.weight == 1).all()) and bool((cm.gn.bias == 0).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    import pointtinybenchmark_amd as P
    kw = dict(type='PAFPN', in_channels=[8, 16, 32], out_channels=32, norm_cfg=dict(type='GN', num_groups=4))
    with pytest.raises(AssertionError, match='num_outs'):
        P.build_neck(dict(kw, num_outs=2))
    with pytest.raises(AssertionError, match='num_outs'):
        P.build_neck(dict(kw, num_outs=1, start_level=1))
    # everything FPN refuses stays refused
    for bad in (dict(norm_cfg=None), dict(norm_cfg=dict(type='BN')), dict(no_norm_on_lateral=True), dict(act_cfg=dict(type='ReLU')),
                dict(add_extra_convs='on_top'), dict(end_level=3, num_outs=4)):
        with pytest.raises(AssertionError):
            P.build_neck(dict(dict(kw, num_outs=3), **bad))
    assert len(P.build_neck(dict(kw, num_outs=2, end_level=2)).pafpn_convs) == 1      # end_level without extras keeps working


def test_single_level_pafpn_has_no_bottom_up_modules():
    import pointtinybenchmark_amd as P
    n = P.build_neck(dict(type='PAFPN', in_channels=[8, 16, 32], out_channels=32, num_outs=1, start_level=2,
                          norm_cfg=dict(type='GN', num_groups=4)))
    assert len(n.downsample_convs) == 0 and len(n.pafpn_convs) == 0 and len(n.fpn_convs) == 1
    f = P.build_neck(dict(type='FPN', in_channels=[8, 16, 32], out_channels=32, num_outs=1, start_level=2,
                          norm_cfg=dict(type='GN', num_groups=4)))
    assert sorted(n.state_dict()) == sorted(f.state_dict())


def test_cpr_head_on_several_pafpn_levels_is_reported_and_refused():
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = model_cfg(18, 1)
    cfg['neck'] = dict(cfg['neck'], type='PAFPN', num_outs=4)
    m = P.build_detector(cfg)
    why = autograd_bridge.unsupported_reason(m)
    assert 'PAFPN' in why and '4 output levels' in why
    with pytest.raises(NotImplementedError, match='4 output levels'):
        CprTrainer(m)
    # one level: a PAFPN that is FPN itself is admitted
    cfg['neck'] = dict(cfg['neck'], start_level=3, num_outs=1)
    assert autograd_bridge.unsupported_reason(P.build_detector(cfg)) is None


# ------------------------------------------------------------------------------------------------ trainer order
@pytest.mark.parametrize('extra', ['on_input', 'on_lateral', 'on_output', False])
def test_backward_order_lists_every_parameter_once_in_the_bottom_up_paths_reverse(extra):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd.training import P2PTrainer
    cfg = p2p_model_cfg(18, 2)
    cfg['neck'] = dict(cfg['neck'], type='PAFPN', num_outs=6, add_extra_convs=extra)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16, 32, 64, 128])
    m = P.build_detector(cfg)
    shell = P2PTrainer.__new__(P2PTrainer)
    shell.model = m
    order = shell._backward_order()
    ids = [id(p) for p in order]
    assert len(set(ids)) == len(ids)
    assert set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
    pos = {i: n for n, i in enumerate(ids)}
    neck = m.neck

    def last(cm):
        assert pos[id(cm.conv.weight)] > pos[id(cm.gn.weight)] and pos[id(cm.conv.weight)] > pos[id(cm.gn.bias)]
        return pos[id(cm.conv.weight)]
    want = [neck.pafpn_convs[2], neck.fpn_convs[3], neck.pafpn_convs[1], neck.downsample_convs[2], neck.fpn_convs[2],
            neck.pafpn_convs[0], neck.downsample_convs[1], neck.fpn_convs[1], neck.downsample_convs[0], neck.fpn_convs[0]]
    seq = [last(cm) for cm in want]
    assert seq == sorted(seq), seq
    head_last = max(pos[id(p)] for p in m.bbox_head.parameters())
    lat_first = min(pos[id(p)] for cm in neck.lateral_convs for p in cm.parameters())
    extras = [last(cm) for cm in list(neck.fpn_convs)[4:]]
    assert head_last < min(extras + seq) and seq[-1] < lat_first, 'head -> extras -> bottom-up path in reverse -> laterals'
    if extras:
        assert max(extras) < seq[0] and extras == sorted(extras, reverse=True), 'the extras, last first, before the regular levels'


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', PR.CASE_NAMES)
def test_fp64_restatement_matches_the_reference_class(name):
    """tests/pafpn_ref.pafpn_forward in fp64 against the reference's own PAFPN class in fp64 (the fixture): the same formulas on both
    sides, bar 1e-9 relative on every output level and every gradient (norm and strided sample)."""
    cfg = PR.cases()[name]
    sd = {k: v.requires_grad_(True) for k, v in PR.case_state_dict(cfg).items()}
    xs = [x.requires_grad_(True) for x in PR.case_inputs(cfg)]
    outs = PR.pafpn_forward(sd, xs, **PR.forward_kwargs(cfg))
    assert [tuple(o.shape) for o in outs] == PR.out_shapes(name)
    worst_o = max(PR.output_error(name, l, o) for l, o in enumerate(outs))
    total = sum((PR.functional_weight(cfg, l, o.shape) * o).sum() for l, o in enumerate(outs))
    total.backward()
    got = dict(sd)
    got.update({'in%d' % i: x for i, x in enumerate(xs)})
    worst_n = worst_s = 0.0
    for k in PR.grad_names(name):
        en, es = PR.grad_errors(name, k, got[k].grad)
        worst_n, worst_s = max(worst_n, en), max(worst_s, es)
    print('ERR restatement %-20s outputs %.2e  grad norms %.2e  grad samples %.2e (bar 1e-9)' % (name, worst_o, worst_n, worst_s))
    assert worst_o <= 1e-9 and worst_n <= 1e-9 and worst_s <= 1e-9, (worst_o, worst_n, worst_s)
    for i in range(cfg.get('start_level', 0)):
        assert xs[i].grad is None


# ------------------------------------------------------------------------------------------------ the walk, HIP ops replaced
@pytest.fixture
def torch_ops(monkeypatch):
    """Torch stand-ins (fp64-capable, CPU) for the HIP entry points the neck's walk calls: what is under test is the walk itself."""
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.necks import fpn, pafpn

    def conv_gn(cache, m, x, in_ab=None, in_relu=False, materialize=True, up=None, save=None, consume_input=False, out_b8=False):
        assert in_ab is None and not out_b8
        raw = F.conv2d(x.permute(0, 3, 1, 2), m.conv.weight, None, m.conv.stride, m.conv.padding).permute(0, 2, 3, 1).contiguous()
        N, C = raw.shape[0], raw.shape[3]
        g = m.gn.num_groups
        r = raw.reshape(N, -1, g, C // g)
        mean, var = r.mean((1, 3)), r.var((1, 3), unbiased=False)
        rstd = (var + m.gn.eps).rsqrt()
        a = rstd.repeat_interleave(C // g, 1) * m.gn.weight
        b = m.gn.bias - mean.repeat_interleave(C // g, 1) * a
        if save is not None:
            save.update(module=m, x=x, in_ab=None, in_relu=False, raw=raw, a=a, b=b, mean=mean, rstd=rstd)
        if not materialize:
            return raw, (a, b)
        return gn_apply(raw, a, b, up=up)

    def gn_apply(x, a, b, relu=False, up=None, out=None):
        y = x * a[:, None, None, :] + b[:, None, None, :]
        if relu:
            y = y.clamp_min(0)
        if up is not None:
            y = y + F.interpolate(up.permute(0, 3, 1, 2), size=x.shape[1:3], mode='nearest').permute(0, 2, 3, 1)
        return y

    def gn_apply2(x1, a1, b1, x2, a2, b2, out=None):
        return gn_apply(x1, a1, b1) + gn_apply(x2, a2, b2)
    monkeypatch.setattr(fpn, 'conv_gn', conv_gn)
    monkeypatch.setattr(pafpn, 'conv_gn', conv_gn)
    monkeypatch.setattr(ops, 'gn_apply', gn_apply)
    monkeypatch.setattr(ops, 'gn_apply2', gn_apply2)
    monkeypatch.setattr(ops, 'subsample2', lambda x, a=None, b=None: x[:, ::2, ::2].contiguous())
    monkeypatch.setattr(ops, 'from_nchw', lambda x: x.permute(0, 2, 3, 1).contiguous())
    monkeypatch.setattr(ops, 'as_nchw', lambda x: x.permute(0, 3, 1, 2))


@pytest.mark.parametrize('name', PR.CASE_NAMES)
def test_walk_tape_kinds_levels_and_outputs(name, torch_ops):
    cfg = PR.cases()[name]
    neck = _build(cfg).double()
    neck.load_state_dict(PR.case_state_dict(cfg), strict=True)
    xs = PR.case_inputs(cfg)
    L = len(cfg['in_channels']) - cfg.get('start_level', 0)
    with torch.no_grad():
        outs = neck(xs)
        tape = []
        lazy = neck.forward_lazy(xs, tape=tape)
        lazy_plain = neck.forward_lazy(xs)
    assert len(outs) == len(lazy) == len(lazy_plain) == cfg['num_outs']
    for l, o in enumerate(outs):
        assert PR.output_error(name, l, o) <= 1e-9, (name, l)
        for raw, (a, b) in (lazy[l], lazy_plain[l]):
            y = (raw * a[:, None, None, :] + b[:, None, None, :]).permute(0, 3, 1, 2)
            assert PR.output_error(name, l, y) <= 1e-9, (name, l)
    kinds = [(r['kind'], r['level']) for r in tape]
    want = [('lateral', i) for i in range(L - 1, -1, -1)] + [('out', i) for i in range(L)]
    for i in range(L - 1):
        want += [('down', i), ('pa_out', i + 1)]
    extra = cfg.get('add_extra_convs', False)
    want += [('extra' if extra else 'pool', L + k) for k in range(cfg['num_outs'] - L)]
    assert kinds == want, kinds
    by = {(r['kind'], r['level']): r for r in tape}
    for i in range(L - 1):
        assert by['down', i]['module'] is neck.downsample_convs[i] and by['pa_out', i + 1]['module'] is neck.pafpn_convs[i]
        # the stride-2 conv reads the MATERIALISED sum of its level, the pafpn conv the materialised sum above it
        assert by['down', i]['in_ab'] is None and by['down', i]['x'].shape[1:3] == by['out', i]['raw'].shape[1:3]
        assert by['pa_out', i + 1]['x'].shape == by['out', i + 1]['raw'].shape
        for k in ('x', 'raw', 'a', 'b', 'mean', 'rstd'):
            assert by['down', i][k] is not None and by['pa_out', i + 1][k] is not None
    # lazy level 0 is fpn_convs[0]'s own raw map and affine; level i >= 1 pafpn_convs[i-1]'s
    assert lazy[0][0] is by['out', 0]['raw'] and all(lazy[i][0] is by['pa_out', i]['raw'] for i in range(1, L))
