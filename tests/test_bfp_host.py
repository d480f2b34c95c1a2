"""CPU: the BFP neck (Balanced Feature Pyramid) and the list-valued neck it comes in -- what runs without a GPU.

  registry   ``dict(type='BFP', ...)`` and ``neck=[dict(type='FPN', ...), dict(type='BFP', ...)]`` resolve through the registry; the shipped
             P2P config with such a neck builds through config.Config / build_detector and the autograd bridge admits it
  module     every fixture case builds; state-dict keys and shapes equal the reference class's, those of the list neck the reference's
             ``Sequential(FPN, BFP)`` (both recorded in the fixture by tools/gen_bfp.py); strict loading both ways
  refusals   refine_type='non_local', a non-GN refine norm, a conv_cfg other than Conv2d: NotImplementedError naming the key; chains other
             than [FPN | PAFPN, BFP]; a BFP that does not fit the neck in front of it; a CPRHead behind a BFP (bridge and CprTrainer)
  trainer    ``_backward_order`` lists every trainable parameter once, the refine layer between the head and the inner neck
  reference  tests/bfp_ref.bfp_forward (the fp64 restatement the GPU tests differentiate) against the fixture, 1e-9
  indices    the host form of the kernels' nearest rule against F.interpolate for EVERY pair in <= 96, out <= 128, the integer rule it
             must not be; the window rule against F.adaptive_max_pool2d(return_indices=True), ties included
  walk       BFP.run / NeckSequence with torch stand-ins for the HIP ops: tape kinds, lazy == forward, outputs against the fixture"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bfp_ref as BR

P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'
GN = dict(type='GN', num_groups=32)


def _build(cfg):
    import pointtinybenchmark_amd as P
    return P.build_neck(dict(type='BFP', **BR.neck_kwargs(cfg)))


def _list_neck(refine_type='conv', inner='FPN', **bfp):
    seq = json.loads(str(BR.fixture()['sequential_cfg']))
    return [dict(seq['fpn'], type=inner), dict(dict(seq['bfp'], refine_type=refine_type, **bfp), type='BFP')]


def test_registry_knows_bfp_and_a_list_valued_neck():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.necks import BFP, FPN, PAFPN, NeckSequence
    assert P.BFP is BFP and P.NeckSequence is NeckSequence
    n = P.build_neck(dict(type='BFP', in_channels=64, num_levels=5, refine_level=1, refine_type='conv', norm_cfg=GN))
    assert type(n) is BFP and tuple(n.refine.conv.weight.shape) == (64, 64, 3, 3) and n.refine.with_activation
    for inner, cls in (('FPN', FPN), ('PAFPN', PAFPN)):
        s = P.build_neck(_list_neck(inner=inner))
        assert isinstance(s, NeckSequence) and isinstance(s, torch.nn.Sequential)
        assert type(s.inner) is cls and type(s.bfp) is BFP and s[0] is s.inner and s[1] is s.bfp
    # a dict-valued neck is what it was
    assert type(P.build_neck(_list_neck()[0])) is FPN


def test_shipped_p2p_config_with_a_list_neck_builds_and_the_bridge_admits_it(golden_dir):
    import pointtinybenchmark_amd as P
    from oracle.gen_golden_configs import decode
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.config import Config, _wrap
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        cfg = Config(_wrap(decode(json.load(f)[P2P_CFG])))
    fpn = dict(cfg.model.neck)
    fpn.update(start_level=1, num_outs=5, add_extra_convs='on_input')
    cfg.model['neck'] = [fpn, dict(type='BFP', in_channels=256, num_levels=5, refine_level=1, refine_type='conv', norm_cfg=GN)]
    cfg.merge_from_dict({'model.bbox_head.strides': [8, 16, 32, 64, 128]})
    m = P.build_detector(cfg.model, train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    assert type(m.neck).__name__ == 'NeckSequence' and m.neck.inner.extra_levels == 2 and m.neck.bfp.num_levels == 5
    assert tuple(m.neck.bfp.refine.conv.weight.shape) == (256, 256, 3, 3)
    assert {'neck.0.lateral_convs.0.conv.weight', 'neck.1.refine.conv.weight', 'neck.1.refine.gn.bias'} <= set(m.state_dict())
    assert autograd_bridge.unsupported_reason(m) is None
    m.bbox_head.strides = [8, 16, 32]
    assert 'one FPN output per stride' in autograd_bridge.unsupported_reason(m)


def test_case_names_are_the_fixtures():
    assert sorted(BR.CASE_NAMES) == sorted(BR.cases())


@pytest.mark.parametrize('name', BR.CASE_NAMES)
def test_fixture_case_builds_with_the_reference_state_dict_layout(name):
    cfg = BR.cases()[name]
    neck = _build(cfg)
    want = [(k, tuple(s)) for k, s in json.loads(str(BR.fixture()['keys:' + name]))]
    got = [(k, tuple(v.shape)) for k, v in neck.state_dict().items()]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    assert (got == []) == (cfg['refine_type'] is None)
    sd = BR.case_state_dict(cfg, torch.float32)
    assert sorted(sd) == sorted(k for k, _ in want)
    neck.load_state_dict(sd, strict=True)                       # reference layout -> the class
    assert sorted(neck.state_dict()) == sorted(sd)              # and back


def test_list_neck_has_the_reference_sequentials_state_dict_layout():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import synthetic
    neck = P.build_neck(_list_neck())
    want = [(k, tuple(s)) for k, s in json.loads(str(BR.fixture()['keys:sequential']))]
    got = [(k, tuple(v.shape)) for k, v in neck.state_dict().items()]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    assert any(k.startswith('0.') for k, _ in got) and any(k.startswith('1.refine.') for k, _ in got)
    seq = json.loads(str(BR.fixture()['sequential_cfg']))
    sd = synthetic.fpn_state_dict(seq['fpn']['in_channels'], 64, 1, 5, seed=3, prefix='0.', add_extra_convs='on_input')
    sd.update(synthetic.bfp_state_dict(64, 'conv', seed=3, prefix='1.'))
    assert sorted(sd) == sorted(k for k, _ in want)
    neck.load_state_dict(sd, strict=True)
    assert sorted(neck.state_dict()) == sorted(sd)
    assert synthetic.bfp_state_dict(64, None) == {}


def test_fixture_covers_every_parameter_and_input_and_admits_no_argmax_flip():
    fx = BR.fixture()
    for name, cfg in BR.cases().items():
        neck = _build(cfg)
        want = {n for n, _ in neck.named_parameters()} | {'in%d' % i for i in range(cfg['num_levels'])}
        assert set(BR.grad_names(name)) == want, (name, sorted(set(BR.grad_names(name)) ^ want))
        for k in want:
            assert float(fx['%s:norm:%s' % (name, k)]) > 0.5, (name, k)
            assert float(fx['%s:fp32:%s' % (name, k)]) <= 2e-3 / 4, (name, k)   # the conditioning the generator admitted
        for l in range(cfg['num_levels']):
            assert float(fx['%s:fp32:out%d' % (name, l)]) <= 2e-4 / 4, (name, l)
        assert float(fx[name + ':pool_gap']) >= 8 * float(fx[name + ':pool_dev']), name


def test_xavier_init_covers_the_refine_conv():
    torch.manual_seed(0)
    n = _build(BR.cases()['l5_r1_conv'])
    w = n.refine.conv.weight.detach()
    bound = (6.0 / (w.shape[1] * 9 + w.shape[0] * 9)) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    assert bool((n.refine.gn.weight == 1).all()) and bool((n.refine.gn.bias == 0).all()) and n.refine.conv.bias is None


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals_name_their_key():
    import pointtinybenchmark_amd as P
    kw = dict(type='BFP', in_channels=64, num_levels=4, refine_level=1)
    with pytest.raises(NotImplementedError, match='non_local'):
        P.build_neck(dict(kw, refine_type='non_local', norm_cfg=GN))
    for norm in (None, dict(type='BN')):
        with pytest.raises(NotImplementedError, match='norm_cfg'):
            P.build_neck(dict(kw, refine_type='conv', norm_cfg=norm))
    with pytest.raises(NotImplementedError, match='conv_cfg'):
        P.build_neck(dict(kw, refine_type='conv', norm_cfg=GN, conv_cfg=dict(type='DCN')))
    with pytest.raises(AssertionError):
        P.build_neck(dict(kw, refine_level=4))
    with pytest.raises(AssertionError):
        P.build_neck(dict(kw, refine_type='mean'))
    # refine_type None takes no norm; a plain Conv2d conv_cfg is the default
    assert sorted(P.build_neck(dict(kw)).state_dict()) == []
    assert len(P.build_neck(dict(kw, refine_type='conv', norm_cfg=GN, conv_cfg=dict(type='Conv2d'))).state_dict()) == 3


def test_list_necks_other_than_fpn_then_bfp_are_refused():
    import pointtinybenchmark_amd as P
    fpn, bfp = _list_neck()
    for bad in ([fpn], [bfp, fpn], [fpn, fpn], [fpn, bfp, bfp], [bfp]):
        with pytest.raises(NotImplementedError, match='FPN'):
            P.build_neck(bad)
    with pytest.raises(ValueError, match='num_levels'):
        P.build_neck([fpn, dict(bfp, num_levels=4)])
    with pytest.raises(ValueError, match='in_channels'):
        P.build_neck([fpn, dict(bfp, in_channels=128)])
    with pytest.raises(TypeError):
        P.build_neck('FPN')


def test_cpr_head_behind_a_bfp_is_reported_and_refused():
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = model_cfg(18, 1)
    assert autograd_bridge.unsupported_reason(P.build_detector(cfg)) is None
    n_outs = cfg['neck']['num_outs']
    cfg['neck'] = [cfg['neck'], dict(type='BFP', in_channels=cfg['neck']['out_channels'], num_levels=n_outs, refine_level=0)]
    m = P.build_detector(cfg)
    why = autograd_bridge.unsupported_reason(m)
    assert 'CPRHead' in why and 'BFP' in why
    with pytest.raises(NotImplementedError, match='BFP'):
        CprTrainer(m)


# ------------------------------------------------------------------------------------------------ trainer order
@pytest.mark.parametrize('inner,refine', [('FPN', 'conv'), ('PAFPN', 'conv'), ('FPN', None)])
def test_backward_order_lists_every_parameter_once_with_the_refine_layer_before_the_inner_neck(inner, refine):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd.training import P2PTrainer
    cfg = p2p_model_cfg(18, 2)
    fpn = dict(cfg['neck'], type=inner, num_outs=6, add_extra_convs='on_output')
    cfg['neck'] = [fpn, dict(type='BFP', in_channels=fpn['out_channels'], num_levels=6, refine_level=2, refine_type=refine, norm_cfg=GN)]
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16, 32, 64, 128])
    m = P.build_detector(cfg)
    shell = P2PTrainer.__new__(P2PTrainer)
    shell.model = m
    order = shell._backward_order()
    ids = [id(p) for p in order]
    assert len(set(ids)) == len(ids)
    assert set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
    pos = {i: n for n, i in enumerate(ids)}
    head_last = max(pos[id(p)] for p in m.bbox_head.parameters())
    inner_first = min(pos[id(p)] for p in m.neck.inner.parameters())
    if refine is None:
        assert head_last + 1 == inner_first
        return
    r = m.neck.bfp.refine
    got = [pos[id(r.gn.weight)], pos[id(r.gn.bias)], pos[id(r.conv.weight)]]
    assert got == [head_last + 1, head_last + 2, head_last + 3] and inner_first == head_last + 4, 'head -> refine (conv last) -> inner neck'


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', BR.CASE_NAMES)
def test_fp64_restatement_matches_the_reference_class(name):
    """tests/bfp_ref.bfp_forward in fp64 against the reference's own BFP class in fp64 (the fixture): the same formulas on both sides,
    bar 1e-9 relative on every output level and every gradient (norm and strided sample)."""
    cfg = BR.cases()[name]
    sd = {k: v.requires_grad_(True) for k, v in BR.case_state_dict(cfg).items()}
    xs = [x.requires_grad_(True) for x in BR.case_inputs(cfg)]
    outs = BR.bfp_forward(sd, xs, **BR.forward_kwargs(cfg))
    assert [tuple(o.shape) for o in outs] == BR.out_shapes(name)
    worst_o = max(BR.output_error(name, l, o) for l, o in enumerate(outs))
    total = sum((BR.functional_weight(cfg, l, o.shape) * o).sum() for l, o in enumerate(outs))
    total.backward()
    got = dict(sd)
    got.update({'in%d' % i: x for i, x in enumerate(xs)})
    worst_n = worst_s = 0.0
    for k in BR.grad_names(name):
        en, es = BR.grad_errors(name, k, got[k].grad)
        worst_n, worst_s = max(worst_n, en), max(worst_s, es)
    print('ERR restatement %-14s outputs %.2e  grad norms %.2e  grad samples %.2e (bar 1e-9)' % (name, worst_o, worst_n, worst_s))
    assert worst_o <= 1e-9 and worst_n <= 1e-9 and worst_s <= 1e-9, (worst_o, worst_n, worst_s)


# ------------------------------------------------------------------------------------------------ the index rules
def test_host_nearest_rule_is_torchs_for_every_pair():
    """ops.nearest_index (the fp32 scale of ops.nearest_scale, what the kernels are handed) against F.interpolate(mode='nearest') for
    every (in <= 96, out <= 128); the integer rule dst * in // out must differ somewhere (it does for in=2, out=82)."""
    from pointtinybenchmark_amd import ops
    wrong_int = 0
    for n_in in range(1, 97):
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        for n_out in range(1, 129):
            want = F.interpolate(src, size=(1, n_out), mode='nearest').reshape(-1).long().numpy()
            got = ops.nearest_index(n_in, n_out)
            assert np.array_equal(got, want), (n_in, n_out)
            wrong_int += int(not np.array_equal(np.arange(n_out) * n_in // n_out, want))
    assert wrong_int > 0
    assert not np.array_equal(np.arange(82) * 2 // 82, ops.nearest_index(2, 82))
    assert not np.array_equal(np.arange(74) * 6 // 74, ops.nearest_index(6, 74))
    assert ops.nearest_scale(6, 74) == float(np.float32(6) / np.float32(74))
    # the fp64 restatement follows the fp32 rule on those axes too (torch's fp64 contiguous path does not)
    x = torch.arange(2 * 6 * 2, dtype=torch.float64).reshape(1, 2, 6, 2)
    assert torch.equal(BR.nearest(x, (74, 82)), F.interpolate(x.float(), size=(74, 82), mode='nearest').double())


def _window_argmax(x, size):
    """adaptive_max_pool2d of a (H, W) map by the project's window rule: first maximum in row-major order -> (values, flat indices)."""
    from pointtinybenchmark_amd import ops
    H, W = x.shape
    val, idx = torch.empty(size, dtype=x.dtype), torch.empty(size, dtype=torch.long)
    for i, (y0, y1) in enumerate(ops.adaptive_windows(H, size[0])):
        for j, (x0, x1) in enumerate(ops.adaptive_windows(W, size[1])):
            best, at = None, None
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    if best is None or x[yy, xx] > best:
                        best, at = x[yy, xx], yy * W + xx
            val[i, j], idx[i, j] = best, at
    return val, idx


@pytest.mark.parametrize('hw,size', [((7, 7), (3, 3)), ((25, 42), (13, 21)), ((13, 21), (4, 6)), ((26, 38), (2, 3)), ((5, 9), (5, 9)),
                                     ((4, 6), (7, 11))])
def test_window_rule_is_torchs_ties_included(hw, size):
    g = torch.Generator().manual_seed(hw[0] * 100 + size[0])
    for x in (torch.zeros(hw), torch.randint(-2, 3, hw, generator=g).float(), torch.randn(hw, generator=g)):
        want_v, want_i = F.adaptive_max_pool2d(x[None, None], size, return_indices=True)
        got_v, got_i = _window_argmax(x, size)
        assert torch.equal(got_v, want_v[0, 0]) and torch.equal(got_i, want_i[0, 0]), (hw, size)
    if hw == (7, 7):        # all-zero 7x7 -> 3x3: the indices are the window origins
        assert want_i[0, 0].tolist() != [] and _window_argmax(torch.zeros(hw), size)[1].tolist() == [[0, 2, 4], [14, 16, 18], [28, 30, 32]]


# ------------------------------------------------------------------------------------------------ the walk, HIP ops replaced
@pytest.fixture
def torch_ops(monkeypatch):
    """Torch stand-ins (fp64-capable, CPU) for the HIP entry points BFP's walk calls: what is under test is the walk itself."""
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.necks import bfp, fpn
    nchw, nhwc = (lambda t: t.permute(0, 3, 1, 2)), (lambda t: t.permute(0, 2, 3, 1).contiguous())

    def conv_gn(cache, m, x, in_ab=None, in_relu=False, materialize=True, up=None, save=None, consume_input=False, out_b8=False):
        assert in_ab is None and not out_b8
        raw = nhwc(F.conv2d(nchw(x), m.conv.weight, None, m.conv.stride, m.conv.padding))
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
            y = y + nhwc(F.interpolate(nchw(up), size=x.shape[1:3], mode='nearest'))
        return y

    def mat(lv):
        return lv if torch.is_tensor(lv) else gn_apply(lv[0], *lv[1])

    def bfp_gather(levels, r, record=False):
        out = nhwc(BR.bfp_gather([nchw(mat(l)) for l in levels], r))
        return (out, [i < r or None for i in range(len(levels))]) if record else out

    def bfp_scatter(levels, r, ref, ref_ab=None, record=False):
        ref = ref if ref_ab is None else gn_apply(ref, *ref_ab, relu=True)
        outs = [nhwc(o) for o in BR.bfp_scatter([nchw(mat(l)) for l in levels], r, nchw(ref))]
        return (outs, [i > r or None for i in range(len(levels))]) if record else outs
    monkeypatch.setattr(fpn, 'conv_gn', conv_gn)
    monkeypatch.setattr(bfp, 'conv_gn', conv_gn)
    monkeypatch.setattr(ops, 'gn_apply', gn_apply)
    monkeypatch.setattr(ops, 'bfp_gather', bfp_gather)
    monkeypatch.setattr(ops, 'bfp_scatter', bfp_scatter)
    monkeypatch.setattr(ops, 'from_nchw', nhwc)
    monkeypatch.setattr(ops, 'as_nchw', nchw)


@pytest.mark.parametrize('name', BR.CASE_NAMES)
def test_walk_tape_kinds_and_outputs(name, torch_ops):
    cfg = BR.cases()[name]
    neck = _build(cfg).double()
    neck.load_state_dict(BR.case_state_dict(cfg), strict=True)
    xs = BR.case_inputs(cfg)
    with torch.no_grad():
        outs = neck(xs)
        tape = []
        taped = neck.run([x.permute(0, 2, 3, 1).contiguous() for x in xs], tape)
    assert isinstance(outs, tuple) and len(outs) == len(taped) == cfg['num_levels']
    for l, o in enumerate(outs):
        assert BR.output_error(name, l, o) <= 1e-9, (name, l)
        assert torch.equal(taped[l].permute(0, 3, 1, 2), o)
    want = ['bfp_gather'] + (['bfp_refine'] if cfg['refine_type'] else []) + ['bfp_scatter']
    assert [r['kind'] for r in tape] == want
    by = {r['kind']: r for r in tape}
    assert len(by['bfp_gather']['args']) == len(by['bfp_scatter']['args']) == cfg['num_levels']
    if cfg['refine_type']:
        rec = by['bfp_refine']
        assert rec['module'] is neck.refine and rec['in_ab'] is None and all(rec[k] is not None for k in ('x', 'raw', 'a', 'b', 'mean', 'rstd'))


def test_list_neck_walk_lazy_equals_forward_and_the_tape_ends_with_bfps_records(torch_ops):
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import synthetic
    from tests.fpn_extra_ref import fpn_forward
    seq = json.loads(str(BR.fixture()['sequential_cfg']))
    neck = P.build_neck(_list_neck()).double()
    sd = synthetic.fpn_state_dict(seq['fpn']['in_channels'], 64, 1, 5, seed=3, prefix='0.', add_extra_convs='on_input')
    sd.update(synthetic.bfp_state_dict(64, 'conv', seed=3, prefix='1.'))
    sd = {k: v.double() for k, v in sd.items()}
    neck.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn((2, c) + hw, generator=g, dtype=torch.float64) for c, hw in zip(seq['fpn']['in_channels'], [(26, 38), (13, 19), (7, 10), (4, 5)])]
    with torch.no_grad():
        outs = neck(xs)
        tape = []
        lazy = neck.forward_lazy(xs, tape=tape)
        mid = fpn_forward(sd, xs, 5, start_level=1, add_extra_convs='on_input', prefix='0.')
        want = BR.bfp_forward(sd, list(mid), 1, 'conv', prefix='1.')
    assert len(outs) == len(lazy) == 5 and all(torch.is_tensor(t) for t in lazy)
    for o, l, w in zip(outs, lazy, want):
        assert torch.equal(o, l.permute(0, 3, 1, 2))
        assert float((o - w).abs().max()) <= 1e-9 * float(w.abs().max())
    kinds = [r['kind'] for r in tape]
    assert kinds[-3:] == ['bfp_gather', 'bfp_refine', 'bfp_scatter'] and not any(k.startswith('bfp_') for k in kinds[:-3])
    assert kinds[:-3] == ['lateral'] * 3 + ['out'] * 3 + ['extra'] * 2
