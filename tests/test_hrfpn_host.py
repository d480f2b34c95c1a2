"""Host-side tests of the HRFPN neck (no GPU):

  restatement  tests/hrfpn_ref.hrfpn_forward in fp64 against the reference's own class (tests/golden/hrfpn.npz): outputs and gradients
               <= 1e-12 relative
  identity     conv-then-upsample (the order the HIP path computes) equals upsample-then-conv (the reference's) in fp64 to rounding,
               outputs and every gradient: the identity csrc/hrfpn.hip rests on
  layout       state-dict keys, order and shapes are the fixture's recorded list; reference-layout state dicts load strictly
  refusals     every constructor refusal names its key; CprTrainer and the autograd bridge refuse more than one level under a CPRHead,
               naming the level count
  registry     a P2P config with neck=dict(type='HRFPN', ...) builds and the bridge admits it; the trainer's flat order lists every
               parameter once, the neck's in its backward's order
  taps         the integer form of the bilinear rule the kernels use is torch's for every destination of every scale"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import hrfpn_ref as HR


def _build(cfg, **kw):
    import pointtinybenchmark_amd as P
    return P.build_neck(dict(type='HRFPN', **dict(HR.neck_kwargs(cfg), **kw)))


def test_case_names_are_the_fixtures_and_cover_the_issue():
    cases = HR.cases()
    assert sorted(HR.CASE_NAMES) == sorted(cases)
    shapes = {(len(c['in_channels']), c['num_outs'], c['stride']) for c in cases.values()}
    assert {(4, 5, 1), (4, 1, 1), (3, 3, 2), (2, 2, 1), (1, 2, 1)} <= shapes
    assert any(len(set(c['in_channels'])) == len(c['in_channels']) > 1 for c in cases.values()), 'one case with unequal channel lists'
    assert any(c['size0'][0] % (1 << (c['num_outs'] - 1)) for c in cases.values()), 'one case leaves a remainder in its coarsest pool'


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_fp64_restatement_matches_the_reference_class(name):
    cfg = HR.cases()[name]
    outs, grads = HR.reference_grads(cfg)
    for l, o in enumerate(outs):
        assert HR.output_error(name, l, o) <= 1e-12, (name, l)
    assert set(HR.grad_names(name)) == set(grads), sorted(set(HR.grad_names(name)) ^ set(grads))
    for key, g in grads.items():
        en, es = HR.grad_errors(name, key, g)
        assert en <= 1e-12 and es <= 1e-12, (name, key, en, es)


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_conv_then_upsample_equals_upsample_then_conv(name):
    """Both steps are linear and bilinear weights sum to one (so the bias passes through): in fp64 the two orders differ by rounding
    alone -- sums of at most sum(in_channels) = 480 terms, relative 1e-12 is a thousand roundings."""
    cfg = HR.cases()[name]
    outs, grads = HR.reference_grads(cfg)
    outs2, grads2 = HR.reference_grads(cfg, conv_first=True)
    for l, (a, b) in enumerate(zip(outs, outs2)):
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), (name, l)
    for key in grads:
        assert float((grads[key] - grads2[key]).norm()) <= 1e-12 * float(grads[key].norm()), (name, key)
    sd, xs = HR.case_state_dict(cfg), HR.case_inputs(cfg)
    a, b = HR.reduced(sd, xs), HR.fused(sd, xs)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_state_dict_layout_is_the_references(name):
    cfg = HR.cases()[name]
    neck = _build(cfg)
    want = HR.state_keys(name)
    got = [(k, tuple(v.shape)) for k, v in neck.state_dict().items()]
    assert got == want, (got, want)          # keys, ORDER and shapes
    assert got[0] == ('reduction_conv.conv.weight', (cfg['out_channels'], sum(cfg['in_channels']), 1, 1))
    assert got[1][0] == 'reduction_conv.conv.bias' and got[2][0] == 'fpn_convs.0.conv.weight' and got[3][0] == 'fpn_convs.0.conv.bias'
    sd = HR.case_state_dict(cfg, torch.float32)
    assert list(sd) == [k for k, _ in want]
    neck.load_state_dict(sd, strict=True)
    assert all(torch.equal(neck.state_dict()[k], v) for k, v in sd.items())
    assert neck.fpn_convs[0].conv.stride == (cfg['stride'],) * 2 and neck.num_ins == len(cfg['in_channels'])


def test_registry_exports_and_init():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.necks import HRFPN
    assert P.HRFPN is HRFPN and P.NECKS.get('HRFPN') is HRFPN
    torch.manual_seed(0)
    n = P.build_neck(dict(type='HRFPN', in_channels=[32, 64], out_channels=64, norm_cfg=dict(type='BN')))
    assert n.num_outs == 5 and n.norm_cfg == dict(type='BN'), 'the reference\'s defaults; norm_cfg stored'
    assert all('bn' not in k and 'gn' not in k for k in n.state_dict()), 'and ignored: the reference never passes it on'
    for conv in [n.reduction_conv.conv] + [m.conv for m in n.fpn_convs]:
        w = conv.weight.detach()
        bound = math.sqrt(3.0 / (w.shape[1] * w.shape[2] * w.shape[3]))       # Kaiming uniform, a = 1, fan_in: gain 1
        assert 0.9 * bound < float(w.abs().max()) <= bound and bool((conv.bias == 0).all())


def test_constructor_refusals_name_their_key():
    import pointtinybenchmark_amd as P
    kw = dict(type='HRFPN', in_channels=[32, 64], out_channels=64)
    for bad, key in ((dict(pooling_type='MAX'), 'pooling_type'), (dict(with_cp=True), 'with_cp'),
                     (dict(conv_cfg=dict(type='DCN')), 'conv_cfg'), (dict(stride=3), 'stride'), (dict(num_outs=0), 'num_outs'),
                     (dict(num_outs=6), 'num_outs'), (dict(in_channels=[32] * 5), 'in_channels'), (dict(in_channels=[]), 'in_channels'),
                     (dict(out_channels=48), 'out_channels')):
        with pytest.raises(NotImplementedError, match=key):
            P.build_neck(dict(kw, **bad))
    assert len(P.build_neck(dict(kw, conv_cfg=dict(type='Conv2d'), stride=2, num_outs=1)).state_dict()) == 4


def test_p2p_config_with_an_hrfpn_neck_builds():
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(18, 1)
    cfg['neck'] = dict(type='HRFPN', in_channels=synthetic.backbone_out_channels(18), out_channels=256, num_outs=3)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16])
    m = P.build_detector(cfg)
    assert type(m.neck).__name__ == 'HRFPN' and m.neck.materialised
    assert {'neck.reduction_conv.conv.weight', 'neck.reduction_conv.conv.bias', 'neck.fpn_convs.2.conv.bias'} <= set(m.state_dict())
    assert tuple(m.state_dict()['neck.reduction_conv.conv.weight'].shape) == (256, 64 + 128 + 256 + 512, 1, 1)
    sd = synthetic.hrfpn_state_dict(synthetic.backbone_out_channels(18), 256, 3)
    assert m.load_state_dict(sd, strict=False).unexpected_keys == []


def test_bridge_admits_hrfpn_and_the_backward_order_lists_every_parameter_once():
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    from pointtinybenchmark_amd import autograd_bridge, synthetic
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    neck = dict(type='HRFPN', in_channels=synthetic.backbone_out_channels(18), out_channels=256)
    cfg = p2p_model_cfg(18, 2)
    cfg['neck'] = dict(neck, num_outs=3)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16])
    m = P.build_detector(cfg)
    assert autograd_bridge.unsupported_reason(m) is None
    m.bbox_head.strides = [4, 8]
    assert 'one FPN output per stride' in autograd_bridge.unsupported_reason(m)
    shell = P2PTrainer.__new__(P2PTrainer)
    shell.model = m
    order = shell._backward_order()
    ids = [id(p) for p in order]
    assert len(set(ids)) == len(ids) and set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
    names = {id(p): k for k, p in m.named_parameters()}
    got = [names[i] for i in ids if names[i].startswith('neck.')]
    want = [k for n in range(3) for k in ('neck.fpn_convs.%d.conv.weight' % n, 'neck.fpn_convs.%d.conv.bias' % n)] + \
        ['neck.reduction_conv.conv.bias', 'neck.reduction_conv.conv.weight']
    assert got == want, got
    pos = {i: n for n, i in enumerate(ids)}
    assert max(pos[id(p)] for p in m.bbox_head.parameters()) + 1 == pos[id(m.neck.fpn_convs[0].conv.weight)], 'head -> neck -> backbone'
    # a CPRHead takes one level
    cfg = model_cfg(18, 1)
    cfg['neck'] = dict(neck, num_outs=1)
    assert autograd_bridge.unsupported_reason(P.build_detector(cfg)) is None
    cfg['neck'] = dict(neck, num_outs=2)
    m = P.build_detector(cfg)
    assert 'one pyramid level' in autograd_bridge.unsupported_reason(m) and 'HRFPN has 2 output levels' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='one pyramid level.*HRFPN has 2 output levels'):
        CprTrainer(m)


@pytest.mark.parametrize('sh', [1, 2, 3])
def test_integer_bilinear_taps_are_torchs(sh):
    """csrc/hrfpn.hip bilinear_tap: src in units of 1 / (2 S) is max(0, 2 dst + 1 - S); x0 a shift, lambda the low bits.  Against torch's
    F.interpolate on a ramp and on one-hot rows, which reveal the taps and their weights, for every destination of in = 1, 2, 5."""
    S = 1 << sh
    for n_in in (1, 2, 5):
        eye = torch.eye(n_in, dtype=torch.float64)[None, :, None, :]             # channel c: one-hot at source c
        w = F.interpolate(eye, scale_factor=(1, S), mode='bilinear', align_corners=False)[0, :, 0]     # (source, destination)
        for d in range(n_in * S):
            t2 = max(0, 2 * d + 1 - S)
            a, lam = t2 >> (sh + 1), (t2 & (2 * S - 1)) / (2.0 * S)
            b = min(a + 1, n_in - 1)
            want = torch.zeros(n_in, dtype=torch.float64)
            want[a] += 1 - lam
            want[b] += lam
            assert torch.equal(w[:, d], want), (sh, n_in, d)
