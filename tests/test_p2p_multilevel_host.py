"""CPU: the pieces of multi-level / multi-point P2PNet training that run without a GPU.

  refusals   autograd_bridge.unsupported_reason admits P2PHead with several FPN output levels and points per cell (the losses of
             forward_train then carry a graph) and keeps refusing a multi-level CPRHead
  bridge     the autograd Functions with several lateral outputs, driven by a CPU stand-in engine with the segment API of
             training.BackwardEngine: loss.backward() equals plain torch autograd of the same math
  fixture    tests/golden/p2p_multilevel_grads.npz holds every head parameter and every level's feature gradient of its cases"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

GRID4 = [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]


def _p2p_locator(num_outs, anchors, C=2):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    cfg = p2p_model_cfg(18, C)
    cfg['neck'] = dict(cfg['neck'], num_outs=num_outs)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16, 32][:num_outs], point_anchor=list(anchors))
    return P.build_detector(cfg)


@pytest.mark.parametrize('num_outs,anchors', [(4, GRID4), (2, [(0., 0.)]), (1, GRID4), (4, [(0., 0.)])])
def test_bridge_admits_multilevel_multipoint_p2p(num_outs, anchors):
    from pointtinybenchmark_amd import autograd_bridge
    m = _p2p_locator(num_outs, anchors)
    assert len(m.neck.fpn_convs) == num_outs and m.bbox_head.num_points == len(anchors)
    assert autograd_bridge.unsupported_reason(m) is None
    br = autograd_bridge.Bridge(m, engine=types.SimpleNamespace())
    fpn = {id(p) for cm in m.neck.fpn_convs for p in cm.parameters()}
    assert fpn <= {id(p) for p in br.head_params}, 'every FPN output conv is a parameter of the head Function'


def test_bridge_refuses_multilevel_cpr_and_mismatched_strides():
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import autograd_bridge
    cfg = model_cfg(18, 1)
    cfg['neck'] = dict(cfg['neck'], num_outs=2)
    assert 'num_outs == 1' in autograd_bridge.unsupported_reason(P.build_detector(cfg))
    m = _p2p_locator(2, GRID4)
    m.bbox_head.strides = [4]
    assert 'one FPN output per stride' in autograd_bridge.unsupported_reason(m)


# ------------------------------------------------------------------------------------------------ the Functions, several levels
class Vec(nn.Module):
    def __init__(self, n, seed):
        super().__init__()
        self.w = nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.5 + 1.0)


class Backbone(nn.Module):
    res_layers = ['layer1', 'layer2']

    def __init__(self, n):
        super().__init__()
        self.layer1, self.layer2 = Vec(n, 1), Vec(n, 2)
        self.conv1, self.bn1 = nn.Identity(), nn.Identity()

    def stem(self, img):
        return img * 0.5

    def run_stage(self, i, x):
        return x * getattr(self, self.res_layers[i]).w


class Neck(nn.Module):
    start_level, in_channels = 0, [0, 0]

    def __init__(self, n):
        super().__init__()
        self.lateral_convs = nn.ModuleList([Vec(n, 3), Vec(n, 4)])
        self.fpn_convs = nn.ModuleList([Vec(n, 5), Vec(n, 6)])


class Head(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.cls = Vec(n, 7)


class Engine:
    """CPU stand-in for training.BackwardEngine with two FPN output levels: lateral sums lat1 = x1*l1, lat0 = x0*l0 + lat1 (the
    top-down add), outputs o_i = lat_i * f_i, losses from both."""
    loss_vector_key = 'out'

    def __init__(self, model):
        self.model, self._sink = model, {}

    def begin_step(self):
        pass

    def collect(self, params):
        return tuple(self._sink.pop(id(p), None) for p in params)

    def forward_stage(self, i, x):
        bb = self.model.backbone
        return bb.run_stage(i, x), [dict(x=x, w=getattr(bb, bb.res_layers[i]).w)]

    def backward_stage(self, tape, dout, need_in):
        rec = tape[0]
        self._sink[id(rec['w'])] = (dout * rec['x']).sum(0)
        return dout * rec['w'].detach() if need_in else None

    def forward_laterals(self, xs):
        l0, l1 = [m.w for m in self.model.neck.lateral_convs]
        lat1 = xs[1] * l1
        lat0 = xs[0] * l0 + lat1
        return (lat0, lat1), dict(xs=list(xs), ws=(l0, l1))

    def backward_laterals(self, recs, dlat, need):
        assert isinstance(dlat, list) and len(dlat) == 2
        (x0, x1), (l0, l1) = recs['xs'], recs['ws']
        d0 = dlat[0]
        d1 = dlat[1] + d0                     # the level's own output gradient plus what flows up from the finer level
        self._sink[id(l0)] = (d0 * x0).sum(0)
        self._sink[id(l1)] = (d1 * x1).sum(0)
        return [d0 * l0.detach() if need[0] else None, d1 * l1.detach() if need[1] else None]

    def forward_head_loss(self, lat, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_true_bboxes=None):
        assert isinstance(lat, tuple) and len(lat) == 2
        f = [cm.w for cm in self.model.neck.fpn_convs]
        c = self.model.bbox_head.cls.w
        o = [t * w * c for t, w in zip(lat, f)]
        out = torch.stack([(o[0] * o[0]).sum() + o[1].sum(), (o[1] * o[1]).sum()])[None]
        return out, dict(lat=lat, f=f, c=c, o=o)

    def backward_head_loss(self, st, up):
        u = up[0]
        o, lat, f, c = st['o'], st['lat'], st['f'], st['c']
        do = [u[0] * 2 * o[0], u[0] + u[1] * 2 * o[1]]
        self._sink[id(f[0])] = (do[0] * lat[0] * c.detach()).sum(0)
        self._sink[id(f[1])] = (do[1] * lat[1] * c.detach()).sum(0)
        self._sink[id(c)] = (do[0] * lat[0] * f[0].detach() + do[1] * lat[1] * f[1].detach()).sum(0)
        return [do[i] * f[i].detach() * c.detach() for i in range(2)]

    def loss_dict(self, out):
        return {'loss_a': [out[0, 0]], 'loss_b': [out[0, 1]]}


class Model(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.backbone, self.neck, self.bbox_head = Backbone(n), Neck(n), Head(n)


def _reference(model, img):
    bb, nk, hd = model.backbone, model.neck, model.bbox_head
    x0 = img * 0.5 * bb.layer1.w
    x1 = x0 * bb.layer2.w
    lat1 = x1 * nk.lateral_convs[1].w
    lat0 = x0 * nk.lateral_convs[0].w + lat1
    o0, o1 = lat0 * nk.fpn_convs[0].w * hd.cls.w, lat1 * nk.fpn_convs[1].w * hd.cls.w
    return (o0 * o0).sum() + o1.sum() + (o1 * o1).sum()


def test_bridge_functions_with_several_lateral_outputs():
    from pointtinybenchmark_amd import autograd_bridge as AB
    model = Model(5)
    model._autograd_bridge_state = AB.Bridge(model, engine=Engine(model))
    img = torch.randn(3, 5, generator=torch.Generator().manual_seed(9))
    losses = AB.forward_train(model, img, [dict()], None, None)
    total = sum(v for vs in losses.values() for v in vs)
    want_total = _reference(model, img)
    assert torch.allclose(total, want_total.detach())
    total.backward()
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad()
    want_total.backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.allclose(got[k], p.grad, rtol=1e-6, atol=1e-6), k


# ------------------------------------------------------------------------------------------------ the fixture
def test_multilevel_grad_fixture_covers_every_tensor():
    import pointtinybenchmark_amd as P
    from oracle.gen_golden import GN
    from tools.gen_p2p_multilevel_grads import CASES
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'p2p_multilevel_grads.npz'))
    for name, cfg in CASES.items():
        head = P.build_head(dict(type='P2PHead', norm_cfg=GN, num_classes=cfg['C'], in_channels=256, feat_channels=256, stacked_convs=4,
                                 strides=cfg['strides'], point_anchor=cfg['anchors'], loss_cls=cfg['loss_cls'],
                                 loss_reg=cfg['loss_reg'], train_cfg=dict(assigner=cfg['assigner'], sampler=dict(type='PseudoSampler'))))
        want = {'bbox_head.' + n for n, _ in head.named_parameters()} | {'feat%d' % l for l in range(len(cfg['strides']))}
        keys = {k.split(':', 2)[2] for k in g.files if k.startswith(name + ':norm:')}
        assert keys == want, (name, sorted(keys ^ want))
        assert np.isfinite(float(g[name + ':total_loss']))
        for k in keys:
            assert float(g['%s:norm:%s' % (name, k)]) > 0, (name, k)
