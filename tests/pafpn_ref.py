"""Plain-torch, differentiable restatement of PAFPN (FPN + the bottom-up path aggregation), written from the formulas of
T/mmdet/models/necks/pafpn.py:96-154 -- the autograd reference of the whole-network tests.  tests/test_pafpn_host.py pins it to
tests/golden/pafpn.npz (the reference's own class, fp64) on outputs and gradients.

Also the readers of that fixture: the cases, their seeded inputs / weights / functional weights (re-derived exactly as
tools/gen_pafpn.py derives them) and the comparison helpers the CPU and GPU tests share."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from pointtinybenchmark_amd import synthetic

from tests.fpn_extra_ref import conv_gn, sample_index

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pafpn.npz')
OUT_K, GRAD_K = 512, 128
NECK_KEYS = ('num_outs', 'start_level', 'add_extra_convs', 'extra_convs_on_inputs', 'relu_before_extra_convs')
CASE_NAMES = ('pa4', 'pa4_c256', 'pa_s1_5_on_input', 'pa6_pool', 'pa6_on_output_relu', 'pa5_on_lateral')


def pafpn_forward(sd, inputs, num_outs, start_level=0, add_extra_convs=False, extra_convs_on_inputs=True,
                  relu_before_extra_convs=False, groups=32, prefix=''):
    """sd: state dict (``prefix`` + lateral_convs.<j>.conv.weight ...); inputs: every backbone level, NCHW -> tuple of num_outs maps."""
    if add_extra_convs is True:
        add_extra_convs = 'on_input' if extra_convs_on_inputs else 'on_output'
    L = len(inputs) - start_level
    assert num_outs >= L
    # 1. laterals + top-down: nearest upsample to the finer level's size, added
    lat = [conv_gn(inputs[start_level + j], sd, '%slateral_convs.%d' % (prefix, j), groups=groups) for j in range(L)]
    for j in range(L - 1, 0, -1):
        lat[j - 1] = lat[j - 1] + F.interpolate(lat[j], size=lat[j - 1].shape[2:], mode='nearest')
    # 2. one 3x3 conv + GN per level
    inter = [conv_gn(lat[j], sd, '%sfpn_convs.%d' % (prefix, j), padding=1, groups=groups) for j in range(L)]
    # 3. bottom-up: the stride-2 conv + GN of the finer sum joins the next level
    for j in range(L - 1):
        inter[j + 1] = inter[j + 1] + conv_gn(inter[j], sd, '%sdownsample_convs.%d' % (prefix, j), stride=2, padding=1, groups=groups)
    # 4. outputs: the finest sum itself, a 3x3 conv + GN on every other
    outs = [inter[0]] + [conv_gn(inter[j], sd, '%spafpn_convs.%d' % (prefix, j - 1), padding=1, groups=groups) for j in range(1, L)]
    # 5. extra levels, FPN's rules
    for k in range(num_outs - L):
        if not add_extra_convs:
            outs.append(outs[-1][:, :, ::2, ::2])           # max_pool2d(kernel 1, stride 2): every second pixel from (0, 0)
            continue
        if k == 0:
            x = {'on_input': inputs[-1], 'on_lateral': lat[-1], 'on_output': outs[-1]}[add_extra_convs]
        else:
            x = outs[-1].clamp_min(0) if relu_before_extra_convs else outs[-1]
        outs.append(conv_gn(x, sd, '%sfpn_convs.%d' % (prefix, L + k), stride=2, padding=1, groups=groups))
    return tuple(outs)


# ------------------------------------------------------------------------------------------------ the fixture
_FIX = {}


def fixture():
    if not _FIX:
        with np.load(GOLDEN) as z:
            _FIX.update({k: z[k] for k in z.files})
        _FIX['_cases'] = json.loads(str(_FIX['cases']))
        _FIX['_sizes'] = [tuple(int(v) for v in hw) for hw in _FIX['sizes']]
    return _FIX


def cases():
    return fixture()['_cases']


def neck_kwargs(cfg):
    kw = {k: cfg[k] for k in NECK_KEYS if k in cfg}
    kw.update(in_channels=list(cfg['in_channels']), out_channels=cfg['out_channels'], norm_cfg=dict(type='GN', num_groups=cfg['groups']))
    return kw


def forward_kwargs(cfg):
    return dict({k: cfg[k] for k in NECK_KEYS if k in cfg}, groups=cfg['groups'])


def case_inputs(cfg, dtype=torch.float64):
    g = torch.Generator().manual_seed(cfg['seed'] + 100)
    return [torch.randn((cfg['batch'], c) + hw, generator=g, dtype=torch.float64).to(dtype)
            for c, hw in zip(cfg['in_channels'], fixture()['_sizes'])]


def case_state_dict(cfg, dtype=torch.float64):
    sd = synthetic.pafpn_state_dict(cfg['in_channels'], cfg['out_channels'], cfg.get('start_level', 0), cfg['num_outs'], cfg['seed'],
                                    prefix='', add_extra_convs=cfg.get('add_extra_convs', False),
                                    extra_convs_on_inputs=cfg.get('extra_convs_on_inputs', True))
    return {k: v.to(dtype) for k, v in sd.items()}


def functional_weight(cfg, level, shape, dtype=torch.float64):
    g = torch.Generator().manual_seed(cfg['seed'] * 1000 + level)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).to(dtype)


def out_shapes(name):
    fx = fixture()
    return [tuple(int(v) for v in fx['%s:out%d:shape' % (name, l)]) for l in range(cases()[name]['num_outs'])]


def output_error(name, level, out):
    """max |out - reference| / max |reference level| over what the fixture holds of the level (all of it, or the strided sample).
    out: NCHW, any dtype / device."""
    fx = fixture()
    key = '%s:out%d' % (name, level)
    o = out.detach().double().cpu()
    assert tuple(o.shape) == out_shapes(name)[level], (tuple(o.shape), out_shapes(name)[level])
    if key in fx:
        diff = (o - torch.from_numpy(fx[key])).abs().max()
    else:
        idx = torch.from_numpy(sample_index(o.numel(), OUT_K))
        diff = (o.contiguous().flatten()[idx] - torch.from_numpy(fx[key + ':sample'])).abs().max()
    return float(diff) / float(fx[key + ':absmax'])


def grad_names(name):
    fx = fixture()
    pre = name + ':norm:'
    return [k[len(pre):] for k in fx if k.startswith(pre)]


def grad_errors(name, key, grad):
    """(relative error of the L2 norm, rel-L2 of the strided sample) of a gradient (NCHW / parameter layout) against the fixture."""
    fx = fixture()
    g = grad.detach().double().cpu().contiguous().flatten()
    norm, ref = float(fx['%s:norm:%s' % (name, key)]), torch.from_numpy(fx['%s:sample:%s' % (name, key)])
    got = g[torch.from_numpy(sample_index(g.numel(), GRAD_K))]
    return abs(float(g.norm()) - norm) / norm, float((got - ref).norm() / ref.norm())
