"""The dilated ResNet / ResNetV1d / ResNeXt cases (``dilations`` in stride-1 stages: the DC5 layout strides (1, 2, 2, 1) / dilations
(1, 1, 1, 2) of configs/_base_/models/faster_rcnn_r50_caffe_dc5.py, and the output-stride-8 layout strides (1, 2, 1, 1) / dilations
(1, 1, 2, 4)) shared by tools/gen_dilated.py, which runs the reference's own classes in fp64 and writes tests/golden/dilated.npz, and
by the tests that read that fixture.  Pure torch-CPU / numpy here: no HIP, no reference import.  Layout, sampling and bars are those of
tests/resnet_variants_ref.py (whose helpers are reused); beside them, per case ``name``,
  convs:<name>    JSON [[conv module name, stride, padding, dilation, groups], ...] of the reference model, in named_modules() order."""
import json
import os

import numpy as np
import torch

from tests.resnet_variants_ref import BAR_GRAD, BAR_OUT, BATCH, FULL, GRAD_K, OUT_K, case_input, functional_weight, grad_sample_index  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dilated.npz')
DC5 = dict(strides=(1, 2, 2, 1), dilations=(1, 1, 1, 2))
OS8 = dict(strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4))
# B = 2, eval BatchNorm (norm_eval=True) with random buffers and affines.  70 x 90 -> 18x23 -> 9x12 -> 5x6 -> 5x6 (DC5) or
# 18x23 -> 9x12 -> 9x12 -> 9x12 (OS8: d = 4 on a 9 x 12 map); 67 x 93 -> 17x24 -> 9x12 -> ...
CASES = {
    'dc5_caffe50': dict(depth=50, style='caffe', hw=(70, 90), frozen_stages=1, seed=111, **DC5),
    'dc5_18': dict(depth=18, hw=(67, 93), frozen_stages=1, seed=113, **DC5),
    'dc5_v1d50': dict(depth=50, deep_stem=True, avg_down=True, hw=(70, 90), frozen_stages=1, seed=115, **DC5),
    'os8_18_fs0': dict(depth=18, hw=(67, 93), frozen_stages=0, seed=126, **OS8),
    'os8_50': dict(depth=50, hw=(70, 90), frozen_stages=1, seed=152, **OS8),
    'dc5_x50': dict(depth=50, groups=32, base_width=4, hw=(70, 90), frozen_stages=1, seed=117, **DC5),
}
CASE_NAMES = list(CASES)


def case_class(cfg):
    """Name of the class that builds the case, here and in the reference."""
    if 'groups' in cfg:
        return 'ResNeXt'
    return 'ResNetV1d' if cfg.get('deep_stem') and cfg.get('avg_down') else 'ResNet'


def kwargs(cfg):
    """Constructor keywords in the form of resnet_variants_ref.resnet_kwargs (deep_stem / avg_down spelled out; a ResNetV1d case is
    built from them without the two, a ResNeXt case with its groups / base_width)."""
    kw = dict(depth=cfg['depth'], style=cfg.get('style', 'pytorch'), deep_stem=cfg.get('deep_stem', False),
              avg_down=cfg.get('avg_down', False), frozen_stages=cfg['frozen_stages'], norm_eval=True,
              strides=tuple(cfg['strides']), dilations=tuple(cfg['dilations']))
    if 'groups' in cfg:
        kw.update(groups=cfg['groups'], base_width=cfg['base_width'])
    return kw


def build(cfg, **over):
    """This package's model of a case (CPU; the caller moves it)."""
    from pointtinybenchmark_amd.backbones import resnet as RN
    kw = dict(kwargs(cfg), **over)
    name = case_class(cfg)
    if name == 'ResNetV1d':
        kw.pop('deep_stem'), kw.pop('avg_down')
    return getattr(RN, name)(**kw)


def state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.resnet_state_dict(cfg['depth'], cfg['seed'], prefix='', deep_stem=cfg.get('deep_stem', False),
                                     avg_down=cfg.get('avg_down', False), groups=cfg.get('groups', 1), base_width=cfg.get('base_width', 4))
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def conv_settings(model):
    """[[name, stride, padding, dilation, groups], ...] of every nn.Conv2d of ``model`` (square settings: the first component)."""
    return [[n, m.stride[0], m.padding[0], m.dilation[0], m.groups] for n, m in model.named_modules() if isinstance(m, torch.nn.Conv2d)]


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(GOLDEN) as z:
            _FIX = {k: z[k] for k in z.files}
    return _FIX


def keys(name):
    return [(k, tuple(s)) for k, s in json.loads(str(fixture()['keys:' + name]))]


def convs(name):
    return json.loads(str(fixture()['convs:' + name]))


def grad_names(name):
    return json.loads(str(fixture()[name + ':grad:names']))


def output_error(name, level, out):
    """max|out - reference| / max|reference level| of an NCHW-shaped stage output (on the sampled positions for a large level)."""
    f = fixture()
    key = '%s:out%d' % (name, level)
    assert tuple(out.shape) == tuple(f[key + ':shape']), (tuple(out.shape), tuple(f[key + ':shape']))
    flat = out.detach().double().cpu().contiguous().flatten()      # (.contiguous(): NCHW element order of a channels_last view)
    if key in f:
        ref = torch.from_numpy(f[key]).flatten()
    else:
        ref = torch.from_numpy(f[key + ':sample'])
        flat = flat[torch.from_numpy(grad_sample_index(flat.numel(), OUT_K))]
    return float((flat - ref).abs().max() / float(f[key + ':absmax']))


def grad_errors(name, pname, grad):
    """(|norm - ref| / ref, rel-L2 on the sampled positions) of one parameter gradient."""
    f = fixture()
    t = grad_names(name).index(pname)
    flat = grad.detach().double().cpu().flatten()
    idx = grad_sample_index(flat.numel(), GRAD_K)
    ref_n = float(f[name + ':grad:norm'][t])
    ref_s = torch.from_numpy(f[name + ':grad:sample'][t, :len(idx)])
    got_s = flat[torch.from_numpy(idx)]
    return abs(float(flat.norm()) - ref_n) / max(ref_n, 1e-300), float((got_s - ref_s).norm() / ref_s.norm().clamp_min(1e-300))
