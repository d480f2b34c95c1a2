"""The ResNeXt cases shared by tools/gen_resnext.py, which runs the reference's own class (mmdet.models.backbones.resnext.ResNeXt) in
fp64 and writes tests/golden/resnext.npz, and by the tests that read that fixture.  Pure torch-CPU / numpy here: no HIP, no reference
import.  Layout, sampling and bars are those of tests/resnet_variants_ref.py (whose helpers are reused): per case ``name``
  keys:<name>, <name>:out<l>[:sample] / :absmax / :norm / :shape, <name>:grad:names / :norm / :sample,
  <name>:fp32:out / :fp32:grad and <name>:perturbed:grad (the two admission rules of tools/gen_resnext.py)."""
import json
import os

import numpy as np
import torch

from tests.resnet_variants_ref import BAR_GRAD, BAR_OUT, BATCH, FULL, GRAD_K, OUT_K, case_input, functional_weight, grad_sample_index  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnext.npz')
# B = 2, eval BatchNorm (norm_eval=True) with random buffers and affines; 70 x 90 -> 18x23 -> 9x12 -> 5x6 -> 3x3 (stride-2 grouped layers
# on even and odd maps), 67 x 93 -> 17x24 -> 9x12 -> 5x6 -> 3x3
CASES = {
    'x50_32x4d': dict(depth=50, groups=32, base_width=4, hw=(70, 90), frozen_stages=1, seed=81),
    'x101_64x4d': dict(depth=101, groups=64, base_width=4, hw=(70, 90), frozen_stages=1, seed=84),
    'x50_32x4d_caffe': dict(depth=50, groups=32, base_width=4, style='caffe', hw=(67, 93), frozen_stages=1, seed=82),
    'x50_32x4d_fs0': dict(depth=50, groups=32, base_width=4, hw=(70, 90), frozen_stages=0, seed=86),
    'x50_32x4d_avgdown': dict(depth=50, groups=32, base_width=4, avg_down=True, hw=(70, 90), frozen_stages=1, seed=87),
}
CASE_NAMES = list(CASES)


def resnext_kwargs(cfg):
    return dict(depth=cfg['depth'], groups=cfg['groups'], base_width=cfg['base_width'], style=cfg.get('style', 'pytorch'),
                avg_down=cfg.get('avg_down', False), frozen_stages=cfg['frozen_stages'], norm_eval=True)


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.resnet_state_dict(cfg['depth'], cfg['seed'], prefix='', avg_down=cfg.get('avg_down', False), groups=cfg['groups'],
                                     base_width=cfg['base_width'])
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(GOLDEN) as z:
            _FIX = {k: z[k] for k in z.files}
    return _FIX


def keys(name):
    return [(k, tuple(s)) for k, s in json.loads(str(fixture()['keys:' + name]))]


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
