"""The RegNet cases shared by tools/gen_regnet.py, which runs the reference's own class (mmdet.models.backbones.regnet.RegNet) in fp64
and writes tests/golden/regnet.npz, and by the tests that read that fixture.  Pure torch-CPU / numpy here: no HIP, no reference import.
Layout, sampling and bars are those of tests/resnet_variants_ref.py (whose helpers are reused): per case ``name``
  keys:<name>, <name>:out<l>[:sample] / :absmax / :norm / :shape, <name>:grad:names / :norm / :sample,
  <name>:fp32:out / :fp32:grad and <name>:perturbed:grad (the two admission rules of tools/gen_regnet.py),
and ``layouts`` (JSON): {arch name: [stage_widths, group_widths, stage_blocks]} as the reference's constructor derived them, for all
eight names of its ``arch_settings``."""
import json
import os

import numpy as np
import torch

from tests.resnet_variants_ref import BAR_GRAD, BAR_OUT, BATCH, FULL, GRAD_K, OUT_K, case_input, functional_weight, grad_sample_index  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regnet.npz')
ARCH_NAMES = ('regnetx_400mf', 'regnetx_800mf', 'regnetx_1.6gf', 'regnetx_3.2gf', 'regnetx_4.0gf', 'regnetx_6.4gf', 'regnetx_8.0gf',
              'regnetx_12gf')
# B = 2, eval BatchNorm (norm_eval=True) with random buffers and affines; the stem and all four stages stride:
# 70 x 90 -> 35x45 -> 18x23 -> 9x12 -> 5x6 -> 3x3, 67 x 93 -> 34x47 -> 17x24 -> 9x12 -> 5x6 -> 3x3
CASES = {
    'x800mf': dict(arch='regnetx_800mf', hw=(70, 90), frozen_stages=1, seed=91),              # no padding, cg 16, new stem / expansion 1
    'x1.6gf': dict(arch='regnetx_1.6gf', hw=(67, 93), frozen_stages=1, seed=92),              # every stage padded, cg 24, odd maps
    'x3.2gf': dict(arch='regnetx_3.2gf', hw=(70, 90), frozen_stages=1, seed=93),              # cg 48, stages 3 - 4 padded
    'x4.0gf_caffe': dict(arch='regnetx_4.0gf', style='caffe', hw=(67, 93), frozen_stages=1, seed=94),      # cg 40
    'x6.4gf': dict(arch='regnetx_6.4gf', hw=(70, 90), frozen_stages=1, seed=95),              # cg 56
    'x1.6gf_fs-1': dict(arch='regnetx_1.6gf', hw=(70, 90), frozen_stages=-1, seed=96),        # conv1.weight, bn1.* gradients
    'x3.2gf_fs0_avgdown': dict(arch='regnetx_3.2gf', avg_down=True, hw=(70, 90), frozen_stages=0, seed=98),
}
CASE_NAMES = list(CASES)


def regnet_kwargs(cfg):
    return dict(arch=cfg['arch'], style=cfg.get('style', 'pytorch'), avg_down=cfg.get('avg_down', False),
                frozen_stages=cfg['frozen_stages'], norm_eval=True)


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.regnet_state_dict(cfg['arch'], cfg['seed'], prefix='', avg_down=cfg.get('avg_down', False))
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(GOLDEN) as z:
            _FIX = {k: z[k] for k in z.files}
    return _FIX


def layouts():
    """{arch name: (stage_widths, group_widths, stage_blocks)} of the reference."""
    return {k: tuple(v) for k, v in json.loads(str(fixture()['layouts'])).items()}


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
