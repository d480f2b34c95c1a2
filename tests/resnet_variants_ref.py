"""The ResNet-variant cases (style='caffe', deep_stem, avg_down, ResNetV1d) shared by tools/gen_resnet_variants.py, which runs the
reference's own classes in fp64 and writes tests/golden/resnet_variants.npz, and by the tests that read that fixture.  Pure
torch-CPU / numpy here: no HIP, no reference import.

Fixture layout, per case ``name``:
  keys:<name>                 JSON [[state-dict key, shape], ...] of the reference class
  <name>:out<l>               stage output l in full where it has <= FULL elements, else
  <name>:out<l>:sample        its values at grad_sample_index(numel, OUT_K); always <name>:out<l>:absmax / :norm / :shape
  <name>:grad:names           JSON list of the trainable parameters, in named_parameters() order
  <name>:grad:norm            (T,)  L2 norm of d(sum_l <w_l, out_l>) / d(parameter), w_l = functional_weight (seeded standard normal)
  <name>:grad:sample          (T, GRAD_K) that gradient at grad_sample_index(numel, GRAD_K), rows of short tensors padded with 0
  <name>:fp32:out / :fp32:grad   conditioning: the reference alone in fp32 against its fp64 run (max|diff| / max|level| per output,
                              rel-L2 per gradient tensor); a case is admitted only within a quarter of the bars below.
  <name>:perturbed:grad       conditioning: the fp64 gradients with every conv output perturbed by one fp32 ulp of its rms, worst of
                              eight trials, rel-L2 per tensor -- the second admission rule (tools/gen_resnet_variants.py)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet_variants.npz')
FULL, OUT_K, GRAD_K = 4096, 512, 64
BAR_OUT, BAR_GRAD = 2e-4, 2e-3           # the a3 bar (outputs, of max|level|) and the reference-golden bar (gradients, rel-L2)
# B = 2, eval BatchNorm (norm_eval=True) with random buffers and affines; 67 x 93 takes an R18 through 17x24 -> 9x12 -> 5x6 -> 3x3
CASES = {
    'v1d50': dict(depth=50, deep_stem=True, avg_down=True, hw=(70, 90), frozen_stages=1, seed=41),
    'v1d18': dict(depth=18, deep_stem=True, avg_down=True, hw=(67, 93), frozen_stages=1, seed=42),
    'caffe50': dict(depth=50, style='caffe', hw=(70, 90), frozen_stages=1, seed=53),
    'avgdown50': dict(depth=50, avg_down=True, hw=(70, 90), frozen_stages=1, seed=44),
    'deepstem18': dict(depth=18, deep_stem=True, hw=(67, 93), frozen_stages=1, seed=45),
    'v1d50_fs0': dict(depth=50, deep_stem=True, avg_down=True, hw=(70, 90), frozen_stages=0, seed=56),
    'caffe101': dict(depth=101, style='caffe', hw=(70, 90), frozen_stages=1, seed=77),
}
CASE_NAMES = list(CASES)
BATCH = 2


def grad_sample_index(numel, k):
    """oracle.gen_golden.grad_sample_index: deterministic flat indices (<= k entries, evenly spread)."""
    return np.unique(np.linspace(0, numel - 1, min(k, numel)).round().astype(np.int64))


def resnet_kwargs(cfg):
    return dict(depth=cfg['depth'], style=cfg.get('style', 'pytorch'), deep_stem=cfg.get('deep_stem', False),
                avg_down=cfg.get('avg_down', False), frozen_stages=cfg['frozen_stages'], norm_eval=True)


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.resnet_state_dict(cfg['depth'], cfg['seed'], prefix='', deep_stem=cfg.get('deep_stem', False),
                                     avg_down=cfg.get('avg_down', False))
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def case_input(cfg, dtype=torch.float32):
    g = torch.Generator().manual_seed(cfg['seed'] + 100)
    return torch.randn((BATCH, 3) + tuple(cfg['hw']), generator=g, dtype=torch.float64).to(dtype)


def functional_weight(cfg, level, shape, dtype=torch.float32):
    """w_l of the linear functional sum_l <w_l, out_l>: NCHW, standard normal, its own seed per (case, level)."""
    g = torch.Generator().manual_seed(cfg['seed'] * 1000 + level)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).to(dtype)


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
