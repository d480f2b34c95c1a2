"""The Res2Net cases shared by tools/gen_res2net.py, which runs the reference's own class (mmdet.models.backbones.res2net.Res2Net) in
fp64 and writes tests/golden/res2net.npz, and by the tests that read that fixture; and a plain-torch restatement of the backbone
(``restated_forward``) the host test holds against the fixture.  Pure torch-CPU / numpy here: no HIP, no reference import.  Layout,
sampling and bars are those of tests/resnet_variants_ref.py (whose helpers are reused): per case ``name``
  keys:<name>, <name>:out<l>[:sample] / :absmax / :norm / :shape, <name>:grad:names / :norm / :sample,
  <name>:fp32:out / :fp32:grad and <name>:perturbed:grad (the two admission rules of tools/gen_res2net.py)."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.resnet_variants_ref import BAR_GRAD, BAR_OUT, BATCH, FULL, GRAD_K, OUT_K, case_input, functional_weight, grad_sample_index  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'res2net.npz')
# B = 2, eval BatchNorm (norm_eval=True) with random buffers and affines; 70 x 90 -> 18x23 -> 9x12 -> 5x6 -> 3x3 (stride-2 slice convs and
# the last-slice pool on even and odd maps), 67 x 93 -> 17x24 -> 9x12 -> 5x6 -> 3x3
CASES = {
    'r50_26w4s': dict(depth=50, scales=4, base_width=26, hw=(70, 90), frozen_stages=1, seed=91),
    'r50_14w8s': dict(depth=50, scales=8, base_width=14, hw=(67, 93), frozen_stages=1, seed=92),      # odd maps, eight slices
    'r50_48w2s': dict(depth=50, scales=2, base_width=48, hw=(70, 90), frozen_stages=1, seed=96),      # empty loop, no pad channels
    'r50_26w4s_fs0': dict(depth=50, scales=4, base_width=26, hw=(70, 90), frozen_stages=0, seed=97),  # layer1.0 (stage block, stride 1) trains
    'r101_26w4s': dict(depth=101, scales=4, base_width=26, hw=(70, 90), frozen_stages=1, seed=95),
}
CASE_NAMES = list(CASES)
STATE_DICT_KEYS = {'r50_26w4s': 522, 'r50_14w8s': 906, 'r50_48w2s': 330}
BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


def res2net_kwargs(cfg):
    return dict(depth=cfg['depth'], scales=cfg['scales'], base_width=cfg['base_width'], frozen_stages=cfg['frozen_stages'], norm_eval=True)


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.res2net_state_dict(cfg['depth'], cfg['scales'], cfg['base_width'], cfg['seed'], prefix='')
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


# ---- the backbone restated in plain torch from its state dict (any dtype): what the issue's "Semantics" section says, nothing else
def _bn(sd, p, x, eps=1e-5):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, eps)


def restated_block(sd, p, x, scales, stride, stage):
    """One Bottle2neck from the keys under prefix ``p``."""
    out = F.relu(_bn(sd, p + 'bn1', F.conv2d(x, sd[p + 'conv1.weight'])))
    width = out.shape[1] // scales
    spx = [out[:, i * width:(i + 1) * width] for i in range(scales)]
    ys = []
    for i in range(scales - 1):
        inp = spx[i] if (i == 0 or stage) else ys[-1] + spx[i]
        ys.append(F.relu(_bn(sd, '%sbns.%d' % (p, i), F.conv2d(inp, sd['%sconvs.%d.weight' % (p, i)], None, stride, 1))))
    last = spx[scales - 1]
    if stage and stride == 2:
        last = F.avg_pool2d(last, 3, 2, 1)                 # count_include_pad: the divisor is always 9
    out = _bn(sd, p + 'bn3', F.conv2d(torch.cat(ys + [last], 1), sd[p + 'conv3.weight']))
    identity = x
    if p + 'downsample.1.weight' in sd:
        if stride > 1:
            identity = F.avg_pool2d(identity, stride, stride, ceil_mode=True, count_include_pad=False)
        identity = _bn(sd, p + 'downsample.2', F.conv2d(identity, sd[p + 'downsample.1.weight']))
    return F.relu(out + identity)


def restated_forward(sd, cfg, x):
    """-> the four stage outputs (NCHW) of the Res2Net of ``cfg`` holding the (prefix-free) state dict ``sd``."""
    for i in (0, 3, 6):
        x = F.relu(_bn(sd, 'stem.%d' % (i + 1), F.conv2d(x, sd['stem.%d.weight' % i], None, 2 if i == 0 else 1, 1)))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    for li, nb in enumerate(BLOCKS[cfg['depth']]):
        for bi in range(nb):
            x = restated_block(sd, 'layer%d.%d.' % (li + 1, bi), x, cfg['scales'], 2 if (bi == 0 and li > 0) else 1, bi == 0)
        outs.append(x)
    return outs


def slice_widths(cfg):
    return [int(math.floor(64 * 2 ** i * (cfg['base_width'] / 64))) for i in range(4)]
