"""The ResNeSt cases shared by tools/gen_resnest.py, which runs the reference's own class (mmdet.models.backbones.resnest.ResNeSt) in
fp64 and writes tests/golden/resnest.npz, and by the tests that read that fixture; and a plain-torch restatement of the split-attention
block and the backbone (``restated_block`` / ``restated_forward``, any dtype, differentiable) that the host test holds against the
fixture and the GPU tests replay in fp64 where the reference tree does not exist.  Pure torch-CPU / numpy here: no HIP, no reference
import.  Layout, sampling and bars are those of tests/resnet_variants_ref.py (whose helpers are reused): per case ``name``
  keys:<name>, <name>:out<l>[:sample] / :absmax / :norm / :shape, <name>:grad:names / :norm / :sample,
  <name>:fp32:out / :fp32:grad and <name>:perturbed:grad (the two admission rules of tools/gen_resnest.py),
and per depth ``d`` the reference's state-dict key list ``depthkeys:<d>`` (JSON [[key, shape], ...])."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.resnet_variants_ref import BAR_GRAD, BAR_OUT, BATCH, FULL, GRAD_K, OUT_K, case_input, functional_weight, grad_sample_index  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnest.npz')
# B = 2, eval BatchNorm (norm_eval=True) with random buffers and affines; 70 x 90 -> 18x23 -> 9x12 -> 5x6 -> 3x3 (the block's 3x3 / 2
# pool on even and odd maps), 67 x 93 -> 17x24 -> 9x12 -> 5x6 -> 3x3
CASES = {
    's50': dict(depth=50, hw=(70, 90), frozen_stages=1, seed=111),
    's50_odd': dict(depth=50, hw=(67, 93), frozen_stages=1, seed=132),                     # pool windows on odd borders at every stage
    's50_fs0': dict(depth=50, hw=(70, 90), frozen_stages=0, seed=113),                     # layer1.0 trains: stride 1, shortcut conv, no pool
    's50_caffe': dict(depth=50, hw=(70, 90), frozen_stages=1, seed=114, style='caffe'),    # the stride on conv1: no pooled block at all
    's50_rf2': dict(depth=50, hw=(70, 90), frozen_stages=1, seed=115, reduction_factor=2),  # inter = w
    's101': dict(depth=101, hw=(70, 90), frozen_stages=1, seed=146),
}
CASE_NAMES = list(CASES)
DEPTHS = (50, 101, 152, 200)
BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3), 200: (3, 24, 36, 3)}
RADIX = 2


def resnest_kwargs(cfg):
    return dict(depth=cfg['depth'], style=cfg.get('style', 'pytorch'), reduction_factor=cfg.get('reduction_factor', 4),
                frozen_stages=cfg['frozen_stages'], norm_eval=True)


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.resnest_state_dict(cfg['depth'], cfg['seed'], reduction_factor=cfg.get('reduction_factor', 4), prefix='')
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


def depth_keys(depth):
    return [(k, tuple(s)) for k, s in json.loads(str(fixture()['depthkeys:%d' % depth]))]


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


# ---- the split attention and the backbone restated in plain torch (any dtype; NCHW): what the block computes, nothing else
def _bn(sd, p, x, eps=1e-5):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, eps)


def splat_attention(g, fc1_w, fc1_b, bn, fc2_w, fc2_b, eps=1e-5):
    """g (N,w) -> (att (N,2,w), z (N,inter)); bn = (weight, bias, running_mean, running_var) of the eval BatchNorm behind fc1."""
    h = F.linear(g, fc1_w.flatten(1), fc1_b)
    z = F.relu((h - bn[2]) / torch.sqrt(bn[3] + eps) * bn[0] + bn[1])
    a = F.linear(z, fc2_w.flatten(1), fc2_b)
    return torch.softmax(a.view(g.shape[0], RADIX, -1), dim=1), z


def splat_apply(u, att, pool):
    """u (N,2w,H,W), att (N,2,w) -> sum_r att[n,r,c] * u[n,r*w+c] (N,w,H,W), or with ``pool`` AvgPool2d(3, 2, padding=1) of it."""
    N, C2, H, W = u.shape
    v = (att.view(N, RADIX, C2 // RADIX, 1, 1) * u.view(N, RADIX, C2 // RADIX, H, W)).sum(1)
    return F.avg_pool2d(v, 3, 2, 1) if pool else v       # count_include_pad: the divisor is always 9


def splat_gap(u):
    N, C2, H, W = u.shape
    return u.view(N, RADIX, C2 // RADIX, H * W).sum(1).mean(-1)


def restated_block(sd, p, x, stride, style='pytorch'):
    """One ResNeSt bottleneck from the keys under prefix ``p``."""
    s1 = stride if style == 'caffe' else 1
    o1 = F.relu(_bn(sd, p + 'bn1', F.conv2d(x, sd[p + 'conv1.weight'], None, s1)))
    u = F.relu(_bn(sd, p + 'conv2.bn0', F.conv2d(o1, sd[p + 'conv2.conv.weight'], None, 1, 1, groups=RADIX)))
    q = p + 'conv2.bn1.'
    att, _ = splat_attention(splat_gap(u), sd[p + 'conv2.fc1.weight'], sd[p + 'conv2.fc1.bias'],
                             (sd[q + 'weight'], sd[q + 'bias'], sd[q + 'running_mean'], sd[q + 'running_var']),
                             sd[p + 'conv2.fc2.weight'], sd[p + 'conv2.fc2.bias'])
    o = splat_apply(u, att, pool=style == 'pytorch' and stride > 1)
    out = _bn(sd, p + 'bn3', F.conv2d(o, sd[p + 'conv3.weight']))
    identity = x
    if p + 'downsample.1.weight' in sd:
        if stride > 1:
            identity = F.avg_pool2d(identity, stride, stride, ceil_mode=True, count_include_pad=False)
        identity = _bn(sd, p + 'downsample.2', F.conv2d(identity, sd[p + 'downsample.1.weight']))
    return F.relu(out + identity)


def restated_forward(sd, cfg, x):
    """-> the four stage outputs (NCHW) of the ResNeSt of ``cfg`` holding the (prefix-free) state dict ``sd``."""
    for i in (0, 3, 6):
        x = F.relu(_bn(sd, 'stem.%d' % (i + 1), F.conv2d(x, sd['stem.%d.weight' % i], None, 2 if i == 0 else 1, 1)))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    for li, nb in enumerate(BLOCKS[cfg['depth']]):
        for bi in range(nb):
            x = restated_block(sd, 'layer%d.%d.' % (li + 1, bi), x, 2 if (bi == 0 and li > 0) else 1, cfg.get('style', 'pytorch'))
        outs.append(x)
    return outs
