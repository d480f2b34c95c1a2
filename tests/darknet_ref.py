"""The cases of tests/golden/darknet.npz (tools/gen_darknet.py) and a torch restatement of the reference's Darknet
(T/mmdet/models/backbones/darknet.py) -- ConvModule, ResBlock, conv_res_block, net -- in the dtype of its arguments, fp64 for the
yardstick: plain torch functions over a reference-layout state dict, no module classes.  tests/test_darknet_host.py pins the
restatement to the archive at 1e-12, so a GPU test may compare against either."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'darknet.npz')
BAR_OUT, BAR_GRAD = 2e-4, 2e-3          # the project's bars for a backbone (tests/test_gpu_hrnet.py, tests/test_gpu_mobilenet_v2.py)
U = 2.0 ** -24                          # fp32 unit roundoff
FULL, OUT_K, GRAD_K = 4096, 512, 64      # the archive's layout (tools/gen_fpn_extra_levels.py)
BN_EPS = 1e-5

# a small architecture added to ``arch_settings`` on both sides (the reference's class and the port's read the dict at construction)
SMALL_DEPTH = 21
SMALL_ARCH = ((1, 2, 1, 1, 1), ((32, 64), (64, 64), (64, 128), (128, 128), (128, 256)))

CASES = {
    'd53': dict(depth=53, input=(2, 3, 64, 96), out_indices=(3, 4, 5), negative_slope=0.1, frozen_stages=-1, seed=502),
    'small': dict(depth=SMALL_DEPTH, input=(2, 3, 40, 56), out_indices=(3, 4, 5), negative_slope=0.1, frozen_stages=-1, seed=511),
    'small_idx': dict(depth=SMALL_DEPTH, input=(2, 3, 40, 56), out_indices=(0, 2, 5), negative_slope=0.2, frozen_stages=-1, seed=521),
    'small_fs2': dict(depth=SMALL_DEPTH, input=(2, 3, 40, 56), out_indices=(3, 4, 5), negative_slope=0.1, frozen_stages=2, seed=531),
}
CASE_NAMES = list(CASES)
FLAG_STAGES = (-1, 1, 3)                 # ``flags:<k>``: requires_grad / training after train() with frozen_stages = k (SMALL_DEPTH)
STEM_IN = 'stage1_in'                    # the image-side input of the first stride-2 conv, LeakyReLU(bn(conv1(img)))


def add_small_arch(cls):
    """Register SMALL_ARCH under SMALL_DEPTH in ``cls.arch_settings`` (the reference's class or the port's)."""
    cls.arch_settings[SMALL_DEPTH] = SMALL_ARCH
    return cls


def arch(depth):
    return SMALL_ARCH if depth == SMALL_DEPTH else ((1, 2, 8, 8, 4), ((32, 64), (64, 128), (128, 256), (256, 512), (512, 1024)))


def constructor_kwargs(cfg):
    return dict(depth=cfg['depth'], out_indices=tuple(cfg['out_indices']), frozen_stages=cfg['frozen_stages'],
                act_cfg=dict(type='LeakyReLU', negative_slope=cfg['negative_slope']))


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.backbones import Darknet
    add_small_arch(Darknet)      # (synthetic.darknet_layout reads the port's arch_settings)
    return {k: (v if v.dtype == torch.long else v.to(dtype)) for k, v in synthetic.darknet_state_dict(cfg['depth'], cfg['seed']).items()}


def case_input(cfg, dtype=torch.float32):
    """Seeded normals rounded to fp32 once."""
    g = torch.Generator().manual_seed(cfg['seed'] + 100)
    return torch.randn(tuple(cfg['input']), generator=g, dtype=torch.float64).float().to(dtype)


def functional_weight(cfg, level, shape, dtype=torch.float32):
    """w_l of the linear functional sum_l <w_l, out_l>: NCHW, seeded normals rounded to fp32 once."""
    g = torch.Generator().manual_seed(cfg['seed'] * 1000 + level)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).float().to(dtype)


# ------------------------------------------------------------------------------------------------ restatement
def conv_module(sd, key, x, stride, slope):
    """mmcv's ConvModule of the reference's Darknet: conv (no bias, padding k // 2) -> eval-mode BN -> LeakyReLU(slope)."""
    w = sd[key + '.conv.weight']
    z = F.conv2d(x, w, None, stride, w.shape[-1] // 2)
    z = F.batch_norm(z, sd[key + '.bn.running_mean'], sd[key + '.bn.running_var'], sd[key + '.bn.weight'], sd[key + '.bn.bias'],
                     False, 0.0, BN_EPS)
    return F.leaky_relu(z, slope)


def res_block(sd, key, x, slope):
    """darknet.py:49-55: conv1 (1x1), conv2 (3x3), ``out + residual``."""
    out = conv_module(sd, key + '.conv1', x, 1, slope)
    out = conv_module(sd, key + '.conv2', out, 1, slope)
    return out + x


def conv_res_block(sd, key, x, n, slope):
    """darknet.py:204-212: the stride-2 ConvModule, then ``n`` ResBlocks."""
    x = conv_module(sd, key + '.conv', x, 2, slope)
    for j in range(n):
        x = res_block(sd, '%s.res%d' % (key, j), x, slope)
    return x


def net(sd, img, depth, out_indices, slope, taps=None):
    """darknet.py:152-160 -> the out_indices stage outputs in stage order (NCHW).  taps (dict): receives STEM_IN."""
    layers, _ = arch(depth)
    x = conv_module(sd, 'conv1', img, 1, slope)
    if taps is not None:
        taps[STEM_IN] = x
    outs = [x] if 0 in out_indices else []
    for i, n in enumerate(layers):
        x = conv_res_block(sd, 'conv_res_block%d' % (i + 1), x, n, slope)
        if i + 1 in out_indices:
            outs.append(x)
    return outs


def frozen_keys(depth, frozen_stages):
    """The parameter-key prefixes ``frozen_stages`` freezes: cr_blocks[:frozen_stages] (darknet.py:162-168)."""
    blocks = ['conv1.'] + ['conv_res_block%d.' % (i + 1) for i in range(len(arch(depth)[0]))]
    return tuple(blocks[:max(frozen_stages, 0)])


def restated_case(cfg, dtype=torch.float64):
    """-> (outputs, {parameter key or STEM_IN: gradient of the linear functional}) of the restatement, as tools/gen_darknet.py
    records them for the reference: frozen parameters have no entry, nor has STEM_IN when nothing in front of it trains."""
    sd = case_state_dict(cfg, dtype)
    frozen = frozen_keys(cfg['depth'], cfg['frozen_stages'])
    params = [k for k, v in sd.items() if v.dtype != torch.long and k.split('.')[-1] in ('weight', 'bias') and not k.startswith(frozen)]
    for k in params:
        sd[k].requires_grad_(True)
    taps = {}
    outs = net(sd, case_input(cfg, dtype), cfg['depth'], cfg['out_indices'], cfg['negative_slope'], taps)
    if taps[STEM_IN].requires_grad:
        taps[STEM_IN].retain_grad()
    total = sum((functional_weight(cfg, l, o.shape, dtype) * o).sum() for l, o in enumerate(outs))
    total.backward()
    grads = {k: sd[k].grad for k in params}
    if taps[STEM_IN].requires_grad:
        grads[STEM_IN] = taps[STEM_IN].grad
    return [o.detach() for o in outs], grads


# ------------------------------------------------------------------------------------------------ the archive
_ARCHIVE = []


def archive():
    if not _ARCHIVE:
        _ARCHIVE.append(np.load(GOLDEN))
    return _ARCHIVE[0]


def archive_keys(name):
    """[(state-dict key, shape)] of the reference class for case ``name``, in its order."""
    return [(k, tuple(s)) for k, s in json.loads(str(archive()['keys:' + name]))]


def grad_names(name):
    a = archive()
    pre = name + ':norm:'
    return sorted(k[len(pre):] for k in a.files if k.startswith(pre))


def output_error(name, level, out):
    """max|diff| / max|level| of NCHW-shaped ``out`` against the archive's fp64 level (in full, or on its strided sample)."""
    from oracle.gen_golden import grad_sample_index
    a = archive()
    key = '%s:out%d' % (name, level)
    o = out.detach().double().cpu().contiguous()
    assert tuple(o.shape) == tuple(int(v) for v in a[key + ':shape']), (tuple(o.shape), a[key + ':shape'])
    if key in a.files:
        d = float(np.abs(o.numpy() - a[key]).max())
    else:
        flat = o.flatten()
        d = float(np.abs(flat[torch.from_numpy(grad_sample_index(flat.numel(), OUT_K))].numpy() - a[key + ':sample']).max())
    return d / float(a[key + ':absmax'])


def grad_errors(name, key, grad):
    """(|norm - ref| / ref norm, rel-L2 on the strided sample) of a gradient against the archive."""
    from oracle.gen_golden import grad_sample_index
    a = archive()
    flat = grad.detach().double().cpu().flatten()
    ref_norm, ref_s = float(a['%s:norm:%s' % (name, key)]), a['%s:sample:%s' % (name, key)]
    s = flat[torch.from_numpy(grad_sample_index(flat.numel(), GRAD_K))].numpy()
    return abs(float(flat.norm()) - ref_norm) / max(ref_norm, 1e-300), float(np.linalg.norm(s - ref_s) / max(np.linalg.norm(ref_s), 1e-300))
