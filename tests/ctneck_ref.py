"""The cases of tests/golden/ctneck.npz (tools/gen_ctneck.py) and a torch restatement of the reference's CTResNetNeck
(T/mmdet/models/necks/ct_resnet_neck.py) in the dtype of its arguments, fp64 for the yardstick: plain torch functions over a
reference-layout state dict, no module classes.  tests/test_ctneck_host.py pins the restatement to the archive at 1e-12, so a GPU test may
compare against either.

Train mode means BatchNorm batch statistics (the reference has no ``norm_eval`` here).  The first four cases are the issue's; the last two
have widths that are multiples of 64 throughout (the batch-statistics kernels' own widths: the 32-wide stages of the others run at a
padded pitch on the device)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ctneck.npz')
BAR_OUT, BAR_GRAD = 2e-4, 2e-3          # the project's bars for backbone and neck fixtures (tests/hrnet_ref.py, tests/darknet_ref.py)
FULL, OUT_K, GRAD_K = 4096, 512, 128     # the archive's layout (tools/gen_fpn_extra_levels.py)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1

CASES = {
    'f64_32_32': dict(in_channel=64, filters=(64, 32, 32), input=(2, 64, 3, 5), train=True, seed=811),
    'f32_row': dict(in_channel=32, filters=(32,), input=(3, 32, 1, 4), train=True, seed=821),
    'f64_32': dict(in_channel=64, filters=(64, 32), input=(1, 64, 2, 2), train=True, seed=831),
    'f64_32_32_eval': dict(in_channel=64, filters=(64, 32, 32), input=(2, 64, 3, 5), train=False, seed=811),
    'f64_64': dict(in_channel=64, filters=(64, 64), input=(2, 64, 3, 5), train=True, seed=841),
    'f128_row': dict(in_channel=32, filters=(128,), input=(3, 32, 1, 4), train=True, seed=851),
}
CASE_NAMES = list(CASES)
DEVICE_TRAIN = [n for n, c in CASES.items() if c['train']]
INPUT = 'in0'


def constructor_kwargs(cfg):
    return dict(in_channel=cfg['in_channel'], num_deconv_filters=tuple(cfg['filters']), num_deconv_kernels=(4,) * len(cfg['filters']),
                use_dcn=False)


def case_state_dict(cfg, dtype=torch.float32):
    from pointtinybenchmark_amd import synthetic
    sd = synthetic.ctneck_state_dict(cfg['in_channel'], cfg['filters'], cfg['seed'], prefix='')
    return {k: (v if v.dtype == torch.long else v.to(dtype)) for k, v in sd.items()}


def case_input(cfg, dtype=torch.float32):
    """Seeded normals rounded to fp32 once."""
    g = torch.Generator().manual_seed(cfg['seed'] + 100)
    return torch.randn(tuple(cfg['input']), generator=g, dtype=torch.float64).float().to(dtype)


def functional_weight(cfg, shape, dtype=torch.float32):
    """w of the linear functional <w, out>: NCHW, seeded normals rounded to fp32 once."""
    g = torch.Generator().manual_seed(cfg['seed'] * 1000)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64).float().to(dtype)


# ------------------------------------------------------------------------------------------------ restatement
def conv_module(sd, key, x, transposed, training, stats=None):
    """mmcv's ConvModule of the reference's neck: conv 3x3 / padding 1, or ConvTranspose2d 4x4 / stride 2 / padding 1 (conv_cfg 'deconv'),
    no bias -> BatchNorm (batch statistics and the running update when ``training``) -> ReLU.  stats (dict): receives the buffers after."""
    w = sd[key + '.conv.weight']
    z = F.conv_transpose2d(x, w, None, 2, 1) if transposed else F.conv2d(x, w, None, 1, 1)
    rm, rv = sd[key + '.bn.running_mean'].clone(), sd[key + '.bn.running_var'].clone()
    z = F.batch_norm(z, rm, rv, sd[key + '.bn.weight'], sd[key + '.bn.bias'], training, BN_MOMENTUM, BN_EPS)
    if stats is not None:
        stats[key + '.bn.running_mean'], stats[key + '.bn.running_var'] = rm, rv
        stats[key + '.bn.num_batches_tracked'] = sd[key + '.bn.num_batches_tracked'] + (1 if training else 0)
    return F.relu(z)


def net(sd, x, n_stages, training, stats=None):
    """ct_resnet_neck.py:37-61, :89-93 on the last backbone map x (NCHW) -> the output map."""
    for s in range(n_stages):
        x = conv_module(sd, 'deconv_layers.%d' % (2 * s), x, False, training, stats)
        x = conv_module(sd, 'deconv_layers.%d' % (2 * s + 1), x, True, training, stats)
    return x


def param_keys(sd):
    return [k for k, v in sd.items() if v.dtype != torch.long and k.split('.')[-1] in ('weight', 'bias')]


def restated_case(cfg, dtype=torch.float64):
    """-> (output, {parameter key or INPUT: gradient of the linear functional}, {buffer key: value after the forward}) of the
    restatement, as tools/gen_ctneck.py records them for the reference."""
    sd = case_state_dict(cfg, dtype)
    params = param_keys(sd)
    for k in params:
        sd[k].requires_grad_(True)
    x = case_input(cfg, dtype).requires_grad_(True)
    stats = {}
    out = net(sd, x, len(cfg['filters']), cfg['train'], stats)
    (functional_weight(cfg, out.shape, dtype) * out).sum().backward()
    grads = {k: sd[k].grad for k in params}
    grads[INPUT] = x.grad
    return out.detach(), grads, stats


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


def stat_names(name):
    a = archive()
    pre = name + ':stat:'
    return sorted(k[len(pre):] for k in a.files if k.startswith(pre))


def stat(name, key):
    return archive()['%s:stat:%s' % (name, key)]


def output_error(name, out):
    """max|diff| / max|output| of NCHW-shaped ``out`` against the archive's fp64 output (in full, or on its strided sample)."""
    from oracle.gen_golden import grad_sample_index
    a = archive()
    key = name + ':out0'
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
