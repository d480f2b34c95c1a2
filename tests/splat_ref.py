"""Shapes, inputs and the fp64 torch reference of the six split-attention kernels (csrc/splat.hip), shared by tests/test_gpu_splat.py and
the CPU conditioning check in tests/test_resnest_host.py.  Pure torch-CPU: no HIP.  The maps are NHWC as the kernels read them; the
arithmetic is tests/resnest_ref's restatement (splat_gap / splat_attention / splat_apply) and its autograd adjoints.

BAR: rel-L2 <= 1e-5 against fp64, the bar tests/test_gpu_bfp.py holds its fp32 kernels to.  The inputs are admitted only when the same
restatement run in fp32 torch stays within a quarter of it (tests/test_resnest_host.py)."""
import torch

from tests import resnest_ref as RS

BAR = 1e-5
# (w, inter, N, H, W): w / 4 = 16, 24, 128 lanes per pixel (24 does not divide the 256 lanes of a workgroup); one pixel; 63 pixels (two
# chunks at w = 512); 17 x 23 and 18 x 24, which pool to the same 9 x 12; 40 x 40 (seven chunks at w = 64, ten at w = 96)
SHAPES = [(64, 32, 1, 1, 1), (96, 48, 3, 7, 9), (512, 256, 1, 7, 9), (64, 32, 3, 17, 23), (64, 32, 3, 18, 24), (512, 256, 3, 18, 24),
          (64, 32, 3, 40, 40), (96, 48, 1, 40, 40)]
IDS = ['w%d_i%d_n%d_%dx%d' % s for s in SHAPES]


def pooled(H, W, pool):
    return ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (H, W)


def inputs(shape, seed=0):
    """fp32 CPU tensors of one shape: the map u (post-ReLU: about half zeros), the gradients reaching o with and without the pool, the
    attention MLP's parameters (an eval BatchNorm with random buffers), dg and datt as the backward kernels take them."""
    w, inter, N, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + w + 7 * inter + 13 * N + 17 * H + W)

    def rn(*s):
        return torch.randn(s, generator=g)
    d = dict(u=torch.relu(rn(N, H, W, 2 * w)), dout=rn(N, H, W, w), dout_pool=rn(N, *pooled(H, W, True), w),
             fc1_w=rn(inter, w, 1, 1) * (2.0 / w) ** 0.5, fc1_b=rn(inter) * 0.1, bn_w=torch.rand(inter, generator=g) * 0.5 + 0.5,
             bn_b=rn(inter) * 0.1, bn_mean=rn(inter) * 0.1, bn_var=torch.rand(inter, generator=g) + 0.5,
             fc2_w=rn(2 * w, inter, 1, 1) * (2.0 / inter) ** 0.5, fc2_b=rn(2 * w) * 0.1, gvec=torch.rand(N, w, generator=g) + 0.25,
             dg=rn(N, w), datt=rn(N, 2, w))
    return d


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bn_tuple(d, dtype):
    return tuple(d[k].to(dtype) for k in ('bn_w', 'bn_b', 'bn_mean', 'bn_var'))


def forward(d, dtype, pool):
    """-> dict(g, att, z, out) of the forward chain gap -> attn -> apply in ``dtype`` (out NHWC)."""
    u = nchw(d['u'].to(dtype))
    g = RS.splat_gap(u)
    att, z = RS.splat_attention(g, d['fc1_w'].to(dtype), d['fc1_b'].to(dtype), bn_tuple(d, dtype), d['fc2_w'].to(dtype), d['fc2_b'].to(dtype))
    return dict(g=g, att=att, z=z, out=nhwc(RS.splat_apply(u, att, pool)))


def attention_from(d, dtype, gvec=None):
    """(att, z) of the MLP alone on the given pooled vector (default d['gvec'])."""
    g = (d['gvec'] if gvec is None else gvec).to(dtype)
    return RS.splat_attention(g, d['fc1_w'].to(dtype), d['fc1_b'].to(dtype), bn_tuple(d, dtype), d['fc2_w'].to(dtype), d['fc2_b'].to(dtype))


def map_backward(d, att, dtype, pool):
    """-> (datt, du, colsum): datt the adjoint of apply wrt att; du = (att * dv + dg / HW) * (u > 0), the adjoint of apply and of the
    pooled mean wrt u through u's ReLU, with its column sums.  ``att`` (N,2,w) is given (the kernels read it)."""
    u = nchw(d['u'].to(dtype)).clone().requires_grad_(True)
    a = att.to(dtype).clone().requires_grad_(True)
    dout = nchw(d['dout_pool' if pool else 'dout'].to(dtype))
    total = (RS.splat_apply(u, a, pool) * dout).sum() + (RS.splat_gap(u) * d['dg'].to(dtype)).sum()
    du, datt = torch.autograd.grad(total, (u, a))
    # datt must not see the dg term: the pooled mean does not depend on att, so it does not
    du = nhwc(du * (u.detach() > 0).to(dtype))
    return datt, du, du.sum((0, 1, 2))


def attn_backward(d, z_mask, dtype):
    """The MLP's backward on (gvec, datt) with the ReLU pattern of ``z_mask`` (N,inter) -> dict(dg, fc1_w, fc1_b, bn_w, bn_b, fc2_w, fc2_b)."""
    P = {k: d[k].to(dtype).clone().requires_grad_(True) for k in ('gvec', 'fc1_w', 'fc1_b', 'bn_w', 'bn_b', 'fc2_w', 'fc2_b')}
    h = torch.nn.functional.linear(P['gvec'], P['fc1_w'].flatten(1), P['fc1_b'])
    hn = (h - d['bn_mean'].to(dtype)) / torch.sqrt(d['bn_var'].to(dtype) + 1e-5) * P['bn_w'] + P['bn_b']
    z = hn * (z_mask > 0).to(dtype)
    a = torch.nn.functional.linear(z, P['fc2_w'].flatten(1), P['fc2_b'])
    att = torch.softmax(a.view(a.shape[0], 2, -1), dim=1)
    grads = torch.autograd.grad((att * d['datt'].to(dtype)).sum(), list(P.values()))
    out = dict(zip(P, grads))
    out['dg'] = out.pop('gvec')
    return out


def rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))
