"""fp64 references and bars for the dilated 3x3 convolution kernels (cpr_conv2d_fwd_dil, cpr_conv2d_wgrad_dil, cpr_conv_group_fwd_dil,
cpr_conv_group_wgrad_dil): forward, data gradient and weight gradient, dense and grouped.  Pure torch-CPU.

Reference: ``F.conv2d(..., padding=d, dilation=d, groups=G)`` in fp64 and its two autograd adjoints (``torch.nn.grad.conv2d_input`` /
``conv2d_weight``) on the fp32 operands as the kernels read them, over the WHOLE tensor (the maps are small).  The bars are the
project's existing ones, with the dilation carried into the magnitude convolutions and nothing else changed:

* dense forward and data gradient (tests/conv_fp64_ref.py): ``ACC_REL * sum_k |x_k w_k| * |scale|`` plus one fp32 ulp of the
  intermediate each rounded epilogue step produces (scale, bias, residual add); a ReLU mask zeroes value and bar together.  The data
  gradient is the same conv over dy with the pack of ``w * scale``: the reference takes that product rounded to fp32, the value the pack
  kernel writes, so no allowance for it is needed.  Column sums: ``conv_fp64_ref.slot_refs`` with the whole tensor as the one slot.
* dense weight gradient (tests/wgrad_fp64_ref.py): ``ACC_REL * |dY|^T |X_tap| + ULP32 * |ref|``; dy is zero-mean.
* grouped layers (tests/grouped_conv_ref.py): the same forms with the magnitudes inside the group only.

One large dense forward case reaches the <128, 128> tile; it is checked on sampled output pixels (conv_fp64_ref.sample_pixels) with
the im2col patches taken at the dilated taps."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import ACC_REL, ULP32, _rows, _threads, _vec, _wmat, sample_pixels, slot_refs  # noqa: F401

# (N, H, W, Cin, Cout, d): stride 1, padding d
DENSE = [
    (2, 5, 6, 64, 64, 2),          # less than one tile, two images inside it
    (1, 3, 3, 64, 32, 4),          # d exceeds the map: only the centre tap is ever in range
    (2, 9, 12, 32, 96, 4),         # one K chunk per tap, ragged cout tile, ragged second pixel tile
    (3, 13, 11, 128, 160, 3),      # odd d, odd map, three images
    (1, 16, 16, 32, 64, 2),        # whole tiles only
    (2, 12, 10, 512, 512, 2),      # the long-K loop at layer4's width
]
WGRAD_SLABS = (4, 40, 40, 64, 64, 2)      # enough pixels (200 chunks of 32) that the split has many slabs of several chunks
BIG_TILE = (1, 512, 512, 64, 256, 2)      # Kpad / 32 = 18 >= 16 and 4096 tiles of 128 x 128: the <128, 128> instance (sampled pixels)
# (N, H, W, C, cg, d)
GROUPED = [
    (2, 5, 6, 128, 4, 2),
    (2, 9, 12, 64, 16, 4),
    (3, 13, 11, 96, 24, 3),
    (1, 3, 3, 256, 32, 4),
    (2, 12, 10, 1024, 32, 2),
]


def dense_id(s):
    return 'n%d_%dx%d_c%d_o%d_d%d' % s


def grouped_id(s):
    return 'n%d_%dx%d_c%d_cg%d_d%d' % s


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def make_dense(shape, seed=0):
    """CPU fp32 operands: x (N,Cin,H,W), w (Cout,Cin,3,3), scale / bias (Cout,), residual (N,Cout,H,W), dy (N,Cout,H,W) zero-mean."""
    N, H, W, Cin, Cout, d = shape
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (2.0 / (9 * Cin)) ** 0.5
    scale = torch.rand((Cout,), generator=g) + 0.5
    scale = scale * torch.where(torch.rand((Cout,), generator=g) < 0.25, -1.0, 1.0)      # some negative BatchNorm weights
    bias = torch.randn((Cout,), generator=g) * 0.3
    res = torch.randn((N, Cout, H, W), generator=g)
    dy = torch.randn((N, Cout, H, W), generator=g)
    return dict(x=x, w=w, scale=scale, bias=bias, res=res, dy=dy, d=d, shape=shape)


def make_grouped(shape, seed=0):
    N, H, W, C, cg, d = shape
    g = torch.Generator().manual_seed(3000 + seed)
    x = torch.randn((N, C, H, W), generator=g)
    w = torch.randn((C, cg, 3, 3), generator=g) * (2.0 / (9 * cg)) ** 0.5
    scale = torch.rand((C,), generator=g) + 0.5
    scale = scale * torch.where(torch.rand((C,), generator=g) < 0.25, -1.0, 1.0)
    bias = torch.randn((C,), generator=g) * 0.3
    dy = torch.randn((N, C, H, W), generator=g)
    return dict(x=x, w=w, scale=scale, bias=bias, dy=dy, d=d, groups=C // cg, shape=shape)


def _conv(x, w, d, groups=1):
    return F.conv2d(x, w, None, 1, d, d, groups)


def dense_fwd_ref(x, w, d, scale=None, bias=None, residual=None, relu=False, res_mask=False):
    """-> (ref, bar) NHWC fp64 over the whole tensor; the epilogue order and the bar terms are conv_fp64_ref.reference's."""
    _threads()
    x64, w64 = x.double(), w.double()
    t = _conv(x64, w64, d)
    bar = ACC_REL * _conv(x64.abs(), w64.abs(), d)
    if scale is not None:
        sc = scale.double().view(1, -1, 1, 1)
        t = t * sc
        bar = bar * sc.abs() + ULP32 * t.abs()
    if bias is not None:
        t = t + bias.double().view(1, -1, 1, 1)
        bar = bar + ULP32 * t.abs()
    if residual is not None:
        r = residual.double()
        if res_mask:
            keep = r > 0
            t = torch.where(keep, t, torch.zeros_like(t))
            bar = torch.where(keep, bar, torch.zeros_like(bar))
        else:
            t = t + r
            bar = bar + ULP32 * t.abs()
    if relu:
        t = t.clamp_min(0)
    return nhwc(t), nhwc(bar)


def colsum_ref(ref, bar):
    """Per-channel sums of a whole NHWC output and their bar: conv_fp64_ref.slot_refs with every pixel in the one slot."""
    C = ref.shape[-1]
    t, e = ref.reshape(-1, C), bar.reshape(-1, C)
    M = t.shape[0]
    refs, bars = slot_refs(dict(ref=t, bar32=e), np.arange(M), [0], M, M)
    return refs[0, :, 0], bars[0, :, 0]


def dense_dgrad_ref(dy, w, d, scale=None, groups=1):
    """Data gradient of conv2d(x, w; padding d, dilation d) * scale[c] with respect to x -> (ref, bar) NHWC fp64.  ``w * scale`` is
    taken in fp32 first: the value the data-gradient pack holds."""
    _threads()
    ws = (w if scale is None else w * scale.view(-1, 1, 1, 1)).double()
    N, _, H, W = dy.shape
    shape = (N, w.shape[1] * groups, H, W)
    ref = torch.nn.grad.conv2d_input(shape, ws, dy.double(), 1, d, d, groups)
    mag = torch.nn.grad.conv2d_input(shape, ws.abs(), dy.double().abs(), 1, d, d, groups)
    return nhwc(ref), nhwc(ACC_REL * mag)


def wgrad_ref(dy, x, w_shape, d, groups=1, base=None):
    """-> (ref, bar) in the parameter's layout, fp64; base: the tensor accumulated into (one more rounded addition)."""
    _threads()
    ref = torch.nn.grad.conv2d_weight(x.double(), tuple(w_shape), dy.double(), 1, d, d, groups)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), tuple(w_shape), dy.double().abs(), 1, d, d, groups)
    bar = ACC_REL * mag + ULP32 * ref.abs()
    if base is not None:
        bar = bar + ULP32 * (base.double() + ref).abs()
    return ref, bar


def grouped_fwd_ref(x, w, groups, d, scale=None, bias=None, relu=False):
    """-> (ref, bar) NHWC fp64: grouped_conv_ref.fwd_ref with the dilation."""
    _threads()
    x64, w64 = x.double(), w.double()
    ref = _conv(x64, w64, d, groups)
    mag = _conv(x64.abs(), w64.abs(), d, groups)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
        mag = mag * scale.double().abs().view(1, -1, 1, 1)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def grouped_dgrad_ref(dy, w, groups, d, scale=None):
    """grouped_conv_ref.dgrad_ref with the dilation (``w * scale`` in fp64, one ulp of the result allowed, as there)."""
    _threads()
    N, C, H, W = dy.shape
    ws = w.double() if scale is None else w.double() * scale.double().view(-1, 1, 1, 1)
    ref = torch.nn.grad.conv2d_input((N, C, H, W), ws, dy.double(), 1, d, d, groups)
    mag = torch.nn.grad.conv2d_input((N, C, H, W), ws.abs(), dy.double().abs(), 1, d, d, groups)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def sampled_fwd_ref(x_nhwc, w, d, m, scale=None, bias=None, relu=False):
    """fp64 outputs at flat output pixels m of the dilated 3x3 over NHWC x (any device): (ref (P, Cout), bar (P, Cout)) -- the
    im2col patches of conv_fp64_ref._patches at the dilated taps."""
    _threads()
    N, H, W, Cin = x_nhwc.shape
    mt = torch.as_tensor(m, device=x_nhwc.device)
    n, rem = mt // (H * W), mt % (H * W)
    oy, ox = rem // W, rem % W
    k = torch.arange(3, device=x_nhwc.device)
    iy = oy.view(-1, 1, 1) - d + k.view(1, 3, 1) * d
    ix = ox.view(-1, 1, 1) - d + k.view(1, 1, 3) * d
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    g = x_nhwc[n.view(-1, 1, 1).expand_as(ok), iy.clamp(0, H - 1), ix.clamp(0, W - 1)].cpu().double()
    g = torch.where(ok.cpu().unsqueeze(-1), g, torch.zeros_like(g)).reshape(len(m), -1)
    wm = _wmat(w)
    t = g @ wm
    bar = ACC_REL * (g.abs() @ wm.abs())
    sc, bi = _vec(scale), _vec(bias)
    if sc is not None:
        t = t * sc
        bar = bar * sc.abs() + ULP32 * t.abs()
    if bi is not None:
        t = t + bi
        bar = bar + ULP32 * t.abs()
    if relu:
        t = t.clamp_min(0)
    return t, bar
