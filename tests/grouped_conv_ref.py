"""fp64 references and per-element bars for the grouped 3x3 convolution kernels (csrc/conv_group.hip): forward, data gradient and
weight gradient.  Pure torch-CPU.

Reference: ``F.conv2d(groups=G)`` in fp64 (and its two adjoints, ``torch.nn.grad.conv2d_input`` / ``conv2d_weight``) on the fp32
operands as the kernels read them.  Bars, from the constants of tests/conv_fp64_ref.py (shared by tests/wgrad_fp64_ref.py):

* forward:          ``ACC_REL * conv2d(|x|, |w|, groups) * |scale| + ULP32 * |ref|``
* data gradient:    the same form over the adjoint: ``ACC_REL * conv2d_input(|dy|, |w * scale|, groups) + ULP32 * |ref|`` (the pack
                    rounds ``w * scale`` once; one fp32 rounding of a factor is 1/16 of ACC_REL of its product)
* weight gradient:  ``ACC_REL * (|dY|^T |X_tap| within the group) + ULP32 * |ref|``; dY is zero-mean (tests/wgrad_fp64_ref.py says why)

The magnitudes run within the group only, so a kernel that leaked a product from another group would not be excused by them.
"""
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import ACC_REL, ULP32, _threads
from tests.wgrad_fp64_ref import ACC_REL as WGRAD_ACC_REL

assert WGRAD_ACC_REL == ACC_REL

# (N, H, W, C, cg, stride): the smallest shapes at which a tile edge, a group boundary or a stride can go wrong
SHAPES = [
    (2, 7, 9, 128, 4, 1),        # map smaller than any tile
    (1, 18, 23, 128, 4, 2),      # both reach 9 x 12: the data gradient must tell the input sizes apart
    (1, 17, 23, 128, 4, 2),
    (3, 17, 24, 256, 8, 1),
    (2, 9, 12, 512, 16, 2),
    (2, 5, 6, 1024, 32, 1),
    (2, 5, 6, 1024, 32, 2),      # -> 3 x 3
    (2, 20, 20, 256, 4, 1),      # G = 64, an image boundary inside a pixel tile
    (2, 6, 6, 2048, 32, 1),
]


def shape_id(s):
    return 'n%d_%dx%d_c%d_cg%d_s%d' % s


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def make_case(shape, seed=0):
    """CPU fp32 operands of one shape: x (N,C,H,W), w (C,cg,3,3), scale / bias (C,), dy (N,C,OH,OW) zero-mean."""
    N, H, W, C, cg, stride = shape
    g = torch.Generator().manual_seed(1000 + seed)
    OH, OW = out_hw(H, W, stride)
    x = torch.randn((N, C, H, W), generator=g)
    w = torch.randn((C, cg, 3, 3), generator=g) * (2.0 / (9 * cg)) ** 0.5
    scale = torch.rand((C,), generator=g) + 0.5
    scale = scale * torch.where(torch.rand((C,), generator=g) < 0.25, -1.0, 1.0)      # some negative BatchNorm weights
    bias = torch.randn((C,), generator=g) * 0.3
    dy = torch.randn((N, C, OH, OW), generator=g)
    return dict(x=x, w=w, scale=scale, bias=bias, dy=dy, groups=C // cg, stride=stride, shape=shape)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def fwd_ref(x, w, groups, stride, scale=None, bias=None, relu=False):
    """-> (ref, bar), NHWC fp64."""
    _threads()
    x64, w64 = x.double(), w.double()
    ref = F.conv2d(x64, w64, None, stride, 1, 1, groups)
    mag = F.conv2d(x64.abs(), w64.abs(), None, stride, 1, 1, groups)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
        mag = mag * scale.double().abs().view(1, -1, 1, 1)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def dgrad_ref(dy, w, groups, stride, in_hw, scale=None):
    """Data gradient of conv2d(x, w, groups) * scale[c] with respect to x -> (ref, bar), NHWC fp64."""
    _threads()
    N, C = dy.shape[:2]
    ws = w.double() if scale is None else w.double() * scale.double().view(-1, 1, 1, 1)
    shape = (N, C) + tuple(in_hw)
    ref = torch.nn.grad.conv2d_input(shape, ws, dy.double(), stride, 1, 1, groups)
    mag = torch.nn.grad.conv2d_input(shape, ws.abs(), dy.double().abs(), stride, 1, 1, groups)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def wgrad_ref(dy, x, w_shape, groups, stride):
    """-> (ref, bar) in the parameter's layout (C, cg, 3, 3), fp64."""
    _threads()
    ref = torch.nn.grad.conv2d_weight(x.double(), tuple(w_shape), dy.double(), stride, 1, 1, groups)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), tuple(w_shape), dy.double().abs(), stride, 1, 1, groups)
    return ref, ACC_REL * mag + ULP32 * ref.abs()
