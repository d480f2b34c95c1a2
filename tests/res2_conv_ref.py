"""fp64 references and per-element bars for the Res2Net slice kernels (csrc/res2net.hip): the slice conv's forward, data gradient and
weight gradient, and the last slice's average pool with its backward.  Pure torch-CPU.

Reference: ``F.conv2d`` in fp64 (and its two adjoints, ``torch.nn.grad.conv2d_input`` / ``conv2d_weight``) on the fp32 operands as the
kernels read them: where an ``add`` operand is given the input is the fp32-rounded sum ``x + add`` (the kernel rounds it once).  Bars, from
the constants of tests/conv_fp64_ref.py, in the form of tests/grouped_conv_ref.py:

* forward:          ``ACC_REL * conv2d(|x|, |w|) * |scale| + ULP32 * |ref|``
* data gradient:    ``ACC_REL * conv2d_input(|dy|, |w * scale|) + ULP32 * |ref|``
* weight gradient:  ``ACC_REL * (|dY|^T |X_tap|) + ULP32 * |ref|``; dY is zero-mean
* pool:             ``ACC_REL * avg_pool2d(|x|) + ULP32 * |ref|`` against fp64 ``F.avg_pool2d(3, 2, 1)`` (count_include_pad: divisor 9),
                    the same count: at most 8 fp32 additions of the 9 taps err by 8 * 2^-24 = 2^-21 of ``sum |x_k|``, and the division
                    by 9 scales sum and error alike and rounds once (the ULP32 term).  The backward is the adjoint, counted likewise
                    (at most 4 windows hold a pixel).

A case is laid out the way a Bottle2neck lays its maps out: the input slice sits at channel ``slice * width`` of a map ``pitch`` channels
wide whose other channels are NaN (the kernel must not read them); the ``add`` operand is another slice of a second such map; the output
goes to yet another slice of a pattern-filled map, of which every other channel must come back unchanged.
"""
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import ACC_REL, ULP32, _threads

# (N, H, W, width, pitch, slice, stride, add): the smallest shapes at which a tile edge, a slice boundary, an odd channel-pair count or
# a stride can go wrong
SHAPES = [
    (2, 7, 9, 26, 128, 0, 1, False),       # map smaller than a block; 13 channel pairs
    (1, 18, 23, 26, 128, 2, 2, False),     # both reach 9 x 12: the data gradient must tell the input sizes apart
    (1, 17, 23, 26, 128, 2, 2, False),
    (3, 17, 24, 52, 224, 1, 1, True),
    (2, 9, 12, 104, 416, 2, 2, False),
    (2, 5, 6, 208, 832, 1, 1, True),
    (2, 5, 6, 208, 832, 0, 2, False),      # -> 3 x 3
    (2, 6, 6, 14, 128, 6, 1, True),        # eight slices of 14: 7 channel pairs, offsets that are no multiple of 4
    (2, 20, 20, 28, 224, 3, 1, True),      # an image boundary inside a pixel quad
    (2, 5, 6, 96, 192, 1, 1, False),       # 48w2s: no pad channels
]


def shape_id(s):
    return 'n%d_%dx%d_w%d_p%d_sl%d_s%d_%s' % (s[:7] + ('add' if s[7] else 'noadd',))


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def slices(shape):
    """-> (input offset, add offset, output offset) in channels: three different slices of the pitch where it holds three."""
    N, H, W, width, pitch, sl, stride, add = shape
    n = pitch // width
    return sl * width, (sl + n - 1) % n * width, (sl + 1) % n * width


def make_case(shape, seed=0):
    """CPU fp32 operands of one shape: x, add (N,width,H,W), w (width,width,3,3), scale / bias (width,), dy (N,width,OH,OW) zero-mean,
    and xin = the operand the conv reads (x, or fl32(x + add))."""
    N, H, W, width, pitch, sl, stride, add = shape
    g = torch.Generator().manual_seed(2000 + seed)
    OH, OW = out_hw(H, W, stride)
    x = torch.randn((N, width, H, W), generator=g)
    a = torch.randn((N, width, H, W), generator=g) if add else None
    w = torch.randn((width, width, 3, 3), generator=g) * (2.0 / (9 * width)) ** 0.5
    scale = torch.rand((width,), generator=g) + 0.5
    scale = scale * torch.where(torch.rand((width,), generator=g) < 0.25, -1.0, 1.0)      # some negative BatchNorm weights
    bias = torch.randn((width,), generator=g) * 0.3
    dy = torch.randn((N, width, OH, OW), generator=g)
    xin = x + a if add else x                  # fp32: rounded once, as the kernel rounds it
    return dict(x=x, add=a, xin=xin, w=w, scale=scale, bias=bias, dy=dy, stride=stride, shape=shape)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def embed(t, pitch, off, fill=float('nan')):
    """NCHW (N,width,H,W) -> the NHWC map (N,H,W,pitch) that holds it at channels [off, off + width) and ``fill`` elsewhere."""
    N, width, H, W = t.shape
    m = torch.full((N, H, W, pitch), fill, dtype=t.dtype)
    m[..., off:off + width] = t.permute(0, 2, 3, 1)
    return m


def pattern(N, H, W, pitch, seed=7):
    """The map an output slice is written into: finite, every element different from its neighbours."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, H, W, pitch), generator=g) * 3.0 + 11.0


def fwd_ref(xin, w, stride, scale=None, bias=None, relu=False):
    """-> (ref, bar), NHWC fp64."""
    _threads()
    x64, w64 = xin.double(), w.double()
    ref = F.conv2d(x64, w64, None, stride, 1)
    mag = F.conv2d(x64.abs(), w64.abs(), None, stride, 1)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
        mag = mag * scale.double().abs().view(1, -1, 1, 1)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def dgrad_ref(dy, w, stride, in_hw, scale=None):
    """Data gradient of conv2d(x, w) * scale[c] with respect to x -> (ref, bar), NHWC fp64."""
    _threads()
    N, C = dy.shape[:2]
    ws = w.double() if scale is None else w.double() * scale.double().view(-1, 1, 1, 1)
    shape = (N, C) + tuple(in_hw)
    ref = torch.nn.grad.conv2d_input(shape, ws, dy.double(), stride, 1)
    mag = torch.nn.grad.conv2d_input(shape, ws.abs(), dy.double().abs(), stride, 1)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def wgrad_ref(dy, xin, stride):
    """-> (ref, bar) in the parameter's layout (width, width, 3, 3), fp64."""
    _threads()
    shape = (dy.shape[1], xin.shape[1], 3, 3)
    ref = torch.nn.grad.conv2d_weight(xin.double(), shape, dy.double(), stride, 1)
    mag = torch.nn.grad.conv2d_weight(xin.double().abs(), shape, dy.double().abs(), stride, 1)
    return ref, ACC_REL * mag + ULP32 * ref.abs()


def pool_ref(x, stride):
    """The last slice: AvgPool2d(3, 2, 1) (divisor 9) at stride 2, the copy at stride 1 -> (ref, bar), NHWC fp64."""
    _threads()
    if stride == 1:
        return nhwc(x.double()), nhwc(torch.zeros_like(x, dtype=torch.float64))
    ref = F.avg_pool2d(x.double(), 3, 2, 1)
    mag = F.avg_pool2d(x.double().abs(), 3, 2, 1)
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())


def pool_bwd_ref(dy, stride, in_hw):
    """Its adjoint -> (ref, bar), NHWC fp64."""
    _threads()
    if stride == 1:
        return nhwc(dy.double()), nhwc(torch.zeros_like(dy, dtype=torch.float64))

    def adj(d):
        z = torch.zeros((d.shape[0], d.shape[1]) + tuple(in_hw), dtype=torch.float64, requires_grad=True)
        F.avg_pool2d(z, 3, 2, 1).backward(d)
        return z.grad
    ref, mag = adj(dy.double()), adj(dy.double().abs())
    return nhwc(ref), nhwc(ACC_REL * mag + ULP32 * ref.abs())
