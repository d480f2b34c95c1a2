"""fp64 reference of the dense conv DATA gradient, written from the forward definition, and the bars a data-gradient route must meet.

For the forward ``y = conv2d(x, w * scale[:, None, None, None], stride, padding)`` (NHWC maps, w (Cout, Cin, KH, KW)):

    dx[n, iy, ix, ci] = sum over (co, kh, kw, oy, ox) with oy * s - p + kh == iy and ox * s - p + kw == ix
                        of dy[n, oy, ox, co] * w[co, ci, kh, kw] * scale[co]

No weights are flipped or transposed here and no gradient is zero-inserted: that is what the code under test does.  Every form
returns ``(t, mag)`` as (pixels, Cin) fp64, ``mag = sum |dy| * |w * scale|`` over the same terms (the map is linear, so the same
computation on the absolute values gives it):

* ``full_map``: fp64 autograd of F.conv2d on the CPU, all input pixels (small shapes);
* ``gather``: the terms of chosen input pixels m = (n * H + iy) * W + ix (conv_fp64_ref.sample_pixels over the INPUT map), gathered
  where dy lives, then fp64 on the CPU (large shapes);
* ``tap_scatter``: all input pixels, one fp64 matrix product per tap added at iy = oy * s - p + kh, on dy's device.  It exists for the
  reduced column sums of the large shapes (they need every pixel); a test that uses it pins it to ``gather`` at the sampled pixels.

``finish`` then applies ``+ add`` and the mask ``mask > 0 ? v : 0`` in the order ops.conv2d_dgrad documents (add before mask) and
returns dict(ref, bar32), the contract of conv_fp64_ref.reference / slot_refs.  Bars, per element (constants: conv_fp64_ref):

* fp32 direct / streamed / phased / zero-insertion routes: ``ACC_REL * mag`` (fp32 accumulation), ``+ U32 * mag`` when a scale was
  folded (one fp32 rounding of w * scale in the pack), ``+ ULP32 * |t|`` for the add (one rounded fp32 addition: the conv epilogue, or
  the phase scatter's ``dx += o`` -- every pixel belongs to exactly one parity class).  A masked-off element has bar 0: exactly 0.
  Where no tap reaches a pixel (mag == 0) the bar is 0 too, or one ulp of the add.
* bf16: the operands are the values the kernel reads (``bf16_operands``), so no pack term: ``ACC_REL * mag + ULP32 * |t|`` for the
  add on the fp32 output, plus ``bf16_half_ulp`` on a bf16 output.
* column sums over n summands (a slot, or all pixels for the reduced vector): any order of fp32 additions errs by at most
  ``(n - 1) * U32 * sum (|t_p| + e_p)``, so ``sum e_p + (n - 1) * U32 * sum (|t_p| + e_p) + ULP32 * |sum|`` (``colsum_ref``; per slot
  it is conv_fp64_ref.slot_refs plus the last term).  It bounds the epilogue partials and the streaming relu_bwd_colsum pass alike.
* Winograd route: the project's stated whole-map bound (tests/test_gpu_wino.py), ``1e-5 * max |ref|``, AND beside it the per-element
  Winograd bound of tests/wino_fp64_ref.py (its bar 1): the route runs the two forward Winograd kernels on dy with a flipped pack, so
  ``bar_wino = ACC_REL * mag_wino`` with ``mag_wino`` the magnitude of that forward convolution carried through the transforms with
  absolute coefficients (``wino_magnitude``), ``+ U32 * mag_wino`` for a folded scale.  Both are asserted.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_fp64_ref as R
from tests.conv_fp64_ref import ACC_REL, ULP32, U32, bf16_half_ulp, check, slot_refs      # noqa: F401  (the tests take them from here)

WINO_REL = 1e-5       # tests/test_gpu_wino.py: |wino - fp64| <= 1e-5 * max |fp64|


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def scaled_weights(w, scale):
    """fp64 w * scale[co] (exact: the fp32 route's bar carries the pack's rounding of this product)."""
    w = w.detach().cpu().double()
    return w if scale is None else w * scale.detach().cpu().double().view(-1, 1, 1, 1)


def bf16_operands(dy, w, scale):
    """The values the bf16 kernels read: dy rounded to bf16, and (w * scale) formed in fp32 and then rounded to bf16 -- the expression
    PackedConv.for_dgrad_bf16 promises bit-equality with.  Returns (dy bf16 on its device, weights fp64)."""
    w = w.detach().cpu().float()
    if scale is not None:
        w = w * scale.detach().cpu().float().view(-1, 1, 1, 1)
    return dy.bfloat16(), w.bfloat16().double()


def full_map(dy, ws, stride, pad, in_hw):
    """(t, mag), each (N * H * W, Cin) fp64: fp64 autograd of F.conv2d on the CPU.  dy NHWC (N, OH, OW, Cout), ws fp64 weights."""
    R._threads()
    N, OH, OW, Cout = dy.shape
    H, W = in_hw
    Cin = ws.shape[1]
    g = dy.detach().cpu().double().permute(0, 3, 1, 2).contiguous()

    def run(g, w):
        x = torch.zeros((N, Cin, H, W), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, w, None, stride, pad)
        assert y.shape == g.shape, (y.shape, g.shape)
        dx, = torch.autograd.grad(y, x, g)
        return dx.permute(0, 2, 3, 1).reshape(-1, Cin)
    return run(g, ws), run(g.abs(), ws.abs())


def gather(dy, ws, stride, pad, in_hw, m):
    """(t, mag), each (len(m), Cin) fp64, of input pixels m: the (kh, kw) terms whose oy = (iy + p - kh) / s is a whole output row (the
    same for columns), gathered from dy on its device (exact copies) and multiplied out in fp64 on the CPU."""
    R._threads()
    N, OH, OW, Cout = dy.shape
    H, W = in_hw
    KH, KW = ws.shape[2:]
    mt = torch.as_tensor(np.asarray(m), device=dy.device)
    n, rem = mt // (H * W), mt % (H * W)
    iy, ix = rem // W, rem % W
    ny = iy.view(-1, 1, 1) + pad - torch.arange(KH, device=dy.device).view(1, KH, 1)
    nx = ix.view(-1, 1, 1) + pad - torch.arange(KW, device=dy.device).view(1, 1, KW)
    oy, ox = torch.div(ny, stride, rounding_mode='floor'), torch.div(nx, stride, rounding_mode='floor')
    ok = (oy * stride == ny) & (oy >= 0) & (oy < OH) & (ox * stride == nx) & (ox >= 0) & (ox < OW)      # (P, KH, KW)
    nn = n.view(-1, 1, 1).expand_as(ok)
    g = dy[nn, oy.clamp(0, OH - 1), ox.clamp(0, OW - 1)].cpu().double()                                    # (P, KH, KW, Cout)
    g = torch.where(ok.cpu().unsqueeze(-1), g, torch.zeros_like(g)).reshape(len(mt), -1)
    wt = ws.permute(2, 3, 0, 1).reshape(KH * KW * Cout, -1)                                                # (kh, kw, co) x ci
    return g @ wt, g.abs() @ wt.abs()


def tap_scatter(dy, ws, stride, pad, in_hw):
    """(t, mag), each (N * H * W, Cin) fp64 on dy's device: per tap, dy @ w[:, :, kh, kw] added at iy = oy * s - p + kh."""
    N, OH, OW, Cout = dy.shape
    H, W = in_hw
    Cin, KH, KW = ws.shape[1:]
    g = dy.double()
    w = ws.to(dy.device)
    t = torch.zeros((N, H, W, Cin), dtype=torch.float64, device=dy.device)
    mag = torch.zeros_like(t)

    def span(O, L, k):       # output indices o with 0 <= o * s - p + k < L
        lo = max(0, -((k - pad) // stride))
        hi = min(O - 1, (L - 1 + pad - k) // stride)
        return lo, hi
    for kh in range(KH):
        y0, y1 = span(OH, H, kh)
        for kw in range(KW):
            x0, x1 = span(OW, W, kw)
            if y1 < y0 or x1 < x0:
                continue
            src = g[:, y0:y1 + 1, x0:x1 + 1]
            iy0, ix0 = y0 * stride - pad + kh, x0 * stride - pad + kw
            dst = (slice(None), slice(iy0, iy0 + (y1 - y0) * stride + 1, stride), slice(ix0, ix0 + (x1 - x0) * stride + 1, stride))
            t[dst] += src @ w[:, :, kh, kw]
            mag[dst] += src.abs() @ w[:, :, kh, kw].abs()
    return t.reshape(-1, Cin), mag.reshape(-1, Cin)


def rows(t, m=None):
    """An NHWC map (any device) as (pixels, C) fp64 on the CPU; m: those flat pixels only."""
    t = t.reshape(-1, t.shape[-1])
    if m is not None:
        t = t[torch.as_tensor(np.asarray(m), device=t.device)]
    return t.cpu().double()


def wino_magnitude(dy, ws, m):
    """``mag_wino`` (len(m), Cin) of the data gradient as the Winograd route computes it: the 3x3 / pad 1 FORWARD convolution of dy with
    the pack's weights w'[ci, co, a, b] = ws[co, ci, 2 - a, 2 - b], through wino_fp64_ref.magnitude."""
    from tests import wino_fp64_ref as WR
    return WR.magnitude(dy, ws.flip(2, 3).transpose(0, 1).contiguous(), m)


def finish(t, mag, add=None, mask=None, scaled=False, bf16=False, wino=False, mag_wino=None):
    """Add, then mask, and the per-element bar.  t, mag, add, mask: (P, C) fp64 rows on one device.  scaled: a scale was folded into an
    fp32 pack; bf16: t was computed from ``bf16_operands``; wino: the Winograd route's bars (mag_wino: ``wino_magnitude`` at the same
    pixels).  Returns dict(ref, bar32), on the Winograd route also bar_wino."""
    if wino:
        assert add is None and mask is None and not bf16 and mag_wino is not None
        return dict(ref=t, bar32=torch.full_like(t, WINO_REL * float(t.abs().max())),
                    bar_wino=(ACC_REL + (U32 if scaled else 0.0)) * mag_wino)
    bar = ACC_REL * mag
    if scaled and not bf16:
        bar = bar + U32 * mag
    if add is not None:
        t = t + add
        bar = bar + ULP32 * t.abs()
    if mask is not None:
        keep = mask > 0
        t = torch.where(keep, t, torch.zeros_like(t))
        bar = torch.where(keep, bar, torch.zeros_like(bar))
    return dict(ref=t, bar32=bar)


def colsum_ref(r):
    """Column sums over ALL rows of r: (ref (C,), bar (C,)), see the module docstring."""
    t, e = r['ref'], r['bar32']
    n = t.shape[0]
    s = t.sum(0)
    return s, e.sum(0) + max(n - 1, 0) * U32 * (t.abs() + e).sum(0) + ULP32 * s.abs()


def all_slot_colsum_refs(r, slot):
    """Column sums of EVERY slot of ``slot`` consecutive rows of r (all rows of the map; the last slot may be short):
    (ref (slots, C), bar (slots, C)), the bound of ``colsum_ref`` per slot."""
    t, e = r['ref'], r['bar32']
    M, C = t.shape
    S = (M + slot - 1) // slot
    pad = (lambda v: torch.cat([v, v.new_zeros((S * slot - M, C))]).view(S, slot, C))
    n = torch.full((S, 1), slot, dtype=t.dtype, device=t.device)
    n[-1] = M - (S - 1) * slot
    s = pad(t).sum(1)
    return s, pad(e).sum(1) + (n - 1) * U32 * pad(t.abs() + e).sum(1) + ULP32 * s.abs()


def slot_colsum_refs(r, m, slots, slot, M):
    """Column sums of whole slots (``slot`` pixels each; m must hold them): (ref (len(slots), C), bar (len(slots), C))."""
    ref, bar = slot_refs(r, m, slots, slot, M)
    ref, bar = ref[..., 0], bar[..., 0]
    return ref, bar + ULP32 * ref.abs()
