"""fp64 reference of the convolution weight gradients from the operands AS THE KERNEL READS THEM, and the per-entry bars a HIP
weight-gradient kernel must meet.  The counterpart of tests/conv_fp64_ref.py (whose constants, ``ratio`` and thread cap are reused).

Reference.  Per tap, ``dW[:, :, kh, kw] = dY^T (Cout x M) @ X_tap (M x Cin)`` in fp64 on the CPU, M = N * OH * OW output pixels,
``X_tap`` the zero-padded, strided, shifted view of the NHWC input.  With the fused input affine the input is
``relu?(x * a[n] + b[n])`` on REAL pixels only: a padded tap reads 0, not ``relu(b)``.  Next to it the magnitude
``mag = |dY|^T @ |X_tap|`` (``|x a| + |b|`` in place of ``|x|`` under the affine: the fp32 products the kernel rounds, not the
possibly cancelled value).  The whole tensor where that is cheap, else the rows ``co`` and columns ``ci`` of ``sample_channels``
(first and last channel of every 128 / 256 tile and of every 32-wide sub-block, the ragged tail, random ones), always all taps.

Bars (per entry; ``got`` passes where ``|got - ref| <= bar``):

* fp32 kernels (direct, stem): ``ACC_REL * mag + ULP32 * |ref|``, and ``+ ULP32 * |base + ref|`` when the kernel accumulates into
  ``base`` (one more rounded addition).  ``ACC_REL = 2^-20`` is the forward bar.  It carries over to a reduction over pixels because
  a sum of zero-mean products errs by about ``2^-24 * sum |dy x|`` WHATEVER its length or grouping (the roundings are independent
  and of either sign; only a worst-case bound grows with M): a sequential fp32 chain over M = 1e3 .. 4e5 random products, plain and
  ReLU'd x, stays at 0.10 .. 0.19 of this bar and a 64-slab split at <= 0.05, while one dropped pixel exceeds it in 38 .. 100 % of the
  entries at every M up to 4e5 (worst entry >= 20x the bar).  That holds for ZERO-MEAN gradient maps only (a biased map makes ``|ref|`` comparable to ``mag``
  and the sum's own ulps dominate), so every case draws dY from a zero-mean normal.  ``ULP32 * |ref|``: the rounded final sum of
  the split-K partials.
* bf16 kernels: any fp32 operand is first rounded to bf16 with round-to-nearest-even (``.bfloat16()``) -- what the kernels' converts
  do -- and the same bar applies on the rounded operands: bf16 x bf16 products are exact in fp32, the accumulation is fp32.  A
  truncating convert changes an operand by up to a bf16 grid spacing, far outside the bar.
* Winograd F(2x2, 3x3) (conv_wino_wgrad.hip): ``dU_f = sum_tiles V_f Z_f``, ``V = B^T d B``, ``Z = A dY A^T``, ``dg = G^T dU G``.  The
  magnitude goes through the transforms with absolute coefficients: ``|V| = |B|^T |d| |B|`` and ``|Z| = |A| |dY| |A|^T`` per tile
  (partial tiles zero-filled, as the kernel fills them), ``sum_t |V_f| |Z_f|`` per frequency, then ``|G|^T . |G|``.  Constant, by
  counting fp32 roundings to first order, each relative to that magnitude (u = 2^-24): B^T d B is one addition per pass = 2u (the
  fused affine's single fma rounding is part of d's magnitude, +1u); A dY A^T one addition per pass = 2u; the product 1u; G^T dU G two
  additions per pass (the halvings are exact) = 4u: 9u (10u fused) counted, and the tile accumulation errs like the direct
  kernel's pixel accumulation, about 1u of ``sum |V Z|`` for zero-mean products.  ``ACC_REL = 16u`` covers the counted 10u with the
  accumulation's allowance on top: the bar is ``ACC_REL * mag_wino + ULP32 * |ref|``, the direct bar's form.  An fp32 emulation
  (transforms in fp32, one sequential chain over 1e3 .. 1e5 tiles) errs by <= 0.022 of it.  ``mag_wino`` is 6 .. 7x the direct
  ``|dY|^T |X|`` (the absolute coefficients), so this bar is that much blunter than the direct one: the GPU test also prints each
  Winograd case's worst ratio against the direct-magnitude bar, and keeps those cases at M <= 1e5 pixels, where a dropped pixel
  still shows.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import ACC_REL, ULP32, _threads, ratio

WHOLE_LIMIT = 3e9         # Cout * Cin * taps * M products up to which the whole tensor is computed
GROUP_BYTES = 1 << 28     # fp64 bytes of the tap matrix of one group of images


def sample_channels(C, seed=0, n_random=12):
    """Channels to check: first and last of every 32-wide sub-block (hence of every 128 / 256 tile), the ragged tail past the last
    whole 128 tile, random ones.  Sorted int64."""
    rng = np.random.default_rng(seed)
    parts = [np.arange(0, C, 32), np.minimum(np.arange(31, C + 31, 32), C - 1), np.arange(C // 128 * 128, C)[-8:],
             rng.integers(0, C, size=min(n_random, C))]
    return np.unique(np.concatenate(parts).astype(np.int64))


def pick_channels(M, Cout, Cin, taps, seed=0):
    """(co, ci): None (= all) where the whole tensor is cheap, else the samples."""
    if float(M) * Cout * Cin * taps <= WHOLE_LIMIT:
        return None, None
    return sample_channels(Cout, seed), sample_channels(Cin, seed + 1)


def _cpu64(t, bf16):
    t = t.detach()
    if bf16 and t.dtype == torch.float32:
        t = t.bfloat16()                      # round to nearest even, as the kernels' converts do
    return t.cpu().double()


def _input(x, ci, in_ab, in_relu, bf16):
    """(value, magnitude) of the NHWC input at channels ci, fp64, after the fused affine."""
    xs = x.detach() if ci is None else x.detach()[..., torch.as_tensor(ci, device=x.device)]
    v = _cpu64(xs, bf16)
    if in_ab is None:
        return v, v.abs()
    a, b = (t.detach().cpu().double() for t in in_ab)
    if ci is not None:
        a, b = a[:, torch.as_tensor(ci)], b[:, torch.as_tensor(ci)]
    a, b = a[:, None, None, :], b[:, None, None, :]
    mag = (v * a).abs() + b.abs()
    v = v * a + b
    return (v.clamp_min(0) if in_relu else v), mag


def _taps(v, k, s, p, OH, OW):
    """X_tap (M, C) of every tap of the zero-padded map v (N, H, W, C), in (kh, kw) order."""
    vp = F.pad(v, (0, 0, p, p, p, p))
    for kh in range(k):
        for kw in range(k):
            yield kh, kw, vp[:, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s].reshape(-1, v.shape[-1])


def reference(dy, x, k, s, p, in_ab=None, in_relu=False, co=None, ci=None, bf16=False):
    """fp64 weight gradient of a k x k / stride s / padding p conv: dy (N, OH, OW, Cout), x (N, H, W, Cin) NHWC on any device, as
    the kernel reads them.  co / ci: channel samples (None = all).  bf16: fp32 operands are rounded to bf16 first.
    Returns dict(ref, mag: (len(co), len(ci), k, k) fp64, co, ci)."""
    _threads()
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    assert (OH, OW) == ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1), (dy.shape, x.shape, k, s, p)
    d = _cpu64(dy if co is None else dy[..., torch.as_tensor(co, device=dy.device)], bf16).reshape(N, OH * OW, -1)
    v, vm = _input(x, ci, in_ab, in_relu, bf16)
    Co, Ci = d.shape[-1], v.shape[-1]
    ref = torch.zeros((Co, k * k * Ci), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    per = max(1, int(GROUP_BYTES // (OH * OW * k * k * Ci * 8)))       # images per group: the taps of a group side by side, one GEMM
    for n0 in range(0, N, per):
        dg = d[n0:n0 + per].reshape(-1, Co).t().contiguous()
        ref += dg @ torch.cat([xt for _, _, xt in _taps(v[n0:n0 + per], k, s, p, OH, OW)], 1)
        mag += dg.abs() @ torch.cat([xt for _, _, xt in _taps(vm[n0:n0 + per], k, s, p, OH, OW)], 1)
    ref, mag = (t.reshape(Co, k, k, Ci).permute(0, 3, 1, 2).contiguous() for t in (ref, mag))
    return dict(ref=ref, mag=mag, co=co, ci=ci)


def stem_reference(dy, xin, layout):
    """The stem's weight gradient (7 x 7, stride 2, padding 3, 3 -> 64): xin NHWC4 (N, H, W, 4) for layout 0 (its fourth channel has
    no weights), the (N, 3, H, W) planes for layout 1."""
    x = xin[..., :3] if layout == 0 else xin.permute(0, 2, 3, 1)
    return reference(dy, x, 7, 2, 3)


# Winograd F(2x2, 3x3) matrices of csrc/conv_wino_wgrad.hip (tx_row, td_rows, wino_wgrad_reduce_kernel)
BT = torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
AM = torch.tensor([[1., 0], [1, 1], [1, -1], [0, -1]], dtype=torch.float64)
GM = torch.tensor([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)


def wino_tiles(v, d, bt=BT, am=AM):
    """Per-tile transforms of the 3x3 / pad 1 problem: v (N, H, W, Ci) input, d (N, H, W, Co) gradient map, same dtype ->
    V (16, T, Ci) = bt d' bt^T over the 4 x 4 patches, Z (16, T, Co) = am e am^T over the 2 x 2 tiles, T = N * ceil(H / 2) * ceil(W / 2)
    tiles, partial tiles zero-filled.  Pass absolute matrices and maps for the magnitudes."""
    N, H, W, _ = v.shape
    TY, TX = (H + 1) // 2, (W + 1) // 2
    vp = F.pad(v, (0, 0, 1, 2 * TX + 1 - W, 1, 2 * TY + 1 - H))
    dp = F.pad(d, (0, 0, 0, 2 * TX - W, 0, 2 * TY - H))
    pat = [[vp[:, i:i + 2 * TY:2, j:j + 2 * TX:2].reshape(N * TY * TX, -1) for j in range(4)] for i in range(4)]
    til = [[dp[:, a::2, b::2].reshape(N * TY * TX, -1) for b in range(2)] for a in range(2)]
    bt, am = bt.to(v.dtype), am.to(v.dtype)
    rows = [[sum(bt[a, i] * pat[i][j] for i in range(4) if bt[a, i] != 0) for j in range(4)] for a in range(4)]      # B^T d
    V = torch.stack([sum(bt[b, j] * rows[a][j] for j in range(4) if bt[b, j] != 0) for a in range(4) for b in range(4)])
    cols = [[sum(am[j, b] * til[a][b] for b in range(2) if am[j, b] != 0) for j in range(4)] for a in range(2)]      # dY A^T
    Z = torch.stack([sum(am[i, a] * cols[a][j] for a in range(2) if am[i, a] != 0) for i in range(4) for j in range(4)])
    return V, Z


def wino_out(U, gm=GM):
    """dg (Co, Ci, 3, 3) = G^T dU G from dU (16, Ci, Co)."""
    U4 = U.reshape(4, 4, *U.shape[1:])
    g = torch.einsum('ik,jl,ijcd->dckl', gm.to(U.dtype), gm.to(U.dtype), U4)
    return g.contiguous()


def wino_magnitude(dy, x, in_ab=None, co=None, ci=None):
    """``|G|^T (sum_t |V_f| |Z_f|) |G|`` (len(co), len(ci), 3, 3): the Winograd bar's magnitude (module docstring)."""
    _threads()
    d = _cpu64(dy if co is None else dy[..., torch.as_tensor(co, device=dy.device)], False)
    _, vm = _input(x, ci, in_ab, False, False)
    V, Z = wino_tiles(vm, d.abs(), BT.abs(), AM.abs())
    return wino_out(torch.bmm(V.transpose(1, 2), Z), GM.abs())


def bar_fp32(r, base=None, mag=None):
    """The fp32 bar on reference r (``mag``: another magnitude than r's, the Winograd one); base: the tensor accumulated into,
    at r's channels."""
    bar = ACC_REL * (r['mag'] if mag is None else mag) + ULP32 * r['ref'].abs()
    if base is not None:
        bar = bar + ULP32 * (base + r['ref']).abs()
    return bar


def rows_cols(t, co, ci):
    """Entries (co, ci) of a (Cout, Cin, k, k) tensor (any device) as fp64 on the CPU."""
    t = t.detach()
    if co is not None:
        t = t[torch.as_tensor(co, device=t.device)]
    if ci is not None:
        t = t[:, torch.as_tensor(ci, device=t.device)]
    return t.cpu().double()


def check(name, got, ref, bar, co=None, ci=None, tile=128):
    """Assert got (Co, Ci, k, k) is within bar of ref; returns the worst error / bar ratio (NaN counts as over).  The message names
    the first failing (co, ci, kh, kw), their tile (edge ``tile``) and 32-wide sub-block coordinates, got / ref / bar."""
    q = ratio(got, ref, bar)
    q = torch.where(torch.isnan(got.double()), torch.full_like(q, float('inf')), q)
    worst = float(q.max()) if q.numel() else 0.0
    if not worst <= 1.0:
        bad = torch.nonzero(~(q <= 1.0))
        lines = []
        for a, b, kh, kw in bad[:8].tolist():
            o, i = (int(co[a]) if co is not None else a), (int(ci[b]) if ci is not None else b)
            lines.append('(co=%d ci=%d kh=%d kw=%d) tile (%d, %d) sub-block (%d, %d) lane (%d, %d) got=%.9g ref=%.9g bar=%.3g' % (
                o, i, kh, kw, o // tile, i // tile, o % tile // 32, i % tile // 32, o % 32, i % 32,
                float(got[a, b, kh, kw]), float(ref[a, b, kh, kw]), float(bar[a, b, kh, kw])))
        raise AssertionError('%s: %d/%d entries over the bar, worst ratio %.3g\n  %s' % (
            name, bad.shape[0], q.numel(), worst, '\n  '.join(lines)))
    return worst
