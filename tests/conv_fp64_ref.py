"""fp64 reference of the forward convolutions on SAMPLED output pixels, and the bars a HIP kernel instance must meet.

The reference builds the im2col patches of the chosen output pixels only (gathered where the operands live, then fp64 on the
CPU), so launches large enough to reach the <128, 128> tiles stay cheap to check while everything is exact in fp64.  The
epilogue is applied in fp64 in the order the kernels apply it: input affine ``relu?(x * a[n, c] + b[n, c])`` (zero padding
stays zero), ``acc * scale[c] + bias[c]``, the second source of the dual launch, ``+ residual`` or the ReLU mask
``residual > 0 ? v : 0``, ``ReLU``.

Bars (``bar`` is per output element; ``got`` passes where ``|got - ref| <= bar``):

* fp32 outputs: ``2^-20 * |scale| * sum_k |x_k * w_k|`` for each accumulation (fp32 accumulation of K products; the typical
  error is near ``2^-24`` of that sum, the factor 16 is the margin), plus one fp32 ulp (``2^-23 * |t|``) of the intermediate
  ``t`` each rounded epilogue operation produces (scale, bias, shortcut add, residual add).  With the input affine the
  magnitude of tap k is ``(|x_k * a| + |b|) * |w_k|``: the fp32 products the kernel rounds, not the possibly cancelled result.
* bf16 outputs: one bf16 rounding unit of ``|ref|`` -- half the spacing of the bf16 grid in the binade of ``|ref|``, which is
  exactly the round-to-nearest-even bound -- plus the fp32 term.  (A full grid spacing would also pass a truncating store:
  truncation errs by less than one spacing.)  The operands are the bf16 values the kernel reads.
* GroupNorm partials and column sums of a whole slot S (the pixels one kernel slot covers): against the fp64 sums of the
  fp64 reference.  Each summand v_p is the kernel's fp32 epilogue value, ``|v_p - t_p| <= e_p`` (the fp32 bar above), and
  any order of |S| - 1 fp32 additions errs by at most ``(|S| - 1) * 2^-24 * sum |v_p|``:
      sum:    ``sum_p e_p + (|S| - 1) * 2^-24 * sum_p (|t_p| + e_p)``
      sumsq:  ``sum_p (2 |t_p| e_p + e_p^2) + |S| * 2^-24 * sum_p (|t_p| + e_p)^2``  (the squares' rounding, then the sum's)
  Statistics are taken from the fp32 value before any bf16 store, so e_p is the fp32 term even for bf16 outputs.
"""
import numpy as np
import torch

ACC_REL = 2.0 ** -20      # fp32 accumulation bar, relative to sum_k |x_k w_k|
ULP32 = 2.0 ** -23        # one fp32 ulp, relative
U32 = 2.0 ** -24          # fp32 unit roundoff
MAX_THREADS = 16


def _threads():
    if torch.get_num_threads() > MAX_THREADS:
        torch.set_num_threads(MAX_THREADS)


def sample_pixels(N, OH, OW, bm, slot=None, n_slots=3, n_random=300, seed=0):
    """Flat output indices m = (n * OH + oy) * OW + ox to check, and the whole slots among them.
    Always: every border row and column of the first and the last image, every pixel of the last M tile at ``bm`` (the ragged
    one when M % bm != 0), the whole ``bm`` tile that holds the first pixel of the second image (it straddles the image
    boundary when OH * OW % bm != 0), ``n_random`` random pixels.  ``slot`` (pixels per statistics / column-sum slot): the
    first, the last and ``n_slots - 2`` random whole slots are added.  Returns (sorted int64 indices, list of slot numbers)."""
    M = N * OH * OW
    rng = np.random.default_rng(seed)
    parts = []
    for n in sorted({0, N - 1}):
        base = n * OH * OW
        oy, ox = np.meshgrid(np.arange(OH), np.arange(OW), indexing='ij')
        border = (oy == 0) | (oy == OH - 1) | (ox == 0) | (ox == OW - 1)
        parts.append(base + (oy * OW + ox)[border])
    last = (M - 1) // bm * bm
    parts.append(np.arange(last, M))
    if N > 1:
        t0 = (OH * OW) // bm * bm
        parts.append(np.arange(t0, min(t0 + bm, M)))
    parts.append(rng.integers(0, M, size=min(n_random, M)))
    slots = []
    if slot:
        ns = (M + slot - 1) // slot
        slots = sorted({0, ns - 1} | set(int(s) for s in rng.integers(0, ns, size=max(n_slots - 2, 0))))
        for s in slots:
            parts.append(np.arange(s * slot, min((s + 1) * slot, M)))
    m = np.unique(np.concatenate(parts).astype(np.int64))
    return m, slots


def _patches(x, m, OH, OW, KH, KW, stride, pad, in_ab=None, in_relu=False):
    """(P, KH * KW * Cin) fp64 patches of output pixels m of NHWC x (any device), K ordered (kh, kw, cin), and the
    per-element magnitudes the bar uses."""
    N, H, W, Cin = x.shape
    mt = torch.as_tensor(m, device=x.device)
    n, rem = mt // (OH * OW), mt % (OH * OW)
    oy, ox = rem // OW, rem % OW
    kh = torch.arange(KH, device=x.device).view(1, KH, 1)
    kw = torch.arange(KW, device=x.device).view(1, 1, KW)
    iy = oy.view(-1, 1, 1) * stride - pad + kh
    ix = ox.view(-1, 1, 1) * stride - pad + kw
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    nn = n.view(-1, 1, 1).expand_as(ok)
    g = x[nn, iy.clamp(0, H - 1), ix.clamp(0, W - 1)].cpu().double()     # (P, KH, KW, Cin): exact copies
    ok = ok.cpu().unsqueeze(-1)
    if in_ab is not None:
        a, b = (t.cpu().double()[n.cpu()].view(-1, 1, 1, Cin) for t in in_ab)
        mag = (g * a).abs() + b.abs()
        g = g * a + b
        if in_relu:
            g = g.clamp_min(0)
    else:
        mag = g.abs()
    g = torch.where(ok, g, torch.zeros_like(g))
    mag = torch.where(ok, mag, torch.zeros_like(mag))
    return g.reshape(len(m), -1), mag.reshape(len(m), -1)


def _wmat(w):
    """(Cout, Cin, KH, KW) -> (K, Cout) fp64 in the (kh, kw, cin) order of the patches."""
    Cout = w.shape[0]
    return w.detach().cpu().double().permute(0, 2, 3, 1).reshape(Cout, -1).t()


def _rows(t, m):
    """Rows m of an NHWC map (any device) as (P, C) fp64."""
    return t.reshape(-1, t.shape[-1])[torch.as_tensor(m, device=t.device)].cpu().double()


def _vec(v):
    return None if v is None else v.detach().cpu().double().view(1, -1)


def reference(x, w, stride, pad, m, scale=None, bias=None, residual=None, relu=False, in_ab=None, in_relu=False,
              res_mask=False, src2=None):
    """fp64 conv outputs at flat output pixels m: dict(ref=(P, Cout), bar32=(P, Cout) fp32 term, out_hw).
    x: NHWC (N, H, W, Cin) as the kernel reads it; w: (Cout, Cin, KH, KW) holding the values the kernel reads (a 4-channel stem
    input takes 3-channel weights: the fourth channel's weights are zero).  src2 = (x2, w2, stride2, scale2, bias2): the 1x1
    second source of the dual launch."""
    _threads()
    N, H, W, Cin = x.shape
    Cout, Cw, KH, KW = w.shape
    if Cw < Cin:
        w = torch.cat([w, w.new_zeros((Cout, Cin - Cw, KH, KW))], 1)
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    g, mag = _patches(x, m, OH, OW, KH, KW, stride, pad, in_ab, in_relu)
    wm = _wmat(w)
    t = g @ wm
    bar = ACC_REL * (mag @ wm.abs())
    sc, bi = _vec(scale), _vec(bias)
    if sc is not None:
        t = t * sc
        bar = bar * sc.abs() + ULP32 * t.abs()
    if bi is not None:
        t = t + bi
        bar = bar + ULP32 * t.abs()
    if src2 is not None:
        x2, w2, s2, sc2, bi2 = src2
        g2, mag2 = _patches(x2, _src2_pixels(m, OH, OW, x2.shape, s2), *x2.shape[1:3], 1, 1, 1, 0)
        wm2 = _wmat(w2)
        t2 = g2 @ wm2
        bar2 = ACC_REL * (mag2 @ wm2.abs())
        sc2, bi2 = _vec(sc2), _vec(bi2)
        if sc2 is not None:
            t2 = t2 * sc2
            bar2 = bar2 * sc2.abs() + ULP32 * t2.abs()
        if bi2 is not None:
            t2 = t2 + bi2
            bar2 = bar2 + ULP32 * t2.abs()
        t = t + t2
        bar = bar + bar2 + ULP32 * t.abs()
    if residual is not None:
        r = _rows(residual, m)
        if res_mask:
            keep = r > 0
            t = torch.where(keep, t, torch.zeros_like(t))
            bar = torch.where(keep, bar, torch.zeros_like(bar))
        else:
            t = t + r
            bar = bar + ULP32 * t.abs()
    if relu:
        t = t.clamp_min(0)
    return dict(ref=t, bar32=bar, out_hw=(OH, OW))


def _src2_pixels(m, OH, OW, x2_shape, s2):
    """The dual launch reads x2 at (n, oy * s2, ox * s2): as a 1x1 / stride 1 / unpadded conv over x2 that is flat pixel
    (n * H2 + oy * s2) * W2 + ox * s2."""
    _, H2, W2, _ = x2_shape
    m = np.asarray(m)
    n, rem = m // (OH * OW), m % (OH * OW)
    oy, ox = rem // OW, rem % OW
    return (n * H2 + oy * s2) * W2 + ox * s2


def bf16_half_ulp(t):
    """Half the bf16 grid spacing in the binade of |t| (0 where t == 0): the round-to-nearest-even bound."""
    _, e = torch.frexp(t)
    return torch.where(t == 0, torch.zeros_like(t), torch.ldexp(torch.ones_like(t), (e - 9).to(torch.int32)))


def out_bar(r, bf16_out):
    """Bar on the stored outputs: the fp32 term, plus the bf16 rounding unit for bf16 stores."""
    return r['bar32'] + bf16_half_ulp(r['ref']) if bf16_out else r['bar32']


def ratio(got, ref, bar):
    """|got - ref| / bar, elementwise (inf where the bar is 0 and the values differ)."""
    d = (got.double() - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / bar)


def check(name, got, ref, bar, m=None, Cout=None, bm=None, OHW=None):
    """Assert got (P, C) is within bar of ref; returns the worst error / bar ratio.  The message names the first failing
    pixels, channels and their tile coordinates (M tile at bm)."""
    q = ratio(got, ref, bar)
    worst = float(q.max()) if q.numel() else 0.0
    if not worst <= 1.0:
        bad = torch.nonzero(~(q <= 1.0))
        lines = []
        for p, c in bad[:8].tolist():
            mm = int(m[p]) if m is not None else p
            where = 'm=%d' % mm
            if OHW is not None:
                n, rem = divmod(mm, OHW[0] * OHW[1])
                where += ' (n=%d oy=%d ox=%d)' % (n, rem // OHW[1], rem % OHW[1])
            if bm is not None:
                where += ' tile_m=%d row=%d' % (mm // bm, mm % bm)
            lines.append('%s c=%d got=%.9g ref=%.9g bar=%.3g' % (where, c, float(got[p, c]), float(ref[p, c]), float(bar[p, c])))
        raise AssertionError('%s: %d/%d outputs over the bar, worst ratio %.3g\n  %s' % (
            name, bad.shape[0], q.numel(), worst, '\n  '.join(lines)))
    return worst


def group_refs(t, e, groups):
    """fp64 (sum, sumsq) per channel over each group of rows of t (P, C) -- ``groups``: index tensors into the rows -- and their bars
    from the per-element bars e (see the module docstring).  Returns (ref (len(groups), C, 2), bar (len(groups), C, 2))."""
    refs, bars = [], []
    for idx in groups:
        ts, es = t[idx], e[idx]
        n = len(idx)
        a = ts.abs() + es
        s_ref, q_ref = ts.sum(0), (ts * ts).sum(0)
        s_bar = es.sum(0) + max(n - 1, 0) * U32 * a.sum(0)
        q_bar = (2 * ts.abs() * es + es * es).sum(0) + n * U32 * (a * a).sum(0)
        refs.append(torch.stack([s_ref, q_ref], -1))
        bars.append(torch.stack([s_bar, q_bar], -1))
    return torch.stack(refs), torch.stack(bars)


def slot_refs(r, m, slots, slot, M):
    """fp64 (sum, sumsq) per channel of each whole slot, and their bars (see the module docstring).
    Returns (ref (len(slots), C, 2), bar (len(slots), C, 2))."""
    pos = {int(v): i for i, v in enumerate(np.asarray(m))}
    return group_refs(r['ref'], r['bar32'], [torch.as_tensor([pos[p] for p in range(s * slot, min((s + 1) * slot, M))]) for s in slots])
