"""fp64 references of the CPR point kernels (csrc/cpr_points.hip: cpr_box_centers, cpr_neg_mask_loss, cpr_bag_sample,
cpr_grid_bag, cpr_mil_loss, cpr_refine), the bars a HIP kernel must meet, and fp32 CPU emulations of the kernels' formulas
(``emu_*``) that tests/test_cpr_points_host.py uses to show the bars pass the right formula and fail the wrong ones.

References are fp64 from the operands AS THE KERNEL READS THEM: the fp32 maps, centres, ring offsets (host made), the fp32
``d2_thr`` / ``radius_px`` / thresholds / eps handed in.  Bag points are one fp32 addition (IEEE: the reference forms the same
fp32 value) and grid points ``x * stride + stride / 2`` are exact at the strides used (asserted), so point coordinates, the
validity against the padded image and the inside-image test are EXACT: compared with ``==``, never ambiguous.

u = U32 = 2^-24 (one rounding errs by at most u of the rounded value), ULP32 = 2u, g(n) = n u / (1 - n u), D64 = 2^-48 for the
order of double additions.  ``got`` passes where ``|got - ref| <= bar`` (conv_fp64_ref.ratio).

TRANS_ULP = 4.  Device expf / logf / powf are not correctly rounded.  The installed ROCm ships no math accuracy table (nothing
under its share/ or doc/ directories states ulp figures), so 4 ulp per call is a stated cap (the published HIP figures are 1 ulp
for expf and powf, 1 - 2 for logf); the Sleef expf replay of sigmoid_torch_cpu is a 1-ulp routine and sits under the same cap.
T = TRANS_ULP * ULP32 is that cap as a relative error.  It is a cap and not a measurement: the errors these tests look for (a
dropped entry, a wrong slot, a wrong tap) are orders of magnitude larger, which the host file shows.

Bars, by counting the kernel's roundings:

* box centres ``(a + b) / 2``: one rounded sum, an exact halving: ``u |ref|``.
* probabilities (``prob``): sigmoid ``1 / (1 + e)``, e = exp(-x) within T: the sum carries ``e T / (1 + e) + u = (1 - p) T + u``,
  the division u: ``p ((1 - p) T + 2 ULP32)``.  softmax: each exponent ``l_j - m`` is rounded (absolute u |l_j - m|, which the
  exponential turns into a relative error) and exponentiated (T), C terms are added, one division:
  ``p (2 T + 2 u max|l - m| + g(C + 1))``.  normed_sigmoid: the norm carries the largest relative sigmoid bar, g(C + 2) for its
  sum, square / root and, for p not in {1, 2}, two powf calls (T / p + T), the rounded exponent 1 / p (``u |ln nrm| / p``) -- and
  the quotient one more u.  identity: the value itself, bar 0.
* squared distance of d2_chain (``[-2x, -2y, |p|^2, 1] . [cx, cy, 1, |c|^2]``, four chained operations on magnitudes up to
  M = |p|^2 + |c|^2, the two squared norms three roundings each): at most ``u (6 M + d2)``, d2 <= 2 M: ``g(8) M``.  On the
  dyadic grid of the EXACT cases (multiples of 1/8 px below 256 px) every product and sum is exact: bar 0.
* grid_select distance ``sqrt(fma(dy, dy, dx * dx))``: dx, dy rounded (u each, 2 u on the squares), the product, the fma, the
  root (half of what is under it, plus u): ``g(4) d``; exact on the dyadic grid (3-4-5 triangles).
* nearest-candidate distance of refine: compared in d2 space with ``g(8) M + 2 ULP32 d2`` (the rounded root may merge squared
  distances one or two ulps apart).
* negative-branch term ``t = -(p p) log(a)``, a = 1 - p + eps: ``da = bar_p + 2 u a``; log(a) errs by ``da / a + T |log a|`` (the
  conditioning of the logarithm near a = 0); ``dt = |log a| (2 p bar_p + 3 u p^2) + p^2 (da / a + T |log a|) + u |t|``.  The
  kernel widens each term to double and adds in double: an image's sum carries ``sum dt + D64 sum |t|``; a pixel whose mask is
  AMBIGUOUS adds its ``|t|`` (either branch).  gfocal_term is the same with ``(p - q)^2`` and ``a = p + eps`` for q = 1.
* bilinear sample: the coordinate round trip ``pt / stride -> normalise -> un-normalise`` reduces to ``ix = pt / stride`` (both
  forms); in fp32 its seven operations on magnitudes up to ``A = 2 |q| + 1`` and W leave ``|d ix| <= 4 u (A + W)`` (border form) or
  ``6 u (|q| + W)`` (align_corners form).  Bilinear sampling -- with the border clip, or extended by the pad value / zero outside the
  map -- is continuous and piecewise linear, so the value moves by at most ``|d ix| Sx + |d iy| Sy`` with Sx, Sy the largest
  difference between neighbouring taps in the 5 x 5 cells around the point (no element is excluded at a cell boundary); the
  weights (one rounded complement, one product), the four products and three sums add ``g(8) sum w |tap|``.
* MIL bag probability ``p = sum_k x_k pi_k / sum_k pi_k``, ``pi_k = exp(l_k - m) / se * w_k``: the same rounded ``se`` divides
  numerator and denominator and cancels; each weight carries ``rho_k = T + u |l_k - m| + 2 u``; a weighted mean moves by
  ``sum_k what_k rho_k |x_k - p|`` under relative weight errors (first order; a 1e-3 margin covers the rest) and by
  ``sum_k what_k bar_x_k`` for the class probabilities; the two sums and the division add
  ``(g(K + 1) + g(K) + u) sum what |x|``.  A bag without a valid entry gives exactly 0.  The ``max(sv, 1e-12)`` clamp is never
  approached by the table (asserted: sv = 0 or sv > 1e-6).  The bag loss adds its C (1 + binary) terms in fp32:
  ``sum dt + g(terms) sum |t|``.  AllPosLoss: ``sum dt w + g(K C + 7) sum |t| w``.
* loss_finalize from the kernel's OWN bag workspace and negative partials (double sums, one float store each):
  ``ULP32 |ref| + D64 (summed magnitudes)``; ``bag_acc`` and ``num_sample`` are integer arithmetic in double: exact.
* refine: the kept probabilities' bars enter the weighted mean as in the MIL bag (``sum |x_k - X| bar_p_k / D``), the
  quotient, product and sums ``(g(n + 2) + 3 u) sum |x| p / D``; ``score = sw / (n + 1e-8)``:
  ``(sum bar_p + g(n) sw) / n + 2 u score``; the ``max`` score: the largest kept bar.

Discrete outputs are compared with the fp64 decision.  An element is AMBIGUOUS when the fp64 margin of its deciding comparison
lies inside the propagated bar (d2 against d2_thr, distance against radius_px, p against merge_th / the gate, the arg-max gap,
the nearest-candidate gap, the score against refine_th); it accepts either branch and counts towards AMBIG_CAP = 1e-3 of the
case's elements of that output.  A bag or gt with an ambiguous member has its dependent float outputs skipped and counts at bag /
gt granularity.  EXACT cases have zero bars on every distance: ties are decided as the kernel documents (``>=`` at the mask
threshold, ``<=`` at the radius, first candidate, lowest class) and nothing may be ambiguous.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import U32, ULP32, ratio  # noqa: F401  (re-exported)
from tests.stream_fp64_ref import D64, g  # noqa: F401

TRANS_ULP = 4
T = TRANS_ULP * ULP32
AMBIG_CAP = 1e-3
MARGIN = 1 + 1e-3        # second-order terms of the weighted-mean bars
F32_EPS_REFINE = float(np.float32(1e-8))
PROB = {'sigmoid': 0, 'softmax': 1, 'normed_sigmoid': 2, 'identity': 3}


def f32(v):
    return float(np.float32(v))


def first_argmax(t, dim=-1):
    """Index of the FIRST maximum (torch.argmax does not promise it)."""
    return torch.from_numpy(np.argmax(t.numpy(), axis=dim))


def first_argmin(t, dim=-1):
    return torch.from_numpy(np.argmin(t.numpy(), axis=dim))


# ---- probabilities ----------------------------------------------------------------------------------------------------
def prob(l, ptype, norm_p=1.0):
    """l (..., C) fp64 class logits -> (p, bar), each (..., C)."""
    C = l.shape[-1]
    if ptype == 3:
        return l, torch.zeros_like(l)
    s = torch.sigmoid(l)
    rs = (1 - s) * T + 2 * ULP32
    if ptype == 0:
        return s, s * rs
    if ptype == 1:
        m = l.max(-1, keepdim=True)[0]
        p = torch.softmax(l, -1)
        spread = (l - m).abs().max(-1, keepdim=True)[0]
        return p, p * (2 * T + 2 * U32 * spread + g(C + 1))
    P = f32(norm_p)
    nrm = (s ** P).sum(-1, keepdim=True) ** (1 / P)
    rel = rs.max(-1, keepdim=True)[0] + g(C + 2)
    if P not in (1.0, 2.0):
        rel = rel + T / P + T + U32 * nrm.log().abs() / P + U32
    p = s / nrm.clamp_min(1e-12)
    return p, p * (rs + rel + U32)


def gfocal_ref(p, bp, q, eps):
    """-(p - q)^2 log(q ? p + eps : 1 - p + eps) and its bar; q a bool tensor broadcastable to p."""
    qd = q.double()
    a = torch.where(q, p + eps, 1 - p + eps)
    L = a.log()
    l1 = (p - qd) ** 2
    t = -(l1 * L)
    da = bp + 2 * U32 * a.abs()
    dt = L.abs() * (2 * (p - qd).abs() * bp + 3 * U32 * l1) + l1 * (da / a + T * L.abs()) + U32 * t.abs()
    return t, dt


# ---- distances ---------------------------------------------------------------------------------------------------------
def grid_xy(H, W, stride):
    """Cell centres as the kernels form them in fp32, ``x * stride + stride * 0.5``; exact at the strides used."""
    s = np.float32(stride)
    x = np.arange(W, dtype=np.float32) * s + s * np.float32(0.5)
    y = np.arange(H, dtype=np.float32) * s + s * np.float32(0.5)
    assert np.array_equal(x.astype(np.float64), np.arange(W) * float(s) + float(s) / 2), 'grid points are not exact at this stride'
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))


def d2_pair(px, py, cx, cy, exact):
    d2 = (px - cx) ** 2 + (py - cy) ** 2
    if exact:
        return d2, torch.zeros_like(d2)
    return d2, g(8) * (px * px + py * py + cx * cx + cy * cy) + torch.zeros_like(d2)


# ---- cpr_box_centers -------------------------------------------------------------------------------------------------
def centers_ref(boxes):
    b = boxes.double()
    ref = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2], -1)
    return ref, U32 * ref.abs()


def emu_centers(boxes):
    return torch.stack([(boxes[:, 0] + boxes[:, 2]) * 0.5, (boxes[:, 1] + boxes[:, 3]) * 0.5], -1)


# ---- cpr_neg_mask_loss -------------------------------------------------------------------------------------------------
def _pixels(H, W, stride):
    gx, gy = grid_xy(H, W, stride)
    return gx.repeat(H), gy.repeat_interleave(W)


def neg_ref(i):
    """-> dict mask (N, HW, C) bool, amb (same), img_sum / img_bar (N), total / total_bar."""
    lg = i['logit'].double()
    N, H, W, J = lg.shape
    C, Cm, HW = i['C'], i['Cm'], H * W
    px, py = (t.double() for t in _pixels(H, W, i['stride']))
    thr, eps = f32(i['d2_thr']), f32(i['eps'])
    mask = torch.zeros((N, HW, C), dtype=torch.bool)
    amb = torch.zeros_like(mask)
    img_sum, img_bar = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    inf = torch.full((HW,), float('inf'), dtype=torch.float64)
    for n in range(N):
        g0, g1 = int(i['gt_start'][n]), int(i['gt_start'][n + 1])
        c, lab = i['ctr'][g0:g1].double(), i['labels'][g0:g1]
        d2, bar = d2_pair(px[:, None], py[:, None], c[None, :, 0], c[None, :, 1], i['exact'])
        ph, pw = float(i['pad_hw'][n][0]), float(i['pad_hw'][n][1])
        ins = (0 <= px) & (px < pw) & (0 <= py) & (py < ph)
        for cls in range(C):
            sel = torch.ones_like(lab, dtype=torch.bool) if not i['class_wise'] else lab == (cls if cls < Cm else Cm - 1)
            if bool(sel.any()):
                lo, hi, mid = (d2 - bar)[:, sel].min(1)[0], (d2 + bar)[:, sel].min(1)[0], d2[:, sel].min(1)[0]
            else:
                lo = hi = mid = inf
            mask[n, :, cls] = ins & (mid >= thr)
            amb[n, :, cls] = ins & ~(lo >= thr) & ~(hi < thr)
        p, bp = prob(lg[n].reshape(HW, J)[:, :C], i['ptype'], i['norm_p'])
        t, dt = gfocal_ref(p, bp, torch.zeros_like(p, dtype=torch.bool), eps)
        keep, either = mask[n] & ~amb[n], amb[n]
        img_sum[n] = (t * (mask[n]).double()).sum()
        img_bar[n] = (dt * keep.double()).sum() + (t.abs() * either.double()).sum() + (dt * either.double()).sum() + D64 * t.abs().sum()
    return dict(mask=mask, amb=amb, img_sum=img_sum, img_bar=img_bar, total=img_sum.sum(), total_bar=img_bar.sum())


def _fma32(a, b, c):
    """fp32 fma through double: the product of two fp32 values is exact in double."""
    return (a.double() * b.double() + c.double()).float()


def _d2_chain32(px, py, cx, cy):
    pn = px * px + py * py
    cn = cx * cx + cy * cy
    acc = (-2 * px) * cx
    acc = _fma32(-2 * py, cy, acc)
    acc = pn + acc
    return (acc + cn).clamp_min(0)


def emu_prob(l, ptype, norm_p=1.0):
    """fp32 torch restatement of cls_prob / bag_prob."""
    if ptype == 3:
        return l
    if ptype == 0:
        return torch.sigmoid(l)
    if ptype == 1:
        return torch.softmax(l, -1)
    s = torch.sigmoid(l)
    return s / (s ** norm_p).sum(-1, keepdim=True).pow(1 / norm_p).clamp_min(1e-12)


def emu_neg(i, wrong=None):
    """wrong: 'gt' (> at the threshold), 'first1024' (the gts past the first LDS chunk unseen), 'noeps'."""
    lg = i['logit']
    N, H, W, J = lg.shape
    C, Cm, HW = i['C'], i['Cm'], H * W
    px, py = _pixels(H, W, i['stride'])
    thr, eps = np.float32(i['d2_thr']), (0.0 if wrong == 'noeps' else f32(i['eps']))
    mask = torch.zeros((N, HW, C), dtype=torch.bool)
    sums = torch.zeros(N, dtype=torch.float64)
    for n in range(N):
        g0, g1 = int(i['gt_start'][n]), int(i['gt_start'][n + 1])
        if wrong == 'first1024':
            g1 = min(g1, g0 + 1024)
        c, lab = i['ctr'][g0:g1], i['labels'][g0:g1]
        d2 = _d2_chain32(px[:, None], py[:, None], c[None, :, 0], c[None, :, 1])
        ph, pw = float(i['pad_hw'][n][0]), float(i['pad_hw'][n][1])
        ins = (0 <= px) & (px < pw) & (0 <= py) & (py < ph)
        for cls in range(C):
            sel = torch.ones_like(lab, dtype=torch.bool) if not i['class_wise'] else lab == (cls if cls < Cm else Cm - 1)
            dmin = d2[:, sel].min(1)[0] if bool(sel.any()) else torch.full((HW,), float('inf'))
            mask[n, :, cls] = ins & ((dmin > float(thr)) if wrong == 'gt' else (dmin >= float(thr)))
        p = emu_prob(lg[n].reshape(HW, J)[:, :C], i['ptype'], i['norm_p'])
        t = -(p * p) * torch.log(1 - p + eps)
        sums[n] = (t.double() * mask[n].double()).sum()
    return dict(mask=mask, img_sum=sums)


# ---- bilinear sampling -------------------------------------------------------------------------------------------------
def sample_ref(m, px, py, stride, align, pad=None):
    """m (H, W, J) fp64 map, px / py (P,) fp64 image points -> ref (P, J), bar (P, J), dropped (P,) taps outside the map
    (align_corners form; always 0 for the border form)."""
    H, W, J = m.shape
    s = f32(stride)
    qx, qy = px / s, py / s
    if align:
        B = 2
        pv = pad.double() if pad is not None else torch.zeros(J, dtype=torch.float64)
        E = pv.view(1, 1, J).expand(H + 2 * B, W + 2 * B, J).clone()
        E[B:B + H, B:B + W] = m
        ix, iy = qx.clamp(-1, W) + B, qy.clamp(-1, H) + B
        dix, diy = 6 * U32 * (qx.abs() + W), 6 * U32 * (qy.abs() + H)
        x0u, y0u = qx.floor(), qy.floor()
        nx = ((x0u >= 0) & (x0u <= W - 1)).long() + ((x0u + 1 >= 0) & (x0u + 1 <= W - 1)).long()
        ny = ((y0u >= 0) & (y0u <= H - 1)).long() + ((y0u + 1 >= 0) & (y0u + 1 <= H - 1)).long()
        dropped = 4 - nx * ny
    else:
        E = m
        ix, iy = qx.clamp(0, W - 1), qy.clamp(0, H - 1)
        dix, diy = 4 * U32 * (2 * qx.abs() + 1 + W), 4 * U32 * (2 * qy.abs() + 1 + H)
        dropped = torch.zeros(px.shape, dtype=torch.long)
    EH, EW = E.shape[:2]
    x0, y0 = ix.floor().clamp(max=EW - 1), iy.floor().clamp(max=EH - 1)
    fx, fy = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=EW - 1), (y0 + 1).clamp(max=EH - 1)
    w = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
    taps = [E[y0, x0], E[y0, x1], E[y1, x0], E[y1, x1]]
    ref = sum(wt[:, None] * tp for wt, tp in zip(w, taps))
    mag = sum(wt[:, None] * tp.abs() for wt, tp in zip(w, taps))

    def slope(axis):
        if E.shape[axis] < 2:
            return torch.zeros((px.shape[0], J), dtype=torch.float64)
        d = (E[:, 1:] - E[:, :-1]).abs() if axis == 1 else (E[1:] - E[:-1]).abs()
        d = F.pad(d.permute(2, 0, 1), (0, 1, 0, 0) if axis == 1 else (0, 0, 0, 1))
        d = F.max_pool2d(d[None], 5, 1, 2)[0]
        return d[:, y0, x0].t()

    bar = dix[:, None] * slope(1) + diy[:, None] * slope(0) + g(8) * mag
    return ref, bar, dropped


def emu_sample(m, px, py, stride, align, pad=None, wrong=None):
    """fp32 restatement of sample_point4 for every channel.  wrong: 'nopad' (a dropped tap without its pad share)."""
    H, W, J = m.shape
    fw, fh, s = np.float32(W), np.float32(H), np.float32(stride)
    if align:
        gx, gy = 2 * (px / s) / (fw - 1) - 1, 2 * (py / s) / (fh - 1) - 1
        ix, iy = (gx + 1) * ((fw - 1) * np.float32(0.5)), (gy + 1) * ((fh - 1) * np.float32(0.5))
        x0f, y0f = ix.floor(), iy.floor()
        ww, wn = ix - x0f, iy - y0f
        we, ws = 1 - ww, 1 - wn
        wt = [ws * we, ws * ww, wn * we, wn * ww]
        xin = [(x0f >= 0) & (x0f <= W - 1), (x0f + 1 >= 0) & (x0f + 1 <= W - 1)]
        yin = [(y0f >= 0) & (y0f <= H - 1), (y0f + 1 >= 0) & (y0f + 1 <= H - 1)]
        xs = [torch.where(xin[0], x0f, torch.zeros_like(x0f)).long(), torch.where(xin[1], x0f + 1, torch.zeros_like(x0f)).long()]
        ys = [torch.where(yin[0], y0f, torch.zeros_like(y0f)).long(), torch.where(yin[1], y0f + 1, torch.zeros_like(y0f)).long()]
        v = torch.zeros((px.shape[0], J))
        wout = torch.zeros(px.shape[0])
        for t, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            ok = yin[a] & xin[b]
            v = v + torch.where(ok[:, None], m[ys[a], xs[b]] * wt[t][:, None], torch.zeros(()))
            wout = wout + torch.where(ok, torch.zeros(()), wt[t])
        if pad is not None and wrong != 'nopad':
            v = v + pad[None] * wout[:, None]
        return v
    gx, gy = (2 * (px / s) + 1) / fw - 1, (2 * (py / s) + 1) / fh - 1
    ix, iy = ((gx + 1) * fw - 1) * 0.5, ((gy + 1) * fh - 1) * 0.5
    ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    x0f, y0f = ix.floor(), iy.floor()
    ww, wn = ix - x0f, iy - y0f
    we, ws = 1 - ww, 1 - wn
    x0, y0 = x0f.long(), y0f.long()
    x1ok, y1ok = x0 + 1 < W, y0 + 1 < H
    x1, y1 = torch.where(x1ok, x0 + 1, x0), torch.where(y1ok, y0 + 1, y0)
    z = torch.zeros(())
    v = m[y0, x0] * (ws * we)[:, None]
    v = v + torch.where(x1ok[:, None], m[y0, x1] * (ws * ww)[:, None], z)
    v = v + torch.where(y1ok[:, None], m[y1, x0] * (wn * we)[:, None], z)
    return v + torch.where((x1ok & y1ok)[:, None], m[y1, x1] * (wn * ww)[:, None], z)


# ---- cpr_bag_sample ----------------------------------------------------------------------------------------------------
def bag_points32(ctr, off, centre_first=False):
    """(G, K, 2) fp32: ring offsets + centre (one IEEE addition each), the centre itself LAST."""
    ring = off[None] + ctr[:, None]
    return torch.cat([ctr[:, None], ring], 1) if centre_first else torch.cat([ring, ctr[:, None]], 1)


def inside(pts, hw):
    """pts (..., 2) against (h, w): 0 <= x < w and 0 <= y < h (exact compares of fp32 values with integers)."""
    return (0 <= pts[..., 0]) & (pts[..., 0] < float(hw[1])) & (0 <= pts[..., 1]) & (pts[..., 1] < float(hw[0]))


def bag_ref(i):
    """-> pts (G, K, 2) fp32, valid (G, K) bool, out / bar (G, K, J) fp64, dropped (G, K)."""
    pts = bag_points32(i['ctr'], i['off'])
    G, K = pts.shape[:2]
    J = i['map'].shape[-1]
    valid = torch.zeros((G, K), dtype=torch.bool)
    out, bar = torch.zeros((G, K, J), dtype=torch.float64), torch.zeros((G, K, J), dtype=torch.float64)
    dropped = torch.zeros((G, K), dtype=torch.long)
    for gi in range(G):
        n = int(i['gt_img'][gi])
        valid[gi] = inside(pts[gi], i['pad_hw'][n])
        out[gi], bar[gi], dropped[gi] = sample_ref(i['map'][n].double(), pts[gi, :, 0].double(), pts[gi, :, 1].double(), i['stride'],
                                                   i['align'], i['pad'])
    return dict(pts=pts, valid=valid, out=out, bar=bar, dropped=dropped)


def emu_bag(i, wrong=None):
    """wrong: 'centre_first', 'nopad'."""
    pts = bag_points32(i['ctr'], i['off'], centre_first=wrong == 'centre_first')
    G, K = pts.shape[:2]
    out = torch.zeros((G, K, i['map'].shape[-1]))
    valid = torch.zeros((G, K), dtype=torch.bool)
    for gi in range(G):
        n = int(i['gt_img'][gi])
        valid[gi] = inside(pts[gi], i['pad_hw'][n])
        out[gi] = emu_sample(i['map'][n], pts[gi, :, 0], pts[gi, :, 1], i['stride'], i['align'], i['pad'], wrong)
    return dict(pts=pts, valid=valid, out=out)


# ---- cpr_grid_bag ------------------------------------------------------------------------------------------------------
def grid_ref(i):
    """-> pts (G, Kt, 2) fp32, valid (G, Kt) bool, cell (G, Kt), count (G), out / bar (G, Kt, J), gt_amb (G) bool, and the
    coverage figures cols (widest selected column span per gt) and on_radius (cells at distance == radius)."""
    m = i['map']
    N, H, W, J = m.shape
    R, Kmax, thr = i['R'], i['Kmax'], f32(i['radius_px'])
    Kt = Kmax + R
    ctr = i['points'].reshape(-1, R, 2)
    G = ctr.shape[0]
    gx, gy = _pixels(H, W, i['stride'])
    pts = torch.zeros((G, Kt, 2))
    valid = torch.zeros((G, Kt), dtype=torch.bool)
    cell = torch.full((G, Kt), -1, dtype=torch.long)
    count = torch.zeros(G, dtype=torch.long)
    out, bar = torch.zeros((G, Kt, J), dtype=torch.float64), torch.zeros((G, Kt, J), dtype=torch.float64)
    gt_amb = torch.zeros(G, dtype=torch.bool)
    cols, on_radius = [], 0
    padv = i['pad'].double() if i['pad'] is not None else torch.zeros(J, dtype=torch.float64)
    for gi in range(G):
        n = int(i['gt_img'][gi])
        c = ctr[gi].double()
        d = ((gx.double()[:, None] - c[None, :, 0]) ** 2 + (gy.double()[:, None] - c[None, :, 1]) ** 2).sqrt()   # (HW, R)
        db = torch.zeros_like(d) if i['exact'] else g(4) * d
        take = (d <= thr).any(1)
        sure = ((d + db) <= thr).any(1)
        never = ((d - db) > thr).all(1)
        gt_amb[gi] = bool((~sure & ~never).any())
        on_radius += int((d == thr).any(1).sum())
        idx = torch.nonzero(take).squeeze(1)
        count[gi] = idx.numel()
        cols.append(int((idx % W).max() - (idx % W).min() + 1) if idx.numel() else 0)
        k = min(idx.numel(), Kmax)
        idx = idx[:k]
        pts[gi, :k, 0], pts[gi, :k, 1] = gx[idx], gy[idx]
        valid[gi, :k] = True
        cell[gi, :k] = idx
        out[gi, :k] = m[n].reshape(H * W, J)[idx].double()
        out[gi, k:Kmax] = padv
        for j in range(R):
            r = R - 1 - j
            pts[gi, Kmax + j] = ctr[gi, r]
            valid[gi, Kmax + j] = True
            cell[gi, Kmax + j] = -2 - r
        rp = pts[gi, Kmax:].double()
        out[gi, Kmax:], bar[gi, Kmax:], _ = sample_ref(m[n].double(), rp[:, 0], rp[:, 1], i['stride'], i['align'], i['pad'])
    return dict(pts=pts, valid=valid, cell=cell, count=count, out=out, bar=bar, gt_amb=gt_amb, cols=cols, on_radius=on_radius)


def emu_grid(i, wrong=None):
    """wrong: 'no_reverse' (refine points in their given order), 'lt' (< at the radius)."""
    m = i['map']
    N, H, W, J = m.shape
    R, Kmax, thr = i['R'], i['Kmax'], np.float32(i['radius_px'])
    Kt = Kmax + R
    ctr = i['points'].reshape(-1, R, 2)
    G = ctr.shape[0]
    gx, gy = _pixels(H, W, i['stride'])
    pts = torch.zeros((G, Kt, 2))
    valid = torch.zeros((G, Kt), dtype=torch.bool)
    cell = torch.full((G, Kt), -1, dtype=torch.long)
    count = torch.zeros(G, dtype=torch.long)
    out = torch.zeros((G, Kt, J))
    for gi in range(G):
        n = int(i['gt_img'][gi])
        dx, dy = gx[:, None] - ctr[gi][None, :, 0], gy[:, None] - ctr[gi][None, :, 1]
        d = _fma32(dy, dy, dx * dx).sqrt()
        take = ((d < float(thr)) if wrong == 'lt' else (d <= float(thr))).any(1)
        idx = torch.nonzero(take).squeeze(1)
        count[gi] = idx.numel()
        k = min(idx.numel(), Kmax)
        idx = idx[:k]
        pts[gi, :k, 0], pts[gi, :k, 1] = gx[idx], gy[idx]
        valid[gi, :k] = True
        cell[gi, :k] = idx
        out[gi, :k] = m[n].reshape(H * W, J)[idx]
        if i['pad'] is not None:
            out[gi, k:Kmax] = i['pad']
        for j in range(R):
            r = j if wrong == 'no_reverse' else R - 1 - j
            pts[gi, Kmax + j] = ctr[gi, r]
            valid[gi, Kmax + j] = True
            cell[gi, Kmax + j] = -2 - r
        rp = pts[gi, Kmax:]
        out[gi, Kmax:] = emu_sample(m[n], rp[:, 0], rp[:, 1], i['stride'], i['align'], i['pad'])
    return dict(pts=pts, valid=valid, cell=cell, count=count, out=out)


# ---- cpr_mil_loss ------------------------------------------------------------------------------------------------------
def _argmax_amb(p, bp, exact_tie):
    """First arg-max of p (n,) and whether another entry comes within the bars (an exact tie decides by position)."""
    c1 = int(np.argmax(p.numpy()))
    if p.numel() == 1:
        return c1, False, c1
    rest = p + bp
    rest[c1] = -float('inf')
    c2 = int(np.argmax(rest.numpy()))
    close = bool(rest[c2] >= p[c1] - bp[c1])
    return c1, close and not exact_tie(c1, c2), c2


def mil_ref(i):
    """-> bag (nb, 5) fp64 {mil_loss, gt_loss, has_valid | #valid, #gt-valid, correct | #correct}, bar (nb, 2) of slots 0 / 1,
    amb4 (nb): slot 4 may differ by this much (0 / 1 per bag; AllPosLoss: the number of ambiguous entries)."""
    J = i['logits'].shape[-1]
    L = i['logits'].double().reshape(-1, J)
    V = i['valid'].reshape(-1).bool()
    nb, bs, bo, K = i['bags']
    co, cs, cc, cm = i['centres']
    C, eps, nj = i['C'], f32(i['eps']), 2 if i['binary'] else 1
    bag, bar = torch.zeros((nb, 5), dtype=torch.float64), torch.zeros((nb, 2), dtype=torch.float64)
    amb4 = torch.zeros(nb, dtype=torch.float64)
    for b in range(nb):
        full = b * bs
        label = int(i['labels'][b])
        wg = float(i['gt_weight'][b]) if i['gt_weight'] is not None else 1.0
        q = (torch.arange(C) == label)
        if cc > 0 and b % cm == 0:
            idx = full + co + torch.arange(cc) * cs
            gtv = V[idx].double() * wg
            p, bp = prob(L[idx, :C], i['ptype'], i['norm_p'])
            t, dt = gfocal_ref(p, bp, q[None].expand(cc, C), eps)
            bag[b, 1] = (t * gtv[:, None]).sum()
            bar[b, 1] = (dt * gtv[:, None]).sum() + g(cc * C + 1) * (t.abs() * gtv[:, None]).sum()
            bag[b, 3] = float((gtv > 0).sum())
        Lb, Vb = L[full + bo:full + bo + K], V[full + bo:full + bo + K]
        pk, bpk = prob(Lb[:, :C], i['ptype'], i['norm_p'])
        w = Vb.double() * wg
        if i['allpos']:
            t, dt = gfocal_ref(pk, bpk, q[None].expand(K, C), eps)
            bag[b, 0] = (t * w[:, None]).sum()
            bar[b, 0] = (dt * w[:, None]).sum() + g(K * C + 7) * (t.abs() * w[:, None]).sum()
            bag[b, 2] = float((w > 0).sum())
            nc = 0
            for k in range(K):
                c1, a, _ = _argmax_amb(pk[k], bpk[k], lambda x, y: bool(Lb[k, x] == Lb[k, y]))
                nc += int(c1 == label)
                amb4[b] += float(a)
            bag[b, 4] = nc
            continue
        lw = 1.0 if float(Vb.double().sum()) * wg > 0 else 0.0
        ins = Lb[:, i['ins_off']:i['ins_off'] + C * nj].reshape(K, C, nj)
        d = ins - ins.max(0, keepdim=True)[0]
        e = d.exp()
        a = e * w[:, None, None]
        sv = a.sum(0)
        svt = sv / e.sum(0)
        assert bool(((svt == 0) | (svt > 1e-6)).all()), 'a bag approaches the 1e-12 clamp of the normalisation'
        what = a / torch.where(sv > 0, sv, torch.ones_like(sv))
        x = pk[:, :, None]
        p = (what * x).sum(0)
        rho = T + U32 * d.abs() + 2 * U32
        bp = (what * (rho * (x - p).abs() + bpk[:, :, None])).sum(0) * MARGIN + (g(K + 1) + g(K) + U32) * (what * x.abs()).sum(0)
        qm = torch.zeros((C, nj), dtype=torch.bool)
        qm[:, 0] = q
        t, dt = gfocal_ref(p, bp, qm, eps)
        bag[b, 0] = t.sum() * lw
        bar[b, 0] = (dt.sum() + g(C * nj) * t.abs().sum()) * lw
        bag[b, 2] = lw
        c1, amb, _ = _argmax_amb(p[:, 0], bp[:, 0], lambda x, y: bool(p[x, 0] == p[y, 0]) and float(bp[x, 0] + bp[y, 0]) == 0.0)
        bag[b, 4] = float(c1 == label)
        amb4[b] = float(amb)
    return dict(bag=bag, bar=bar, amb4=amb4)


def finalize_ref(bag32, neg_partial, w_mil, w_gt, w_neg, acc_den, neg_from_gt):
    """bag32 (nb, 5): the kernel's OWN fp32 workspace; neg_partial (n,) double or None -> out5 ref, bar (5,) fp64; slots 2 and 4
    are exact (bar 0: compare the float32 of ref)."""
    t = bag32.double().sum(0)
    ta = bag32.double().abs().sum(0)
    neg = float(neg_partial.sum()) if neg_partial is not None and neg_partial.numel() else 0.0
    nega = float(neg_partial.abs().sum()) if neg_partial is not None and neg_partial.numel() else 0.0
    ns, npg = max(float(t[2]), 1.0), max(float(t[3]), 1.0)
    w_mil, w_gt, w_neg = f32(w_mil), f32(w_gt), f32(w_neg)
    den = npg if neg_from_gt else ns
    ref = torch.tensor([w_gt * (float(t[1]) / npg), float(t[0]) / ns * w_mil, float(t[4]) * 100.0 / acc_den if acc_den > 0 else 0.0,
                        w_neg * (neg / den), ns], dtype=torch.float64)
    mags = torch.tensor([abs(w_gt) * float(ta[1]) / npg, float(ta[0]) / ns * abs(w_mil), 0.0, abs(w_neg) * nega / den, 0.0],
                        dtype=torch.float64)
    bar = ULP32 * ref.abs() + 4 * D64 * mags
    bar[2] = bar[4] = 0.0
    return ref, bar


def emu_mil(i, wrong=None):
    """fp32.  wrong: 'drop_entry' (the last entry of a bag left out of the softmax), 'noeps'."""
    J = i['logits'].shape[-1]
    L = i['logits'].reshape(-1, J)
    V = i['valid'].reshape(-1).bool()
    nb, bs, bo, K = i['bags']
    co, cs, cc, cm = i['centres']
    C, nj = i['C'], 2 if i['binary'] else 1
    eps = 0.0 if wrong == 'noeps' else f32(i['eps'])
    bag = torch.zeros((nb, 5))

    def gf(p, q):
        return -((p - q) ** 2 * (q * torch.log(p + eps) + (1 - q) * torch.log(1 - p + eps)))

    for b in range(nb):
        full = b * bs
        label = int(i['labels'][b])
        wg = float(i['gt_weight'][b]) if i['gt_weight'] is not None else 1.0
        q = (torch.arange(C) == label).float()
        if cc > 0 and b % cm == 0:
            idx = full + co + torch.arange(cc) * cs
            gtv = V[idx].float() * wg
            bag[b, 1] = (gf(emu_prob(L[idx, :C], i['ptype'], i['norm_p']), q[None]) * gtv[:, None]).sum()
            bag[b, 3] = float((gtv > 0).sum())
        Lb, Vb = L[full + bo:full + bo + K], V[full + bo:full + bo + K]
        pk = emu_prob(Lb[:, :C], i['ptype'], i['norm_p'])
        w = Vb.float() * wg
        if i['allpos']:
            bag[b, 0] = (gf(pk, q[None]) * w[:, None]).sum()
            bag[b, 2] = float((w > 0).sum())
            bag[b, 4] = float((first_argmax(pk, 1) == label).sum())
            continue
        lw = 1.0 if float(Vb.float().sum()) * wg > 0 else 0.0
        ins = Lb[:, i['ins_off']:i['ins_off'] + C * nj].reshape(K, C, nj)
        if wrong == 'drop_entry' and K > 1:
            ins, pk, w = ins[:-1], pk[:-1], w[:-1]
        e = (ins - ins.max(0, keepdim=True)[0]).exp()
        pi = e / e.sum(0, keepdim=True) * w[:, None, None]
        p = (pk[:, :, None] * pi).sum(0) / pi.sum(0).clamp_min(1e-12)
        qm = torch.zeros((C, nj))
        qm[:, 0] = q
        bag[b, 0] = float(gf(p, qm).sum()) * lw
        bag[b, 2] = lw
        bag[b, 4] = float(int(np.argmax(p[:, 0].numpy())) == label)
    return dict(bag=bag)


def emu_finalize(bag32, neg_partial, w_mil, w_gt, w_neg, acc_den, neg_from_gt, wrong=None):
    """wrong: 'noclamp' (num_sample / num_pos_gt not clamped at 1)."""
    t = bag32.double().sum(0)
    neg = float(neg_partial.sum()) if neg_partial is not None and neg_partial.numel() else 0.0
    ns, npg = float(t[2]), float(t[3])
    if wrong != 'noclamp':
        ns, npg = max(ns, 1.0), max(npg, 1.0)
    div = lambda a, b: a / b if b != 0 else (float('nan') if a == 0 else math.copysign(float('inf'), a))
    return torch.tensor([f32(w_gt) * div(float(t[1]), npg), div(float(t[0]), ns) * f32(w_mil),
                         float(t[4]) * 100.0 / acc_den if acc_den > 0 else 0.0,
                         f32(w_neg) * div(neg, npg if neg_from_gt else ns), ns], dtype=torch.float64).float()


# ---- cpr_refine --------------------------------------------------------------------------------------------------------
def refine_ref(i):
    """-> chosen (G, Kt) bool, chosen_amb (G, Kt) bool, not_refine (G) bool, nr_amb (G), gt_amb (G): floats of the gt skipped,
    refine_pts / rp_bar (G, 2), scores / sc_bar (G), and coverage figures (dist_ties, prob_ties, none_kept, single_class)."""
    Lg = i['logits'].double()
    G, Kt, J = Lg.shape
    C, Kv, Rv, cs = i['C'], i['Kv'], i['Rv'], i['ctr_stride']
    ctr = i['ctr']
    alpha, mth, rth = f32(i['gt_alpha']), f32(i['merge_th']), f32(i['refine_th'])
    chosen, camb = torch.zeros((G, Kt), dtype=torch.bool), torch.zeros((G, Kt), dtype=torch.bool)
    nr, nr_amb, gt_amb = torch.zeros(G, dtype=torch.bool), torch.zeros(G, dtype=torch.bool), torch.zeros(G, dtype=torch.bool)
    rp, rpb = torch.zeros((G, 2), dtype=torch.float64), torch.zeros((G, 2), dtype=torch.float64)
    sc, scb = torch.zeros(G, dtype=torch.float64), torch.zeros(G, dtype=torch.float64)
    cov = dict(dist_ties=0, prob_ties=0, none_kept=0, single_class=0, multi_class=0)
    ks = torch.arange(Kt)
    for gi in range(G):
        n, label = int(i['gt_img'][gi]), int(i['labels'][gi])
        g0, g1 = int(i['gt_start'][n]), int(i['gt_start'][n + 1])
        pa, bpa = prob(Lg[gi][:, :C], i['ptype'], i['norm_p'])
        p, bp = pa[:, label], bpa[:, label]
        gate = p[Kv - 1] * alpha
        bgate = alpha * bp[Kv - 1] + U32 * gate
        pts = i['pts'][gi].double()
        ok = i['valid'][gi].bool().clone()
        amb = torch.zeros(Kt, dtype=torch.bool)
        mates = [o for o in range(g0, g1) if int(i['labels'][o]) == label]
        if i['use_nearest'] and len(mates) > 1:
            cov['multi_class'] += 1
            owner = torch.tensor([(o, r) for o in mates for r in range(Rv)])
            cc = torch.stack([ctr[o * cs + r] for o in mates for r in range(Rv)]).double()
            d2, b2 = d2_pair(pts[:, 0:1], pts[:, 1:2], cc[None, :, 0], cc[None, :, 1], i['exact'])
            if not i['exact']:
                b2 = b2 + 2 * ULP32 * d2
            poss = (d2 - b2) <= (d2 + b2).min(1, keepdim=True)[0]
            match = (owner[None, :, 0] == gi) & (owner[None, :, 1] == (ks // Kv)[:, None])
            some, other = (poss & match).any(1), (poss & ~match).any(1)
            first = first_argmin(d2, 1)
            cov['dist_ties'] += int(((d2 == d2.min(1, keepdim=True)[0]).sum(1) > 1).sum())
            near = torch.where(some & other, match[ks, first], some)
            if not i['exact']:
                amb |= some & other
            ok &= near
        elif i['use_nearest']:
            cov['single_class'] += 1
        if i['use_classify']:
            for k in range(Kt):
                c1, a, c2 = _argmax_amb(pa[k], bpa[k], lambda x, y: bool(Lg[gi, k, x] == Lg[gi, k, y]))
                cov['prob_ties'] += int(bool(pa[k, c1] == pa[k, c2]) and c1 != c2)
                if a and label in (c1, c2):
                    amb[k] = True
                ok[k] &= (c1 == label)
        amb |= ((p - mth).abs() <= bp) | ((p - gate).abs() <= bp + bgate)
        ok &= (p > mth) & (p > gate)
        ok &= (pts[:, 0] < float(i['img_hw'][n][1])) & (pts[:, 0] >= 0) & (pts[:, 1] < float(i['img_hw'][n][0])) & (pts[:, 1] >= 0)
        # an ambiguous comparison matters only where every other condition of the entry holds
        sure_false = ~_definite(i, gi, pts, p, bp, gate, bgate, mth)
        amb &= ~sure_false
        chosen[gi], camb[gi] = ok, amb
        gt_amb[gi] = bool(amb.any())
        kc = ok.double()
        cnt = float(kc.sum())
        sw = float((p * kc).sum())
        D = sw + F32_EPS_REFINE
        score = sw / (cnt + F32_EPS_REFINE)
        bsw = float((bp * kc).sum()) + float(g(cnt)) * sw
        bscore = bsw / max(cnt, 1.0) + 2 * U32 * score
        nr_amb[gi] = abs(score - rth) <= bscore
        nr[gi] = score < rth
        if i['not_refine_in'] is not None and bool(i['not_refine_in'][gi]):
            nr[gi], nr_amb[gi] = True, False
        cov['none_kept'] += int(cnt == 0)
        if bool(nr[gi]):
            rp[gi] = ctr[gi * cs].double()
        else:
            for ax in range(2):
                x = pts[:, ax]
                X = float((x * p * kc).sum()) / D
                rp[gi, ax] = X
                rpb[gi, ax] = float(((x - X).abs() * bp * kc).sum()) / D * MARGIN + (float(g(cnt + 2)) + 3 * U32) * float((x.abs() * p * kc).sum()) / D
        if i['score_max']:
            sc[gi] = float((p * kc).max()) if cnt else rth * 0.5
            scb[gi] = float((bp * kc).max()) if cnt else 0.0
        else:
            sc[gi], scb[gi] = score, bscore
    return dict(chosen=chosen, chosen_amb=camb, not_refine=nr, nr_amb=nr_amb, gt_amb=gt_amb | nr_amb, refine_pts=rp, rp_bar=rpb,
                scores=sc, sc_bar=scb, cov=cov)


def _definite(i, gi, pts, p, bp, gate, bgate, mth):
    """Entries that no rounding can reject through the exact conditions or the clear side of a threshold: False where the
    entry is certainly out (invalid, outside the image, p clearly below a threshold)."""
    n = int(i['gt_img'][gi])
    ins = (pts[:, 0] < float(i['img_hw'][n][1])) & (pts[:, 0] >= 0) & (pts[:, 1] < float(i['img_hw'][n][0])) & (pts[:, 1] >= 0)
    return i['valid'][gi].bool() & ins & (p + bp > mth) & (p + bp + bgate > gate)


def emu_refine(i, wrong=None):
    """fp32.  wrong: 'last_argmin' (the last of equal nearest candidates wins)."""
    Lg = i['logits']
    G, Kt, J = Lg.shape
    C, Kv, Rv, cs = i['C'], i['Kv'], i['Rv'], i['ctr_stride']
    ctr = i['ctr']
    alpha, mth, rth = np.float32(i['gt_alpha']), f32(i['merge_th']), f32(i['refine_th'])
    chosen = torch.zeros((G, Kt), dtype=torch.bool)
    nr = torch.zeros(G, dtype=torch.bool)
    rp, sc = torch.zeros((G, 2)), torch.zeros(G)
    ks = torch.arange(Kt)
    for gi in range(G):
        n, label = int(i['gt_img'][gi]), int(i['labels'][gi])
        g0, g1 = int(i['gt_start'][n]), int(i['gt_start'][n + 1])
        pa = emu_prob(Lg[gi][:, :C], i['ptype'], i['norm_p'])
        p = pa[:, label]
        gate = p[Kv - 1] * alpha
        pts = i['pts'][gi]
        ok = i['valid'][gi].bool().clone()
        mates = [o for o in range(g0, g1) if int(i['labels'][o]) == label]
        if i['use_nearest'] and len(mates) > 1:
            owner = torch.tensor([(o, r) for o in mates for r in range(Rv)])
            cc = torch.stack([ctr[o * cs + r] for o in mates for r in range(Rv)])
            d = _d2_chain32(pts[:, 0:1], pts[:, 1:2], cc[None, :, 0], cc[None, :, 1]).sqrt()
            if wrong == 'last_argmin':
                win = d.shape[1] - 1 - first_argmin(d.flip(1), 1)
            else:
                win = first_argmin(d, 1)
            ok &= (owner[win, 0] == gi) & (owner[win, 1] == ks // Kv)
        if i['use_classify']:
            ok &= first_argmax(pa, 1) == label
        ok &= (p > mth) & (p > gate)
        ok &= (pts[:, 0] < float(i['img_hw'][n][1])) & (pts[:, 0] >= 0) & (pts[:, 1] < float(i['img_hw'][n][0])) & (pts[:, 1] >= 0)
        pm = torch.where(ok, p, torch.zeros(()))
        chosen[gi] = pm > 0
        sw, cnt = pm.sum(), (pm > 0).float().sum()
        w = pm / (sw + np.float32(1e-8))
        score = sw / (cnt + np.float32(1e-8))
        nr[gi] = bool(score < rth) or (i['not_refine_in'] is not None and bool(i['not_refine_in'][gi]))
        rp[gi] = ctr[gi * cs] if bool(nr[gi]) else (pts * w[:, None]).sum(0)
        sc[gi] = (float(pm.max()) if float(pm.max()) != 0 else float(np.float32(rth) * np.float32(0.5))) if i['score_max'] else float(score)
    return dict(chosen=chosen, not_refine=nr, refine_pts=rp, scores=sc)


# ---- comparison ------------------------------------------------------------------------------------------------------
def worst(got, ref, bar, keep=None):
    """Largest |got - ref| / bar over the kept elements (0 when nothing is kept); NaN in got counts as infinite."""
    r = ratio(got, ref, bar)
    r = torch.where(torch.isnan(got.double()), torch.full_like(r, float('inf')), r)
    if keep is not None:
        r = r[keep.expand_as(r)] if keep.dim() == r.dim() else r[keep]
    return float(r.max()) if r.numel() else 0.0


def disc(got, ref, amb=None):
    """(mismatches outside the ambiguous set, ambiguous count)."""
    bad = got != ref
    if amb is None:
        return int(bad.sum()), 0
    return int((bad & ~amb).sum()), int(amb.sum())


def compare(op, i, got, ref):
    """got: the kernel's (or an emulation's) outputs of one case as CPU tensors -> dict(ratios={name: worst error / bar},
    wrong={name: discrete mismatches outside the ambiguous set}, amb={name: (ambiguous, elements)})."""
    ratios, wrong, amb = {}, {}, {}
    if op == 'centers':
        ratios['centers'] = worst(got['centers'], *ref)
    elif op == 'neg':
        wrong['mask'], a = disc(got['mask'].bool(), ref['mask'], ref['amb'])
        amb['mask'] = (a, ref['mask'].numel())
        ratios['img_sum'] = worst(got['img_sum'], ref['img_sum'], ref['img_bar'])
        ratios['total'] = worst(got['img_sum'].sum(), ref['total'], ref['total_bar'])
    elif op == 'bag':
        wrong['pts'] = int((got['pts'] != ref['pts']).sum())
        wrong['valid'] = disc(got['valid'].bool(), ref['valid'])[0]
        ratios['out'] = worst(got['out'], ref['out'], ref['bar'])
    elif op == 'grid':
        keep = ~ref['gt_amb']
        for k in ('pts', 'valid', 'cell', 'count'):
            gk, rk = got[k][keep], ref[k][keep]
            wrong[k] = int((gk.to(rk.dtype) != rk).sum())
        amb['gt'] = (int(ref['gt_amb'].sum()), ref['gt_amb'].numel())
        amb['cell'] = (int(ref['gt_amb'].sum()) * ref['cell'].shape[1], ref['cell'].numel())
        ratios['out'] = worst(got['out'], ref['out'], ref['bar'], keep)
    elif op == 'mil':
        bag = got['bag'].double()
        ratios['bag_mil'] = worst(bag[:, 0], ref['bag'][:, 0], ref['bar'][:, 0])
        ratios['bag_gt'] = worst(bag[:, 1], ref['bag'][:, 1], ref['bar'][:, 1])
        wrong['bag2'] = int((bag[:, 2] != ref['bag'][:, 2]).sum())
        wrong['bag3'] = int((bag[:, 3] != ref['bag'][:, 3]).sum())
        wrong['bag4'] = int(((bag[:, 4] - ref['bag'][:, 4]).abs() > ref['amb4']).sum())
        amb['bag4'] = (int(ref['amb4'].sum()), bag.shape[0] * (i['bags'][3] if i['allpos'] else 1))
        if 'out5' in got:
            fr, fb = finalize_ref(got['bag'], i['neg_partial'], i['w_mil'], i['w_gt'], i['w_neg'],
                                  float(bag.shape[0] * (i['bags'][3] if i['allpos'] else 1)), i['neg_from_gt'])
            ratios['out5'] = worst(got['out5'][[0, 1, 3]], fr[[0, 1, 3]], fb[[0, 1, 3]])
            wrong['out5_acc'] = int(float(got['out5'][2]) != f32(float(fr[2])))
            wrong['out5_num'] = int(float(got['out5'][4]) != f32(float(fr[4])))
    elif op == 'refine':
        wrong['chosen'], a = disc(got['chosen'].bool(), ref['chosen'], ref['chosen_amb'])
        amb['chosen'] = (a, ref['chosen'].numel())
        wrong['not_refine'], a = disc(got['not_refine'].bool(), ref['not_refine'], ref['gt_amb'])
        amb['gt'] = (int(ref['gt_amb'].sum()), ref['gt_amb'].numel())
        keep = ~ref['gt_amb']
        ratios['refine_pts'] = worst(got['refine_pts'], ref['refine_pts'], ref['rp_bar'], keep)
        ratios['scores'] = worst(got['scores'], ref['scores'], ref['sc_bar'], keep)
    return dict(ratios=ratios, wrong=wrong, amb=amb)


def amb_ok(res, exact):
    """Every ambiguous share inside AMBIG_CAP; none at all for an exact case."""
    return all((a == 0) if exact else (a <= AMBIG_CAP * n) for a, n in res['amb'].values())


def passes(res, exact=False):
    return all(r <= 1 for r in res['ratios'].values()) and all(w == 0 for w in res['wrong'].values()) and amb_ok(res, exact)
