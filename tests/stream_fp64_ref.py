"""fp64 references of the streaming kernels around the conv stack (csrc/norm_pool.hip, csrc/backward.hip lines 1-540) and the
bars a HIP kernel must meet, every bar derived by counting the roundings the kernel performs.

References are fp64 from the operands AS THE KERNEL READS THEM: bf16 operands are the bf16 values themselves (widened exactly);
``a``, ``b``, ``mean``, ``rstd``, ``k2``, ``k3`` are the fp32 values handed to the kernel or read back from its workspace; the
ReLU mask of relu_bwd_colsum comes from the stored ``y``.  u = U32 = 2^-24 is the fp32 unit roundoff (one rounding errs by at
most u of the rounded value), ULP32 = 2u one fp32 ulp, g(n) = n u / (1 - n u) the bound on n chained roundings.  ``got``
passes where ``|got - ref| <= bar`` (conv_fp64_ref.ratio).

Exact kernels (bit equality with the torch expression, no bar): max-pool values and recorded argmax bytes (first window
position of a tie, 255 where the maximum is 0, bf16 compared as values), zero_insert, both layout kernels, phase_scatter_add
(one fp32 add: IEEE addition is the torch addition), ``g`` / ``g16`` of relu_bwd_colsum (with ``add`` one fp32 add, then the
mask, then round-to-nearest-even) and ``Gw * scale`` of bn_fold_bwd (one fp32 multiply).  axpby is ``alpha * x + beta * y``
with up to three roundings, fused or not: ``ULP32 * (|alpha x| + |beta y|)``.

* gn_apply, every instance: ``v = x a + b`` is one fma (u |v|) or a rounded product and a rounded sum (u |x a| + u |v|), so
  ``ULP32 * (|x a| + |b|)`` covers both.  ReLU is 1-Lipschitz, so no element is excluded.  With the upsample add one more
  rounded sum: ``+ ULP32 * |y + up|``.  A bf16 store rounds to nearest even: half a bf16 grid step in the binade of the stored
  fp32 value (|ref| + the fp32 bar bounds it) -- a full step would also pass a truncating store.
* gn_stats / gn_stats_bf16 slot partials, n pixels per channel in the slot, any order of additions:
      sum    ``g(n - 1) * sum |x|``
      sumsq  ``g(n) * sum x^2``                  (n - 1 additions and the square's own rounding)
  An empty slot stores exact zeros.  A CPU emulation of the kernel's order stays at 0.016 .. 0.019 of these worst-case bars
  (tests/test_stream_instances_host.py repeats it and shows that the bars are nevertheless sharp against one dropped pixel).
* gn_finalize from GIVEN partials: the kernel adds the partials in double and rounds each stored quantity once, so against
  fp64 on the same fp32 partials: ``mean`` and ``rstd`` 1 ulp each; ``a = float(rstd) * gamma`` two roundings, 2 ulp;
  ``b = beta - float(mean) * a`` ``2 * ULP32 * (|beta| + |mean a|)`` (float(mean) u, a 2 u, then the fma the build contracts
  this expression into, u |b|: 4 u |mean a| + u |beta|).  D64 = 2^-48 of the summed magnitudes stands for the order of the
  double additions and the cancellation of ``E[x^2] - mean^2`` in double.
* gn_stats then gn_finalize against fp64 GroupNorm of x: the slot bars propagate,
      ``|dmean| <= sum(bar_sum) / count``, ``|dvar| <= sum(bar_sumsq) / count + 2 |mean| |dmean| + dmean^2``,
      ``|drstd| <= rstd^3 |dvar| / 2``,
  plus the ulps above.  sum(bar_sumsq) / count is n u E[x^2] = n u (var + mean^2), so the bar on rstd grows with
  mean^2 / var: that is the conditioning of the kernel's ``E[x^2] - mean^2`` form itself (a shifted form, as bn_train.hip
  uses, would not have it).  The table therefore runs at stated |mean| / std ratios and a GPU test bounds the ratio the
  product's GroupNorm inputs reach.
* gn_bwd slot partials: ``sum dy``: ``g(n - 1) * sum |dy|``; ``sum dy * xhat``, each term ``dy * (x - mean) * rstd`` carries
  three roundings: ``g(n + 2) * sum |dy xhat|``.  The ReLU mask is recomputed in fp32 from ``x a + b``, so it may differ from
  the fp64 mask where ``|y|`` lies inside the gn_apply bar: such elements are AMBIGUOUS; their ``|term|`` is added to the bar
  of the sums and either branch is accepted for dx.  At most AMBIG_CAP = 1e-5 of a case's elements may be ambiguous.
* gn_bwd dgamma / dbeta: the slot bars summed over slots and images; the kernel adds slots in double and stores one float per
  image and channel (``ULP32 * |per-image sum|`` per stored float), adds images in double and rounds once
  (``ULP32 * |ref|``); accumulating adds ``ULP32 * |base + ref|``.
* gn_bwd k2 / k3 (read from ws_k): the fp64 formulas ``m1 = sum_c gamma S1 / count``, ``m2 = sum_c gamma S2 / count``,
  ``k2 = -rstd^2 m2``, ``k3 = -rstd m1 + mean rstd^2 m2`` with the partial bars pushed through them and one ulp of each
  rounded magnitude.
* gn_bwd dx = ``dy a + x k2 + k3`` from the kernel's OWN k2 / k3 (so this is a pure elementwise check): two products, two
  sums, ``2 * ULP32 * (|dy a| + |x k2| + |k3|)``; dx16 adds the bf16 half step.
* upsample_add_bwd: k children in any order ``g(k - 1) * sum |children|``; accumulating ``+ ULP32 * |base + ref|``.
* relu_bwd_colsum column sums: fp32 inside a row block ``g(rows - 1) * sum |g|``; the block partial is a stored float and so
  is every split sum of the two-pass fold (``ULP32 * |partial|`` each); double across them; ``ULP32 * |ref|`` at the end
  (``+ ULP32 * |base + ref|`` accumulating).  part_colsum: the same without the first term and without the block floats.
* bn_fold_bwd dgamma / dbeta: double arithmetic and one float rounding of each stored value (``ULP32 * |ref|``); from tile
  partials the column sum is rounded to float first, which enters dgamma as ``u |inv_sigma mean dshift|``.
"""
import numpy as np
import torch

from tests.conv_fp64_ref import ACC_REL, MAX_THREADS, U32, ULP32, _threads, bf16_half_ulp, ratio  # noqa: F401  (re-exported)

D64 = 2.0 ** -48          # order of double additions / double cancellation, relative to the summed magnitudes
AMBIG_CAP = 1e-5          # largest share of a case's elements whose fp32 ReLU mask may differ from the fp64 one


def g(n):
    """n chained fp32 roundings: n u / (1 - n u) (0 for n <= 0); n a number or a tensor."""
    n = torch.as_tensor(n, dtype=torch.float64).clamp_min(0)
    return n * U32 / (1 - n * U32)


def half_step(ref, bar32):
    """Round-to-nearest-even bound of a bf16 store of an fp32 value within bar32 of ref."""
    return bf16_half_ulp(ref.abs() + bar32)


# ---- launch rules, restated (tests/test_stream_instances_host.py pins each to the library or to the source text) ----------
GRID_CAPS = dict(gn_apply=32768, gn_apply_bf16=32768, gn_apply_bf16_wide=8192, gn_bwd_apply=32768, upsample_add_bwd=32768,
                 axpby=32768, zero_insert=32768, phase_scatter_add=32768, maxpool=16384, maxpool_bf16=16384, nchw_to_nhwc4=8192)
BLOCK = 256
COLSUM_SPLIT_ROWS, COLSUM_MAX_SPLITS = 256, 64
RELU_COL_GROUP = 1024


def cdiv(a, b):
    return (a + b - 1) // b


def grid_blocks(total, cap):
    return min(cdiv(total, BLOCK), cap)


def wraps(total, cap):
    """A grid-stride loop makes a second trip somewhere."""
    return total > cap * BLOCK


def rows_per_block(M):
    rows = 128
    while rows > 16 and cdiv(M, rows) < 2048:
        rows >>= 1
    return rows


def colsum_plan(rows):
    """(splits, rows per split) of launch_colsum; splits == 1: a single pass."""
    nsplit = min(cdiv(rows, COLSUM_SPLIT_ROWS), COLSUM_MAX_SPLITS)
    if nsplit <= 1:
        return 1, rows
    per = cdiv(rows, nsplit)
    return cdiv(rows, per), per


def relu_bwd_ws(M, C):
    return (cdiv(M, rows_per_block(M)) + COLSUM_MAX_SPLITS) * C


def slot_extents(HW, P):
    """[p0, p1) of every statistics slot (p0 == p1: an empty slot)."""
    per = cdiv(HW, P)
    return [(min(s * per, HW), min(HW, s * per + per)) for s in range(P)]


def default_slots(HW):
    return max(1, min(256, HW // 256))


def bf16_wide(C, npix):
    return C % 8 == 0 and C // 8 <= 256 and 256 % (C // 8) == 0 and npix < (1 << 31)


def lanes_ok(C):
    return C > 0 and C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0


def nearest_index(out_len, in_len):
    """The kernels' float32 index rule: min(floor(dst * (float)in / (float)out), in - 1)."""
    s = np.float32(in_len) / np.float32(out_len)
    return np.minimum(np.floor(np.arange(out_len, dtype=np.float32) * s).astype(np.int64), in_len - 1)


def bwd_window(u, in_len, out_len):
    """Candidate window [y0, y1] of coarse index u in upsample_add_bwd (float32, truncating casts)."""
    s = np.float32(in_len) / np.float32(out_len)
    y0 = max(0, int(np.float32(u) / s) - 1)
    y1 = min(out_len - 1, int(np.float32(u + 1) / s) + 1)
    return y0, y1


def sample_rows(total, marks=(), n_random=2000, seed=0, edge=4):
    """Rows to check of a map too large for a full CPU reference: the first and last ``edge`` rows, ``edge`` rows either side
    of every mark (wrap points, image boundaries) and ``n_random`` random ones.  Sorted unique int64."""
    rng = np.random.default_rng(seed)
    parts = [np.arange(0, min(edge, total)), np.arange(max(0, total - edge), total), rng.integers(0, total, size=min(n_random, total))]
    for m in marks:
        parts.append(np.arange(max(0, m - edge), min(total, m + edge)))
    return np.unique(np.concatenate(parts).astype(np.int64))


# ---- GroupNorm forward ---------------------------------------------------------------------------------------------
def apply_ref(x, a, b, relu, up=None, bf16=False):
    """x, a, b, up: fp64, broadcastable to one shape -> (ref, bar)."""
    t = x * a + b
    bar = ULP32 * ((x * a).abs() + b.abs())
    if relu:
        t = t.clamp_min(0)
    if up is not None:
        t = t + up
        bar = bar + ULP32 * t.abs()
    if bf16:
        bar = bar + half_step(t, bar)
    return t, bar


def _slots(v, P):
    """(N, HW, C) -> (N, P, per, C), zero-padded past HW, and the pixel count of each slot."""
    N, HW, C = v.shape
    per = cdiv(HW, P)
    if P * per != HW:
        v = torch.cat([v, v.new_zeros((N, P * per - HW, C))], 1)
    n = torch.tensor([p1 - p0 for p0, p1 in slot_extents(HW, P)], dtype=torch.float64).view(1, P, 1)
    return v.view(N, P, per, C), n


def stats_slots(x, P):
    """x (N, HW, C) fp64 -> (ref, bar), each (N, P, C, 2): (sum, sumsq) per slot and channel."""
    xs, n = _slots(x, P)
    s, sa, q = xs.sum(2), xs.abs().sum(2), (xs * xs).sum(2)
    return torch.stack([s, q], -1), torch.stack([g(n - 1) * sa, g(n) * q], -1)


def _group(v, G):
    """(N, C) -> (N, G) sums over each group's channels."""
    N, C = v.shape
    return v.view(N, G, C // G).sum(2)


def finalize_from_partials(part, gamma, beta, G, HW, eps):
    """part (N, P, C, 2), gamma, beta (C): fp64 of the fp32 values -> {name: (ref, bar)} for mean, rstd (N, G), a, b (N, C)."""
    N, P, C, _ = part.shape
    cpg = C // G
    count = float(HW) * cpg
    ts, tq = _group(part[..., 0].sum(1), G), _group(part[..., 1].sum(1), G)
    tsa = _group(part[..., 0].abs().sum(1), G)
    mean = ts / count
    ex2 = tq / count
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = (var + eps) ** -0.5
    d_mean = D64 * tsa / count
    d_rstd = 0.5 * rstd ** 3 * D64 * (ex2 + mean * mean + 2 * mean.abs() * d_mean)
    rep = lambda t: t.repeat_interleave(cpg, dim=1)
    a = rep(rstd) * gamma
    b = beta - rep(mean) * a
    bar_a = 2 * ULP32 * a.abs() + gamma.abs() * rep(d_rstd)
    bar_b = 2 * ULP32 * (beta.abs() + (rep(mean) * a).abs()) + a.abs() * rep(d_mean) + rep(mean.abs()) * gamma.abs() * rep(d_rstd)
    return dict(mean=(mean, ULP32 * mean.abs() + d_mean), rstd=(rstd, ULP32 * rstd + d_rstd), a=(a, bar_a), b=(b, bar_b))


def groupnorm_end_to_end(x, slot_bar, gamma, beta, G, eps):
    """x (N, HW, C) fp64, slot_bar (N, P, C, 2) of stats_slots -> {name: (ref, bar)} against fp64 GroupNorm of x."""
    N, HW, C = x.shape
    cpg = C // G
    count = float(HW) * cpg
    xg = x.view(N, HW, G, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(N, 1, G, 1)) ** 2).mean((1, 3))
    rstd = (var + eps) ** -0.5
    dmean = _group(slot_bar[..., 0].sum(1), G) / count
    dvar = _group(slot_bar[..., 1].sum(1), G) / count + 2 * mean.abs() * dmean + dmean * dmean
    drstd = 0.5 * rstd ** 3 * dvar
    rep = lambda t: t.repeat_interleave(cpg, dim=1)
    a = rep(rstd) * gamma
    b = beta - rep(mean) * a
    bar_a = 2 * ULP32 * a.abs() + gamma.abs() * rep(drstd)
    bar_b = 2 * ULP32 * (beta.abs() + (rep(mean) * a).abs()) + a.abs() * rep(dmean) + rep(mean.abs()) * gamma.abs() * rep(drstd)
    return dict(mean=(mean, ULP32 * mean.abs() + dmean), rstd=(rstd, ULP32 * rstd + drstd), a=(a, bar_a), b=(b, bar_b),
                ratio=float((mean.abs() * var.clamp_min(1e-300) ** -0.5).max()))


# ---- GroupNorm backward ----------------------------------------------------------------------------------------------
def gn_bwd_ref(x, dz, a, b, mean, rstd, gamma, G, P, relu):
    """x, dz (N, HW, C); a, b (N, C); mean, rstd (N, G); gamma (C): all fp64 of what the kernel reads.
    -> dict: part (ref, bar) (N, P, C, 2); dbeta, dgamma (ref, bar) (C) without the accumulate term; k2, k3 (ref, bar) (N, G);
    dy (N, HW, C) the fp64-masked gradient; amb (N, HW, C) bool; amb_share."""
    N, HW, C = x.shape
    cpg = C // G
    count = float(HW) * cpg
    rep = lambda t: t.repeat_interleave(cpg, dim=1).view(N, 1, C)
    xa = x * a.view(N, 1, C)
    y = xa + b.view(N, 1, C)
    if relu:
        amb = y.abs() <= ULP32 * (xa.abs() + b.abs().view(N, 1, C))
        dy = torch.where(y > 0, dz, torch.zeros_like(dz))
    else:
        amb = torch.zeros_like(y, dtype=torch.bool)
        dy = dz
    del xa, y
    xhat = (x - rep(mean)) * rep(rstd)
    t2 = dy * xhat
    d1, n = _slots(dy, P)
    d2, _ = _slots(t2, P)
    ambz = torch.where(amb, dz.abs(), torch.zeros_like(dz))
    e1, _ = _slots(ambz, P)
    e2, _ = _slots(ambz * xhat.abs(), P)
    ref = torch.stack([d1.sum(2), d2.sum(2)], -1)
    bar = torch.stack([g(n - 1) * (d1.abs().sum(2) + e1.sum(2)) + e1.sum(2), g(n + 2) * (d2.abs().sum(2) + e2.sum(2)) + e2.sum(2)], -1)
    S, SB = ref.sum(1), bar.sum(1)                                      # (N, C, 2): per-image sums over slots
    tot = S.sum(0)
    pbar = SB.sum(0) + ULP32 * S.abs().sum(0) + ULP32 * tot.abs()
    gm = gamma.view(1, C)
    A, B = _group(gm * S[..., 0], G), _group(gm * S[..., 1], G)
    Aa, Ba = _group(gm.abs() * S[..., 0].abs(), G), _group(gm.abs() * S[..., 1].abs(), G)
    bA = _group(gm.abs() * SB[..., 0], G) + D64 * Aa
    bB = _group(gm.abs() * SB[..., 1], G) + D64 * Ba
    m1, m2, bm1, bm2 = A / count, B / count, bA / count, bB / count
    r2 = rstd * rstd
    k2 = -r2 * m2
    k3 = -rstd * m1 + mean * r2 * m2
    bk2 = r2 * bm2 + ULP32 * k2.abs()
    bk3 = rstd * bm1 + mean.abs() * r2 * bm2 + ULP32 * ((rstd * m1).abs() + (mean * r2 * m2).abs())
    return dict(part=(ref, bar), dbeta=(tot[:, 0], pbar[:, 0]), dgamma=(tot[:, 1], pbar[:, 1]), k2=(k2, bk2), k3=(k3, bk3),
                dy=dy, amb=amb, amb_share=float(amb.double().mean()))


def gn_bwd_dx(x, dz, dy, amb, a, k2, k3, G, bf16):
    """Rows of x, dz, dy, amb (R, C); a (R, C) and the kernel's own k2, k3 (R, G) gathered per row: fp64.
    -> (ref, bar, alt): alt is the other ReLU branch, which an ambiguous element may take (equal to ref elsewhere)."""
    C = x.shape[-1]
    cpg = C // G
    k2c, k3c = k2.repeat_interleave(cpg, dim=-1), k3.repeat_interleave(cpg, dim=-1)
    rest = x * k2c + k3c
    mag = (x * k2c).abs() + k3c.abs()

    def one(d):
        t = d * a + rest
        bar = 2 * ULP32 * ((d * a).abs() + mag)
        return t, (bar + half_step(t, bar) if bf16 else bar)

    ref, bar = one(dy)
    other = torch.where(amb, dz - dy, dy)           # dy is 0 or dz on an ambiguous element: the other of the two
    alt, bar_alt = one(other)
    return ref, bar, alt, bar_alt


def ratio2(got, ref, bar, alt, bar_alt):
    """Elementwise: the smaller of the two error / bar ratios (either ReLU branch of an ambiguous element)."""
    return torch.minimum(ratio(got, ref, bar), ratio(got, alt, bar_alt))


# ---- FPN top-down add backward ---------------------------------------------------------------------------------------
def upsample_add_bwd_ref(dfine, UH, UW, base=None):
    """dfine (N, H, W, C) fp64 -> (ref, bar) (N, UH, UW, C); base: the map accumulated into."""
    N, H, W, C = dfine.shape
    iy, ix = torch.as_tensor(nearest_index(H, UH)), torch.as_tensor(nearest_index(W, UW))

    def fold(v):
        t = v.new_zeros((N, UH, W, C)).index_add_(1, iy, v)
        return v.new_zeros((N, UH, UW, C)).index_add_(2, ix, t)

    s, sa = fold(dfine), fold(dfine.abs())
    k = torch.bincount(iy, minlength=UH).view(1, UH, 1, 1) * torch.bincount(ix, minlength=UW).view(1, 1, UW, 1)
    bar = g(k.double() - 1) * sa
    if base is not None:
        s = base + s
        bar = bar + ULP32 * s.abs()
    return s, bar


# ---- column sums ------------------------------------------------------------------------------------------------
def _fold_bar(partials):
    """Double fold of (rows, C) stored floats through launch_colsum: the bar its own stored split sums add."""
    rows = partials.shape[0]
    nsplit, per = colsum_plan(rows)
    if nsplit == 1:
        return torch.zeros_like(partials[0])
    pad = torch.cat([partials, partials.new_zeros((nsplit * per - rows,) + partials.shape[1:])], 0)
    return ULP32 * pad.view(nsplit, per, -1).sum(1).abs().sum(0)


def relu_colsum_ref(gmat, base=None):
    """gmat (M, C) fp64 of the fp32 g the kernel stores -> (ref, bar) (C)."""
    M, C = gmat.shape
    rpb = rows_per_block(M)
    blocks = cdiv(M, rpb)
    pad = torch.cat([gmat, gmat.new_zeros((blocks * rpb - M, C))], 0).view(blocks, rpb, C)
    nrow = torch.full((blocks, 1), float(rpb), dtype=torch.float64)
    nrow[-1] = M - (blocks - 1) * rpb
    part = pad.sum(1)
    ref = part.sum(0)
    bar = (g(nrow - 1) * pad.abs().sum(1)).sum(0) + ULP32 * part.abs().sum(0) + _fold_bar(part) + ULP32 * ref.abs() + D64 * part.abs().sum(0)
    if base is not None:
        ref = base + ref
        bar = bar + ULP32 * ref.abs()
    return ref, bar


def part_colsum_ref(part):
    """part (tiles, C, 2) fp64 -> (ref, bar) (C) of element 0's column sums."""
    p = part[..., 0]
    ref = p.sum(0)
    return ref, _fold_bar(p) + ULP32 * ref.abs() + D64 * p.abs().sum(0)


def bn_fold_bwd_ref(Gw, Wt, mean, inv_sigma, colsum=None, part=None):
    """Gw, Wt (Cout, K); mean, inv_sigma (Cout); colsum (Cout) or part (tiles, Cout, 2): fp64 -> dgamma, dbeta (ref, bar)."""
    dscale = (Gw * Wt).sum(1)
    dmag = (Gw * Wt).abs().sum(1)
    if part is not None:
        dshift = part[..., 0].sum(0)
        dsh_bar = U32 * dshift.abs() + D64 * part[..., 0].abs().sum(0)      # rounded to float before use
    else:
        dshift, dsh_bar = colsum, torch.zeros_like(colsum)
    dgamma = inv_sigma * (dscale - mean * dshift)
    bar_g = ULP32 * dgamma.abs() + inv_sigma.abs() * (D64 * (dmag + (mean * dshift).abs()) + mean.abs() * dsh_bar)
    return dict(dgamma=(dgamma, bar_g), dbeta=(dshift, ULP32 * dshift.abs() + dsh_bar))


def axpby_ref(y, x, alpha, beta):
    al, be = float(np.float32(alpha)), float(np.float32(beta))
    return al * x + be * y, ULP32 * ((al * x).abs() + (be * y).abs())
