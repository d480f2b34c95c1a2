"""fp64 references of the batch-statistics BatchNorm kernels (csrc/bn_train.hip), of bn_fold / bn_fold_multi (csrc/pack.hip) and
of the clip-norm and SGD kernels (csrc/backward.hip: sumsq_kernel, sumsq_final_kernel, sgd_kernel), and the bars a HIP kernel must
meet, every bar derived from the fp64 reference and a count of the roundings the kernel performs -- never from its output.

References are fp64 from the operands AS THE KERNEL READS THEM, stage by stage: a stage is judged on what that stage read (the
partials, records or vectors of the stage before it, read back from the device), so one stage's error is never charged to the
next.  ``eps`` and every float scalar are the fp32 values, widened.  u = U32 = 2^-24, ULP32 = 2u, g(n) = n u / (1 - n u),
D64 = 2^-48 (order and cancellation of double arithmetic, relative to the summed magnitudes), U64 = 2^-53.  ``got`` passes where
``|got - ref| <= bar`` (conv_fp64_ref.ratio).  Every function works on CPU or device tensors alike (plain torch in fp64).

Launch rules, restated (tests/test_bn_instances_host.py ties each to the source or the library): a workgroup of THREADS = 256
serves one group of <= GROUP = 1024 channels with Q = min(1024, C - c0) / 4 channel lanes and PP = 256 / Q row lanes (256 - Q PP
threads idle), UNROLL = 4 rows in flight per thread, over rows_per_block = max(64, ceil(M / (2048 / groups))) rows; the workspace
holds blocks x C x 2 floats of partials and C x 4 of coef; the finalize / local kernels run 16 channels x SLICES = 16 row-block
slices; the statistics merge runs MERGE_THREADS = 1024 threads in one workgroup; sumsq runs min(ceil(n / 1024), SUMSQ_CAP = 1024)
blocks of 256, sgd min(ceil(n / 256), SGD_CAP = 8192).

* bn_stats_part, per (row block, channel), v = fl32(y - y[0]) (one fp32 subtraction, reproduced exactly in torch fp32), n rows in
  the block, nl = ceil(n / PP) rows on the longest lane, L = min(PP, n) lanes that own rows, A = max |v|, D = max |v - mean_b|
  over the block.  Welford on a lane: ``d = v - mean; mean += d / k; M2 += d (v - mean)``.  Step k of the mean rounds d, 1 / k,
  their product and the sum: 3 u |d| / k + u |mean_k|, damped by k / nl on the way to the lane's end: with |d| <= 2 A and
  |mean_k| <= A the lane mean errs by at most ``u A c``, c = 6 + (nl + 1) / 2.  Chan's merge keeps a convex combination and adds
  four roundings per lane merged, <= 7 u A each:
      mean_b   ``u A (c + 7 (L - 1))``
  M2: every term is rounded four times and added (g(nl + 3) of the lane's M2, all terms being >= 0); a running mean that is off
  by e changes a term by <= 2 e |d| and sum |d| <= 2 n D; the merge adds ``d^2 na nb / nn`` (seven roundings, L - 1 additions,
  between-lane sum <= M2_b) and sees lane means that are off by the mean bar (na nb / nn <= nl, nl L ~ n):
      M2_b     ``g(nl + L + 10) M2_b + u n D (A (8 c + 28 (L - 1) + 2) + 12 D)``
  These are worst-case first-order bounds; the emulation of the kernel's order stays far below them and one row dropped or
  counted twice is 10^3 bars away (tests/test_bn_instances_host.py).  A constant channel gives v = 0, bars 0 and exact zeros.
* bn_stats_finalize / bn_stats_local / bn_stats_merge from GIVEN partials / records: the arithmetic is double and every stored
  float is rounded once.  ``mean``, ``rstd``, ``scale``, ``cmean``: 1 ulp (``ULP32 |ref|``); ``shift``, ``cshift``:
  ``ULP32 (|beta| + |mean scale|)``; running buffers ``ULP32 |ref|``; all plus D64 of the summed magnitudes pushed through the
  formula (``|drstd| <= rstd^3 |dvar| / 2``); fp64 records: D64 of the summed magnitudes alone.  ``center == y[0]`` bit for bit;
  the count is an exact integer; ``nbt`` is incremented once; ``running_var`` is unbiased (M - 1, the global M - 1 for SyncBN);
  momentum < 0 uses 1 / nbt (the incremented value).  The square root and the division are double: their last bit is far
  inside D64.
* bn_apply from the vectors it was handed, elementwise: ``fma(y - ce, sc, sh)`` is one exact-or-rounded difference (u |y - ce|,
  times |sc|; none without a center) and one fma (u |t| <= u (|(y - ce) sc| + |sh|)); one ulp for each:
  ``ULP32 (2 |(y - ce) sc| + |sh|)`` (``ULP32 (|y sc| + |sh|)`` without a center); the residual form adds a rounded sum
  ``ULP32 |t + res|``; the two-input form a second such fma and a sum ``+ ULP32 |t + t2|``.  ReLU is 1-Lipschitz: no element
  is excluded.
* bn_bwd_part per (row block, channel), mask = the stored ``z > 0`` (exact: no element is ambiguous), x = (y - ce) - mu:
      sum g       ``2 g(nl + L - 2) sum |g|``                                  (fp32 lane sums, then L lanes in fp32)
      sum g x     ``ULP32 sum |g| (|y - ce| + |x|) + 2 g(nl + L) sum |g x|``     (two differences, an fma chain, L lanes)
  one ulp, not half, for every rounding: a block of one or two rows has too few roundings for their errors to average out.
* bn_bwd_finalize / bn_bwd_local / bn_bwd_merge from GIVEN partials / records: ``dgamma``, ``dbeta`` and the four ``coef``
  entries 1 ulp each plus D64 of the summed magnitudes; ``coef[3] == mean`` bit for bit.
* bn_bwd_apply from its OWN coef, elementwise ``cf0 (g - cf1 - ((y - ce) - cf3) cf2)``: six roundings, one ulp each:
      ``|cf0| ULP32 ((|y - ce| + |x|) |cf2| + |x cf2| + |g - cf1| + |r|) + ULP32 |cf0 r|``,  r = g - cf1 - x cf2.
* end to end against fp64 ``F.batch_norm(training=True)`` and its autograd with the kernel's ``z`` as mask: the stage bars
  pushed through the formulas per element (end_to_end below states each line).
* bn_fold against fp64 from the fp32 inputs: three roundings for ``scale`` (add, sqrt, divide), the sqrt given a full ulp:
  ``scale`` and ``inv_sigma`` ``2 ULP32 |ref|``; ``shift`` ``|mean| bar(scale) + ULP32 (|mean scale| + |shift|)``.
  bn_fold_multi: bit-equal to bn_fold, job by job; a null output pointer leaves its guard untouched.
* sumsq: double accumulation, ``D64 sum g^2`` plus one double rounding (U64) of every partial, ``(D64 + U64) sum g^2``
  (33 double roundings of the sum; the longest chain of the largest case has 34 -- 12 terms per thread, 9 per workgroup
  reduction, twice, and 4 partials per thread -- and reaches a few U64 in practice); accumulating: ``out = base + ref``,
  ``+ U64 |base + ref|``.
* sgd: ``coef = gs min(1, max_norm / (fl32(sqrt(norm2)) gs + 1e-6))`` has up to five chained fp32 roundings after the double
  sqrt (the division allowed a full ulp: g(6)); then per element, unfused (a fused form has fewer), one ulp per rounding:
  ``g = grad coef [+ wd p]``, ``b = first ? g : mu buf + g``, ``p - lr b``.  mu == 0: ``buf`` is not touched.
"""
import numpy as np
import torch

from tests.conv_fp64_ref import U32, ULP32, check, ratio  # noqa: F401  (re-exported)
from tests.stream_fp64_ref import D64, cdiv, g  # noqa: F401  (re-exported)

U64 = 2.0 ** -53

# ---- launch rules, restated ------------------------------------------------------------------------------------------
THREADS, UNROLL, GROUP = 256, 4, 1024
MIN_ROWS, TARGET_BLOCKS = 64, 2048
SLICES, FIN_CHANNELS = 16, 16
MERGE_THREADS = 1024
SUMSQ_CAP, SUMSQ_PER_BLOCK, SGD_CAP, BLOCK = 1024, 1024, 8192, 256


def groups(C):
    return cdiv(C, GROUP)


def lane_layout(C):
    """[(c0, channels, Q, PP, idle threads)] of every channel group of a launch."""
    out = []
    for c0 in range(0, C, GROUP):
        ch = min(GROUP, C - c0)
        Q = ch // 4
        PP = THREADS // Q
        out.append((c0, ch, Q, PP, THREADS - Q * PP))
    return out


def rows_per_block(M, C):
    return max(MIN_ROWS, cdiv(M, max(1, TARGET_BLOCKS // groups(C))))


def blocks(M, C):
    return cdiv(M, rows_per_block(M, C))


def ws_floats(M, C):
    return blocks(M, C) * C * 2 + C * 4


def block_rows(M, C):
    """Rows of every row block (the last may be short)."""
    rpb, nb = rows_per_block(M, C), blocks(M, C)
    return [min(rpb, M - b * rpb) for b in range(nb)]


def lane_rows(n, PP):
    """Rows each of the PP row lanes owns in a block of n rows (lane p: rows p, p + PP, ...)."""
    return [len(range(p, n, PP)) for p in range(PP)]


def tail_trips(n, PP):
    """Row lanes whose last trip of the 4-row unroll is partial (ok[u] false for some u: the clamped reload is taken)."""
    return [p for p, k in enumerate(lane_rows(n, PP)) if k % UNROLL]


def sumsq_grid(n):
    return min(cdiv(n, SUMSQ_PER_BLOCK), SUMSQ_CAP)


def sgd_grid(n):
    return min(cdiv(n, BLOCK), SGD_CAP)


def f32(v):
    """A Python number as the fp32 value a C float argument carries, widened."""
    return float(np.float32(v))


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _blocked(t, M, C, fill=0.0):
    """(M, C) -> (blocks, rows_per_block, C), padded past M with ``fill``."""
    rpb, nb = rows_per_block(M, C), blocks(M, C)
    if nb * rpb != M:
        t = torch.cat([t, t.new_full((nb * rpb - M, C), fill)], 0)
    return t.view(nb, rpb, C)


def _counts(M, C, like):
    """-> n (blocks, 1), nl, L (blocks, C): rows of each block, rows on its longest lane, lanes that own rows, per channel."""
    n = torch.tensor(block_rows(M, C), dtype=torch.float64, device=like.device).view(-1, 1)
    pp = torch.empty(C, dtype=torch.float64, device=like.device)
    for c0, ch, _, PP, _ in lane_layout(C):
        pp[c0:c0 + ch] = PP
    pp = pp.view(1, C)
    return n, torch.ceil(n / pp), torch.minimum(pp.expand(n.shape[0], C), n.expand(-1, C))


def shifted(y):
    """v = fl32(y - y[0]) widened: what bn_stats_part accumulates.  y (M, C) fp32."""
    assert y.dtype == torch.float32
    return (y - y[0:1]).double()


# ---- statistics ------------------------------------------------------------------------------------------------------
def stats_part_ref(y):
    """y (M, C) fp32 -> (ref, bar) (blocks, C, 2): (mean_b, M2_b) of v = fl32(y - y[0]) over each row block."""
    M, C = y.shape
    v = _blocked(shifted(y), M, C)
    n, nl, L = _counts(M, C, v)
    valid = (torch.arange(v.shape[1], device=v.device).view(1, -1, 1) < n.view(-1, 1, 1))
    mean = v.sum(1) / n
    A = v.abs().amax(1)
    dev = torch.where(valid, v - mean.unsqueeze(1), torch.zeros_like(v))
    del v
    m2 = (dev * dev).sum(1)
    D = dev.abs().amax(1)
    del dev
    c = 6 + (nl + 1) / 2
    bar_mean = U32 * A * (c + 7 * (L - 1))
    bar_m2 = g(nl + L + 10) * m2 + U32 * n * D * (A * (8 * c + 28 * (L - 1) + 2) + 12 * D)
    return torch.stack([mean, m2], -1), torch.stack([bar_mean, bar_m2], -1)


def combine_partials(part, M, C):
    """part (blocks, C, 2) fp64 -> msh, m2 (C) by Chan's k-group form, and their D64 bars."""
    n = torch.tensor(block_rows(M, C), dtype=torch.float64, device=part.device).view(-1, 1)
    pm, p2 = part[..., 0], part[..., 1]
    msh = (n * pm).sum(0) / M
    d = pm - msh
    m2 = (p2 + n * d * d).sum(0)
    dmsh = D64 * (n * pm.abs()).sum(0) / M
    dm2 = D64 * (p2.abs() + n * (pm.abs() + msh.abs()) ** 2).sum(0) + 2 * (n * d.abs()).sum(0) * dmsh
    return msh, m2, dmsh, dm2


def combine_records(recs, C):
    """recs (R, 2C + 1) fp64 -> mu, m2 (C), the global count, and their D64 bars."""
    cnt = recs[:, 2 * C].view(-1, 1)
    Mg = cnt.sum()
    rm, r2 = recs[:, :C], recs[:, C:2 * C]
    mu = (cnt * rm).sum(0) / Mg
    d = rm - mu
    m2 = (r2 + cnt * d * d).sum(0)
    dmu = D64 * (cnt * rm.abs()).sum(0) / Mg
    dm2 = D64 * (r2.abs() + cnt * (rm.abs() + mu.abs()) ** 2).sum(0) + 2 * (cnt * d.abs()).sum(0) * dmu
    return mu, m2, float(Mg), dmu, dm2


def stat_vectors(mu, msh, m2, count, gamma, beta, eps, dmu, dmsh, dm2, rm=None, rv=None, momentum=0.1, nbt_after=None):
    """The stored vectors of bn_stats_finalize / bn_stats_merge from the combined (mu, msh, m2): {name: (ref, bar)}.
    count: the (global) row count; momentum < 0: 1 / nbt_after."""
    eps = f32(eps)
    var = m2 / count
    rstd = (var + eps) ** -0.5
    drstd = 0.5 * rstd ** 3 * (dm2 / count + D64 * (var + eps))
    sc = gamma * rstd
    dsc = gamma.abs() * drstd
    out = dict(mean=(mu, ULP32 * mu.abs() + dmu), rstd=(rstd, ULP32 * rstd + drstd), scale=(sc, ULP32 * sc.abs() + dsc),
               shift=(beta - mu * sc, ULP32 * (beta.abs() + (mu * sc).abs()) + sc.abs() * dmu + mu.abs() * dsc),
               cmean=(msh, ULP32 * msh.abs() + dmsh),
               cshift=(beta - msh * sc, ULP32 * (beta.abs() + (msh * sc).abs()) + sc.abs() * dmsh + msh.abs() * dsc))
    if rm is not None:
        m = f32(momentum) if momentum >= 0 else 1.0 / nbt_after
        unb = m2 / (count - 1)
        nm, nv = (1 - m) * rm + m * mu, (1 - m) * rv + m * unb
        out['running_mean'] = (nm, ULP32 * nm.abs() + D64 * (((1 - m) * rm).abs() + (m * mu).abs()) + m * dmu)
        out['running_var'] = (nv, ULP32 * nv.abs() + D64 * (((1 - m) * rv).abs() + (m * unb).abs()) + m * dm2 / (count - 1))
    return out


def finalize_ref(part, y0, M, gamma, beta, eps, rm=None, rv=None, momentum=0.1, nbt_after=None):
    """part (blocks, C, 2), y0 = y[0] (C), gamma, beta, rm, rv: fp64 of the fp32 values the kernel reads -> {name: (ref, bar)}."""
    C = y0.numel()
    msh, m2, dmsh, dm2 = combine_partials(part, M, C)
    mu = y0 + msh
    return stat_vectors(mu, msh, m2, float(M), gamma, beta, eps, dmsh + D64 * (y0.abs() + msh.abs()), dmsh, dm2, rm, rv, momentum, nbt_after)


def local_record_ref(part, y0, M):
    """-> (ref, bar) (2C + 1): [absolute mean | M2 | count] of one rank; the count's bar is 0 (exact)."""
    C = y0.numel()
    msh, m2, dmsh, dm2 = combine_partials(part, M, C)
    one = msh.new_tensor([float(M)])
    return torch.cat([y0 + msh, m2, one]), torch.cat([dmsh + D64 * (y0.abs() + msh.abs()), dm2 + D64 * m2, 0 * one])


def merge_ref(recs, y0, gamma, beta, eps, rm=None, rv=None, momentum=0.1, nbt_after=None):
    """recs (R, 2C + 1) fp64 as the kernel reads them, y0: THIS rank's first row -> ({name: (ref, bar)}, global count)."""
    C = y0.numel()
    mu, m2, Mg, dmu, dm2 = combine_records(recs, C)
    msh = mu - y0
    return stat_vectors(mu, msh, m2, Mg, gamma, beta, eps, dmu, dmu + D64 * (mu.abs() + y0.abs()), dm2, rm, rv, momentum, nbt_after), Mg


# ---- apply -----------------------------------------------------------------------------------------------------------
def _affine(y, ce, sc, sh):
    d = y if ce is None else y - ce
    return d * sc + sh, ULP32 * ((1 if ce is None else 2) * (d * sc).abs() + sh.abs())


def apply_ref(y, ce, sc, sh, relu, residual=None, y2=None, ce2=None, sc2=None, sh2=None):
    """Everything fp64 of the fp32 values, (M, C) maps and (C) vectors (None: absent) -> (ref, bar)."""
    t, bar = _affine(y, ce, sc, sh)
    if residual is not None:
        t = t + residual
        bar = bar + ULP32 * t.abs()
    elif y2 is not None:
        t2, bar2 = _affine(y2, ce2, sc2, sh2)
        t = t + t2
        bar = bar + bar2 + ULP32 * t.abs()
    return (t.clamp_min(0) if relu else t), bar


# ---- backward --------------------------------------------------------------------------------------------------------
def masked(dout, z):
    return dout if z is None else torch.where(z > 0, dout, torch.zeros_like(dout))


def bwd_part_ref(dout, z, y, ce, mu):
    """dout, y (M, C) fp64, z (M, C) the stored output or None, ce (C) or None, mu (C) -> (ref, bar) (blocks, C, 2)."""
    M, C = y.shape
    gm = masked(dout, z)
    d1 = y if ce is None else y - ce
    x = d1 - mu
    n, nl, L = _counts(M, C, y)
    B = lambda t: _blocked(t, M, C).sum(1)                                       # noqa: E731
    sa, sb = B(gm), B(gm * x)
    bar_a = 2 * g(nl + L - 2) * B(gm.abs())
    bar_b = ULP32 * B(gm.abs() * (d1.abs() + x.abs())) + 2 * g(nl + L) * B((gm * x).abs())
    return torch.stack([sa, sb], -1), torch.stack([bar_a, bar_b], -1)


def _coef(sa, sb, dsa, dsb, count, mean, rstd, gamma):
    dg = rstd * sb
    one = lambda r, d: (r, ULP32 * r.abs() + d)                                  # noqa: E731
    coef = torch.stack([gamma * rstd, sa / count, rstd * dg / count, mean], -1)
    cbar = torch.stack([ULP32 * (gamma * rstd).abs(), ULP32 * (sa / count).abs() + dsa / count,
                        ULP32 * (rstd * dg / count).abs() + rstd * rstd * dsb / count, 0 * mean], -1)
    return dict(dgamma=one(dg, rstd * dsb), dbeta=one(sa, dsa), coef=(coef, cbar))


def bwd_finalize_ref(part, count, mean, rstd, gamma):
    """part (blocks, C, 2) fp64 of the stored partials; mean, rstd, gamma fp64 of the fp32 vectors -> dgamma, dbeta (C), coef (C, 4)."""
    sa, sb = part[..., 0].sum(0), part[..., 1].sum(0)
    return _coef(sa, sb, D64 * part[..., 0].abs().sum(0), D64 * part[..., 1].abs().sum(0), float(count), mean, rstd, gamma)


def bwd_local_record_ref(part):
    """-> (ref, bar) (2C): [sum g | sum g (y - mean)] of one rank."""
    return torch.cat([part[..., 0].sum(0), part[..., 1].sum(0)]), D64 * torch.cat([part[..., 0].abs().sum(0), part[..., 1].abs().sum(0)])


def bwd_merge_ref(recs, count, mean, rstd, gamma):
    """recs (R, 2C) fp64 -> coef (C, 4) (ref, bar) from the sums over all ranks."""
    C = mean.numel()
    sa, sb = recs[:, :C].sum(0), recs[:, C:].sum(0)
    return _coef(sa, sb, D64 * recs[:, :C].abs().sum(0), D64 * recs[:, C:].abs().sum(0), float(count), mean, rstd, gamma)['coef']


def bwd_apply_ref(dout, z, y, coef, ce):
    """coef (C, 4) fp64 of the kernel's own workspace -> (ref, bar) (M, C)."""
    cf0, cf1, cf2, cf3 = coef.unbind(-1)
    gm = masked(dout, z)
    d1 = y if ce is None else y - ce
    x = d1 - cf3
    w = x * cf2
    s = gm - cf1
    r = s - w
    bar = cf0.abs() * ULP32 * ((d1.abs() + x.abs()) * cf2.abs() + w.abs() + s.abs() + r.abs()) + ULP32 * (cf0 * r).abs()
    return cf0 * r, bar


# ---- end to end ------------------------------------------------------------------------------------------------------
def end_to_end(y32, gamma, beta, eps, relu, z_kernel, dout, part_bar, bwd_part_bar_fn, center):
    """Against fp64 F.batch_norm(training=True) of y32 (M, C) fp32 and its autograd, the ReLU mask being the kernel's stored z.
    part_bar (blocks, C, 2): stats_part_ref's bars; bwd_part_bar_fn(mu_center) -> bwd_part_ref's bars at the true operands;
    center: whether the centred form is applied (ce = y[0]).  -> {name: (ref, bar)} for mean, rstd, z, dbeta, dgamma, dy.

    The stage bars, pushed through per element (first order; every stored float adds its ulp):
      dmsh  = sum_b n_b bar(mean_b) / M,   dmean = dmsh + ULP32 |mean|
      dm2   = sum_b (bar(M2_b) + 2 n_b |mean_b - msh| (bar(mean_b) + dmsh)),   dvar = dm2 / M
      drstd = rstd^3 dvar / 2 + ULP32 rstd,   dscale = |gamma| drstd + ULP32 |scale|
      z     : apply bar + |y - ce| dscale + (|scale| (dmsh + ULP32 |msh|) + |msh| dscale + ULP32 (|beta| + |msh scale|))
      Sa, Sb: the partial bars summed, + sum |g| (dmsh + ULP32 |msh|) for the mean inside x
      dbeta = Sa, dgamma = rstd Sb: rstd dSb + |Sb| drstd, one ulp each
      dy    = cf0 (g - cf1 - x cf2): |inner| dcf0 + |cf0| (dcf1 + dx |cf2| + |x| dcf2) + the bwd_apply bar
    """
    import torch.nn.functional as F
    M, C = y32.shape
    eps = f32(eps)
    yd = y32.double()
    x = yd.detach().clone().requires_grad_(True)
    gm_, bt_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    lin = F.batch_norm(x, None, None, gm_, bt_, True, 0.0, eps)
    mask = (z_kernel > 0).double() if relu else torch.ones_like(yd)
    (lin * mask * dout).sum().backward()
    lin = lin.detach()
    mu = yd.mean(0)
    var = ((yd - mu) ** 2).mean(0)
    rstd = (var + eps) ** -0.5
    sc = gamma * rstd
    y0 = yd[0]
    msh = mu - y0
    n = torch.tensor(block_rows(M, C), dtype=torch.float64, device=yd.device).view(-1, 1)
    vb = _blocked(shifted(y32), M, C).sum(1) / n                                  # block means of v
    dmsh = (n * part_bar[..., 0]).sum(0) / M
    dm2 = (part_bar[..., 1] + 2 * n * (vb - msh).abs() * (part_bar[..., 0] + dmsh)).sum(0)
    drstd = 0.5 * rstd ** 3 * dm2 / M + ULP32 * rstd
    dsc = gamma.abs() * drstd + ULP32 * sc.abs()
    ce = y0 if center else None
    off = msh if center else mu
    dcm = dmsh + ULP32 * off.abs() + D64 * (y0.abs() + msh.abs())                 # error of center + cmean (or mean) against the true mean
    d1 = yd - y0 if center else yd
    zref, zbar = apply_ref(yd, ce, sc, beta - off * sc, relu)
    zbar = zbar + d1.abs() * dsc + sc.abs() * dcm + off.abs() * dsc + ULP32 * (beta.abs() + (off * sc).abs())
    out = dict(mean=(mu, dmsh + ULP32 * mu.abs() + D64 * (y0.abs() + msh.abs())), rstd=(rstd, drstd), z=(zref, zbar))
    # backward
    g_ = mask * dout
    xc = yd - mu
    pb = bwd_part_bar_fn(off)
    Sa, Sb = g_.sum(0), (g_ * xc).sum(0)
    dSa = pb[..., 0].sum(0) + D64 * g_.abs().sum(0)
    dSb = pb[..., 1].sum(0) + g_.abs().sum(0) * dcm + D64 * (g_ * xc).abs().sum(0)
    dgam = rstd * Sb
    out['dbeta'] = (Sa, dSa + ULP32 * Sa.abs())
    out['dgamma'] = (dgam, rstd * dSb + Sb.abs() * drstd + ULP32 * dgam.abs())
    cf0, cf1, cf2 = sc, Sa / M, rstd * dgam / M
    dcf0 = dsc
    dcf1 = dSa / M + ULP32 * cf1.abs()
    dcf2 = (2 * rstd * drstd * Sb.abs() + rstd * rstd * dSb) / M + ULP32 * cf2.abs()
    inner = g_ - cf1 - xc * cf2
    coef = torch.stack([cf0, cf1, cf2, off], -1)
    _, abar = bwd_apply_ref(dout, z_kernel if relu else None, yd, coef, ce)
    dybar = abar + inner.abs() * dcf0 + cf0.abs() * (dcf1 + dcm * cf2.abs() + xc.abs() * dcf2)
    out['dy'] = (x.grad, dybar)
    out['dgamma_autograd'], out['dbeta_autograd'] = gm_.grad, bt_.grad
    return out


# ---- bn_fold ---------------------------------------------------------------------------------------------------------
def bn_fold_ref(gamma, beta, mean, var, eps):
    """fp64 of the fp32 inputs -> {scale, shift, inv_sigma: (ref, bar)}."""
    sd = (var + f32(eps)).sqrt()
    sc, inv = gamma / sd, 1.0 / sd
    bsc = 2 * ULP32 * sc.abs()
    sh = beta - mean * sc
    return dict(scale=(sc, bsc), inv_sigma=(inv, 2 * ULP32 * inv), shift=(sh, mean.abs() * bsc + ULP32 * ((mean * sc).abs() + sh.abs())))


# ---- optimiser -------------------------------------------------------------------------------------------------------
def sumsq_ref(gd, base=None):
    """gd: fp64 of the fp32 gradient -> (ref, bar) of out[0]; base: the value accumulated into (a Python float) or None."""
    s = float((gd * gd).sum())
    ref = s if base is None else base + s
    return ref, (D64 + U64) * s + (U64 * abs(ref) if base is not None else 0.0)


def sgd_coef_ref(norm2, max_norm, grad_scale):
    """-> (coef, relative bar): the clip coefficient in fp64 from the fp32 scalars (norm2 a Python double or None)."""
    gs = f32(grad_scale)
    if not f32(max_norm) > 0:
        return gs, 0.0
    c = f32(max_norm) / (norm2 ** 0.5 * gs + f32(1e-6))
    return gs * min(c, 1.0), float(g(6))


def sgd_ref(p, grad, buf, coef, coef_rel, lr, mu, wd, first):
    """p, grad, buf (None with mu == 0): fp64 of the fp32 buffers BEFORE the step -> {p: (ref, bar), buf: (ref, bar) | None}."""
    lr, mu, wd = f32(lr), f32(mu), f32(wd)
    gv = grad * coef
    eg = (coef_rel + ULP32) * gv.abs()
    if wd != 0:
        w = wd * p
        gv = gv + w
        eg = eg + ULP32 * w.abs() + ULP32 * gv.abs()
    b, eb, bufout = gv, eg, None
    if mu != 0:
        if not first:
            mb = mu * buf
            b = mb + gv
            eb = eg + ULP32 * mb.abs() + ULP32 * b.abs()
        bufout = (b, eb)
    step = lr * b
    pn = p - step
    return dict(p=(pn, lr * eb + ULP32 * step.abs() + ULP32 * pn.abs()), buf=bufout)
