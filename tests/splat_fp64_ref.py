"""fp64 references of the nine split-attention kernels (csrc/splat.hip) stage by stage, and the bars a HIP kernel must meet, every bar
derived by counting the roundings the kernel performs.  Pure torch, fp64, on CPU or device tensors.

Every stage is judged on the operands THAT STAGE read: chunk partials, per-image column sums and the ``da | dh' | dh | xhat`` records
are read back from the workspace and fed to the reference of the launch that consumes them.  u = U32 = 2^-24 is the fp32 unit
roundoff, ULP32 = 2 u, g(n) = n u / (1 - n u) the bound on n chained roundings (tests/stream_fp64_ref.py); ``got`` passes where
``|got - ref| <= bar`` (conv_fp64_ref.ratio).  Every source-level operation counts as one rounding; splat.hip is built with
contraction on and fusing only removes roundings, so the bars hold either way.  Sums get ``g(n) * sum |terms|``; results of at most
four roundings get one WHOLE ulp per rounding, ``g(2 n)`` (half-ulp counting can be met exactly there -- the lesson of the BatchNorm
pins; ``gs(n)`` below is that rule: a two-chunk per-image sum is ONE addition, which reaches the whole of ``g(1)``); a masked-out
element (``u <= 0``, ``z <= 0``) must be bit +0.0.

Launch rules, restated (tests/test_splat_instances_host.py ties each to the source text or the library):
  WV = w / 4 lanes per pixel, PP = 256 // WV pixels per workgroup step, chunk CH = 16 PP pixels, K = ceil(HW / CH) chunks per image.
  Lane (prow, cv) of chunk k walks pixels k CH + prow, + PP, ... in order; lanes with prow >= PP (256 - PP WV of them) are idle.
  The lanes of a channel are added with prow ascending, then the chunks ascending, then (column sums) the images ascending.
  Workspaces (floats): N K w (gap), N K 2w (attn_grad), N K 2w + N 2w (apply_bwd, the per-image sums at offset N K 2w),
  N (2w + 3 inter) (attn_bwd, per image ``da | dh' | dh | xhat``).
  Pooled size ((H - 1) // 2 + 1, (W - 1) // 2 + 1); the pool's adjoint at input pixel (ih, iw) reads the outputs
  ih >> 1 .. (ih + 1) >> 1 clipped at OH, the same in w.  splat_apply runs min(ceil(NP / PP), 65536) workgroups.
  The attention kernels run 1024 lanes, one wave per output row; a dot product is a lane stride of 64, then the xor butterfly
  32, 16, .., 1: ceil(len / 64) fma roundings and 6 additions.

Bars (cnt = pixels of the chunk, lane = ceil(cnt / PP) the longest walk):
  gap partial     ref sum_chunk (u0 + u1); n = 1 + lane + PP - 1 (the pair's own sum, the walk, the lanes) on sum (|u0| + |u1|)
  gap final       from the kernel's own partials: sum_k / HW; n = K + 1 (K - 1 additions, the rounded 1.f / (float)HW, the product)
  gap end to end  against the fp64 mean of u: the partial bars / HW plus g(K + 1) of (|partial| + bar) / HW
  apply           n = 3 on |a0 x0| + |a1 x1| (g(6)); pooled n = 3 + 9 + 2 on (1 / 9) sum_taps (...): the divisor is always 9
  attn_grad       partial n = 1 + lane + PP - 1 on sum |dv| |u|; pooled: dv carries 6 more roundings on (1 / 9) sum |dout| (up to
                  four additions, the rounded 1.f / 9.f, the product); final n = K - 1 on the own partials
  attn h          n = ceil(w / 64) + 6 + 1 on sum |fc1| |g| + |b1|
  attn z          |s1| bar_h + g(2) (|s1 h| + |t1|); relu is 1-Lipschitz, no element is excluded; where the pre-activation y is
                  negative the bar shrinks to max(y + bar, 0): a z the reference clips by more than its bar must be exactly 0
  attn logits     fp64 from the kernel's OWN z (record): n = ceil(inter / 64) + 6 + 1 on sum |fc2| |z| + |b2| -> bar_a
  attn att_r      r0 r1 (bar_a0 + bar_a1 + U32 |a0 - a1|) + 6 ULP32 att_r + 2^-126.  d att_r / d a_r = r0 r1, first order; the rounded
                  subtraction a_r - max errs by U32 |a0 - a1|; 6 = 2 E_EXP + 2 with E_EXP = 2: the 1 ulp the HIP math documentation
                  states for expf (no other figure is given in the ROCm documentation installed with the toolchain), doubled, plus
                  the sum, a reciprocal not assumed correctly rounded, and the product; 2^-126 covers a denormal or flushed expf
                  result.  The first-order push needs bar_a <= BAR_A_MAX = 1e-4: asserted per case from fp64 alone.
  attn end to end from g: the bars of h, z, a pushed through in fp64; bar_a is larger here (up to 6.1e-4 at w = inter = 1024), so the
                  first-order term carries the factor exp(2 delta) that bounds r0 r1 over the whole interval (softmax_ref)
  attn_bwd da_r   s = a0 d0 + a1 d1, da_r = a_r (d_r - s): |a_r| (g(6) (|a0 d0| + |a1 d1|) + ULP32 (|d_r| + |s|)) + ULP32 |da_r|
  attn_bwd xhat   (h - mean) inv: |inv| (bar_h + ULP32 (|h| + |mean|)) + ULP32 |xhat|
  attn_bwd dh'    from the own da: a serial fma chain, n = 2w on sum |fc2| |da|; the mask is the input z; masked: bit +0.0
  attn_bwd dh     s1 dh': |s1| bar_dh' + ULP32 |dh|
  attn_bwd dg     from the own dh: n = inter on sum |fc1| |dh|
  parameter sums  from the own workspace and the inputs z, g: n = N on sum |terms| (order-free: any order of images passes)
  apply_bwd du    |a| bar_dv + g(4) (|a dv| + |dg| / HW) + g(4) |dg| / HW (the last term: dg fl(1 / HW)); u <= 0: bit +0.0
  apply_bwd sums  chunk partial from the own du: n = lane + PP - 1; per image n = K - 1; colsum n = N - 1
"""
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import U32, ULP32, check, ratio  # noqa: F401  (re-exported)
from tests.stream_fp64_ref import D64, g  # noqa: F401  (re-exported)

MAX_W, MAX_INTER, WALK, THREADS, ATTN_THREADS = 1024, 1024, 16, 256, 1024
APPLY_GRID_CAP, N_CAP = 65536, 65535
E_EXP = 2
TINY = 2.0 ** -126
BAR_A_MAX = 1e-4


# ---- integer rules ---------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def wv(w):
    return w // 4


def pp(w):
    return THREADS // wv(w)


def idle_lanes(w):
    return THREADS - pp(w) * wv(w)


def chunk(w):
    return WALK * pp(w)


def chunks(HW, w):
    return cdiv(HW, chunk(w))


def chunk_counts(HW, w):
    CH = chunk(w)
    return [min(HW, (k + 1) * CH) - k * CH for k in range(chunks(HW, w))]


def lane_pixels(HW, w, k):
    """The pixels lane prow = 0 .. PP - 1 of chunk k walks, in order."""
    CH, P = chunk(w), pp(w)
    return [list(range(k * CH + r, min(HW, (k + 1) * CH), P)) for r in range(P)]


def pooled(H, W, pool):
    return ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (H, W)


def adjoint_window(i, O):
    """Output indices whose 3x3 / 2 window (padding 1) holds input index i."""
    return [o for o in range(i >> 1, ((i + 1) >> 1) + 1) if o < O]


def ws_gap(N, HW, w):
    return N * chunks(HW, w) * w


def ws_attn_grad(N, HW, w):
    return N * chunks(HW, w) * 2 * w


def ws_apply_bwd(N, HW, w):
    return N * chunks(HW, w) * 2 * w + N * 2 * w


def ws_attn_bwd(N, w, inter):
    return N * (2 * w + 3 * inter)


def apply_grid(NP, w):
    return min(cdiv(NP, pp(w)), APPLY_GRID_CAP)


def apply_strides(NP, w):
    """Trips of splat_apply's grid-stride loop on the longest lane."""
    return cdiv(NP, apply_grid(NP, w) * pp(w))


def apply_reloads(N, OHW, w):
    """Lanes of splat_apply whose next pixel lies in a later image (the ``n != ncur`` reload after the first trip)."""
    NP, step = N * OHW, apply_grid(N * OHW, w) * pp(w)
    if NP <= step:
        return 0
    p = torch.arange(0, NP - step, dtype=torch.int64)
    return int(((p // OHW) != ((p + step) // OHW)).sum())


def gs(n):
    """The bound of a sum of n roundings: g(n), and one whole ulp per rounding, g(2 n), where n <= 4 (n a number or a tensor)."""
    n = torch.as_tensor(n, dtype=torch.float64)
    return g(torch.where(n <= 4, 2 * n, n))


def dot_n(length):
    return cdiv(length, 64) + 6 + 1


# ---- chunk sums --------------------------------------------------------------------------------------------------
def _chunk_sum(v, w):
    """v (N, HW, C) -> (N, K, C): the sum over each pixel chunk."""
    N, HW, C = v.shape
    K, CH = chunks(HW, w), chunk(w)
    if K == 1:
        return v.sum(1, keepdim=True)
    if K * CH != HW:
        v = torch.cat([v, v.new_zeros((N, K * CH - HW, C))], 1)
    return v.view(N, K, CH, C).sum(2)


def _chunk_n(HW, w, device):
    """(1, K, 1): lane + PP - 1 of every chunk (the walk of the longest lane and the additions over the lanes)."""
    P = pp(w)
    return torch.tensor([cdiv(c, P) + P - 1 for c in chunk_counts(HW, w)], dtype=torch.float64, device=device).view(1, -1, 1)


def rows_sum_ref(part, scale_n=0, scale=1.0):
    """part (B, rows, C) fp64 of the kernel's own stored partials -> (ref, bar) (B, C): ascending fp32 additions, n = rows - 1 +
    scale_n roundings."""
    ref = part.sum(1) * scale
    return ref, gs(part.shape[1] - 1 + scale_n) * part.abs().sum(1) * abs(scale)


# ---- gap ---------------------------------------------------------------------------------------------------------
def gap_partial_ref(u, w):
    """u (N, HW, 2w) fp64 -> (ref, bar) (N, K, w)."""
    N, HW, _ = u.shape
    ref = _chunk_sum(u[..., :w] + u[..., w:], w)
    mag = _chunk_sum(u[..., :w].abs() + u[..., w:].abs(), w)
    return ref, gs(1 + _chunk_n(HW, w, u.device)) * mag


def gap_final_ref(part, HW):
    """part (N, K, w): the kernel's own partials -> (ref, bar) (N, w)."""
    return rows_sum_ref(part, scale_n=2, scale=1.0 / HW)


def gap_end_to_end(u, w):
    N, HW, _ = u.shape
    pref, pbar = gap_partial_ref(u, w)
    K = pref.shape[1]
    ref = (u[..., :w] + u[..., w:]).sum(1) / HW
    return ref, pbar.sum(1) / HW + gs(K + 1) * (pref.abs() + pbar).sum(1) / HW


# ---- the fused average pool and its adjoint ----------------------------------------------------------------------------
def pool9(v):
    """v (N, H, W, C) -> AvgPool2d(3, 2, 1) with the divisor always 9, (N, OH, OW, C)."""
    return F.avg_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1, count_include_pad=True).permute(0, 2, 3, 1)


def _gather_windows(d, dim, L):
    O = d.shape[dim]
    i = torch.arange(L, device=d.device)
    lo, hi = i >> 1, (i + 1) >> 1
    second = (hi != lo) & (hi < O)
    shape = [1] * d.dim()
    shape[dim] = L
    a = d.index_select(dim, lo)
    b = d.index_select(dim, hi.clamp(max=O - 1))
    return a + torch.where(second.view(shape), b, torch.zeros_like(b))


def pool9_adjoint(dout, H, W):
    """dout (N, OH, OW, C) -> (dv, mag) (N, H, W, C): the adjoint of pool9 in gather form and (1 / 9) sum |dout| over the same windows."""
    dv = _gather_windows(_gather_windows(dout, 1, H), 2, W) / 9
    mag = _gather_windows(_gather_windows(dout.abs(), 1, H), 2, W) / 9
    return dv, mag


def dv_ref(dout, H, W, pool):
    """-> (dv, bar_dv, mag, extra roundings) of the gradient reaching v, (N, HW, w)."""
    N, C = dout.shape[0], dout.shape[-1]
    if not pool:
        d = dout.reshape(N, H * W, C)
        return d, torch.zeros_like(d), d.abs(), 0
    dv, mag = pool9_adjoint(dout, H, W)
    dv, mag = dv.reshape(N, H * W, C), mag.reshape(N, H * W, C)
    return dv, g(6) * mag, mag, 6


# ---- apply -------------------------------------------------------------------------------------------------------
def apply_ref(u, att, pool):
    """u (N, H, W, 2w), att (N, 2, w) fp64 -> (ref, bar) (N, OH, OW, w)."""
    w = att.shape[-1]
    t0, t1 = att[:, 0].view(-1, 1, 1, w) * u[..., :w], att[:, 1].view(-1, 1, 1, w) * u[..., w:]
    v, mag = t0 + t1, t0.abs() + t1.abs()
    if not pool:
        return v, gs(3) * mag
    return pool9(v), g(3 + 9 + 2) * pool9(mag)


# ---- attn_grad ---------------------------------------------------------------------------------------------------
def attn_grad_partial_ref(dout, u, pool):
    """dout (N, OH, OW, w), u (N, H, W, 2w) fp64 -> (ref, bar) (N, K, 2w)."""
    N, H, W, w2 = u.shape
    w = w2 // 2
    dv, _, mag, extra = dv_ref(dout, H, W, pool)
    uf = u.reshape(N, H * W, w2)
    ref = _chunk_sum(torch.cat([dv, dv], 2) * uf, w)
    m = _chunk_sum(torch.cat([mag, mag], 2) * uf.abs(), w)
    return ref, gs(1 + extra + _chunk_n(H * W, w, u.device)) * m


# ---- attention forward -------------------------------------------------------------------------------------------
def attn_h_ref(gv, fc1w, fc1b):
    """gv (N, w), fc1w (inter, w), fc1b (inter) fp64 -> (h, bar_h) (N, inter)."""
    h = gv @ fc1w.t() + fc1b
    return h, g(dot_n(gv.shape[1])) * (gv.abs() @ fc1w.abs().t() + fc1b.abs())


def attn_z_ref(gv, fc1w, fc1b, s1, t1):
    h, bh = attn_h_ref(gv, fc1w, fc1b)
    y = s1 * h + t1
    bar = s1.abs() * bh + g(2) * ((s1 * h).abs() + t1.abs())
    return y.clamp_min(0), torch.where(y < 0, (y + bar).clamp_min(0), bar)


def logits_ref(z, fc2w, fc2b, bar_z=None):
    """z (N, inter), fc2w (2w, inter), fc2b (2w) fp64 -> (a, bar_a) (N, 2w); bar_z: the bar of z where z is not the kernel's own."""
    a = z @ fc2w.t() + fc2b
    zm = z.abs() if bar_z is None else z.abs() + bar_z
    bar = g(dot_n(z.shape[1])) * (zm @ fc2w.abs().t() + fc2b.abs())
    if bar_z is not None:
        bar = bar + bar_z @ fc2w.abs().t()
    return a, bar


def softmax_ref(a, bar_a, exact=False):
    """a, bar_a (N, 2w) fp64 -> (att, bar) (N, 2, w).  exact: the first-order term times exp(2 delta), which bounds the derivative
    r0 r1 over the whole interval of width delta = bar_a0 + bar_a1 + U32 |a0 - a1| (each of r0, r1 grows by at most exp(delta))."""
    N = a.shape[0]
    a, bar_a = a.view(N, 2, -1), bar_a.view(N, 2, -1)
    att = torch.softmax(a, 1)
    rr = (att[:, 0] * att[:, 1]).unsqueeze(1)
    diff = (a[:, 0] - a[:, 1]).abs().unsqueeze(1)
    delta = bar_a.sum(1, keepdim=True) + U32 * diff
    first = rr * delta * (torch.exp(2 * delta) if exact else 1.0)
    return att, first + (2 * E_EXP + 2) * ULP32 * att + TINY


def attn_end_to_end(gv, fc1w, fc1b, s1, t1, fc2w, fc2b):
    z, bz = attn_z_ref(gv, fc1w, fc1b, s1, t1)
    a, ba = logits_ref(z, fc2w, fc2b, bar_z=bz)
    return softmax_ref(a, ba, exact=True) + (ba,)


# ---- attention backward ------------------------------------------------------------------------------------------
def da_ref(att, datt):
    """att, datt (N, 2, w) fp64 -> (da, bar) (N, 2w)."""
    N = att.shape[0]
    p = att * datt
    s = p.sum(1, keepdim=True)
    da = att * (datt - s)
    bar = att.abs() * (g(6) * p.abs().sum(1, keepdim=True) + ULP32 * (datt.abs() + s.abs())) + ULP32 * da.abs()
    return da.reshape(N, -1), bar.reshape(N, -1)


def xhat_ref(gv, fc1w, fc1b, mean, inv):
    h, bh = attn_h_ref(gv, fc1w, fc1b)
    x = (h - mean) * inv
    return x, inv.abs() * (bh + ULP32 * (h.abs() + mean.abs())) + ULP32 * x.abs()


def dhp_ref(da, fc2w, z):
    """da (N, 2w): the kernel's own record; z (N, inter) the input -> (dh', bar, mask)."""
    keep = z > 0
    s = da @ fc2w
    bar = gs(da.shape[1]) * (da.abs() @ fc2w.abs())
    zero = torch.zeros_like(s)
    return torch.where(keep, s, zero), torch.where(keep, bar, zero), keep


def dh_ref(dhp, bar_dhp, s1):
    dh = s1 * dhp
    return dh, s1.abs() * bar_dhp + ULP32 * dh.abs()


def dg_ref(dh, fc1w):
    """dh (N, inter): the kernel's own record -> (dg, bar) (N, w)."""
    return dh @ fc1w, gs(dh.shape[1]) * (dh.abs() @ fc1w.abs())


def param_refs(rec, z, gv, w, inter):
    """rec (N, 2w + 3 inter): the kernel's own workspace; z (N, inter), gv (N, w) the inputs -> {name: (ref, bar)}."""
    N = rec.shape[0]
    da, dhp, dh, xh = rec[:, :2 * w], rec[:, 2 * w:2 * w + inter], rec[:, 2 * w + inter:2 * w + 2 * inter], rec[:, 2 * w + 2 * inter:]
    gn = gs(N)
    return dict(fc2_w=(da.t() @ z, gn * (da.abs().t() @ z.abs())), fc2_b=(da.sum(0), gn * da.abs().sum(0)),
                fc1_w=(dh.t() @ gv, gn * (dh.abs().t() @ gv.abs())), fc1_b=(dh.sum(0), gn * dh.abs().sum(0)),
                bn_w=((dhp * xh).sum(0), gn * (dhp * xh).abs().sum(0)), bn_b=(dhp.sum(0), gn * dhp.abs().sum(0)))


# ---- apply_bwd ---------------------------------------------------------------------------------------------------
def du_ref(dout, u, att, dg, pool):
    """-> (du, bar, keep) (N, HW, 2w)."""
    N, H, W, w2 = u.shape
    w, HW = w2 // 2, H * W
    dv, bdv, _, _ = dv_ref(dout, H, W, pool)
    a = att.reshape(N, 1, w2)
    dv2, bdv2 = torch.cat([dv, dv], 2), torch.cat([bdv, bdv], 2)
    gm = torch.cat([dg, dg], 1).view(N, 1, w2) / HW
    keep = u.reshape(N, HW, w2) > 0
    t = a * dv2 + gm
    bar = a.abs() * bdv2 + g(4) * ((a * dv2).abs() + gm.abs()) + g(4) * gm.abs()
    zero = torch.zeros_like(t)
    return torch.where(keep, t, zero), torch.where(keep, bar, zero), keep


def du_partial_ref(du, w):
    """du (N, HW, 2w): the kernel's own output -> (ref, bar) (N, K, 2w)."""
    return _chunk_sum(du, w), gs(_chunk_n(du.shape[1], w, du.device)) * _chunk_sum(du.abs(), w)


def positive_zero(t):
    """Every element is bit +0.0."""
    return bool((t.contiguous().view(torch.int32) == 0).all())
