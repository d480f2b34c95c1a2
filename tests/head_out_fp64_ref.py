"""fp64 references of the small-J head output kernels -- ``logit_project_kernel<J, KC>`` (csrc/project.hip), the taps / dgrad / wgrad /
finalize kernels of csrc/p2p_out_bf16.hip and ``tap_sum3x3_kernel`` (csrc/postproc.hip) -- stage by stage, and the bars a HIP kernel
must meet, every bar derived by counting the roundings the kernel performs.  Pure torch, fp64, on CPU or device tensors.

Every stage is judged on the operands THAT STAGE read: the tap responses, the per-range partials and the bias partials are read back
from the workspaces and fed to the reference of the launch that consumes them.  u = U32 = 2^-24, ULP32 = 2 u, g(n) = n u / (1 - n u)
the bound on n chained roundings (tests/stream_fp64_ref.py); ``got`` passes where ``|got - ref| <= bar`` (conv_fp64_ref.ratio).  Every
source-level operation counts as one rounding (contraction only removes roundings).  Sums get ``g(n) * sum |terms|``; a result of at
most four roundings gets one WHOLE ulp per rounding, ``g(2 n)`` (``gs`` below, the rule of the BatchNorm and split-attention pins).
No bar is measured on a GPU; tests/test_head_out_instances_host.py holds float32 emulations of every kernel below half of each.

Launch rules, restated (tests/test_head_out_instances_host.py ties each to the source text or the library):
  logit_project  16 lanes per pixel, lane q owns channels 4q + 64k + {0..3}, k < KC = Cin / 64; blocks = min(ceil(npix / 16), 256 * 7)
                 of 256 threads, so blocks * 16 pixel slots in a grid-stride walk; the ReLU applies only when an affine is given.
  p2p_out fwd    one thread per pixel, blocks of 256; taps R[p][t * J + j], t = kh * 3 + kw; then tap_sum3x3.
  p2p_out dgrad  ppw = 16 pixels per wave; KW = Cin / 64 and G = 1 for J <= 4, KW = 1 and G = Cin / 64 for J > 4; block b serves channel
                 group b % G of pixel range b / G.
  p2p_out wgrad  G as above; R = min(2048 / G, ceil(npix / 64)) ranges of ppw = ceil(npix / R) pixels (range r = pixels [r ppw,
                 min((r + 1) ppw, npix)), EMPTY where r ppw >= npix: written as zeros); workspace ws[r][c][t][j], then wsb[r][j] at
                 offset R Cin 9 J: R (Cin 9 J + J) floats; a, b are reloaded where the image index changes inside a range; finalize
                 sums the ranges ascending.
  tap_sum3x3     taps added with kh then kw ascending, out-of-map taps skipped, then the bias (0.f when null).

Bars (act = relu?(a x + b), bar_act its bar; mag sums use |act| + bar_act):
  activation     p2p_out: ``fmaxf(fmaf(a, x, b), 0.f)``, n = 1.  logit_project: ``xv * a4 + b4`` is a product and a sum in the source, so
                 n = 2 there (the issue's starting count of one fma holds only if the compiler contracts it).  gs(n) (|a x| + |b|).
                 relu is 1-Lipschitz, no element is excluded; where the fp64 pre-activation y is negative the bar shrinks to
                 max(y + bar, 0): an activation the reference clips by more than its bar must contribute exactly 0.  The activation is
                 never stored, so this bar is applied through the stages that read it.
  logit_project  n = 4 KC + 4 + 1 (the lane's fma chain, four xor-shuffle additions, the bias) on sum |w| |act| + |bias|, plus
                 sum |w| bar_act.
  taps           n = Cin (one serial fma chain per (t, j)) on sum |act| |w|, plus sum |w| bar_act.
  tap_sum        from the kernel's OWN taps: n = in-map taps + 1 on sum |R| + |bias|.
  forward e2e    against fp64 conv2d: the tap bars summed over the in-map taps + gs(taps + 1) (sum (|R| + bar_R) + |bias|).
  dgrad          n = 9 J (one fma chain, t then j ascending; out-of-map rows are zeros) on sum |dout| |w|.  The bf16 output must be
                 the round-to-nearest-even of the fp32 output bit for bit (both are run).
  wgrad partial  n = pixels of the range on sum |act| |dout|, plus sum bar_act |dout|; an empty range: bit +0.0.
  bias partial   n = pixels of the range on sum |dout|.
  finalize       from the kernel's OWN partials: n = R - 1 (R = 1: exact).
  gw / gb e2e    against fp64 conv2d autograd: the partial bars summed + gs(R - 1) sum (|partial| + bar).
"""
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import U32, ULP32, bf16_half_ulp, check, ratio  # noqa: F401  (re-exported)
from tests.stream_fp64_ref import g  # noqa: F401  (re-exported)

CINS = (64, 128, 192, 256)
JS = tuple(range(1, 9))
PROJ_LANES, PROJ_THREADS, PROJ_BLOCK_CAP = 16, 256, 256 * 7
FWD_THREADS = 256
DGRAD_PPW = 16
WGRAD_WAVES, WGRAD_MIN_PIX = 2048, 64
ERR_ARG, ERR_UNSUPPORTED = -1001, -1002


# ---- integer rules ---------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def gs(n):
    """The bound of a sum of n roundings: g(n), and one whole ulp per rounding, g(2 n), where n <= 4 (n a number or a tensor)."""
    n = torch.as_tensor(n, dtype=torch.float64)
    return g(torch.where(n <= 4, 2 * n, n))


def proj_channels(q, KC):
    """The channels lane q of a pixel's 16 lanes owns, in the order its fma chain takes them."""
    return [4 * q + 64 * k + i for k in range(KC) for i in range(4)]


def proj_blocks(npix):
    return min(cdiv(npix, PROJ_LANES), PROJ_BLOCK_CAP)


def proj_slots(npix):
    return proj_blocks(npix) * (PROJ_THREADS // PROJ_LANES)


def proj_passes(npix):
    """Trips of the grid-stride loop on the busiest slot."""
    return cdiv(npix, proj_slots(npix))


def proj_n(Cin):
    return 4 * (Cin // 64) + 4 + 1


def fwd_blocks(npix):
    return cdiv(npix, FWD_THREADS)


def groups(Cin, J):
    """(KW, G): 64-channel blocks per wave and waves per pixel range, for the dgrad and the wgrad kernel alike."""
    return (Cin // 64, 1) if J <= 4 else (1, Cin // 64)


def dgrad_grid(npix, Cin, J):
    return cdiv(npix, DGRAD_PPW) * groups(Cin, J)[1]


def wgrad_plan(npix, Cin, J):
    """(G, R, ppw)."""
    G = groups(Cin, J)[1]
    R = min(WGRAD_WAVES // G, cdiv(npix, WGRAD_MIN_PIX))
    return G, R, cdiv(npix, R)


def wgrad_ws(npix, Cin, J):
    return wgrad_plan(npix, Cin, J)[1] * (Cin * 9 * J + J)


def wgrad_ranges(npix, Cin, J):
    """[(p0, pend)] of every range; pend <= p0 marks an empty one."""
    _, R, ppw = wgrad_plan(npix, Cin, J)
    return [(r * ppw, min((r + 1) * ppw, npix)) for r in range(R)]


def empty_ranges(npix, Cin, J):
    return sum(1 for p0, p1 in wgrad_ranges(npix, Cin, J) if p1 <= p0)


def straddling_ranges(npix, HW, Cin, J):
    """Ranges that hold pixels of more than one image (the a / b reload inside a range)."""
    return sum(1 for p0, p1 in wgrad_ranges(npix, Cin, J) if p1 > p0 and p0 // HW != (p1 - 1) // HW)


# ---- operand layouts ---------------------------------------------------------------------------------------------
def w9(w):
    """w (J, Cin, 3, 3) -> (9 J, Cin), row t * J + j = w[j, :, kh, kw]: the taps / dgrad / wgrad operand order."""
    J, C = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(9 * J, C)


def shifted_dout(dout):
    """dout (N, H, W, J) -> (N, H, W, 9 J): [t * J + j] = dout[n, y - kh + 1, x - kw + 1, j], 0 outside the map (``load_taps``)."""
    N, H, W, J = dout.shape
    dp = F.pad(dout, (0, 0, 1, 1, 1, 1))
    return torch.cat([dp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W] for kh in range(3) for kw in range(3)], 3)


def _gather_taps(R, J):
    """R (N, H, W, 9 J) -> (N, H, W, J): sum over (kh, kw) of R[n, y + kh - 1, x + kw - 1, t * J + j], 0 outside the map."""
    N, H, W, _ = R.shape
    Rp = F.pad(R, (0, 0, 1, 1, 1, 1))
    return sum(Rp[:, kh:kh + H, kw:kw + W, (kh * 3 + kw) * J:(kh * 3 + kw + 1) * J] for kh in range(3) for kw in range(3))


def in_map_taps(H, W, device=None):
    """(1, H, W, 1): how many of a pixel's nine taps lie inside the map."""
    ones = torch.ones((1, H, W, 9), dtype=torch.float64, device=device)
    return _gather_taps(ones, 1)


# ---- activation --------------------------------------------------------------------------------------------------
def act_ref(x, a, b, relu=True, n=1):
    """x (N, H, W, C), a / b (N, C) fp64 -> (act, bar); a None: the map as it is, exact."""
    if a is None:
        return x, torch.zeros_like(x)
    t = a[:, None, None, :] * x
    y = t + b[:, None, None, :]
    bar = gs(n) * (t.abs() + b.abs()[:, None, None, :])
    if not relu:
        return y, bar
    return y.clamp_min(0), torch.where(y < 0, (y + bar).clamp_min(0), bar)


# ---- logit_project -----------------------------------------------------------------------------------------------
def project_ref(x, w, bias, a=None, b=None, in_relu=True):
    """x (N, H, W, Cin), w (J, Cin), bias (J) fp64 -> (ref, bar) (N, H, W, J).  The ReLU belongs to the affine."""
    act, ba = act_ref(x, a, b, relu=bool(in_relu), n=2)
    ref = act @ w.t() + bias
    mag = (act.abs() + ba) @ w.abs().t() + bias.abs()
    return ref, g(proj_n(x.shape[-1])) * mag + ba @ w.abs().t()


# ---- p2p_out forward ---------------------------------------------------------------------------------------------
def taps_ref(act, bar_act, w):
    """act (N, H, W, Cin), w (J, Cin, 3, 3) fp64 -> (ref, bar) (N, H, W, 9 J)."""
    m = w9(w)
    return act @ m.t(), g(act.shape[-1]) * ((act.abs() + bar_act) @ m.abs().t()) + bar_act @ m.abs().t()


def tap_sum_ref(R, bias, J, bar_R=None):
    """R (N, H, W, 9 J) fp64, the kernel's own taps (bar_R None) or the taps reference with its bar; bias (J) or None."""
    N, H, W, _ = R.shape
    bz = torch.zeros(J, dtype=R.dtype, device=R.device) if bias is None else bias
    ref = _gather_taps(R, J) + bz
    mag = _gather_taps(R.abs() if bar_R is None else R.abs() + bar_R, J) + bz.abs()
    bar = gs(in_map_taps(H, W, R.device) + 1) * mag
    if bar_R is not None:
        bar = bar + _gather_taps(bar_R, J)
    return ref, bar


def conv_ref(act, w, bias):
    """fp64 conv2d of the NHWC activation, on the CPU: (N, H, W, J)."""
    return F.conv2d(act.cpu().permute(0, 3, 1, 2), w.cpu(), bias.cpu(), padding=1).permute(0, 2, 3, 1)


def conv_grads_ref(act, w, dout):
    """fp64 autograd of conv2d on the CPU: (dact (N, H, W, Cin), gw (J, Cin, 3, 3), gb (J))."""
    a = act.cpu().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wd = w.cpu().clone().requires_grad_(True)
    bd = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(a, wd, bd, padding=1).backward(dout.cpu().permute(0, 3, 1, 2))
    return a.grad.permute(0, 2, 3, 1), wd.grad, bd.grad


# ---- p2p_out dgrad -----------------------------------------------------------------------------------------------
def dgrad_ref(dout, w):
    """dout (N, H, W, J) (the live channels), w (J, Cin, 3, 3) fp64 -> (ref, bar) (N, H, W, Cin)."""
    d, m = shifted_dout(dout), w9(w)
    return d @ m, gs(9 * w.shape[0]) * (d.abs() @ m.abs())


def bf16_rne(t):
    """The round-to-nearest-even bf16 of an fp32 tensor (torch's conversion)."""
    return t.to(torch.bfloat16)


# ---- p2p_out wgrad -----------------------------------------------------------------------------------------------
def _by_range(v, R, ppw):
    """v (npix, K) -> (R, ppw, K), zero rows past npix."""
    npix, K = v.shape
    if R * ppw != npix:
        v = torch.cat([v, v.new_zeros((R * ppw - npix, K))], 0)
    return v.view(R, ppw, K)


def wgrad_partial_ref(act, bar_act, dout, Cin, J):
    """act, bar_act (N, H, W, Cin), dout (N, H, W, J) fp64 -> (ws_ref, ws_bar (R, Cin, 9 J), wsb_ref, wsb_bar (R, J), counts (R))."""
    npix = act.shape[0] * act.shape[1] * act.shape[2]
    _, R, ppw = wgrad_plan(npix, Cin, J)
    d = _by_range(shifted_dout(dout).reshape(npix, 9 * J), R, ppw)
    v = _by_range(act.reshape(npix, Cin), R, ppw).transpose(1, 2)
    bv = _by_range(bar_act.reshape(npix, Cin), R, ppw).transpose(1, 2)
    cnt = torch.tensor([max(p1 - p0, 0) for p0, p1 in wgrad_ranges(npix, Cin, J)], dtype=torch.float64, device=act.device)
    gn = gs(cnt).view(R, 1, 1)
    ws_bar = gn * ((v.abs() + bv) @ d.abs()) + bv @ d.abs()
    db = _by_range(dout.reshape(npix, J), R, ppw)
    return v @ d, ws_bar, db.sum(1), gn.view(R, 1) * db.abs().sum(1), cnt


def finalize_ref(ws, wsb):
    """ws (R, Cin, 9, J), wsb (R, J): the kernel's own partials -> (gw (J, Cin, 3, 3), its bar, gb (J), its bar)."""
    R, Cin, _, J = ws.shape
    gn = gs(R - 1)
    to_w = lambda t: t.permute(2, 0, 1).reshape(J, Cin, 3, 3)           # noqa: E731
    return to_w(ws.sum(0)), gn * to_w(ws.abs().sum(0)), wsb.sum(0), gn * wsb.abs().sum(0)


def wgrad_end_to_end_bars(ws_ref, ws_bar, wsb_ref, wsb_bar):
    """The bars of gw (J, Cin, 3, 3) and gb (J) against fp64 autograd: the partial bars pushed through the finalize sum."""
    R, Cin, _ = ws_ref.shape
    J = wsb_ref.shape[1]
    gn = gs(R - 1)
    bw = ws_bar.sum(0) + gn * (ws_ref.abs() + ws_bar).sum(0)
    bb = wsb_bar.sum(0) + gn * (wsb_ref.abs() + wsb_bar).sum(0)
    return bw.view(Cin, 9, J).permute(2, 0, 1).reshape(J, Cin, 3, 3), bb


def positive_zero(t):
    """Every element is bit +0.0."""
    return bool((t.contiguous().view(torch.int32) == 0).all())
