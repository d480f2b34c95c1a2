"""fp64 references of the kernels in front of layer1 on WHOLE maps, and the bars a launch must meet per element: the fused
7x7 / 2 conv + BN + ReLU + max-pool (csrc/stem_f32.hip), the bf16 conv and its pools (csrc/stem_bf16.hip), the three launches of the
deep stem (csrc/stem_deep.hip) and the max-pool + ReLU backward with its column-sum slots (stem_pool_bwd_kernel, csrc/stem_bwd.hip).
Pure torch on the CPU; the constants and ``check`` are those of tests/conv_fp64_ref.py.

Conv value and bar of one output element (``conv_ref``): ``acc = sum x w`` in fp64, ``t = acc * scale + bias``,
    ``e = ACC_REL * |scale| * sum |x| |w| + ULP32 * |acc * scale| + ULP32 * |t|``
(an absent scale or bias drops its term).  The ReLU is 1-Lipschitz: ``relu(t)`` keeps ``e``.

Pooled value and bar (``pool_ref``): ``|max_w a_w - max_w b_w| <= max_w |a_w - b_w|``, so the reference is ``max_w relu(t_w)`` and the bar
``max_w e_w`` over the in-map positions of the 3x3 / 2 / pad 1 window.

bf16 conv outputs: the operands are the ones the kernel reads (``bf16_operands``: the image rounded to bf16 RNE, the weights read back from
ops.stem_weight_bf16); the bar is ``e`` plus half the bf16 grid spacing at ``|ref|``.

Byte map (``check_argmap``), per pooled element with ``E = max_w e_w``: ``out == 0`` needs ``arg == 255`` and ``t_w <= e_w`` on the whole
window; otherwise ``arg`` is an in-map position 0..8, ``t_arg >= max_w t_w - 2 E`` and ``out`` lies within ``e_arg`` of ``relu(t_arg)``.  An
element is DECIDED by the fp64 reference alone when its top two window values differ by more than ``2 E`` and the top one exceeds its own
``e`` (``arg`` must then be the fp64 argmax, first of ties by window order), or when every window value lies below ``-e_w`` (the element must
be 0 / 255).  The share of elements not decided this way is returned; a case admits at most ``UNDECIDED_MAX`` of them.

The byte map of bf16 values is checked exactly instead (``pool_exact``: the first of tied positions, 255 at 0): the pooled bf16 map is the
maximum of the kernel's own bf16 conv map, no rounding in between, and ties are common on the bf16 grid.

Deep stem: launch B is judged against the fp64 conv of the kernel's own mid1, launch C against the fp64 conv + pool of the kernel's own mid2, so no
chain error enters a bar.  Slots of stem_pool_bwd (``slot_refs``): the fp64 sum of the kernel's own dy over pixels
``[SLOT s, min(SLOT s + SLOT, M))`` with bar ``(n - 1) * U32 * sum |dy| + ULP32 * |sum|``.

Everything here is NCHW fp64 (``nchw`` turns a kernel's NHWC map into it)."""
import torch
import torch.nn.functional as F

from tests.conv_fp64_ref import ACC_REL, ULP32, U32, _threads, bf16_half_ulp, check, ratio  # noqa: F401  (re-exported)

UNDECIDED_MAX = 1e-3
SLOT = 1024                                   # conv pixels per column-sum slot of stem_pool_bwd

# ---- restated geometry ------------------------------------------------------------------------------------------------------------
FUSED_TILE = (8, 16)                          # pooled rows x columns of a fused 7x7 tile (f32 and bf16): conv rows r0 = 16 ty - 1, columns c0 = 32 tx - 1
FUSED_PATCH = (39, 72)
CONV_TILE = (16, 32)                          # conv rows x columns of a tile: the bf16 7x7 conv, deep-stem launches A and B
DEEP_C_TILE = (4, 16)                         # pooled rows x columns of a launch-C tile: conv rows r0 = 8 ty - 1, columns c0 = 32 tx - 1


def half(n):
    """Size of a stride-2 map over n: the 7x7 / 2 / pad 3 and 3x3 / 2 / pad 1 convs and the 3x3 / 2 / pad 1 pool."""
    return (n - 1) // 2 + 1


def cdiv(a, b):
    return -(-a // b)


def fused_geom(H, W):
    OH, OW = half(H), half(W)
    PH, PW = half(OH), half(OW)
    return dict(OH=OH, OW=OW, PH=PH, PW=PW, tilesY=cdiv(PH, FUSED_TILE[0]), tilesX=cdiv(PW, FUSED_TILE[1]),
                lastY=PH - (cdiv(PH, FUSED_TILE[0]) - 1) * FUSED_TILE[0], lastX=PW - (cdiv(PW, FUSED_TILE[1]) - 1) * FUSED_TILE[1])


def conv_tiles(OH, OW):
    """Tile rows / columns of a 16 x 32 conv-tile kernel and the rows / columns of its last tiles."""
    ty, tx = cdiv(OH, CONV_TILE[0]), cdiv(OW, CONV_TILE[1])
    return dict(tilesY=ty, tilesX=tx, lastY=OH - (ty - 1) * CONV_TILE[0], lastX=OW - (tx - 1) * CONV_TILE[1])


def deep_geom(H, W):
    OH, OW = half(H), half(W)
    PH, PW = half(OH), half(OW)
    g = dict(OH=OH, OW=OW, PH=PH, PW=PW, ab=conv_tiles(OH, OW))
    ty, tx = cdiv(PH, DEEP_C_TILE[0]), cdiv(PW, DEEP_C_TILE[1])
    g['c'] = dict(tilesY=ty, tilesX=tx, lastY=PH - (ty - 1) * DEEP_C_TILE[0], lastX=PW - (tx - 1) * DEEP_C_TILE[1])
    return g


def slots(N, OH, OW):
    """[(first pixel, pixels)] of the column-sum slots of an (N, OH, OW) conv map."""
    M = N * OH * OW
    return [(s, min(s + SLOT, M) - s) for s in range(0, M, SLOT)]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def fold_recipe(C, g):
    """(scale, bias): scale in [0.5, 1.5) with about 15 % of the channels negated, bias = 0.6 randn - 0.3 -- channels with a clearly
    positive bias, about half of the conv map clipped."""
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.15, -1.0, 1.0)
    bias = torch.randn(C, generator=g) * 0.6 - 0.3
    return scale, bias


def stem7_inputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn((N, 3, H, W), generator=g) * 1.2
    w = torch.randn((64, 3, 7, 7), generator=g) * 0.08
    scale, bias = fold_recipe(64, g)
    return dict(img=img, w=w, scale=scale, bias=bias)


def deep_inputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn((N, 3, H, W), generator=g) * 1.2
    ws = [torch.randn(s, generator=g) * (2.0 / (s[1] * 9)) ** 0.5 for s in ((32, 3, 3, 3), (32, 32, 3, 3), (64, 32, 3, 3))]
    folds = [fold_recipe(s, g) for s in (32, 32, 64)]
    return dict(img=img, w=ws, folds=folds)


def nhwc4(img, fill=0.0):
    """(N, 3, H, W) -> the (N, H, W, 4) input layout, the 4th channel ``fill``."""
    N, _, H, W = img.shape
    x = torch.full((N, H, W, 4), fill, dtype=img.dtype)
    x[..., :3] = img.permute(0, 2, 3, 1)
    return x


def nchw(t):
    """A kernel's NHWC map (any device, fp32 or bf16) -> NCHW fp64 on the CPU, exact."""
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def bf16_operands(img, wpack):
    """What the bf16 7x7 kernels multiply: the image rounded to bf16 (RNE), and (64, 3, 7, 7) from the (64, 224) bf16 weight image
    (k = (kh * 8 + kw) * 4 + c) of ops.stem_weight_bf16."""
    w = wpack.detach().cpu().float().view(64, 7, 8, 4)
    assert not bool(w[:, :, 7].any()) and not bool(w[..., 3].any())
    return img.to(torch.bfloat16).float(), w[:, :, :7, :3].permute(0, 3, 1, 2).contiguous()


# ---- conv and pool references -----------------------------------------------------------------------------------------------------
def _cvec(v):
    return None if v is None else v.detach().cpu().double().view(1, -1, 1, 1)


def conv_ref(x, w, stride, pad, scale=None, bias=None):
    """x (N, Cin, H, W), w (Cout, Cin, KH, KW): the values the kernel reads.  -> (t, e) NCHW fp64: the value before the ReLU and its bar."""
    _threads()
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    acc = F.conv2d(x, w, None, stride, pad)
    e = ACC_REL * F.conv2d(x.abs(), w.abs(), None, stride, pad)
    t = acc
    sc, bi = _cvec(scale), _cvec(bias)
    if sc is not None:
        t = acc * sc
        e = e * sc.abs() + ULP32 * t.abs()
    if bi is not None:
        t = t + bi
        e = e + ULP32 * t.abs()
    return t, e


def windows(t, fill):
    """(N, C, OH, OW) -> (N, C, 9, PH, PW): the 3x3 / 2 / pad 1 windows, position dy * 3 + dx, out-of-map positions ``fill``."""
    N, C, OH, OW = t.shape
    p = F.pad(t, (1, 1, 1, 1), value=fill)
    PH, PW = half(OH), half(OW)
    return torch.stack([p[:, :, dy:dy + 2 * PH - 1:2, dx:dx + 2 * PW - 1:2] for dy in range(3) for dx in range(3)], 2)


def in_map(OH, OW):
    """(9, PH, PW) bool: window position inside the conv map."""
    return windows(torch.ones((1, 1, OH, OW), dtype=torch.float64), 0.0)[0, 0] > 0


def pool_ref(t, e):
    """-> (ref, bar) (N, C, PH, PW): max_w relu(t_w), max_w e_w over the in-map positions."""
    return windows(t.clamp_min(0), 0.0).amax(2), windows(e, 0.0).amax(2)


def first_argmax(w9):
    """Position of the maximum along dim 2, the first of ties by window order."""
    pos = torch.arange(9).view(1, 1, 9, 1, 1)
    return torch.where(w9 == w9.amax(2, keepdim=True), pos, torch.full_like(pos, 9)).amin(2)


def pool_exact(z):
    """The pool and its byte map on an exact ReLU output z (N, C, OH, OW) >= 0: (max, position of the first maximum, 255 where it is 0)."""
    w9 = windows(z, -1.0)
    mx = w9.amax(2)
    return mx, torch.where(mx > 0, first_argmax(w9), torch.full((1,), 255))


def pool_exact_last_of_ties(z):
    """The deliberately wrong twin of pool_exact: the LAST of tied positions."""
    w9 = windows(z, -1.0)
    mx = w9.amax(2)
    return mx, torch.where(mx > 0, 8 - first_argmax(w9.flip(2)), torch.full((1,), 255))


def decide(t, e):
    """What the fp64 reference alone fixes of the byte map.  -> dict(E, top (fp64 argmax), must_pos (arg must be top), must_zero (out
    must be 0 / arg 255), undecided share)."""
    OH, OW = t.shape[2:]
    ok = in_map(OH, OW).view(1, 1, 9, half(OH), half(OW))
    wt, we = windows(t, float('-inf')), windows(e, 0.0)
    E = we.amax(2)
    top2 = wt.topk(2, dim=2).values
    top = first_argmax(wt)
    e_top = we.gather(2, top.unsqueeze(2)).squeeze(2)
    must_pos = (top2[:, :, 0] - top2[:, :, 1] > 2 * E) & (top2[:, :, 0] > e_top)
    must_zero = ((wt < -we) | ~ok).all(2)
    und = ~(must_pos | must_zero)
    return dict(E=E, top=top, must_pos=must_pos, must_zero=must_zero, wt=wt, we=we, ok=ok, undecided=float(und.double().mean()))


def argmap_violations(out, arg, t, e):
    """out (N, C, PH, PW) fp64, arg the same shape (integers), t / e the conv reference (N, C, OH, OW).  -> (bool map of the pooled
    elements that break a rule of the module docstring, the decide() dict)."""
    d = decide(t, e)
    wt, we, ok = d['wt'], d['we'], d['ok']
    arg = arg.long()
    zero = out == 0
    bad_zero = zero & ((arg != 255) | ((wt > we) & ok).any(2))
    a = arg.clamp(0, 8).unsqueeze(2)
    t_arg, e_arg = wt.gather(2, a).squeeze(2), we.gather(2, a).squeeze(2)
    inside = ok.expand_as(wt).gather(2, a).squeeze(2)
    bad_pos = ~zero & ((arg > 8) | ~inside | (t_arg < wt.amax(2) - 2 * d['E']) | ~((out - t_arg.clamp_min(0)).abs() <= e_arg))
    bad_decided = (d['must_pos'] & (arg != d['top'])) | (d['must_zero'] & ~(zero & (arg == 255)))
    return bad_zero | bad_pos | bad_decided, d


def check_argmap(name, out, arg, t, e):
    """Assert the byte-map rules on every pooled element; returns the undecided share."""
    bad, d = argmap_violations(out, arg, t, e)
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        lines = ['n=%d c=%d py=%d px=%d out=%.9g arg=%d fp64 argmax=%d window=%s' % (
            n, c, py, px, float(out[n, c, py, px]), int(arg[n, c, py, px]), int(d['top'][n, c, py, px]),
            ['%.6g' % v for v in d['wt'][n, c, :, py, px].tolist()]) for n, c, py, px in idx[:6].tolist()]
        raise AssertionError('%s: %d/%d byte-map elements break a rule\n  %s' % (name, idx.shape[0], bad.numel(), '\n  '.join(lines)))
    return d['undecided']


def check_map(name, got, ref, bar):
    """conv_fp64_ref.check on whole NCHW maps (rows = pixels, columns = channels); the message names (n, oy, ox)."""
    N, C, H, W = ref.shape
    rows = (lambda v: v.permute(0, 2, 3, 1).reshape(-1, C))
    return check(name, rows(got), rows(ref), rows(bar), OHW=(H, W))


def over_pixels(got, ref, bar):
    """(N, H, W) bool: some channel of the pixel misses the bar."""
    return (ratio(got, ref, bar) > 1.0).any(1)


# ---- column-sum slots of stem_pool_bwd ----------------------------------------------------------------------------------------------
def slot_refs(dy):
    """dy (N, OH, OW, 64) as the kernel wrote it -> (ref, bar) (slots, 64) fp64 of the slot sums."""
    v = dy.detach().cpu().double().reshape(-1, dy.shape[-1])
    refs, bars = [], []
    for s, n in slots(1, v.shape[0], 1):
        blk = v[s:s + n]
        r = blk.sum(0)
        refs.append(r)
        bars.append((n - 1) * U32 * blk.abs().sum(0) + ULP32 * r.abs())
    return torch.stack(refs), torch.stack(bars)


def slot_sums32(dy):
    """The kernel's own order in fp32: 16 pixel lanes each add every 16th pixel of the slot, the 16 lane sums are added in order."""
    v = dy.detach().cpu().float().reshape(-1, dy.shape[-1])
    out = []
    for s, n in slots(1, v.shape[0], 1):
        blk = torch.zeros((SLOT, v.shape[1]))
        blk[:n] = v[s:s + n]
        lanes = blk.view(SLOT // 16, 16, -1)
        cs = torch.zeros((16, v.shape[1]))
        for it in range(SLOT // 16):
            cs = cs + lanes[it]
        tot = torch.zeros(v.shape[1])
        for i in range(16):
            tot = tot + cs[i]
        out.append(tot)
    return torch.stack(out)


# ---- fp32 emulations (the host test: the bars admit an honest fp32 kernel and refuse the wrong ones) ----------------------------------
def conv_emulate(x, w, stride, pad, scale=None, bias=None, relu=True):
    """torch fp32 conv and the kernels' epilogue order: acc * scale + bias, ReLU.  NCHW fp32."""
    _threads()
    y = F.conv2d(x.float(), w.float(), None, stride, pad)
    if scale is not None:
        y = y * scale.float().view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    return y.clamp_min(0) if relu else y


def pool_tiles(z, tile, hook=None):
    """The pooling epilogue of the fused kernels tile by tile on a ReLU output z (N, C, OH, OW): a tile of ``tile`` = (TH, TW) pooled pixels
    holds the (2 TH + 1) x (2 TW + 1) conv positions from (r0, c0) = (2 TH ty - 1, 2 TW tx - 1), out-of-map positions 0; column 0 of the
    tile is the halo column.  hook(ct (N, C, 2 TH + 1, 2 TW + 1), ok (rows, columns) in-map, ty, tx) may change the tile before it is pooled."""
    N, C, OH, OW = z.shape
    TH, TW = tile
    PH, PW = half(OH), half(OW)
    out = torch.zeros((N, C, PH, PW), dtype=z.dtype)
    for ty in range(cdiv(PH, TH)):
        for tx in range(cdiv(PW, TW)):
            r0, c0 = 2 * TH * ty - 1, 2 * TW * tx - 1
            rr, cc = torch.arange(r0, r0 + 2 * TH + 1), torch.arange(c0, c0 + 2 * TW + 1)
            ok = ((rr >= 0) & (rr < OH)).view(-1, 1) & ((cc >= 0) & (cc < OW)).view(1, -1)
            ct = z[:, :, rr.clamp(0, OH - 1)][:, :, :, cc.clamp(0, OW - 1)] * ok
            if hook is not None:
                ct = hook(ct.clone(), ok, ty, tx)
            mx = torch.stack([ct[:, :, dy:dy + 2 * TH - 1:2, dx:dx + 2 * TW - 1:2] for dy in range(3) for dx in range(3)], 2).amax(2).clamp_min(0)
            h, w_ = min(TH, PH - TH * ty), min(TW, PW - TW * tx)
            out[:, :, TH * ty:TH * ty + h, TW * tx:TW * tx + w_] = mx[:, :, :h, :w_]
    return out
