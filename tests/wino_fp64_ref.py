"""fp64 reference of the fused Winograd F(2x2, 3x3) forward kernels (csrc/conv_wino.hip: kind '64', 16 x 16 pixel regions, 8-channel
chunks; csrc/conv_wino32.hip: kind '32', 8 x 16 regions, 4-channel chunks), the per-element bars they must meet, and their launch
rules restated.  The counterpart of tests/conv_fp64_ref.py, whose reference, constants, ``ratio`` / ``check`` and slot formulas are reused.

Reference.  The fp64 DIRECT 3x3 / pad 1 convolution of the operands as the kernel reads them (conv_fp64_ref.reference at chosen
pixels: input affine ``relu?(x a[n, c] + b[n, c])`` on real pixels only, padding 0 after the affine, then ``* scale[c]``, ``+ bias[c]``,
ReLU).  Never an fp64 Winograd: a wrong transform would be wrong on both sides.

Bars (per output element; ``got`` passes where ``|got - ref| <= bar``; u = 2^-24 = U32):

1. The Winograd bound.  ``Y = A^T [ sum_c (G g G^T) (.) (B^T d B) ] A`` per 4 x 4 patch d -> 2 x 2 outputs.  The magnitude goes through
   the algorithm with absolute coefficients,
       ``mag_wino = |A|^T [ sum_c (|G| |g| |G|^T) (.) (|B|^T |d| |B|) ] |A|``,
   ``|d|`` the post-affine magnitude ``|x a| + |b|`` under a fused affine (the fp32 products the kernel rounds), padding and the pixels
   right of / below the map zero as the kernel fills them.  Roundings to first order, each relative to that magnitude:
   the weight pass G g G^T = two additions per pass (the halvings are exact) = 4u; B^T d B = one addition per entry and pass = 2u (a row
   of B^T has two non-zeros; counted as two additions per pass it is 4u), the fused affine's fma +1u on ``|d|``; the product 1u; the two
   three-term passes of A^T M A = two additions each = 4u: 12u counted (14u with the generous count), and the chain over Cin errs like
   the direct kernel's K chain, about 1u of ``sum |V U|`` for products of either sign (only a worst-case bound grows with Cin).
   ``ACC_REL = 16u`` covers it: the bar is ``ACC_REL * mag_wino`` through the epilogue (``* |scale|``), plus ``ULP32 * |t|`` of the
   intermediate each rounded epilogue operation produces -- the form tests/wgrad_fp64_ref.py uses for the Winograd weight gradient.
   Asserted on EVERY case.
2. The direct bar of conv_fp64_ref, ``ACC_REL * sum_k |x_k w_k|`` (+ the same epilogue terms): what every other forward instance meets.
   It is no worst-case bound for Winograd (``mag_wino`` is 6 .. 15x the direct magnitude), so it is asserted on the zero-mean cases
   without a fused affine, and a case is ELIGIBLE only if an fp32 emulation of F(2x2, 3x3) on its own operands (``emulate``: the
   transforms in fp32, one sequential chain over 8- or 4-channel chunks) stays at or below ``EMU_SHARE = 0.25`` of it -- the host test
   checks that for every such case; the GPU gets the remaining factor 4 for its other accumulation order.
3. Statistics slots: conv_fp64_ref's slot bars (sum and sum of squares, see its docstring) over the pixels of ONE region that lie inside
   the map, with ``e_p`` taken from bar 1.

Sampling takes WHOLE regions (``sample``): a persistent-loop fault hits the tiles of one workgroup's run, not scattered pixels.
"""
import numpy as np
import torch

from tests import conv_fp64_ref as R
from tests.conv_fp64_ref import ACC_REL, ULP32, U32, check, ratio      # noqa: F401  (the tests take them from here)
from tests.wgrad_fp64_ref import AM, BT, GM      # A (4 x 2), B^T (4 x 4), G (4 x 3): the same F(2x2, 3x3) as the weight gradient's

EMU_SHARE = 0.25          # bar 2 eligibility: the fp32 emulation's share of the direct bar
ALL_PIXELS = 6000         # maps up to this many pixels are checked whole

# ---- the launch rules of the two kernels, restated (tests/test_wino_instances_host.py finds each constant in the source text) ------
REGION = {'64': (16, 16), '32': (8, 16)}      # output pixels (rows, columns) of one region = one GEMM M tile
CHUNK = {'64': 8, '32': 4}                    # input channels per K chunk
XFMAX = {'64': 512, '32': 256}                # widest fused affine table
WG_PER_CU = {'64': 1, '32': 2}                # resident workgroups per CU = the grid cap in units of roundup8(CUs)
COUT_TILE = 64


def _cdiv(a, b):
    return (a + b - 1) // b


def regions(H, W, kind):
    """(RY, RX) regions per image."""
    return _cdiv(H, REGION[kind][0]), _cdiv(W, REGION[kind][1])


def tiles(N, H, W, Cout, kind):
    RY, RX = regions(H, W, kind)
    return N * RY * RX * (Cout // COUT_TILE)


def grid_size(T, kind, ncu):
    return min(_cdiv(T, 8) * 8, WG_PER_CU[kind] * (_cdiv(ncu, 8) * 8))


def run_tiles(T, kind, ncu):
    """The tile walk of a launch of T tiles: (tile, live, has), each (steps, grid): workgroup b visits the virtual ids vb = b + step * grid,
    tile = (vb & 7) * per + (vb >> 3) with per = ceil(T / 8), grid = min(roundup8(T), ncu | 2 ncu); ``has``: the id has a tile
    (vb < 8 per and tile < T); a run ends at its first id without one, so ``live`` is the running AND of ``has`` down a column."""
    per = (T + 7) >> 3
    grid = grid_size(T, kind, ncu)
    steps = _cdiv(per * 8, grid) + 1
    vb = np.arange(grid)[None, :] + grid * np.arange(steps)[:, None]
    tile = (vb & 7) * per + (vb >> 3)
    has = (vb < per * 8) & (tile < T)
    return tile, np.logical_and.accumulate(has, axis=0), has


def walk(N, H, W, Cout, kind, ncu):
    """Every workgroup's run as a list of (tile, region, image, cout tile), cout tiles fastest within a region (``run_tiles``)."""
    RY, RX = regions(H, W, kind)
    tn = Cout // COUT_TILE
    tile, live, _ = run_tiles(N * RY * RX * tn, kind, ncu)
    return [[(int(t), int(t) // tn, int(t) // tn // (RY * RX), int(t) % tn) for t in tile[live[:, b], b]] for b in range(tile.shape[1])]


def run_kinds(runs):
    """What the runs of one launch reach: lengths, and whether some pair of consecutive tiles changes / keeps the image."""
    lens = {len(r) for r in runs}
    change = any(a[2] != b[2] for r in runs for a, b in zip(r, r[1:]))
    stay = any(a[2] == b[2] for r in runs for a, b in zip(r, r[1:]))
    return dict(lens=lens, change=change, stay=stay)


def u_index(kind, Cin, co, ci, f):
    """Float offset of U[f = 4i + j][ci][co] in the image wino_pack_kernel ('64') / wino32_pack_kernel ('32') writes (numpy arrays or ints).
    '64': [cout tile][chunk of 8][f][cout 64][slot], slot = 4 * ((k >> 2) ^ ((cout >> 3) & 1)) + (k & 3); '32': [cout tile][chunk of 4][f][cout 64][k]."""
    tn, cl = co >> 6, co & 63
    if kind == '64':
        chunk, k, nch = ci >> 3, ci & 7, Cin >> 3
        return ((tn * nch + chunk) * 16 + f) * 512 + cl * 8 + 4 * ((k >> 2) ^ ((cl >> 3) & 1)) + (k & 3)
    chunk, k, nch = ci >> 2, ci & 3, Cin >> 2
    return ((tn * nch + chunk) * 16 + f) * 256 + cl * 4 + k


def u_layout(kind, Cin, Cout):
    """(16, Cin, Cout) int64 offsets of the whole image."""
    f, ci, co = np.meshgrid(np.arange(16), np.arange(Cin), np.arange(Cout), indexing='ij')
    return u_index(kind, Cin, co, ci, f).astype(np.int64)


# ---- regions and sampling -----------------------------------------------------------------------------------------------------------
def region_pixels(rg, N, H, W, kind):
    """Flat output pixels (n * H + oy) * W + ox of region rg that lie inside the map, row-major."""
    RY, RX = regions(H, W, kind)
    rh, rw = REGION[kind]
    n, rem = divmod(rg, RY * RX)
    ry, rx = divmod(rem, RX)
    oy = np.arange(ry * rh, min(ry * rh + rh, H))
    ox = np.arange(rx * rw, min(rx * rw + rw, W))
    return ((n * H + oy[:, None]) * W + ox[None, :]).reshape(-1).astype(np.int64)


def partial_regions(n, H, W, kind):
    """Regions of image n cut by the right or the bottom edge of the map."""
    RY, RX = regions(H, W, kind)
    rh, rw = REGION[kind]
    return [(n * RY + ry) * RX + rx for ry in range(RY) for rx in range(RX)
            if (ry == RY - 1 and H % rh) or (rx == RX - 1 and W % rw)]


def pick_runs(runs):
    """Three runs of a launch: the first whose consecutive tiles change image, the first with two consecutive tiles in one image, the
    first of the longest ones (fewer where the launch has none)."""
    picked = []
    for want in ('change', 'stay'):
        for r in runs:
            pairs = list(zip(r, r[1:]))
            if any((a[2] != b[2]) == (want == 'change') for a, b in pairs):
                picked.append(r)
                break
    longest = max(len(r) for r in runs)
    picked.append(next(r for r in runs if len(r) == longest))
    return picked


def sample(N, H, W, Cout, kind, ncu, n_random=300, seed=0):
    """(sorted int64 pixels, whole regions among them).  Small maps: every pixel, every region.  Else whole regions -- the first and last
    region of the first and last image, every partial region of one image, all regions of three workgroups' runs (``pick_runs``) -- and
    ``n_random`` random pixels."""
    RY, RX = regions(H, W, kind)
    P, M = RY * RX, N * H * W
    if M <= ALL_PIXELS:
        return np.arange(M, dtype=np.int64), list(range(N * P))
    rgs = {0, P - 1, (N - 1) * P, N * P - 1}
    rgs.update(partial_regions(min(1, N - 1), H, W, kind))
    for r in pick_runs(walk(N, H, W, Cout, kind, ncu)):
        rgs.update(t[1] for t in r)
    rgs = sorted(rgs)
    rng = np.random.default_rng(seed)
    parts = [region_pixels(rg, N, H, W, kind) for rg in rgs] + [rng.integers(0, M, size=n_random)]
    return np.unique(np.concatenate(parts).astype(np.int64)), rgs


# ---- F(2x2, 3x3) on the 2 x 2 tiles of chosen pixels --------------------------------------------------------------------------------
def tiles_of(m, H, W):
    """The distinct Winograd tiles (n, oy >> 1, ox >> 1) of pixels m as flat keys, and per pixel (its tile's index, row, column in it).
    Regions start at even coordinates, so the kernels' tiles are the global even-aligned 2 x 2 blocks."""
    m = np.asarray(m)
    n, rem = m // (H * W), m % (H * W)
    oy, ox = rem // W, rem % W
    TY, TX = (H + 1) // 2, (W + 1) // 2
    key, inv = np.unique((n * TY + oy // 2) * TX + ox // 2, return_inverse=True)
    return key, inv, oy & 1, ox & 1


def patches(x, key, in_ab=None, in_relu=False, dtype=torch.float64, magnitude=False, pad_relu_b=False, table_shift=0):
    """(T, 4, 4, Cin) input patches of tiles ``key`` of the NHWC map x (any device), after the fused affine, zero outside the map.
    magnitude: ``|x a| + |b|`` (``|x|`` without an affine).  The two mutants of the host test: pad_relu_b fills the outside with relu?(b)
    instead of 0; table_shift reads the (a, b) rows of image n - table_shift."""
    N, H, W, Cin = x.shape
    TY, TX = (H + 1) // 2, (W + 1) // 2
    t = torch.as_tensor(np.asarray(key), device=x.device)
    n, ty, tx = t // (TY * TX), t % (TY * TX) // TX, t % TX
    iy = (2 * ty - 1).view(-1, 1, 1) + torch.arange(4, device=x.device).view(1, 4, 1)
    ix = (2 * tx - 1).view(-1, 1, 1) + torch.arange(4, device=x.device).view(1, 1, 4)
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    g = x[n.view(-1, 1, 1).expand_as(ok), iy.clamp(0, H - 1), ix.clamp(0, W - 1)].cpu().to(dtype)
    ok = ok.cpu().unsqueeze(-1)
    fill = torch.zeros((), dtype=dtype)
    if in_ab is not None:
        rows = (n.cpu() - table_shift) % N
        a, b = (v.detach().cpu().to(dtype)[rows].view(-1, 1, 1, Cin) for v in in_ab)
        if magnitude:
            g = (g * a).abs() + b.abs()
        else:
            g = g * a + b
            if in_relu:
                g = g.clamp_min(0)
            if pad_relu_b:
                fill = (b.clamp_min(0) if in_relu else b).expand_as(g)
    elif magnitude:
        g = g.abs()
    return torch.where(ok, g, fill)


def weight_images(w, gm=GM, dtype=torch.float64):
    """U (16, Cin, Cout) = G g G^T of w (Cout, Cin, 3, 3), f = 4i + j."""
    gm = gm.to(dtype)
    Cout, Cin = w.shape[:2]
    return torch.einsum('ik,ockl,jl->ijco', gm, w.detach().cpu().to(dtype), gm).reshape(16, Cin, Cout)


def winograd(d, U, bt=BT, am=AM, chunk=None):
    """Y (T, 2, 2, Cout) = A^T [ sum_c U (.) (B^T d B) ] A of patches d (T, 4, 4, Cin) and weight images U (16, Cin, Cout), in their
    dtype.  chunk: the sum over Cin as ONE sequential chain over chunks of that many channels (the kernels' K loop)."""
    dt = d.dtype
    bt, am = bt.to(dt), am.to(dt)
    T, Cin = d.shape[0], d.shape[-1]
    V = torch.einsum('ar,trsc,bs->abtc', bt, d, bt).reshape(16, T, Cin)
    if chunk is None:
        M = torch.bmm(V, U)
    else:
        M = torch.zeros((16, T, U.shape[-1]), dtype=dt)
        for c0 in range(0, Cin, chunk):
            M = M + torch.bmm(V[:, :, c0:c0 + chunk], U[:, c0:c0 + chunk])
    return torch.einsum('ia,jb,ijto->tabo', am, am, M.view(4, 4, T, -1))


def magnitude(x, w, m, in_ab=None, block=2048):
    """``mag_wino`` (len(m), Cout) fp64 at pixels m (module docstring)."""
    R._threads()
    N, H, W, Cin = x.shape
    key, inv, py, px = tiles_of(m, H, W)
    U = weight_images(w.detach().abs(), GM.abs())
    Y = torch.cat([winograd(patches(x, key[i:i + block], in_ab, magnitude=True), U, BT.abs(), AM.abs())
                   for i in range(0, len(key), block)])
    return Y[torch.as_tensor(inv), torch.as_tensor(py), torch.as_tensor(px)]


def emulate(x, w, m, in_ab=None, in_relu=False, kind='64', scale=None, bias=None, relu=False, dtype=torch.float32, block=2048, **mut):
    """fp32 emulation of the kernels at pixels m -> (len(m), Cout): the transforms and the epilogue in fp32, one sequential chain over
    the kind's chunks.  ``mut`` (the host test's mutants): gm, u_hook (U -> U), d_hook (patches, tile keys -> patches), and the
    ``patches`` mutants pad_relu_b / table_shift."""
    R._threads()
    N, H, W, Cin = x.shape
    key, inv, py, px = tiles_of(m, H, W)
    U = weight_images(w, mut.get('gm', GM), dtype)
    if mut.get('u_hook'):
        U = mut['u_hook'](U)
    ys = []
    for i in range(0, len(key), block):
        d = patches(x, key[i:i + block], in_ab, in_relu, dtype, pad_relu_b=mut.get('pad_relu_b', False),
                    table_shift=mut.get('table_shift', 0))
        if mut.get('d_hook'):
            d = mut['d_hook'](d, key[i:i + block])
        ys.append(winograd(d, U, chunk=CHUNK[kind]))
    y = torch.cat(ys)[torch.as_tensor(inv), torch.as_tensor(py), torch.as_tensor(px)]
    if scale is not None:
        y = y * scale.detach().cpu().to(dtype).view(1, -1)
    if bias is not None:
        y = y + bias.detach().cpu().to(dtype).view(1, -1)
    return y.clamp_min(0) if relu else y


# ---- the reference and its bars -----------------------------------------------------------------------------------------------------
def _epilogue(t, bar, scale, bias, relu):
    """``t * scale + bias`` (ReLU) in fp64 and the bar through it, as conv_fp64_ref.reference does it."""
    sc, bi = R._vec(scale), R._vec(bias)
    if sc is not None:
        t = t * sc
        bar = bar * sc.abs() + ULP32 * t.abs()
    if bi is not None:
        t = t + bi
        bar = bar + ULP32 * t.abs()
    if relu:
        t = t.clamp_min(0)
    return t, bar


def reference(x, w, m, scale=None, bias=None, relu=False, in_ab=None, in_relu=False, block=4096):
    """fp64 direct convolution at flat output pixels m of NHWC x (N, H, W, Cin), w (Cout, Cin, 3, 3):
    dict(ref, bar_wino = bar 1, bar_direct = bar 2, mag_wino, mag_direct), each (len(m), Cout) fp64."""
    m = np.asarray(m)
    raw = [R.reference(x, w, 1, 1, m[i:i + block], in_ab=in_ab, in_relu=in_relu) for i in range(0, len(m), block)]
    t = torch.cat([r['ref'] for r in raw])
    bar_d = torch.cat([r['bar32'] for r in raw])      # ACC_REL * sum |x w|: no epilogue was passed
    mag_w = magnitude(x, w, m, in_ab)
    ref, bar_w = _epilogue(t, ACC_REL * mag_w, scale, bias, relu)
    _, bar_d2 = _epilogue(t, bar_d, scale, bias, relu)
    return dict(ref=ref, bar_wino=bar_w, bar_direct=bar_d2, mag_wino=mag_w, mag_direct=bar_d / ACC_REL)


def _region_rows(m, rgs, N, H, W, kind):
    """Per region of ``rgs``: the rows of its pixels inside the map among the sampled pixels m."""
    pos = {int(p): i for i, p in enumerate(np.asarray(m))}
    return [torch.as_tensor([pos[int(p)] for p in region_pixels(rg, N, H, W, kind)]) for rg in rgs]


def slot_sums(v, m, rgs, N, H, W, kind):
    """(len(rgs), C, 2) sums and sums of squares of the rows of v (len(m), C) over each region's pixels inside the map."""
    return torch.stack([torch.stack([v[i].sum(0), (v[i] * v[i]).sum(0)], -1) for i in _region_rows(m, rgs, N, H, W, kind)])


def slot_refs(r, m, rgs, N, H, W, kind):
    """fp64 (sum, sumsq) per channel of each whole region of ``rgs`` and their bars: conv_fp64_ref.group_refs over the region's pixels
    inside the map, e_p = bar 1.  Returns (ref (len(rgs), C, 2), bar (len(rgs), C, 2))."""
    return R.group_refs(r['ref'], r['bar_wino'], _region_rows(m, rgs, N, H, W, kind))


def pack_reference(w):
    """fp64 U (16, Cin, Cout) of w and the bar of the pack kernels: each pass is ``0.5 * (p + q + r)`` = two rounded additions and an
    exact halving (rows 0 and 3 are copies), so the value errs by at most ``((1 + g2)^2 - 1) * |G| |g| |G|^T`` with g2 = 2u / (1 - 2u)."""
    g2 = 2 * U32 / (1 - 2 * U32)
    return weight_images(w), ((1 + g2) ** 2 - 1) * weight_images(w.detach().abs(), GM.abs())
