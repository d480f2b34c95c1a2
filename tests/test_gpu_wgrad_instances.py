"""-m gpu: every weight-gradient kernel pinned to the fp64 reference of tests/wgrad_fp64_ref.py, in steady state and at its edges.

One table for the direct fp32 kernel (csrc/conv_wgrad.hip, all eight <XF, GEO> instances), the Winograd weight gradient
(csrc/conv_wino_wgrad.hip, plain and XF), the bf16 rewriting path (csrc/conv_wgrad_bf16.hip, NT), the bf16 pixel-major kernel
(csrc/conv_wgrad_bf16_tn.hip, TN) and stem_wgrad_f32 (csrc/stem_bwd.hip, both input layouts).  The shapes of the older kernel-level
tests are all in it; the new ones are long enough in the pixel axis that the kernels' main loops run in steady state (the direct
kernel's loads issued inside the chunk loop, its pair-unrolled loop and odd tail, the 16-split loop of the bf16 reduce kernel, the
three-deep Winograd staging pipeline), at maps whose image boundaries, ragged ends and empty slabs fall inside those loops.

Every case is launched through the C entry point with a workspace of the size the workspace query reports, filled with NaN, and --
unless it accumulates -- into a NaN-filled gradient (a partial or an entry the kernel forgets to write reads as NaN, not as the
plausible value the caching allocator left there); twice, bit-equal; and checked entry by entry.  tests/test_wgrad_instances_host.py
pins the plan restatements below to the library's workspace queries and asserts what the table must cover."""
import pytest
import torch

from tests import wgrad_fp64_ref as R
from tests.test_gpu_backward import GRAD_CASES
from tests.test_gpu_bf16 import WGRAD_BF16_CASES, WGRAD_TN_CASES

ERR_ARG, ERR_UNSUPPORTED = -1001, -1002


def _cdiv(a, b):
    return (a + b - 1) // b


# flags: xf (fused input affine), relu (its ReLU), acc (accumulate into a random base), ops (also through the ops.* wrapper)
def DIRECT(N, H, W, Cin, Cout, k, s, p, flags, why=''):
    return dict(kind='direct', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p, flags=flags, why=why)


def WINO(N, H, W, Cin, Cout, flags, why=''):
    return dict(kind='wino', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=3, s=1, p=1, flags=flags, why=why)


def NT(N, H, W, Cin, Cout, k, dy_dt, x_dt, flags, why=''):
    """dy_dt / x_dt: 'f32' or 'bf16' -- not both bf16 (that pair is the pixel-major kernel's)."""
    return dict(kind='nt', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=1, p=k // 2, dy_dt=dy_dt, x_dt=x_dt, flags=flags, why=why)


def TN(N, H, W, Cin, Cout, k, s, flags, why=''):
    return dict(kind='tn', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=k // 2, dy_dt='bf16', x_dt='bf16', flags=flags, why=why)


def STEM(N, H, W, layout, flags='', why=''):
    """layout 0: NHWC4 input, 1: the (N, 3, H, W) planes."""
    return dict(kind='stem', N=N, H=H, W=W, Cin=3, Cout=64, k=7, s=2, p=3, layout=layout, flags=flags, why=why)


# Winograd weight-gradient shapes of tests/test_gpu_wino.py::test_wino_wgrad_matches_autograd (N, H, W, Cin, Cout, xf; ReLU on)
WINO_OLD = [(2, 16, 16, 64, 64, False), (1, 20, 40, 128, 64, True), (3, 18, 34, 64, 128, True), (1, 19, 21, 64, 64, True),
            (2, 32, 32, 256, 256, False), (5, 16, 16, 256, 256, True), (7, 24, 40, 128, 128, True)]
# stem shapes of tests/test_gpu_stem_train.py::test_stem_backward_kernels_match_fp64 (N, H, W), each in both layouts
STEM_OLD = [(2, 37, 53), (1, 9, 11), (3, 70, 130), (4, 640, 640)]

OLD_CASES = (
    [DIRECT(N, H, W, Cin, Cout, k, s, p, 'ops' if i == 0 else '', 'test_gpu_backward.GRAD_CASES')
     for i, (N, Cin, H, W, Cout, k, s, p) in enumerate(GRAD_CASES)] +
    [DIRECT(2, 16, 16, 256, 256, 3, 1, 1, 'xf relu', 'test_gpu_backward.test_conv_wgrad_fused_gn_input'),
     DIRECT(2, 16, 16, 256, 256, 3, 1, 1, 'xf', 'test_gpu_backward.test_conv_wgrad_fused_gn_input'),
     DIRECT(2, 12, 10, 64, 128, 1, 1, 0, '', 'test_gpu_backward.test_bn_fold_relu_backward')] +
    [WINO(N, H, W, Cin, Cout, 'xf relu' if xf else '', 'test_gpu_wino.test_wino_wgrad_matches_autograd')
     for N, H, W, Cin, Cout, xf in WINO_OLD] +
    [NT(N, H, W, Cin, Cout, k, 'f32', xdt, '', 'test_gpu_bf16.WGRAD_BF16_CASES') for N, H, W, Cin, Cout, k, xdt in WGRAD_BF16_CASES] +
    [TN(N, H, W, Cin, Cout, k, s, '', 'test_gpu_bf16.WGRAD_TN_CASES') for N, H, W, Cin, Cout, k, s in WGRAD_TN_CASES] +
    [STEM(N, H, W, layout, '', 'test_gpu_stem_train.test_stem_backward_kernels_match_fp64')
     for N, H, W in STEM_OLD for layout in (1, 0)])

NEW_CASES = [
    # ---- direct fp32, <plain, GEO 2> (1x1 / stride 1 / unpadded): linear addresses
    DIRECT(3, 61, 53, 512, 388, 1, 1, 0, '', '64 slabs of 5 chunks (odd: pair loop twice + tail), last slab 4, 3 empty; Cout 388 = 3 * 128 + 4'),
    DIRECT(9, 61, 53, 256, 128, 1, 1, 0, 'acc', '256 slabs of exactly 4 chunks, last slab 2, 28 empty; accumulates'),
    DIRECT(3, 31, 1, 64, 64, 1, 1, 0, '', 'OH * OW = 31: the last GEO -1 size; OW = 1'),
    DIRECT(3, 4, 8, 64, 64, 1, 1, 0, '', 'OH * OW = 32: the first GEO >= 0 size'),
    DIRECT(3, 3, 11, 64, 64, 1, 1, 0, '', 'OH * OW = 33'),
    # ---- <XF, GEO 2>: the 1x1 output convs of the heads, Cout padded to 4
    DIRECT(5, 83, 80, 256, 4, 1, 1, 0, 'xf relu', '256 slabs of 5 chunks, last slab 3, 48 empty; the (a, b) table moves inside slabs'),
    # ---- <plain, GEO 1> ('same' convolutions)
    DIRECT(13, 37, 41, 128, 256, 3, 1, 1, '', '112 slabs of 6 chunks (even), last slab 5, 9 empty; OW = 41 > 32'),
    DIRECT(5, 37, 41, 192, 132, 3, 1, 1, '', '56 slabs of 5 chunks, last slab 3; Cin 192, Cout 132 = 128 + 4'),
    DIRECT(3, 45, 1, 64, 64, 3, 1, 1, '', 'OW = 1: every pixel is a left and a right border'),
    # ---- <XF, GEO 1>: 3x3 convs whose Cout is a padded handful of channels
    DIRECT(17, 33, 31, 256, 4, 3, 1, 1, 'xf relu ops', '112 slabs of 5 chunks, last slab 4, 3 empty; OW = 31 < 32'),
    DIRECT(7, 33, 32, 256, 4, 3, 1, 1, 'xf', 'OW = 32: the column never changes from chunk to chunk (r32 = 0); no ReLU'),
    # ---- <plain, GEO 0> (strided or unpadded)
    DIRECT(14, 75, 67, 128, 256, 3, 2, 1, '', '112 slabs of 6 chunks, last slab 2; stride 2 on odd H and odd W (the bN term)'),
    DIRECT(7, 75, 67, 128, 256, 3, 2, 1, '', '112 slabs of exactly 3 chunks: the odd tail right after one pair'),
    DIRECT(7, 39, 43, 128, 132, 3, 1, 0, '', 'stride-1 unpadded 3x3: GEO 0 without stride'),
    DIRECT(3, 70, 1, 64, 64, 3, 2, 1, '', 'OW = 1 under stride 2'),
    # ---- <XF, GEO 0>
    DIRECT(14, 75, 67, 256, 8, 3, 2, 1, 'xf', '112 slabs of 6 chunks, last slab 2, 17 empty; Cout 8'),
    # ---- <plain, GEO -1> and <XF, GEO -1>: images smaller than a chunk, several image boundaries in every chunk
    DIRECT(301, 5, 6, 256, 256, 3, 1, 1, '', '56 slabs of 6 chunks, last slab 1, 8 empty'),
    DIRECT(481, 5, 6, 256, 8, 3, 1, 1, 'xf relu', '112 slabs of 5 chunks, last slab 1, 21 empty'),
    # ---- Winograd weight gradient
    WINO(3, 45, 50, 192, 192, 'ops', '28 slices of 10 strips (92 per image: slices cross images), last 6; odd H, W % 16 = 2; 192 channels'),
    WINO(7, 33, 47, 128, 128, 'xf relu', '60 slices of 6 strips (51 per image), last 3; odd H, odd W'),
    WINO(6, 63, 64, 64, 192, 'xf', '86 slices of 9 strips (128 per image), last 3; Cin 64; no ReLU'),
    WINO(5, 37, 61, 192, 64, 'acc', '76 slices of 5 strips; accumulates'),
    # ---- bf16 rewriting path (NT): the three operand dtype pairs that reach it, k = 3 and k = 1
    NT(5, 37, 45, 256, 256, 3, 'f32', 'f32', 'ops', '16 splits of 10 chunks, one empty; W + 2 = 47'),
    NT(7, 29, 37, 256, 64, 3, 'f32', 'bf16', 'acc', '16 splits of 9; Cout 64: a quarter of the 256-row tile; accumulates'),
    NT(13, 80, 95, 256, 256, 3, 'bf16', 'f32', '', '112 splits of 16 chunks, 3 empty: the 16-split loop of the reduce kernel seven times'),
    NT(9, 37, 45, 256, 320, 1, 'f32', 'f32', '', '24 splits of 11, one empty; Cout 320'),
    NT(3, 61, 53, 256, 256, 1, 'f32', 'bf16', '', '16 splits of 11, one empty'),
    NT(5, 45, 70, 512, 256, 1, 'bf16', 'f32', '', '24 splits of 11; two cin tiles'),
    # ---- bf16 pixel-major kernel (TN)
    TN(13, 80, 95, 256, 256, 3, 1, '', '56 splits (16-split loop three times + two single steps) of 28 chunks; OW = 95 > 64'),
    TN(5, 61, 53, 128, 256, 3, 1, 'ops', '24 splits of 11 chunks (odd), one empty; Cin 128'),
    TN(7, 61, 53, 192, 320, 1, 1, 'acc', '40 splits of 9; Cin 192, Cout 320: a partial second cout tile; accumulates'),
    TN(40, 7, 9, 192, 128, 3, 1, '', '63-pixel images: every chunk spans images; 8 splits of 5'),
    TN(9, 61, 67, 128, 320, 3, 2, '', 'stride 2 on an odd map (31 x 34 outputs); 16 splits of 10 (even), one empty'),
    TN(3, 61, 53, 256, 256, 1, 1, '', '16 splits of 10'),
    # ---- stem
    STEM(5, 131, 197, 1, 'ops', '100 tiles; OH = 66, OW = 99: ragged tile rows and columns; odd H and W'),
    STEM(5, 131, 197, 0, '', 'the same in NHWC4'),
    STEM(9, 301, 333, 1, '', '540 tiles > 512: the grid-stride loop wraps on ragged tiles'),
    STEM(9, 301, 333, 0, '', 'the same in NHWC4'),
]

ALL_CASES = OLD_CASES + NEW_CASES


def case_id(c):
    tail = {'direct': '', 'wino': '', 'nt': '_%s-%s' % (c.get('dy_dt'), c.get('x_dt')), 'tn': '',
            'stem': '_%s' % ('planar' if c.get('layout') else 'nhwc4')}[c['kind']]
    return '%s_n%d_%dx%d_c%d_o%d_k%d_s%d_p%d%s_%s' % (c['kind'], c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['k'], c['s'], c['p'],
                                                    tail, c['flags'].replace(' ', '-') or 'plain')


def out_hw(c):
    return (c['H'] + 2 * c['p'] - c['k']) // c['s'] + 1, (c['W'] + 2 * c['p'] - c['k']) // c['s'] + 1


# ---- the split rules, restated (tests/test_wgrad_instances_host.py pins each to the library's workspace query) ------------
def wgrad_split(M, Cout, Cin, KK):
    """csrc/conv_wgrad.hip, wgrad_split (lines 350-370): the slab count S."""
    tiles = _cdiv(Cout, 128) * _cdiv(Cin, 128) * KK
    chunks = _cdiv(M, 32)
    smax = min(_cdiv(_cdiv(4096, tiles), 8) * 8, 256)
    while smax > 8 and smax > chunks:
        smax -= 8
    smin = min(_cdiv(_cdiv(1024, tiles), 8) * 8, smax)
    S, best = smin, 0.0
    for c in range(smin, smax + 1, 8):
        eff = (c * tiles / 512.0) / float(_cdiv(c * tiles, 512))
        if eff > best + 0.02:
            best, S = eff, c
    return S


def direct_plan(c):
    """S, chunks per slab (conv2d_wgrad_launch, lines 407-409), the geometry class (line 412) and the workspace floats
    (cpr_conv2d_wgrad_workspace, lines 380-385).  Derived: chunks, used (slabs with at least one chunk), last (chunks of the last
    used slab)."""
    OH, OW = out_hw(c)
    M, KK = c['N'] * OH * OW, c['k'] * c['k']
    S = wgrad_split(M, c['Cout'], c['Cin'], KK)
    chunks = _cdiv(M, 32)
    cps = _cdiv(chunks, S)
    geo = -1 if OH * OW < 32 else 2 if (KK == 1 and c['s'] == 1 and c['p'] == 0) else \
        1 if (c['s'] == 1 and OH == c['H'] and OW == c['W']) else 0
    ws = S * c['Cout'] * KK * c['Cin']
    used = _cdiv(chunks, cps)
    return dict(S=S, cps=cps, geo=geo, ws=ws if ws < (1 << 31) else ERR_UNSUPPORTED, M=M, chunks=chunks, used=used,
                last=chunks - (used - 1) * cps)


def bf16_plan(N, H, W, Cin, Cout, k, stride=1):
    """csrc/conv_wgrad_bf16.hip, wgrad_bf16_plan (lines 40-80): None where the plan itself refuses, else nt_ok / tn_ok, the
    rewriting path's splits / chunks over the padded cells Q, the pixel-major kernel's tn_splits / tn_chunks over the output pixels
    P, and the workspace bytes."""
    if k not in (1, 3) or N <= 0 or H <= 0 or W <= 0 or Cin % 64 or Cout % 64 or stride not in (1, 2):
        return None
    pad = k // 2
    Hp, Wp = H + 2 * pad, _cdiv(W + 2 * pad, 8) * 8
    G = Wp + 8
    Q = N * Hp * Wp
    taps = k * k
    tilesMN = _cdiv(Cout, 256) * _cdiv(Cin, 256)
    chunks_all = _cdiv(Q, 64)
    splits = max(min(1024 // (8 * taps * tilesMN) * 8, chunks_all // 8 // 8 * 8), 8)
    chunks = _cdiv(chunks_all, splits)
    Qk = splits * chunks * 64
    rs = _cdiv(G + Qk + G, 256) * 256
    nt_ok = stride == 1 and Cin % 256 == 0 and not (rs >= (1 << 30) or Cout * rs * 2 >= (1 << 31) or Cin * rs * 2 >= (1 << 31))
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if OH <= 0 or OW <= 0:
        return None
    P = N * OH * OW
    pchunks = _cdiv(P, 64)
    ts = max(min(512 // (8 * taps * tilesMN) * 8, pchunks // 8 // 8 * 8), 8)
    tn_ok = P * Cout * 2 < (1 << 31) and N * H * W * Cin * 2 < (1 << 31)
    if not nt_ok and not tn_ok:
        return None
    off_part = (Cout * rs * 2 + k * Cin * rs * 2) if nt_ok else 0
    nbytes = off_part + max(splits, ts) * taps * Cout * Cin * 4
    return dict(nt_ok=nt_ok, tn_ok=tn_ok, splits=splits, chunks=chunks, tn_splits=ts, tn_chunks=_cdiv(pchunks, ts), Q=Q, P=P,
                Wp=Wp, bytes=nbytes, used=_cdiv(chunks_all, chunks), tn_used=_cdiv(pchunks, _cdiv(pchunks, ts)))


def bf16_units(N, H, W, Cin, Cout, k, stride, dy_bf16, x_bf16):
    """cpr_conv_wgrad_bf16_workspace_s (lines 217-222): 256-byte units, or ERR_UNSUPPORTED."""
    pl = bf16_plan(N, H, W, Cin, Cout, k, stride)
    if pl is None or not ((dy_bf16 and x_bf16 and pl['tn_ok']) or pl['nt_ok']):
        return ERR_UNSUPPORTED
    units = _cdiv(pl['bytes'], 256)
    return units if units < (1 << 31) else ERR_UNSUPPORTED


def wino_plan(N, H, W, Cin, Cout):
    """csrc/conv_wino_wgrad.hip, wino_wgrad_split (lines 338-346) and cpr_conv3x3_wino_wgrad_workspace (349-355): K slices of spp
    strips (2 x 16 output pixels) out of N * ceil(H / 2) * ceil(W / 16)."""
    if N <= 0 or H <= 0 or W <= 0 or Cin <= 0 or Cout <= 0 or Cin % 64 or Cout % 64:
        return dict(ws=ERR_ARG)
    spi = _cdiv(H, 2) * _cdiv(W, 16)
    total = N * spi
    blocks = (Cin // 64) * (Cout // 64)
    want = min(_cdiv(256, blocks), total)
    spp = _cdiv(total, want)
    slices = _cdiv(total, spp)
    ws = slices * 16 * Cin * Cout
    return dict(slices=slices, spp=spp, total=total, spi=spi, last=total - (slices - 1) * spp, ws=ws if ws < (1 << 31) else ERR_UNSUPPORTED)


def stem_plan(N, H, W):
    """csrc/stem_bwd.hip, stem_wgrad_shape (lines 223-230) and cpr_stem_wgrad_f32_workspace (233-239): 16 x 32 output tiles dealt to
    S <= 512 workgroups (grid-stride), one 64 x 154 partial each."""
    if N <= 0 or H <= 0 or W <= 0:
        return dict(ws=ERR_ARG)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tiles = N * _cdiv(OH, 16) * _cdiv(OW, 32)
    S = min(tiles, 512)
    return dict(OH=OH, OW=OW, tiles=tiles, S=S, ws=S * 64 * 154)


def plan(c):
    if c['kind'] == 'direct':
        return direct_plan(c)
    if c['kind'] == 'wino':
        return wino_plan(c['N'], c['H'], c['W'], c['Cin'], c['Cout'])
    if c['kind'] == 'stem':
        return stem_plan(c['N'], c['H'], c['W'])
    return bf16_plan(c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['k'], c['s'])


def plan_text(c):
    pl = plan(c)
    if c['kind'] == 'direct':
        return 'S %d chunks/slab %d geo %d xf %d (slabs used %d, last %d)' % (pl['S'], pl['cps'], pl['geo'], 'xf' in c['flags'].split(),
                                                                              pl['used'], pl['last'])
    if c['kind'] == 'wino':
        return 'slices %d strips/slice %d (last %d, strips/image %d) xf %d' % (pl['slices'], pl['spp'], pl['last'], pl['spi'],
                                                                               'xf' in c['flags'].split())
    if c['kind'] == 'stem':
        return 'tiles %d S %d' % (pl['tiles'], pl['S'])
    if c['kind'] == 'nt':
        return 'nt_ok %d splits %d chunks %d (used %d)' % (pl['nt_ok'], pl['splits'], pl['chunks'], pl['used'])
    return 'tn_splits %d tn_chunks %d (used %d)' % (pl['tn_splits'], pl['tn_chunks'], pl['tn_used'])


def wino_route(c, fp32=True):
    """ops.conv2d_wgrad's rule (ops.py, conv2d_wgrad): Winograd for 3x3 / stride 1 / pad 1 layers with whole 64-channel blocks whose
    width fills its 16-pixel strips to WINO_MIN_FILL = 0.6 and whose map has at least 1024 pixels (fused affine: Cin <= 512)."""
    xf = 'xf' in c['flags'].split()
    return (c['k'] == 3 and c['s'] == 1 and c['p'] == 1 and c['Cin'] % 64 == 0 and c['Cout'] % 64 == 0 and fp32 and
            c['W'] / float(_cdiv(c['W'], 16) * 16) >= 0.6 and c['H'] * c['W'] >= 1024 and (not xf or c['Cin'] <= 512))


# ---- the GPU run ------------------------------------------------------------------------------------------------------------
def _operands(c):
    """Operands as the kernel reads them.  The gradient map is ZERO-MEAN normal in every case: the bars of wgrad_fp64_ref rest on it."""
    f = c['flags'].split()
    N, H, W, Cin, Cout, k = (c[n] for n in ('N', 'H', 'W', 'Cin', 'Cout', 'k'))
    OH, OW = out_hw(c)
    seed = (N * 7 + H * 131 + W * 17 + Cin * 3 + Cout * 5 + k * 11 + c['s'] + len(c['flags'])) % 100003
    g = torch.Generator(device='cuda').manual_seed(seed)
    dy = torch.randn((N, OH, OW, Cout), device='cuda', generator=g)
    if c['kind'] == 'stem':
        x = torch.randn((N, 3, H, W) if c['layout'] else (N, H, W, 4), device='cuda', generator=g)
    else:
        x = torch.randn((N, H, W, Cin), device='cuda', generator=g)
    if c.get('dy_dt') == 'bf16':
        dy = dy.bfloat16()
    if c.get('x_dt') == 'bf16':
        x = x.bfloat16()
    ab = None
    if 'xf' in f:
        ab = (torch.rand((N, Cin), device='cuda', generator=g) + 0.5, torch.randn((N, Cin), device='cuda', generator=g) * 0.5)
    base = None
    if 'acc' in f:
        base = torch.randn((Cout, Cin, k, k), device='cuda', generator=g) * (float(N * OH * OW) ** 0.5)   # the gradient's own scale
    return dy, x, ab, base


def _nan(n, dtype=torch.float32):
    return torch.full((n,), float('nan'), device='cuda', dtype=dtype)


def _launch(c, dy, x, ab, base):
    """One launch through the C entry point: NaN workspace of the queried size, NaN gradient (or a copy of base)."""
    from pointtinybenchmark_amd import _lib
    from pointtinybenchmark_amd.ops import _ptr, _stream
    f = c['flags'].split()
    N, H, W, Cin, Cout, k, s, p = (c[n] for n in ('N', 'H', 'W', 'Cin', 'Cout', 'k', 's', 'p'))
    OH, OW = out_hw(c)
    shape = (Cout, Cin, k, k)
    grad = base.clone() if base is not None else _nan(Cout * Cin * k * k).view(shape)
    a, b = ab if ab is not None else (None, None)
    relu, acc = int('relu' in f), int(base is not None)
    if c['kind'] == 'direct':
        n = _lib.call('cpr_conv2d_wgrad_workspace', N, OH, OW, Cin, Cout, k, k, positive=True)
        ws = _nan(n)
        _lib.call('cpr_conv2d_wgrad', _ptr(dy), _ptr(x), _ptr(a), _ptr(b), _ptr(grad), _ptr(ws), N, H, W, Cin, Cout, k, k, s, p, relu,
                  acc, _stream())
    elif c['kind'] == 'wino':
        n = _lib.call('cpr_conv3x3_wino_wgrad_workspace', N, H, W, Cin, Cout, positive=True)
        ws = _nan(n)
        _lib.call('cpr_conv3x3_wino_wgrad', _ptr(dy), _ptr(x), _ptr(a), _ptr(b), _ptr(grad), _ptr(ws), N, H, W, Cin, Cout, relu, acc,
                  _stream())
    elif c['kind'] == 'stem':
        n = _lib.call('cpr_stem_wgrad_f32_workspace', N, H, W, positive=True)
        ws = _nan(n)
        _lib.call('cpr_stem_wgrad_f32', _ptr(dy), _ptr(x), _ptr(grad), _ptr(ws), N, H, W, c['layout'], _stream())
    else:
        d16, x16 = int(dy.dtype == torch.bfloat16), int(x.dtype == torch.bfloat16)
        n = _lib.call('cpr_conv_wgrad_bf16_workspace_s', N, H, W, Cin, Cout, k, s, d16, x16, positive=True)
        ws = torch.full((n * 256,), 0xFF, device='cuda', dtype=torch.uint8)      # all-ones bytes: NaN as fp32 and as bf16
        _lib.call('cpr_conv_wgrad_bf16_s', _ptr(dy), d16, _ptr(x), x16, _ptr(grad), _ptr(ws), N, H, W, Cin, Cout, k, s, acc, _stream())
    torch.cuda.synchronize()
    return grad, n


def _through_ops(c, dy, x, ab, base):
    """The same case through the ops.* wrapper -> (gradient, kernel kind the wrapper chose)."""
    from pointtinybenchmark_amd import ops
    f = c['flags'].split()
    shape = (c['Cout'], c['Cin'], c['k'], c['k'])
    grad = base.clone() if base is not None else None
    if c['kind'] in ('direct', 'wino'):
        took = []
        inner = ops.conv3x3_wino_wgrad

        def spy(*args, **kw):
            took.append('wino')
            return inner(*args, **kw)
        ops.conv3x3_wino_wgrad = spy
        try:
            out = ops.conv2d_wgrad(dy, x, shape, c['s'], c['p'], in_ab=ab, in_relu='relu' in f, grad=grad)
        finally:
            ops.conv3x3_wino_wgrad = inner
        route = 'wino' if took else 'direct'
    elif c['kind'] == 'stem':
        out, route = ops.stem_wgrad_f32(dy, x, planar=bool(c['layout'])), 'stem'
    else:
        out = ops.conv_wgrad_bf16(dy, x, shape, out=grad, accumulate=grad is not None, stride=c['s'])
        route = c['kind']
    torch.cuda.synchronize()
    return out, route


@pytest.mark.gpu
@pytest.mark.parametrize('c', ALL_CASES, ids=case_id)
def test_wgrad_instance_vs_fp64(c):
    f = c['flags'].split()
    pl = plan(c)
    dy, x, ab, base = _operands(c)
    got, n = _launch(c, dy, x, ab, base)
    want_ws = _cdiv(pl['bytes'], 256) if c['kind'] in ('nt', 'tn') else pl['ws']
    assert n == want_ws, 'workspace query %d, the restated plan %d' % (n, want_ws)
    again, _ = _launch(c, dy, x, ab, base)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two launches differ: the kernel is not deterministic'
    OH, OW = out_hw(c)
    M = c['N'] * OH * OW
    bf16 = c['kind'] in ('nt', 'tn')
    if c['kind'] == 'stem':
        co = ci = None                            # 9408 entries: always the whole tensor
        r = R.stem_reference(dy, x, c['layout'])
    else:
        co, ci = R.pick_channels(M, c['Cout'], c['Cin'], c['k'] * c['k'], seed=M % 9973)
        r = R.reference(dy, x, c['k'], c['s'], c['p'], in_ab=ab, in_relu='relu' in f, co=co, ci=ci, bf16=bf16)
    b64 = None if base is None else R.rows_cols(base, co, ci)
    want = r['ref'] if b64 is None else r['ref'] + b64
    g64 = R.rows_cols(got, co, ci)
    tile = 256 if bf16 else 64 if c['kind'] == 'wino' else 128
    info = ''
    if c['kind'] == 'wino':
        assert M <= 100000, 'Winograd cases stay at M <= 1e5 pixels (wgrad_fp64_ref: a dropped pixel must still show)'
        mw = R.wino_magnitude(dy, x, in_ab=ab, co=co, ci=ci)
        worst = R.check(case_id(c), g64, want, R.bar_fp32(r, b64, mag=mw), co, ci, tile)
        info = ' (%.4f of the direct-magnitude bar)' % float(R.ratio(g64, want, R.bar_fp32(r, b64)).max())
    else:
        worst = R.check(case_id(c), g64, want, R.bar_fp32(r, b64), co, ci, tile)
    if 'ops' in f:
        out, route = _through_ops(c, dy, x, ab, base)
        expect = ('wino' if wino_route(c) else 'direct') if c['kind'] in ('direct', 'wino') else c['kind']
        assert route == expect, 'ops took the %s kernel, its rule says %s' % (route, expect)
        assert route == c['kind'], 'the case is listed under %s but ops routes it to %s' % (c['kind'], route)
        assert torch.equal(out.view(torch.int32), got.view(torch.int32)), 'the ops wrapper and the C entry point differ'
    print('\nWGRAD %s %s worst %.4f%s entries %d  %s' % (c['kind'], plan_text(c), worst, info, g64.numel(), case_id(c)))
