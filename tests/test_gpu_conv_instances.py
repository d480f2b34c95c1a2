"""-m gpu: every template instance the forward-conv launchers choose, pinned by its variant word and checked against the fp64
reference of tests/conv_fp64_ref.py at its tile edges (ragged last M tile, Cout not a multiple of the tile, padding borders,
stride 2 on odd maps, the tile that straddles two images, whole statistics slots) with each epilogue it takes.

Instances come from shapes alone, through the product library's dispatch (no measurement build, no forced tile).  Variant
words (ops.TRACE_CONV_VARIANT): fp32 ``bm * 1e6 + bn * 1e3 + (mode1 ? 100) + (in_a ? 10) + 1``, ``... + 2`` for the dual
launch, ``... + 3`` for the streamed 1x1 kernel; bf16 as conv_bf16_dma_launch / conv2d_fwd_bf16_launch report them."""
import pytest
import torch

from tests import conv_fp64_ref as R
from tests.test_gpu_bf16 import BIG, BIG_LDS, DMA_CASES, MASK_CASES, PP, SMALL

# Every instance the forward launchers can choose, as (kind, variant word):
#   csrc/conv_mfma.hip, conv2d_fwd_launch (tile rule lines 634-642, launches 673-681): the plain 64 x 64 tile; 128 x 128 for
#     long-K wide launches and GroupNorm-fused launches with Cout > 64; 128 x 64 for GroupNorm-fused launches with Cout <= 64
#     (and later chunks of a chunked column-sum launch, bm_fix); the fused-input (in_a, XF) and the stem (mode1, Cin == 4)
#     instances at bn 64 and 128.  <64, 128> is reached only through the measurement build's forced tiles: not listed.
#   csrc/conv_mfma.hip, conv2d_dual_launch (lines 746-755): the dual-source 64 x 64 and 128 x 128 instances.
#   csrc/conv1x1_stream.hip, conv1x1_stream_launch (lines 360-376), reported by conv_mfma.hip line 626: K = 64, 128, 256.
#   csrc/conv_mfma_bf16.hip, conv2d_fwd_bf16_launch (lines 388-397): register-staged 64 x 64 and 128 x 128.
#   csrc/conv_bf16_dma.hip, conv_bf16_dma_launch (lines 446-467; rule: bf16_dma_shape in conv_mfma_bf16.hip 344-354): 256 x 256
#     ping-pong (PP), weights direct to registers (BIG), both operands through LDS (BIG_LDS, ops.WFRAG off) and 128 x 128 (SMALL).
#     (The four-wave 256 x 256 tile exists in the measurement build only; the training epilogue of conv2d_dgrad_bf16_fused
#     reports the BIG / PP words and is covered by test_gpu_bf16.py.)
INSTANCES = [
    ('fp32', 64064001), ('fp32', 128064001), ('fp32', 128128001),
    ('fp32', 128064011), ('fp32', 128128011),
    ('fp32', 128064101), ('fp32', 128128101),
    ('fp32', 64064002), ('fp32', 128128002),
    ('fp32', 128256003), ('fp32', 64128003), ('fp32', 128064003),
    ('bf16', 64064), ('bf16', 128128),
    ('bf16', PP), ('bf16', BIG), ('bf16', BIG_LDS), ('bf16', SMALL),
]


def F32(N, H, W, Cin, Cout, k, s, p, flags, want, why=''):
    return dict(kind='fp32', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p, flags=flags, want=('fp32', want), why=why)


def BF(N, H, W, Cin, Cout, k, s, p, flags, want, why=''):
    return dict(kind='bf16', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p, flags=flags, want=('bf16', want), why=why)


def DUAL(N, H, W, Cin, Cout, k, s, p, Cin2, s2, flags, want, why=''):
    return dict(kind='dual', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p, Cin2=Cin2, s2=s2, flags=flags,
                want=('fp32', want), why=why)


# flags: bn (scale + bias), bias, res (residual add), relu, bf16out (fp32 kernel, bf16 store), f32out (bf16 kernel, fp32 store),
# mask (res_mask + colsum: ReLU-mask epilogue and column-sum slots), resmask (mask epilogue alone), gn (GroupNorm partials),
# inab / inrelu (fused input affine, with ReLU), nowfrag (ops.WFRAG off)
CASES = [
    # ---- fp32 <64, 64>
    F32(2, 17, 23, 64, 96, 3, 1, 1, 'bn res relu', 64064001, 'ragged M (782 = 12 * 64 + 14), Cout 96, borders'),
    F32(1, 33, 29, 32, 2, 3, 2, 1, 'bias', 64064001, 'stride 2 on an odd map, Cout 2'),
    F32(2, 19, 21, 128, 4, 1, 2, 0, 'bn relu', 64064001, '1x1 stride 2 on an odd map, Cout 4'),
    F32(2, 20, 20, 64, 64, 3, 1, 1, 'bias relu bf16out', 64064001, 'bf16 store'),
    F32(2, 15, 17, 64, 160, 1, 1, 0, 'bn mask', 64064001, 'ReLU mask + column sums, ragged slots'),
    F32(3, 9, 11, 256, 64, 1, 1, 0, 'bn res', 64064001, 'plain-GEMM rows, ragged'),
    F32(1, 31, 27, 96, 96, 3, 1, 1, '', 64064001, 'three K chunks per tap, no epilogue'),
    # ---- fp32 <128, 128>: Kpad / 32 >= 16 and >= 4096 tiles of 128 x 128
    F32(2, 725, 725, 64, 160, 3, 2, 1, 'bn res relu', 128128001, 'stride 2 odd map, ragged M (263538), Cout 160'),
    F32(1, 512, 512, 64, 256, 3, 1, 1, 'mask', 128128001, 'column-sum slots of 128 rows'),
    F32(1, 520, 513, 64, 256, 3, 1, 1, 'bias bf16out', 128128001, 'bf16 store, ragged M'),
    F32(1, 256, 513, 512, 500, 1, 1, 0, 'bn relu', 128128001, '1x1 GEMM rows, Cout 500'),
    # ---- fp32 GroupNorm-fused: 128 x 64 (Cout <= 64), 128 x 128
    F32(2, 16, 24, 64, 48, 3, 1, 1, 'bias relu gn', 128064001, 'Cout 48'),
    F32(2, 31, 63, 128, 64, 3, 2, 1, 'bn res gn', 128064001, 'stride 2 odd map'),
    F32(1, 31, 15, 64, 32, 1, 2, 0, 'gn', 128064001, '1x1 stride 2 odd map, Cout 32'),
    F32(2, 16, 16, 64, 96, 3, 1, 1, 'bn relu gn', 128128001, 'Cout 96'),
    F32(1, 16, 32, 256, 256, 1, 1, 0, 'bias res relu gn', 128128001, '1x1'),
    F32(2, 8, 16, 32, 130, 3, 1, 1, 'gn', 128128001, 'Cout 130: a two-channel second cout tile'),
    # ---- fp32 fused input affine (XF): OH * OW % 128 == 0, Cin <= 512
    F32(2, 16, 16, 64, 64, 3, 1, 1, 'inab inrelu res', 128064011, 'borders read zeros, not relu(b)'),
    F32(2, 8, 16, 512, 48, 3, 1, 1, 'inab bias gn', 128064011, 'Cin 512: the whole (a, b) table, Cout 48'),
    F32(1, 16, 8, 96, 2, 1, 1, 0, 'inab inrelu relu', 128064011, '1x1, Cout 2'),
    F32(2, 16, 16, 128, 160, 3, 1, 1, 'inab inrelu bn relu gn', 128128011, 'Cout 160'),
    F32(1, 24, 16, 256, 128, 3, 1, 1, 'inab bf16out', 128128011, 'bf16 store'),
    F32(3, 8, 16, 64, 96, 1, 1, 0, 'inab bias res', 128128011, '1x1, three images'),
    # ---- fp32 stem (mode1: Cin 4, one tap per float4)
    F32(2, 61, 75, 4, 64, 7, 2, 3, 'bn relu', 128064101, 'ragged M (2356)'),
    F32(1, 32, 64, 4, 64, 7, 2, 3, 'bias gn', 128064101, 'statistics slots'),
    F32(2, 45, 37, 4, 48, 7, 2, 3, 'bias relu', 128064101, 'Cout 48, ragged'),
    F32(1, 67, 53, 4, 128, 7, 2, 3, 'bn relu bf16out', 128128101, 'Cout 128, bf16 store, ragged'),
    F32(2, 40, 36, 4, 96, 7, 2, 3, 'bias res', 128128101, 'Cout 96'),
    # ---- streamed 1x1 (>= 1024 tiles; M % bm == 0 and Cout % bn == 0 by its own rule)
    F32(2, 256, 256, 64, 256, 1, 1, 0, 'bn res relu', 128256003, 'K = 64'),
    F32(1, 256, 512, 64, 512, 1, 1, 0, 'bias', 128256003, 'K = 64, two cout panels'),
    F32(1, 256, 256, 128, 128, 1, 1, 0, 'bn relu', 64128003, 'K = 128'),
    F32(1, 256, 256, 128, 256, 1, 1, 0, 'resmask', 64128003, 'K = 128, ReLU mask'),
    F32(1, 128, 256, 256, 256, 1, 1, 0, 'bias res', 128064003, 'K = 256, four cout panels'),
    F32(2, 256, 256, 256, 64, 1, 1, 0, 'bn relu', 128064003, 'K = 256, one cout panel'),
    # ---- dual source (conv + 1x1 projection shortcut)
    DUAL(2, 15, 17, 64, 96, 1, 1, 0, 32, 2, 'bn relu', 64064002, 'ragged, stride-2 shortcut on an odd map, Cout 96'),
    DUAL(1, 13, 19, 64, 64, 3, 1, 1, 128, 1, 'relu', 64064002, '3x3 main source: borders'),
    DUAL(2, 256, 256, 256, 480, 1, 1, 0, 256, 1, 'bn relu', 128128002, 'Cout 480'),
    DUAL(2, 263, 257, 64, 480, 3, 1, 1, 64, 2, 'bn', 128128002, 'ragged M, borders, stride-2 shortcut on an odd map'),
    # ---- bf16 register-staged
    BF(2, 23, 19, 64, 96, 3, 1, 1, 'bn res relu', 64064, 'ragged M, Cout 96'),
    BF(1, 33, 31, 128, 2, 3, 2, 1, 'bias', 64064, 'stride 2 odd map, Cout 2 (pair stores)'),
    BF(2, 19, 21, 64, 3, 1, 2, 0, 'bias relu', 64064, '1x1 stride 2 odd map, Cout 3 (single stores)'),
    BF(2, 13, 17, 256, 160, 1, 1, 0, 'bn f32out', 64064, 'fp32 store'),
    BF(2, 16, 24, 64, 96, 3, 1, 1, 'bias relu gn', 128128, 'statistics, Cout 96'),
    BF(1, 32, 32, 128, 256, 3, 1, 1, 'gn', 128128, 'statistics: too few tiles for the 256 x 256 tile'),
    BF(1, 16, 40, 64, 4, 1, 1, 0, 'gn f32out', 128128, 'statistics, Cout 4'),
    BF(2, 363, 363, 64, 192, 3, 1, 1, 'bn res relu', 128128, 'long K, Cout 192: the LDS-DMA rule declines; ragged M'),
    # ---- bf16 LDS-DMA (more in test_gpu_bf16.DMA_CASES / MASK_CASES, run through the same bars below)
    BF(8, 128, 128, 64, 256, 1, 1, 0, 'bn res relu nowfrag', BIG_LDS, 'both operands through LDS'),
    BF(7, 121, 119, 256, 256, 3, 1, 1, 'bias relu nowfrag', BIG_LDS, 'ragged M (100793), 3x3 borders'),
]


def case_id(c):
    extra = '_x2c%d_s%d' % (c['Cin2'], c['s2']) if c['kind'] == 'dual' else ''
    return '%s_%d_n%d_%dx%d_c%d_o%d_k%d_s%d%s_%s' % (c['kind'], c['want'][1], c['N'], c['H'], c['W'], c['Cin'], c['Cout'],
                                                 c['k'], c['s'], extra, c['flags'].replace(' ', '-') or 'plain')


def from_dma_case(t):
    N, Cin, H, W, Cout, k, s, p, flags = t[:9]
    return BF(N, H, W, Cin, Cout, k, s, p, flags, t[9] if len(t) > 9 else BIG, 'test_gpu_bf16.DMA_CASES')


def from_mask_case(t):
    N, Cin, H, W, Cout, k, f32out, want = t
    return BF(N, H, W, Cin, Cout, k, 1, k // 2, 'bf16mask' + (' f32out' if f32out else ''), want, 'test_gpu_bf16.MASK_CASES')


ALL_CASES = CASES + [from_dma_case(t) for t in DMA_CASES] + [from_mask_case(t) for t in MASK_CASES]


# ---- the dispatch rules, restated (the CPU test checks every case's expected word against them) ---------------------------
def out_hw(c):
    return (c['H'] + 2 * c['p'] - c['k']) // c['s'] + 1, (c['W'] + 2 * c['p'] - c['k']) // c['s'] + 1


def _cdiv(a, b):
    return (a + b - 1) // b


def predict_variant(c):
    """(kind, word) the product dispatch gives this case -- a restatement of ops.conv2d / conv2d_fwd_launch /
    conv2d_dual_launch / conv1x1_stream_launch / conv2d_fwd_bf16_launch / bf16_dma_shape / conv_bf16_dma_launch."""
    f = c['flags'].split()
    N, H, W, Cin, Cout, k, s, p = (c[n] for n in ('N', 'H', 'W', 'Cin', 'Cout', 'k', 's', 'p'))
    OH, OW = out_hw(c)
    M = N * OH * OW
    Kpad = _cdiv(k * k * Cin, 32) * 32
    if c['kind'] == 'dual':
        big = (Kpad + c['Cin2']) // 32 >= 16 and _cdiv(M, 128) * _cdiv(Cout, 128) >= 4096 and Cout > 64
        return ('fp32', 128128002 if big else 64064002)
    if c['kind'] == 'bf16':
        gn = 'gn' in f
        mask = 'bf16mask' in f
        K = k * k * Cin
        kch = K // 64
        t256 = _cdiv(M, 256) * (Cout // 256) if Cout % 256 == 0 else 0
        shape = -1
        if Cin % 64 == 0:
            if t256 >= 384:
                shape = 0
            elif not (gn and not mask) and Cout % 128 == 0 and _cdiv(M, 128) * (Cout // 128) >= 256:
                shape = 3
        if shape >= 0:
            bm = 128 if shape == 3 else 256
            bn = 128 if shape == 3 else 256
            stats = gn and not mask
            ok = Cout % bn == 0 and not (stats and ((OH * OW) % 128 != 0 or M % 256 != 0 or bm != 256))
            if ok:
                if shape == 3:
                    return ('bf16', SMALL)
                wfrag = 'nowfrag' not in f and Cout % 256 == 0 and K % 64 == 0
                if wfrag and kch >= 4:
                    return ('bf16', PP)
                return ('bf16', BIG if wfrag else BIG_LDS)
        if mask:
            return None
        big = gn or (kch >= 8 and _cdiv(M, 128) * _cdiv(Cout, 128) >= 4096 and Cout > 64)
        return ('bf16', 128128 if big else 64064)
    inab, gn, colsum = 'inab' in f, 'gn' in f, 'mask' in f
    res = 'res' in f or 'mask' in f or 'resmask' in f
    f32 = 'bf16out' not in f
    if not res and f32 and k == 3 and s == 1 and p == 1 and Cin % 16 == 0 and Cin >= 32 and Cout % 64 == 0 and \
            H * W / float(_cdiv(H, 16) * 16 * _cdiv(W, 16) * 16) >= 0.6 and (not inab or Cin <= 512):
        return ('wino', None)
    mode1 = Cin == 4
    if not mode1 and k == 1 and s == 1 and p == 0 and not inab and not gn and not colsum and f32 and Cin in (64, 128, 256):
        bm = 128 if Cin == 256 else 8192 // Cin
        bn = 64 if Cin == 256 else 16384 // Cin
        tn = Cout // bn
        if M % bm == 0 and Cout % bn == 0 and tn <= 32 and 32 % tn == 0 and (M // bm) * tn >= 1024:
            return ('fp32', bm * 1000000 + bn * 1000 + 3)
    bm, bn = 128, (64 if Cout <= 64 else 128)
    if not (gn and not colsum) and not inab and not mode1:
        if not (Kpad // 32 >= 16 and _cdiv(M, 128) * _cdiv(Cout, 128) >= 4096 and Cout > 64):
            bm, bn = 64, 64
    return ('fp32', bm * 1000000 + bn * 1000 + (100 if mode1 else 0) + (10 if inab else 0) + 1)


def slot_pixels(c, variant):
    """Pixels per statistics / column-sum slot of this case (None: the case writes no slots)."""
    f = c['flags'].split()
    if 'gn' in f:
        return 128
    if 'mask' in f:
        return variant[1] // 1000000          # fp32 column sums: one slot per M tile
    if 'bf16mask' in f:                        # conv_bf16_dma.h: slot tm * 2 + wm of the 256-pixel tiles, one slot per 128-pixel
        return 64 if (variant[1] == SMALL and 'f32out' in f) else 128    # tile (or per 64-pixel wave row: direct fp32 epilogue)
    return None


def tile_m(c):
    """M-tile edge of the case's expected instance (for the ragged-tile sample)."""
    kind, w = c['want']
    if kind == 'bf16':
        return {PP: 256, BIG: 256, BIG_LDS: 256, SMALL: 128, 128128: 128, 64064: 64}[w]
    return w // 1000000


# ---- the GPU run ------------------------------------------------------------------------------------------------------------
def _run(c):
    from pointtinybenchmark_amd import ops
    f = c['flags'].split()
    N, H, W, Cin, Cout, k, s, p = (c[n] for n in ('N', 'H', 'W', 'Cin', 'Cout', 'k', 's', 'p'))
    OH, OW = out_hw(c)
    bf = c['kind'] == 'bf16'
    seed = (N * 7 + H * 131 + W * 17 + Cin * 3 + Cout * 5 + k * 11 + s) % 100003
    gd = torch.Generator(device='cuda').manual_seed(seed)
    gc = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if bf else torch.float32
    x = torch.randn((N, H, W, Cin), device='cuda', generator=gd).to(dt)
    cw = 3 if Cin == 4 else Cin
    w = torch.randn((Cout, cw, k, k), generator=gc) / (cw * k * k) ** 0.5
    if bf:
        w = w.bfloat16().float()          # the values the bf16 pack holds
    scale = bias = res = in_ab = None
    if 'bn' in f:
        scale = torch.rand(Cout, generator=gc) + 0.5
    if 'bn' in f or 'bias' in f:
        bias = torch.randn(Cout, generator=gc)
    if 'res' in f or 'mask' in f or 'resmask' in f or 'bf16mask' in f:
        res = torch.randn((N, OH, OW, Cout), device='cuda', generator=gd)
        if 'bf16mask' in f:
            res = res.clamp_min(0)
        res = res.to(dt)
    if 'inab' in f:
        in_ab = ((torch.rand((N, Cin), device='cuda', generator=gd) + 0.5),
                 torch.randn((N, Cin), device='cuda', generator=gd) * 0.5)
    src2 = None
    cuda = (lambda t: None if t is None else t.cuda())
    ops.TRACE_CONV_VARIANT[0] = True
    if 'nowfrag' in f:
        ops.WFRAG[0] = False
    part = None
    try:
        pc = ops.PackedConv(w.cuda(), s, p, dt)
        if c['kind'] == 'dual':
            s2 = c['s2']
            x2 = torch.randn((N, (OH - 1) * s2 + 1, (OW - 1) * s2 + 1, c['Cin2']), device='cuda', generator=gd)
            w2 = torch.randn((Cout, c['Cin2'], 1, 1), generator=gc) / c['Cin2'] ** 0.5
            sc2 = (torch.rand(Cout, generator=gc) + 0.5) if 'bn' in f else None
            bi2 = torch.randn(Cout, generator=gc) if 'bn' in f else None
            pc2 = ops.PackedConv(w2.cuda(), s2, 0)
            out = ops.conv2d_dual(x, pc, x2, pc2, scale=cuda(scale), bias=cuda(bias), scale2=cuda(sc2), bias2=cuda(bi2),
                                  relu='relu' in f)
            src2 = (x2, w2, s2, sc2, bi2)
        elif 'bf16mask' in f:
            out, tp = ops.conv2d(x, pc, residual=res, res_mask=True, colsum=True,
                                 out_dtype=torch.float32 if 'f32out' in f else None)
            part = tp.part
        else:
            odt = torch.bfloat16 if 'bf16out' in f else (torch.float32 if 'f32out' in f else None)
            out = ops.conv2d(x, pc, scale=cuda(scale), bias=cuda(bias), residual=res, relu='relu' in f, in_ab=in_ab,
                             in_relu='inrelu' in f, gn_part='gn' in f, out_dtype=odt, res_mask='mask' in f or 'resmask' in f,
                             colsum='mask' in f)
            if 'gn' in f:
                out, part = out
            elif 'mask' in f:
                out, tp = out
                part = tp.part
        variant = ops.TRACE_CONV_VARIANT[1]
        torch.cuda.synchronize()
    finally:
        ops.TRACE_CONV_VARIANT[0] = False
        ops.WFRAG[0] = True
    return dict(out=out, part=part, variant=variant, x=x, w=w, scale=scale, bias=bias, res=res, in_ab=in_ab, src2=src2)


@pytest.mark.gpu
@pytest.mark.parametrize('c', ALL_CASES, ids=case_id)
def test_conv_instance_vs_fp64(c):
    f = c['flags'].split()
    g = _run(c)
    assert g['variant'] == c['want'], 'expected instance %r, the launcher chose %r' % (c['want'], g['variant'])
    OH, OW = out_hw(c)
    M = c['N'] * OH * OW
    slot = slot_pixels(c, g['variant'])
    bm = tile_m(c)
    m, slots = R.sample_pixels(c['N'], OH, OW, bm, slot=slot, seed=M % 9973)
    r = R.reference(g['x'], g['w'], c['s'], c['p'], m, scale=g['scale'], bias=g['bias'], residual=g['res'],
                    relu='relu' in f, in_ab=g['in_ab'], in_relu='inrelu' in f,
                    res_mask=bool({'mask', 'resmask', 'bf16mask'} & set(f)), src2=g['src2'])
    assert r['out_hw'] == (OH, OW)
    out = g['out']
    bf16_store = out.dtype == torch.bfloat16
    got = R._rows(out, m)
    worst = R.check(case_id(c), got, r['ref'], R.out_bar(r, bf16_store), m=m, bm=bm, OHW=(OH, OW))
    worst_s = 0.0
    if slot is not None:
        part = g['part'].reshape(-1, c['Cout'], 2).cpu().double()
        sref, sbar = R.slot_refs(r, m, slots, slot, M)
        got_s = part[torch.as_tensor(slots)]
        if 'gn' not in f:        # column sums: element 0 alone
            got_s, sref, sbar = got_s[..., :1], sref[..., :1], sbar[..., :1]
        worst_s = R.check(case_id(c) + ' slots', got_s.reshape(len(slots), -1), sref.reshape(len(slots), -1),
                          sbar.reshape(len(slots), -1))
    print('\nINSTANCE %s %d worst_out %.4f worst_slots %.4f  %s' % (c['want'][0], c['want'][1], worst, worst_s, case_id(c)))
