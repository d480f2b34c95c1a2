"""The partition plans of the two-pass reduction entries restated in Python, their case tables, seeded operands, fp64 references and a
guarded arena -- shared by tests/test_reduce_instances_host.py (CPU) and tests/test_gpu_reduce_instances.py (-m gpu).

The entries write per-workgroup partials into a caller-allocated workspace; a second kernel (or, for the two HR entries, the later
``cpr_part_colsum``) adds them in a fixed order:

  cpr_leaky_bwd_colsum, cpr_stem3x3s1_wgrad                      csrc/darknet.hip
  cpr_relu6_bwd_colsum, cpr_dw3x3_wgrad, cpr_dw3x3_dgrad         csrc/mbv2.hip
  cpr_res2_relu_bwd_colsum, cpr_res2_conv_wgrad                  csrc/res2net.hip
  cpr_conv_group_wgrad[_pitch|_dil]                              csrc/conv_group.hip
  cpr_stem3x3s2_wgrad                                            csrc/stem3x3_bwd.hip
  cpr_hrnet_fuse_bwd                                             csrc/hrnet.hip
  cpr_hrfpn_pool_bwd                                             csrc/hrfpn.hip

Every plan function returns the integers the C launcher computes; the host test holds them to the source text and to the library's own
workspace queries.  The tables name, per state of a plan (cap, floor, ragged last slice, idle lanes, a second channel block ..), the
smallest shape that reaches it; ``coverage()`` says which states a table reaches.

Bars are the ones the families' existing tests use, none is new:
  column sums (leaky)          gamma_M * sum|g|, gamma_M = M u / (1 - M u)          tests/test_gpu_darknet_kernels.py
  column sums (relu6, res2)    (M - 1) * u * sum|g|                                  mobilenet_v2_ref.colsum_ref / test_gpu_res2_conv.py
  g of the column-sum passes   bit-equal to torch's fp32 expression                  the same tests
  res2 / grouped wgrad         ACC_REL * |dY|^T|X| + ULP32 |ref|                     res2_conv_ref.wgrad_ref / grouped_conv_ref.wgrad_ref
  dilated grouped wgrad        the same form                                         dilated_conv_ref.wgrad_ref
  dw3x3 wgrad                  the same form                                         mobilenet_v2_ref.dw_wgrad_ref
  dw3x3 dgrad, column sums     per element and summed bars                           mobilenet_v2_ref.dw_dgrad_ref / colsum_ref
  stem 3x3 / 1 wgrad           gamma_n * conv(|dy|, |x|), n = N H W                  tests/test_gpu_darknet_kernels.py
                               and, where it is the smaller one, the stride-2 sibling's bar (the next line)
  stem 3x3 / 2 wgrad           wgrad_fp64_ref.reference + bar_fp32                   tests/test_gpu_regnet_conv.py
  hrnet_fuse_bwd               g, pools bit-equal to hrnet_ref.fuse_bwd_ref; column sums (n - 1) u sum|g|     tests/test_gpu_hrnet.py
  hrfpn_pool_bwd               d_out and column sums rel-L2 <= 1e-5 of fp64 autograd                          tests/test_gpu_hrfpn.py
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
SLOPE = 0.1


def cdiv(a, b):
    return (a + b - 1) // b


def gamma(n):
    return n * U / (1 - n * U)


# ---- the plans ------------------------------------------------------------------------------------------------------
LEAKY_ROWS = (512, 16, 2048)       # csrc/darknet.hip leaky_rows_per_block: start, floor, workgroups aimed at
RELU6_ROWS = (128, 16, 2048)       # csrc/mbv2.hip relu6_rows_per_block
LK_FIN_CHAINS = 64
R2_CS_PIX = 256
R2_WG_THREADS, R2_WG_MIN_PIX = 65536, 16
GC_WG_THREADS, GC_WG_MIN_PIX = 65536, 16
S1_MAX_SLICES, S1_MIN_PIX, S1_OUT = 2048, 64, 864
S3_MAX_SLICES, S3_MIN_PIX, S3_OUT = 2048, 64, 864
DW_DGRAD_WGS, DW_WGRAD_WGS, DW_MIN_ROWS = 4096, 1024, 4
HPB_PIX = 256
HRNET_MAX_K, HRFPN_MAX_OUTS = 3, 5


def rows_per_block(M, rule):
    rows, floor, wgs = rule
    while rows > floor and cdiv(M, rows) < wgs:
        rows >>= 1
    return rows


def leaky_rows_per_block(M):
    return rows_per_block(M, LEAKY_ROWS)


def relu6_rows_per_block(M):
    return rows_per_block(M, RELU6_ROWS)


def colsum_rule(kind):
    return LEAKY_ROWS if kind == 'leaky' else RELU6_ROWS


def colsum_split(C):
    """(Q, PP, grid.y) of leaky_bwd_colsum_kernel / relu6_bwd_colsum_kernel: Q channel quads x PP row lanes per workgroup."""
    Qtot = C // 4
    Q = Qtot if Qtot < 256 else 256
    return Q, 256 // Q, cdiv(Qtot, Q)


def colsum_ws(kind, M, C):
    return cdiv(M, rows_per_block(M, colsum_rule(kind))) * C


def res2_cs_chunks(M):
    return cdiv(M, R2_CS_PIX)


def res2_cs_ws(M, width):
    return res2_cs_chunks(M) * width


def _thread_split(M, T, threads, min_pix):
    s = threads // T
    smax = cdiv(M, min_pix)
    if s > smax:
        s = smax
    if s < 1:
        s = 1
    P = cdiv(M, s)
    return dict(T=T, S=cdiv(M, P), P=P, cap=max(threads // T, 1))


def r2_wg_plan(M, width):
    return _thread_split(M, (width >> 1) * (width >> 1), R2_WG_THREADS, R2_WG_MIN_PIX)


def r2_wg_ws(M, width):
    pl = r2_wg_plan(M, width)
    return pl['S'] * pl['T'] * 36


def gc_wg_plan(M, C, cg):
    return _thread_split(M, (C >> 2) * (cg >> 2), GC_WG_THREADS, GC_WG_MIN_PIX)


def gc_wg_ws(M, C, cg):
    pl = gc_wg_plan(M, C, cg)
    return pl['S'] * pl['T'] * 144


def _slice_plan(M, min_pix, max_slices):
    s = cdiv(M, min_pix)
    if s > max_slices:
        s = max_slices
    P = cdiv(M, s)
    return dict(S=cdiv(M, P), P=P, cap=max_slices)


def s1_plan(M):
    return _slice_plan(M, S1_MIN_PIX, S1_MAX_SLICES)


def s3_plan(M):
    return _slice_plan(M, S3_MIN_PIX, S3_MAX_SLICES)


def pad32(c):
    return (c + 31) // 32 * 32


def dw_grid(N, rows, cols, C, min_wgs=DW_DGRAD_WGS):
    """DwGrid of csrc/mbv2.hip: rows / cols are the rows and columns the strips divide."""
    Cp = pad32(C)
    Qtot = Cp // 4
    Q = Qtot if Qtot < 256 else 256
    PP = 256 // Q
    CG = cdiv(Qtot, Q)
    colblocks = cdiv(cols, PP)
    R = rows
    while R > DW_MIN_ROWS and N * CG * colblocks * cdiv(rows, R) < min_wgs:
        R = (R + 1) >> 1
    strips = cdiv(rows, R)
    return dict(Cp=Cp, Qtot=Qtot, Q=Q, PP=PP, CG=CG, colblocks=colblocks, R=R, strips=strips, P=N * strips * colblocks,
                ok=N * CG <= 65535 and strips <= 65535)


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def dw_wgrad_ws(N, H, W, C, stride):
    OH, OW = out_hw(H, W, stride)
    return dw_grid(N, OH, OW, C, DW_WGRAD_WGS)['P'] * 9 * C


def dw_dgrad_ws(N, H, W, C):
    return dw_grid(N, H, W, C, DW_DGRAD_WGS)['P'] * C


def hrnet_cells_per_lane(K):
    return 1 if K >= 2 else (4 if K == 1 else 16)


def hrnet_bwd_grid_x(H, W, C, K):
    CV = C // 4
    cw = CV if CV < 256 else 256
    return cdiv((H >> K) * (W >> K), (256 // cw) * hrnet_cells_per_lane(K))


def hrnet_bwd_blocks(N, H, W, C, K):
    return N * hrnet_bwd_grid_x(H, W, C, K)


def hrfpn_pool_bwd_blocks(N, H0, W0):
    return N * cdiv(H0 * W0, HPB_PIX)


# ---- case tables ----------------------------------------------------------------------------------------------------
def _cs(kind, M, C, add, want_g, y=True):
    return dict(fam='colsum', kind=kind, M=M, C=C, add=add, want_g=want_g, y=y)


def _colsum_table(kind):
    start, floor, wgs = colsum_rule(kind)
    t = [
        _cs(kind, floor, 32, False, True),                       # M exactly one block
        _cs(kind, floor + 1, 32, True, True),                    # a ragged last block of 1 row
        _cs(kind, 53, 96, True, False),                          # Q = 24, PP = 10: 16 idle threads
        _cs(kind, 33, 1024, False, True),                        # Q == 256 exactly
        _cs(kind, 37, 1280, True, True),                         # grid.y == 2, 64 live quads in the second block
        _cs(kind, 19, 1028, False, False),                       # grid.y == 2, one live quad in the second block
        _cs(kind, 5, 4, True, True),                             # C = 4: one quad, 256 row lanes
        _cs(kind, (wgs - 1) * (start // 2) + 1, 4, False, True),      # rows one halving below the ceiling, a last block of 1 row
        _cs(kind, (wgs - 1) * start + 1, 4, True, True),              # rows at the ceiling, a last block of 1 row
    ]
    if kind == 'relu6':
        t.append(_cs(kind, 21, 32, False, False, y=False))       # y NULL: the column sums of dy alone
    return t


COLSUM_CASES = _colsum_table('leaky') + _colsum_table('relu6')


def _r2cs(N, H, W, width, pitch, off, carry):
    return dict(fam='res2cs', N=N, H=H, W=W, width=width, pitch=pitch, off=off, carry=carry)


RES2CS_CASES = [
    _r2cs(1, 5, 7, 26, 128, 26, True),           # M = 35 < 256
    _r2cs(1, 16, 16, 2, 8, 2, False),            # M == 256, width 2
    _r2cs(1, 1, 257, 26, 64, 26, False),         # M = 257: a second chunk of one pixel
    _r2cs(1, 257, 1, 2, 6, 2, True),             # the same at width 2
    _r2cs(2, 50, 60, 26, 128, 78, True),         # 24 chunks x 13 pairs: two workgroups, the second with threads past the last chunk
]


def _wg(fam, N, H, W, acc, stride=1, **kw):
    return dict(fam=fam, N=N, H=H, W=W, stride=stride, acc=acc, **kw)


WGRAD_CASES = [
    # res2 slice conv, width 26: T = 169 threads per slice, cap 387 slices, >= 16 pixels per slice
    _wg('res2', 1, 4, 4, 0, width=26, pitch=128, sl=1, add=False),          # S == 1
    _wg('res2', 2, 7, 9, 1, width=26, pitch=128, sl=0, add=True),           # boundaries inside image rows, last slice 14 of 16
    _wg('res2', 1, 13, 21, 0, width=26, pitch=128, sl=2, add=False),        # M = 273 = 17 * 16 + 1: a last slice of one pixel
    _wg('res2', 2, 4, 8, 0, width=26, pitch=128, sl=1, add=True),           # P = 16, an image is 32 pixels: a boundary at the image boundary
    _wg('res2', 2, 9, 11, 1, stride=2, width=26, pitch=128, sl=2, add=False),      # stride 2, odd H and W -> 5 x 6
    _wg('res2', 3, 29, 71, 0, width=26, pitch=64, sl=1, add=False),         # M = 6177 = 386 * 16 + 1: S at the cap, last slice 1 pixel
    _wg('res2', 2, 5, 5, 1, width=14, pitch=128, sl=3, add=True),           # 7 channel pairs, offset 42
    # grouped 3x3
    _wg('group', 1, 4, 4, 0, C=16, cg=4),                                    # S == 1
    _wg('group', 2, 7, 9, 1, C=16, cg=4),
    _wg('group', 1, 13, 21, 0, C=16, cg=4),                                  # M = 273 = 17 * 16 + 1
    _wg('group', 2, 4, 8, 1, C=32, cg=8),
    _wg('group', 2, 9, 11, 0, stride=2, C=16, cg=4),
    _wg('group', 1, 37, 221, 0, C=64, cg=32),                                # M = 8177 = 511 * 16 + 1: S at the cap (512), last slice 1 pixel
    _wg('group_pitch', 2, 7, 9, 0, C=24, cg=8, Cp=32),
    _wg('group_pitch', 1, 13, 21, 1, C=24, cg=8, Cp=32),
    _wg('group_pitch', 2, 9, 11, 0, stride=2, C=72, cg=24, Cp=96),
    _wg('group_pitch', 1, 4, 4, 1, C=24, cg=8, Cp=32),                       # S == 1
    _wg('group_dil', 2, 7, 9, 0, C=16, cg=4, dil=2),
    _wg('group_dil', 1, 13, 21, 1, C=16, cg=4, dil=3),
    _wg('group_dil', 1, 4, 4, 0, C=16, cg=4, dil=2),                         # S == 1
    # depthwise 3x3: workgroups (image, strip of R rows, block of PP columns); "slices" are those workgroups
    _wg('dw', 1, 4, 5, 0, C=32, clamp=0),                                    # one workgroup
    _wg('dw', 1, 10, 5, 1, C=32, clamp=1),                                   # R at its floor: strips 3, 3, 3 and a last strip of one row
    _wg('dw', 2, 6, 33, 0, C=32, clamp=0),                                   # PP = 32: a second column block of one column; N = 2
    _wg('dw', 2, 9, 11, 1, stride=2, C=24, clamp=1),                         # stride 2, odd H and W; pad channels
    _wg('dw', 2, 3, 256, 0, C=1280, clamp=0),                                # 1024 workgroups at once: R = the whole column; CG = 2
    # stem 3x3: >= 64 pixels per slice, at most 2048 slices
    _wg('stem_s1', 1, 5, 7, 0, layout=0),                                    # S == 1
    _wg('stem_s1', 2, 8, 16, 0, layout=1),                                   # P = 64: a boundary at the image boundary
    _wg('stem_s1', 2, 5, 13, 0, layout=0),                                   # M = 130, P = 44: boundaries inside image rows
    _wg('stem_s1', 1, 37, 109, 0, layout=1),                                 # M = 4033 = 63 * 64 + 1: a last slice of one pixel
    _wg('stem_s1', 1, 252, 528, 0, layout=0),                                # M = 133056 = 2047 * 65 + 1: S at the cap, last slice 1 pixel
    _wg('stem_s2', 1, 9, 13, 0, stride=2, layout=0),                         # -> 5 x 7, S == 1
    _wg('stem_s2', 2, 15, 31, 0, stride=2, layout=1),                        # -> 8 x 16 = 128 per image
    _wg('stem_s2', 2, 9, 25, 0, stride=2, layout=0),                         # -> 5 x 13
    _wg('stem_s2', 1, 73, 217, 0, stride=2, layout=1),                       # -> 37 x 109
    _wg('stem_s2', 1, 503, 1055, 0, stride=2, layout=1),                     # -> 252 x 528: S at the cap
]


def _hr(fam, N, H, W, C, K):
    return dict(fam=fam, N=N, H=H, W=W, C=C, K=K)


HR_CASES = [
    _hr('hrnet', 1, 4, 4, 32, 0),            # K = 0: 16 cells, 32 lanes x 16 cells per block: one block
    _hr('hrnet', 2, 24, 40, 32, 0),          # several blocks per image, N = 2, a ragged last block
    _hr('hrnet', 2, 8, 8, 64, 3),            # K = 3: one cell per image
    _hr('hrnet', 2, 16, 24, 1028, 3),        # K = 3, CV = 257: a second channel block of one quad; 6 cells over 6 blocks
    _hr('hrnet', 1, 12, 20, 96, 1),          # 256 % 24 != 0: 16 idle threads
    _hr('hrfpn', 1, 16, 16, 32, 1),          # K = 1, exactly one block
    _hr('hrfpn', 2, 17, 19, 32, 5),          # K = 5 (the coarsest level 1 x 1), two blocks per image, the second ragged; dropped rows / columns
    _hr('hrfpn', 2, 24, 40, 1028, 3),        # CV = 257: a second channel block of one quad
    _hr('hrfpn', 1, 8, 12, 96, 2),           # 256 % 24 != 0
]



def _dd(N, H, W, C, stride, mask, add):
    return dict(fam='dwdgrad', N=N, H=H, W=W, C=C, stride=stride, mask=mask, add=add)


# cpr_dw3x3_dgrad with column sums: the workgroups (image, strip of R input rows, block of PP input columns) each write one partial row
DWDGRAD_CASES = [
    _dd(1, 4, 5, 32, 1, False, False),           # one workgroup
    _dd(1, 10, 33, 32, 1, True, True),           # R = 3: a last strip of one row; PP = 32: a second column block of one column
    _dd(2, 9, 11, 24, 2, True, False),           # stride 2, odd H and W (dy 5 x 6); pad channels; N = 2
    _dd(2, 2, 1024, 1280, 1, False, True),       # 4096 workgroups at once: R = the whole column; CG = 2, the second group 64 quads
]

ALL_CASES = COLSUM_CASES + RES2CS_CASES + WGRAD_CASES + DWDGRAD_CASES + HR_CASES


def case_id(c):
    keys = [k for k in c if k != 'fam']
    return c['fam'] + '-' + '-'.join('%s%s' % (k, int(c[k]) if isinstance(c[k], bool) else c[k]) for k in keys)


# ---- what a case's plan looks like ----------------------------------------------------------------------------------
def wgrad_pixels(c):
    """(M, OH, OW) of a weight-gradient case: the flattened output pixels the slices divide."""
    OH, OW = out_hw(c['H'], c['W'], c['stride'])
    return c['N'] * OH * OW, OH, OW


def wgrad_plan(c):
    """dict(S, P, cap[, T]) of a slice-split weight gradient (not 'dw')."""
    M = wgrad_pixels(c)[0]
    fam = c['fam']
    if fam == 'res2':
        return r2_wg_plan(M, c['width'])
    if fam.startswith('group'):
        return gc_wg_plan(M, c['C'], c['cg'])
    return s1_plan(M) if fam == 'stem_s1' else s3_plan(M)


def wgrad_ws(c):
    fam = c['fam']
    if fam == 'dw':
        return dw_wgrad_ws(c['N'], c['H'], c['W'], c['C'], c['stride'])
    pl = wgrad_plan(c)
    if fam == 'res2':
        return pl['S'] * pl['T'] * 36
    if fam.startswith('group'):
        return pl['S'] * pl['T'] * 144
    return pl['S'] * S1_OUT


def wgrad_family(c):
    return {'group_pitch': 'group', 'group_dil': 'group'}.get(c['fam'], c['fam'])


def coverage(colsum=None, res2cs=None, wgrad=None, hr=None, dwdgrad=None):
    """name of a state -> whether the tables reach it."""
    dwdgrad = DWDGRAD_CASES if dwdgrad is None else dwdgrad
    colsum = COLSUM_CASES if colsum is None else colsum
    res2cs = RES2CS_CASES if res2cs is None else res2cs
    wgrad = WGRAD_CASES if wgrad is None else wgrad
    hr = HR_CASES if hr is None else hr
    cov = {}
    for kind in ('leaky', 'relu6'):
        rule = colsum_rule(kind)
        start, floor, _ = rule
        cs = [c for c in colsum if c['kind'] == kind]

        def any_(f):
            return any(f(c, rows_per_block(c['M'], rule), colsum_split(c['C'])) for c in cs)
        p = kind + ': '
        cov[p + 'rows at the floor'] = any_(lambda c, r, s: r == floor)
        cov[p + 'rows at the ceiling'] = any_(lambda c, r, s: r == start)
        cov[p + 'rows one halving below the ceiling'] = any_(lambda c, r, s: r == start // 2)
        cov[p + 'M exactly one block'] = any_(lambda c, r, s: c['M'] == r)
        cov[p + 'a ragged last block of 1 row'] = any_(lambda c, r, s: c['M'] > r and c['M'] % r == 1)
        cov[p + 'ragged last block of 1 row at the ceiling'] = any_(lambda c, r, s: r == start and c['M'] % r == 1)
        cov[p + '256 % Q != 0 (C = 96)'] = any_(lambda c, r, s: 256 % s[0] != 0 and c['C'] == 96)
        cov[p + 'Q == 256 exactly'] = any_(lambda c, r, s: c['C'] == 1024 and s == (256, 1, 1))
        cov[p + 'grid.y == 2, C = 1280'] = any_(lambda c, r, s: c['C'] == 1280 and s[2] == 2)
        cov[p + 'grid.y == 2, one live quad (C = 1028)'] = any_(lambda c, r, s: c['C'] == 1028 and s[2] == 2 and c['C'] // 4 - s[0] == 1)
        cov[p + 'C = 4'] = any_(lambda c, r, s: c['C'] == 4 and s == (1, 256, 1))
        for add in (False, True):
            cov[p + 'add=%d' % add] = any_(lambda c, r, s: c['add'] == add)
            cov[p + 'g_out=%d' % add] = any_(lambda c, r, s: c['want_g'] == add)
    cov['relu6: y NULL'] = any(c['kind'] == 'relu6' and not c['y'] for c in colsum)

    def m_of(c):
        return c['N'] * c['H'] * c['W']
    cov['res2cs: M < 256'] = any(m_of(c) < R2_CS_PIX for c in res2cs)
    cov['res2cs: M == 256'] = any(m_of(c) == R2_CS_PIX for c in res2cs)
    cov['res2cs: M = 257'] = any(m_of(c) == R2_CS_PIX + 1 for c in res2cs)
    cov['res2cs: more than one workgroup'] = any(res2_cs_chunks(m_of(c)) * (c['width'] // 2) > 256 for c in res2cs)
    for w in (2, 26):
        cov['res2cs: width %d, pitched, offset %% 4 != 0' % w] = any(c['width'] == w and c['pitch'] > w and c['off'] % 4 for c in res2cs)
    for carry in (False, True):
        cov['res2cs: carry=%d' % carry] = any(c['carry'] == carry for c in res2cs)

    for fam in ('res2', 'group', 'stem_s1', 'stem_s2'):
        cs = [c for c in wgrad if wgrad_family(c) == fam]
        pls = [(c, wgrad_plan(c), wgrad_pixels(c)) for c in cs]
        p = fam + ' wgrad: '
        cov[p + 'S == 1'] = any(pl['S'] == 1 for c, pl, m in pls)
        cov[p + 'S at the cap'] = any(pl['S'] == pl['cap'] for c, pl, m in pls)
        cov[p + 'a ragged last slice of one pixel'] = any(pl['S'] > 1 and m[0] - (pl['S'] - 1) * pl['P'] == 1 for c, pl, m in pls)
        cov[p + 'a slice boundary inside an image row'] = any(pl['S'] > 1 and any((s * pl['P']) % m[2] for s in range(1, pl['S']))
                                                             for c, pl, m in pls)
        cov[p + 'a slice boundary at an image boundary, N >= 2'] = any(
            c['N'] >= 2 and any((s * pl['P']) % (m[1] * m[2]) == 0 for s in range(1, pl['S'])) for c, pl, m in pls)
        if fam != 'stem_s1':
            cov[p + 'stride 2, odd H and W'] = any(c['stride'] == 2 and c['H'] % 2 and c['W'] % 2 for c in cs)
        if fam in ('res2', 'group'):
            for acc in (0, 1):
                cov[p + 'accumulate=%d' % acc] = any(c['acc'] == acc for c in cs)
    for sub in ('group', 'group_pitch', 'group_dil'):
        cs = [c for c in wgrad if c['fam'] == sub]
        cov[sub + ' wgrad: S == 1 and S > 1'] = {min(wgrad_plan(c)['S'], 2) for c in cs} == {1, 2}
        cov[sub + ' wgrad: accumulate 0 and 1'] = {c['acc'] for c in cs} == {0, 1}
        cov[sub + ' wgrad: a ragged last slice of one pixel'] = any(
            wgrad_plan(c)['S'] > 1 and wgrad_pixels(c)[0] - (wgrad_plan(c)['S'] - 1) * wgrad_plan(c)['P'] == 1 for c in cs)
    cov['stem wgrad: both layouts'] = all({c['layout'] for c in wgrad if c['fam'] == f} == {0, 1} for f in ('stem_s1', 'stem_s2'))

    dws = [(c, dw_grid(c['N'], *out_hw(c['H'], c['W'], c['stride']), c['C'], DW_WGRAD_WGS), out_hw(c['H'], c['W'], c['stride']))
           for c in wgrad if c['fam'] == 'dw']
    p = 'dw wgrad: '
    cov[p + 'one workgroup (S == 1)'] = any(g['P'] == 1 and g['CG'] == 1 for c, g, o in dws)
    cov[p + 'R = the whole column (the plan needs no halving)'] = any(g['R'] == o[0] and o[0] > 1 and g['P'] * g['CG'] >= DW_WGRAD_WGS
                                                                       for c, g, o in dws)
    cov[p + 'R below its floor of 4 after a halving, a last strip of one row'] = any(
        g['R'] < o[0] and g['R'] <= DW_MIN_ROWS and o[0] - (g['strips'] - 1) * g['R'] == 1 for c, g, o in dws)
    cov[p + 'a second column block of one column (a boundary inside an image row)'] = any(
        g['colblocks'] > 1 and o[1] - (g['colblocks'] - 1) * g['PP'] == 1 for c, g, o in dws)
    cov[p + 'N >= 2'] = any(c['N'] >= 2 for c, g, o in dws)
    cov[p + 'stride 2, odd H and W'] = any(c['stride'] == 2 and c['H'] % 2 and c['W'] % 2 for c, g, o in dws)
    cov[p + 'CG == 2 with a ragged second channel group'] = any(g['CG'] == 2 and g['Qtot'] % g['Q'] for c, g, o in dws)
    cov[p + 'pad channels'] = any(c['C'] % 32 for c, g, o in dws)
    for acc in (0, 1):
        cov[p + 'accumulate=%d' % acc] = any(c['acc'] == acc for c, g, o in dws)
        cov[p + 'in_clamp6=%d' % acc] = any(c['clamp'] == acc for c, g, o in dws)

    dds = [(c, dw_grid(c['N'], c['H'], c['W'], c['C'], DW_DGRAD_WGS)) for c in dwdgrad]
    p = 'dw dgrad column sums: '
    cov[p + 'one workgroup'] = any(g['P'] == 1 and g['CG'] == 1 for c, g in dds)
    cov[p + 'R = the whole column (the plan needs no halving)'] = any(g['R'] == c['H'] > 1 and g['P'] * g['CG'] >= DW_DGRAD_WGS for c, g in dds)
    cov[p + 'a last strip of one row'] = any(g['strips'] > 1 and c['H'] - (g['strips'] - 1) * g['R'] == 1 for c, g in dds)
    cov[p + 'a second column block of one column'] = any(g['colblocks'] > 1 and c['W'] - (g['colblocks'] - 1) * g['PP'] == 1 for c, g in dds)
    cov[p + 'stride 2, odd H and W, N >= 2'] = any(c['stride'] == 2 and c['H'] % 2 and c['W'] % 2 and c['N'] >= 2 for c, g in dds)
    cov[p + 'CG == 2 with a ragged second channel group'] = any(g['CG'] == 2 and g['Qtot'] % g['Q'] for c, g in dds)
    cov[p + 'pad channels'] = any(c['C'] % 32 for c, g in dds)
    for f in (False, True):
        cov[p + 'mask=%d' % f] = any(c['mask'] == f for c, g in dds)
        cov[p + 'add=%d' % f] = any(c['add'] == f for c, g in dds)

    hn = [(c, hrnet_bwd_grid_x(c['H'], c['W'], c['C'], c['K'])) for c in hr if c['fam'] == 'hrnet']
    cov['hrnet_fuse_bwd: one block'] = any(gx * c['N'] == 1 for c, gx in hn)
    cov['hrnet_fuse_bwd: several blocks per image, N >= 2'] = any(gx > 1 and c['N'] >= 2 for c, gx in hn)
    cov['hrnet_fuse_bwd: K = 0'] = any(c['K'] == 0 for c, gx in hn)
    cov['hrnet_fuse_bwd: K = %d' % HRNET_MAX_K] = any(c['K'] == HRNET_MAX_K for c, gx in hn)
    cov['hrnet_fuse_bwd: idle threads and a second channel block'] = any(256 % min(c['C'] // 4, 256) for c, gx in hn) and \
        any(c['C'] // 4 > 256 for c, gx in hn)
    hf = [(c, cdiv(c['H'] * c['W'], HPB_PIX)) for c in hr if c['fam'] == 'hrfpn']
    cov['hrfpn_pool_bwd: one block'] = any(gx * c['N'] == 1 for c, gx in hf)
    cov['hrfpn_pool_bwd: several blocks per image, N >= 2'] = any(gx > 1 and c['N'] >= 2 for c, gx in hf)
    cov['hrfpn_pool_bwd: K = 1'] = any(c['K'] == 1 for c, gx in hf)
    cov['hrfpn_pool_bwd: K = %d' % HRFPN_MAX_OUTS] = any(c['K'] == HRFPN_MAX_OUTS for c, gx in hf)
    cov['hrfpn_pool_bwd: idle threads and a second channel block'] = any(256 % min(c['C'] // 4, 256) for c, gx in hf) and \
        any(c['C'] // 4 > 256 for c, gx in hf)
    return cov


# ---- seeded operands (CPU fp32) and fp64 references, computed once per case and left unchanged -----------------------------------------
def _gen(c):
    return torch.Generator().manual_seed(int(np.frombuffer(case_id(c).encode(), dtype=np.uint8).astype(np.int64).sum()) * 7919 + 13)


def embed_nhwc(t, pitch, off, fill=float('nan')):
    """NHWC (N,H,W,width) -> the (N,H,W,pitch) map that holds it at channels [off, off + width) and ``fill`` elsewhere."""
    m = torch.full(tuple(t.shape[:3]) + (pitch,), fill, dtype=t.dtype)
    m[..., off:off + t.shape[3]] = t
    return m


@functools.lru_cache(maxsize=4)
def _colsum_data(key):
    c = dict(key)
    g = _gen(c)
    M, C = c['M'], c['C']
    dy = torch.randn((M, C), generator=g)
    add = torch.randn((M, C), generator=g) if c['add'] else None
    if c['kind'] == 'leaky':
        y = torch.randn((M, C), generator=g)
        y.view(-1)[::7] = 0.0
        y.view(-1)[3::11] = -0.0
    else:
        y = (torch.randn((M, C), generator=g) * 4).clamp_min(0) if c['y'] else None       # half zeros, 7 % above 6
    s = dy + add if add is not None else dy
    if c['kind'] == 'leaky':
        want = torch.where(y > 0, s, s * SLOPE)
    else:
        want = torch.where((y > 0) & (y < 6), s, torch.zeros(())) if y is not None else s
    w64 = want.double()
    M1 = gamma(M) if c['kind'] == 'leaky' else (M - 1) * U
    return dict(dy=dy, add=add, y=y, g=want, cs=w64.sum(0), cs_bar=M1 * w64.abs().sum(0))


def colsum_data(c):
    return _colsum_data(tuple(sorted(c.items())))


def res2cs_data(c):
    g = _gen(c)
    shape = (c['N'], c['H'], c['W'], c['width'])
    dy = torch.randn(shape, generator=g)
    y = torch.randn(shape, generator=g).clamp_min(0)
    carry = torch.randn(shape, generator=g) if c['carry'] else None
    want = torch.where(y > 0, dy + carry if carry is not None else dy, torch.zeros(()))       # (a masked element is +0.0)
    flat = want.double().reshape(-1, c['width'])
    return dict(dy=dy, y=y, carry=carry, g=want, cs=flat.sum(0), cs_bar=(flat.shape[0] - 1) * U * flat.abs().sum(0))


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def wgrad_reference(c, x, dy, add=None):
    """(ref, bar) in the parameter's layout, fp64, by the family's own reference module, from the NHWC fp32 operands."""
    from tests import dilated_conv_ref as DL
    from tests import grouped_conv_ref as G
    from tests import mobilenet_v2_ref as MB
    from tests import res2_conv_ref as R2
    from tests import wgrad_fp64_ref as WF
    fam, stride = c['fam'], c['stride']
    if fam == 'res2':
        return R2.wgrad_ref(nchw(dy), nchw(x + add if add is not None else x), stride)        # fl32(x + add): rounded once, as the kernel rounds it
    if fam == 'group_dil':
        return DL.wgrad_ref(nchw(dy), nchw(x), (c['C'], c['cg'], 3, 3), c['dil'], groups=c['C'] // c['cg'])
    if fam.startswith('group'):
        return G.wgrad_ref(nchw(dy), nchw(x), (c['C'], c['cg'], 3, 3), c['C'] // c['cg'], stride)
    if fam == 'dw':
        return MB.dw_wgrad_ref(nchw(dy), nchw(x), stride, bool(c['clamp']))
    if fam == 'stem_s1':
        x64, d64 = nchw(x[..., :3]).double(), nchw(dy).double()
        ref = torch.nn.grad.conv2d_weight(x64, (32, 3, 3, 3), d64, stride=1, padding=1)
        mag = torch.nn.grad.conv2d_weight(x64.abs(), (32, 3, 3, 3), d64.abs(), stride=1, padding=1)
        # gamma_n grows with n (133056 pixels: 0.8 % of sum |dy x|, 65 whole slices); the stride-2 sibling's bar does not, and is the
        # tighter one from n = 16 on: the smaller of the two, so the bar never widens with the map
        return ref, torch.minimum(gamma(wgrad_pixels(c)[0]) * mag, WF.bar_fp32(dict(ref=ref, mag=mag)))
    r = WF.reference(dy, x[..., :3].contiguous(), 3, 2, 1)
    return r['ref'], WF.bar_fp32(r)


def wgrad_data(c):
    """NHWC fp32 operands as the kernel reads them (without pitch), ``base`` for accumulate, and (ref, bar) in the parameter's layout."""
    g = _gen(c)
    fam, N, H, W = c['fam'], c['N'], c['H'], c['W']
    M, OH, OW = wgrad_pixels(c)
    add = None
    if fam == 'res2':
        ch, shape = c['width'], (c['width'], c['width'], 3, 3)
    elif fam.startswith('group'):
        ch, shape = c['C'], (c['C'], c['cg'], 3, 3)
    elif fam == 'dw':
        ch, shape = c['C'], (c['C'], 1, 3, 3)
    else:
        ch, shape = 32, (32, 3, 3, 3)
    if fam in ('stem_s1', 'stem_s2'):
        x = torch.randn((N, H, W, 4), generator=g)
        x[..., 3] = 9.0                                            # the 4th channel is ignored
    elif fam == 'dw':
        x = (torch.randn((N, H, W, ch), generator=g) * 4).clamp_min(0)       # a ReLU(v) map: half zeros, 7 % above 6
    else:
        x = torch.randn((N, H, W, ch), generator=g)
    dy = torch.randn((N, OH, OW, ch), generator=g)
    if fam == 'res2' and c['add']:
        add = torch.randn((N, H, W, ch), generator=g)
    base = torch.randn(shape, generator=g) if c['acc'] else None
    ref, bar = wgrad_reference(c, x, dy, add)
    return dict(x=x, dy=dy, add=add, shape=shape, base=base, ref=ref, bar=bar)


def dwdgrad_data(c):
    """NHWC fp32 operands (without pitch), the (C,1,3,3) weight and folded scale, and the fp64 (ref, bar) of dx and of its column sums
    by tests/mobilenet_v2_ref.py."""
    from tests import mobilenet_v2_ref as MB
    g = _gen(c)
    N, H, W, C, stride = c['N'], c['H'], c['W'], c['C'], c['stride']
    OH, OW = out_hw(H, W, stride)
    dy = torch.randn((N, OH, OW, C), generator=g)
    w = torch.randn((C, 1, 3, 3), generator=g) * (2.0 / 9) ** 0.5
    scale = torch.rand((C,), generator=g) + 0.5
    mask = (torch.randn((N, H, W, C), generator=g) * 4).clamp_min(0) if c['mask'] else None
    add = torch.randn((N, H, W, C), generator=g) if c['add'] else None
    ref, bar = MB.dw_dgrad_ref(nchw(dy), w, stride, (H, W), scale, None if mask is None else nchw(mask), None if add is None else nchw(add))
    cs, cs_bar = MB.colsum_ref(ref, bar)
    return dict(dy=dy, w=w, scale=scale, mask=mask, add=add, ref=ref, bar=bar, cs=cs, cs_bar=cs_bar)


def hr_data(c):
    from tests import hrfpn_ref as HF
    from tests import hrnet_ref as HN
    g = _gen(c)
    N, H, W, C, K = c['N'], c['H'], c['W'], c['C'], c['K']
    if c['fam'] == 'hrnet':
        dy = torch.randn((N, H, W, C), generator=g)
        y = torch.randn((N, H, W, C), generator=g).clamp_min(0)
        g32, pools32, _ = HN.fuse_bwd_ref(dy.numpy(), y.numpy(), K)
        g64, _, cs64 = HN.fuse_bwd_ref64(dy.numpy(), y.numpy(), K)
        bound = (N * H * W - 1) * U * np.abs(g64).reshape(-1, C).sum(0)
        return dict(dy=dy, y=y, g=g32, pools=pools32, cs=cs64, cs_bar=bound)
    gs = [torch.randn((N, H >> k, W >> k, C), generator=g) for k in range(K)]
    out = torch.zeros((N, C, H, W), dtype=torch.float64, requires_grad=True)
    sum((o * nchw(gk).double()).sum() for o, gk in zip(HF.pools(out, K), gs)).backward()
    return dict(gs=gs, d_out=out.grad.permute(0, 2, 3, 1).contiguous(), cs=out.grad.sum((0, 2, 3)))


# ---- the guarded arena ----------------------------------------------------------------------------------------------
GUARD_BYTES = 256        # 64 fp32 elements before and after every slice
POISON_WS, POISON_OUT = 3e38, -7.25


class Arena:
    """fp32 slices in the middle of one uint8 device buffer of 0xFF bytes (NaN as fp32), after tests/test_gpu_pack_instances.py's class:
    every slice starts on a 256-byte boundary and has at least GUARD_BYTES of 0xFF on either side.  specs: [(name, floats)]."""

    def __init__(self, specs, device='cuda'):
        pos, self.spans = GUARD_BYTES, {}
        for name, n in specs:
            assert n > 0 and name not in self.spans, (name, n)
            self.spans[name] = (pos, 4 * n)
            pos += (4 * n + 255) // 256 * 256 + GUARD_BYTES
        self.size = pos
        self.buf = torch.full((pos,), 0xFF, dtype=torch.uint8, device=device)

    def __getitem__(self, name):
        o, nb = self.spans[name]
        return self.buf[o:o + nb].view(torch.float32)

    def gaps(self):
        """[(begin, end)] byte ranges outside every slice."""
        out, pos = [], 0
        for o, nb in sorted(self.spans.values()):
            out.append((pos, o))
            pos = o + nb
        out.append((pos, self.size))
        return out

    def intact(self, label):
        for a, b in self.gaps():
            bad = torch.nonzero(self.buf[a:b] != 0xFF)
            assert bad.numel() == 0, '%s: %d guard bytes changed, the first at byte %d of the arena (slices %s)' % (
                label, bad.numel(), a + int(bad[0]), self.spans)

    def unwritten(self, name):
        """Elements of a slice that still hold the arena's 0xFFFFFFFF."""
        return int((self[name].view(torch.int32) == -1).sum())
