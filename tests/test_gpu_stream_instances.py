"""-m gpu: the streaming kernels of csrc/norm_pool.hip and csrc/backward.hip (lines 1-540) through their C entry points, each
against the fp64 reference and the derived bars of tests/stream_fp64_ref.py, at the states the small-shape tests never reach:
grid-stride loops that wrap, image boundaries inside a block, channel counts where a thread's four channels span two groups,
ragged / empty / 256 statistics slots, the two-pass column-sum fold and its 64-split cap, second trips of bn_fold_bwd's loops.

One table (CASES).  Outputs and workspaces are NaN-filled; every case runs twice and the two runs must be bit-equal (fixed
summation orders); cases marked ``ops`` also go through the ops.* wrapper, which must give the same bits.  Every case prints its
worst error / bar ratio per output.  tests/test_stream_instances_host.py asserts, without a GPU, that the table meets its
coverage conditions and that the bars are sharp."""
import time

import pytest
import torch
import torch.nn.functional as F

from tests import stream_fp64_ref as R

pytestmark = pytest.mark.gpu

EPS = 1e-5
RATIOS = (0, 4)            # |mean| / std of the GroupNorm inputs the table runs at (per group, nominal)
FULL_REF_ELEMS = 6_000_000  # maps above this are checked on sampled pixel rows (R.sample_rows)


def _case(op, why='', **kw):
    return dict(op=op, why=why, **kw)


def GN(N, H, W, C, G, P, dt='f32', ratio=0, relu=False, up=None, ops=False, why=''):
    """gn_stats -> gn_finalize -> gn_apply chain; P: slots or None for the ops default."""
    return _case('gn', why, N=N, H=H, W=W, C=C, G=G, P=P, dt=dt, ratio=ratio, relu=relu, up=up, ops=ops)


def AP(N, H, W, C, dt='f32', relu=False, up=None, ops=False, why=''):
    """gn_apply alone with a given affine (channel counts the statistics kernels do not take, upsample size pairs)."""
    return _case('apply', why, N=N, H=H, W=W, C=C, dt=dt, relu=relu, up=up, ops=ops)


def B8(N, H, W, C, affine, relu, ops=False, why=''):
    return _case('b8', why, N=N, H=H, W=W, C=C, affine=affine, relu=relu, ops=ops)


def GNB(N, H, W, C, G, P, entry, out, relu=True, acc=False, ratio=0, ops=False, why=''):
    """entry: f32 | bf16 | dz16 (cpr_gn_bwd, cpr_gn_bwd_bf16, cpr_gn_bwd_bf16_dz16); out: dx | dx16 | both."""
    return _case('gnbwd', why, N=N, H=H, W=W, C=C, G=G, P=P, entry=entry, out=out, relu=relu, acc=acc, ratio=ratio, ops=ops)


def UPS(N, H, W, UH, UW, C, acc=False, ops=False, why=''):
    return _case('ups', why, N=N, H=H, W=W, UH=UH, UW=UW, C=C, acc=acc, ops=ops)


def RBC(M, C, y=None, add=False, want16=False, gout=True, acc=False, ops=False, why=''):
    return _case('rbc', why, M=M, C=C, y=y, add=add, want16=want16, gout=gout, acc=acc, ops=ops)


def PCS(tiles, C, why=''):
    return _case('pcs', why, tiles=tiles, C=C)


def BNF(Cout, K, tiles, null=False, ops=False, why=''):
    """tiles 0: cpr_bn_fold_bwd from a column-sum vector; > 0: cpr_bn_fold_bwd_part.  Channel 3 has gamma (scale) 0."""
    return _case('bnf', why, Cout=Cout, K=K, tiles=tiles, null=null, ops=ops)


def AXPBY(n, alpha, beta, ops=False, why=''):
    return _case('axpby', why, n=n, alpha=alpha, beta=beta, ops=ops)


def PSA(N, H, W, C, s, py, px, sh, sw, why=''):
    return _case('psa', why, N=N, H=H, W=W, C=C, s=s, py=py, px=px, sh=sh, sw=sw)


def ZI(N, OH, OW, C, H, W, s, why=''):
    return _case('zi', why, N=N, OH=OH, OW=OW, C=C, H=H, W=W, s=s)


def POOL(N, H, W, C, dt='f32', rec=False, data='normal', ops=False, why=''):
    """data: normal | nonpos (no positive value: REC records 255 where the maximum is 0) | ties (values from {-1, 0, 1, 2})."""
    return _case('pool', why, N=N, H=H, W=W, C=C, dt=dt, rec=rec, data=data, ops=ops)


def NHWC4(N, C, H, W, ops=False, why=''):
    return _case('nhwc4', why, N=N, C=C, H=H, W=W, ops=ops)


def NCHW(N, H, W, C, ops=False, why=''):
    return _case('nchw', why, N=N, H=H, W=W, C=C, ops=ops)


# shapes of the existing kernel tests (tests/test_stream_instances_host.py asserts every one is in CASES)
EXISTING = dict(
    gn=[(2, 16, 24, 256, None), (2, 20, 28, 256, (10, 14)), (1, 25, 21, 256, (13, 11)), (2, 32, 48, 64, None), (1, 40, 24, 128, None)],
    gn_bf16=[(2, 20, 28, 256, (10, 14))],
    apply=[(2, 32, 48, 64), (1, 40, 24, 256), (2, 16, 16, 512)],
    b8=[(2, 32, 48, 128), (1, 40, 24, 64), (2, 16, 16, 64)],
    gnbwd=[(2, 16, 16, 256), (3, 13, 9, 256), (1, 40, 40, 256)],
    gnbwd_bf16=[(3, 24, 40, 256)],
    ups=[(2, 16, 16, 8, 8, 64), (2, 10, 13, 5, 7, 64), (2, 7, 8, 4, 4, 64)],
    rbc=[(240, 128), (105, 160), (105, 2048), (105, 1028)],
    bnf=[(128, 64, 0), (128, 64, 37)],
    pool=[(2, 32, 48, 64, 'f32'), (1, 33, 31, 64, 'f32'), (2, 33, 31, 64, 'bf16')],
    nhwc4=[(2, 3, 17, 23)],
    nchw=[(2, 19, 21, 70)],
)

CASES = [
    # ---- GroupNorm forward chain: existing shapes
    GN(2, 16, 24, 256, 32, None, ops=True, why='test_gpu_kernels chain shape'),
    GN(2, 20, 28, 256, 32, None, up=(10, 14), ratio=4, why='exact 2x upsample add'),
    GN(1, 25, 21, 256, 32, None, up=(13, 11), why='2U - 1: the odd FPN level'),
    GN(2, 20, 28, 256, 32, None, dt='bf16', relu=True, up=(10, 14), ops=True, why='test_gpu_bf16 shape: wide kernel, up + ReLU'),
    GN(2, 32, 48, 64, 32, None, relu=True, why='test_gpu_wino shape; C 64 / G 32: a thread spans two groups'),
    GN(1, 40, 24, 128, 32, None, ratio=4, why='test_gpu_wino shape'),
    # ---- C, G, slots
    GN(2, 12, 12, 64, 32, 1, ratio=4, relu=True, why='one slot; cpg 2'),
    GN(1, 3, 3, 64, 64, None, why='G = C; 9 pixels < one pass of the block (16); less than one block of outputs'),
    GN(2, 3, 3, 64, 64, None, dt='bf16', ratio=4, why='the same in bf16'),
    GN(1, 40, 40, 128, 1, 6, ratio=4, why='G = 1; 6 slots of 267: ragged last slot (265)'),
    GN(2, 64, 64, 512, 32, 32, relu=True, why='P = OH * OW / 128: the conv epilogue slot count'),
    GN(1, 16, 16, 1024, 32, 256, ratio=4, why='C 1024: one pixel per pass; 256 slots of one pixel'),
    GN(1, 10, 10, 256, 256, 30, why='G = C; 30 slots of 4 over 100 pixels: slots 25 .. 29 empty'),
    GN(2, 10, 10, 256, 32, 7, dt='bf16', ratio=4, up=(7, 10), why='7 slots of 15: ragged last (10); 10 <- 7 rows, equal columns'),
    GN(2, 260, 256, 256, 32, None, ratio=4, relu=True, up=(130, 128), why='gn_apply wraps (8.52 M > 8.39 M lanes); real-size slots of 260'),
    GN(8, 128, 128, 256, 32, None, dt='bf16', ratio=0, why='the 8 x 128 x 128 x 256 head map in bf16: the wide kernel wraps (16384 blocks of 8 pixels > 8192)'),
    GN(3, 150, 150, 256, 32, None, dt='bf16', ratio=4, why='wide kernel wraps with N = 3: threads cross image boundaries; ragged slots'),
    GN(3, 7, 9, 64, 32, None, dt='bf16', up=(4, 5), why='wide kernel, 32 pixel rows per block, HW 63: a block straddles two images'),
    # ---- gn_apply alone
    AP(2, 32, 48, 64, relu=True, ops=True, why='test_gpu_wino shape'),
    AP(1, 40, 24, 256, why='test_gpu_wino shape'),
    AP(2, 16, 16, 512, relu=True, why='test_gpu_wino shape'),
    AP(1, 2, 3, 16, why='less than one block'),
    AP(2, 25, 8, 64, up=(13, 7), why='13 -> 25 and 7 -> 8: non-integer ratios, different in H and W'),
    AP(2, 5, 3, 64, up=(1, 1), relu=True, why='U = 1'),
    AP(2, 6, 6, 64, up=(6, 6), why='equal sizes'),
    AP(3, 200, 180, 320, dt='bf16', relu=True, up=(100, 90), why='generic bf16 kernel (256 % 40 != 0), wraps (8.64 M lanes)'),
    AP(2, 9, 7, 12, dt='bf16', why='generic bf16 kernel: C % 8 != 0'),
    AP(2, 25, 8, 320, dt='bf16', up=(13, 7), why='generic bf16 kernel with non-integer upsample ratios'),
    AP(1, 3, 5, 36, dt='bf16', relu=True, ops=True, why='generic bf16 kernel, less than one block'),
    AP(2, 5, 3, 64, dt='bf16', up=(1, 1), why='wide kernel, U = 1'),
    AP(2, 13, 21, 128, dt='bf16', relu=True, why='wide kernel, ReLU without up'),
    B8(2, 32, 48, 128, True, True, ops=True, why='test_gpu_wino shape'),
    B8(1, 40, 24, 64, False, False, why='test_gpu_wino shape: layout change alone (exact)'),
    B8(2, 16, 16, 64, True, False, why='test_gpu_wino shape'),
    B8(2, 7, 9, 40, True, True, why='HW 63 and C 40: ragged 32 x 32 tiles on both sides'),
    # ---- GroupNorm backward
    GNB(2, 16, 16, 256, 32, None, 'f32', 'dx', relu=True, ops=True, why='test_gpu_backward shape'),
    GNB(3, 13, 9, 256, 32, None, 'f32', 'dx', relu=False, acc=True, why='test_gpu_backward shape'),
    GNB(1, 40, 40, 256, 32, None, 'f32', 'dx', relu=True, ratio=4, why='test_gpu_backward shape'),
    GNB(3, 24, 40, 256, 32, None, 'bf16', 'both', relu=True, ops=True, why='test_gpu_train_step shape'),
    GNB(3, 24, 40, 256, 32, None, 'dz16', 'both', relu=False, ops=True, why='test_gpu_train_step shape'),
    GNB(2, 12, 12, 64, 32, 1, 'f32', 'dx', relu=True, ratio=4, why='one slot; cpg 2: a thread spans two groups'),
    GNB(2, 3, 3, 64, 64, None, 'bf16', 'dx16', relu=True, why='G = C; fewer pixels than one pass; less than two blocks'),
    GNB(1, 40, 40, 128, 1, 6, 'dz16', 'dx', relu=True, ratio=4, why='G = 1; ragged last slot'),
    GNB(2, 64, 64, 512, 32, 32, 'bf16', 'dx', relu=True, acc=True, why='C 512'),
    GNB(1, 16, 16, 1024, 32, 256, 'dz16', 'dx16', relu=True, acc=True, ratio=4, why='C 1024; 256 slots'),
    GNB(1, 10, 10, 256, 256, 30, 'bf16', 'dx16', relu=False, why='G = C; empty slots'),
    GNB(1, 5, 3, 16, 4, None, 'f32', 'dx', relu=True, why='less than one block'),
    GNB(2, 260, 256, 256, 32, None, 'f32', 'dx', relu=True, ratio=4, why='gn_bwd_apply wraps; real-size slots'),
    # ---- FPN top-down add backward
    UPS(2, 16, 16, 8, 8, 64, ops=True, why='exact 2x (test_gpu_backward)'),
    UPS(2, 10, 13, 5, 7, 64, acc=True, why='2x and 2U - 1 (test_gpu_backward)'),
    UPS(2, 7, 8, 4, 4, 64, why='2U - 1 and 2x (test_gpu_backward)'),
    UPS(1, 25, 21, 13, 11, 256, acc=True, why='2U - 1 both ways: the odd FPN level'),
    UPS(2, 25, 8, 13, 7, 64, why='13 -> 25 and 7 -> 8: non-integer, different in H and W'),
    UPS(1, 5, 3, 1, 1, 4, acc=True, why='U = 1: 15 children; less than one block'),
    UPS(2, 6, 6, 6, 6, 64, why='equal sizes'),
    UPS(2, 132, 128, 132, 128, 1024, acc=True, why='wraps (8.65 M lanes), equal sizes keep it small'),
    UPS(1, 199, 3, 67, 2, 8, why='ratio 199 / 67: truncating window casts at a non-representable scale'),
    # ---- ReLU backward + column sums (rows per block: 16 up to 65 504 rows, then 32, 64 from 131 009, 128 from 262 017)
    RBC(240, 128, y='f32', ops=True, why='test_gpu_backward shape'),
    RBC(105, 160, gout=False, why='test_gpu_backward shape: sums only, 40 lanes per row'),
    RBC(105, 2048, y='bf16', add=True, want16=True, ops=True, why='test_gpu_backward shape: two column groups'),
    RBC(105, 1028, y='f32', add=True, want16=True, acc=True, why='test_gpu_backward shape: a 4-channel second column group'),
    RBC(105, 4, add=True, why='one lane per row: 256 rows per pass'),
    RBC(4100, 1024, y='bf16', why='257 row blocks of 16: the two-pass fold'),
    RBC(70000, 1028, y='bf16', add=True, want16=True, why='32 rows per block, 2188 blocks, second column group at real M'),
    RBC(140001, 64, y='f32', acc=True, why='64 rows per block, ragged last block'),
    RBC(262244, 4, y='f32', gout=False, why='128 rows per block'),
    # ---- column sums of tile partials
    PCS(37, 128, why='single pass'),
    PCS(300, 36, why='two splits; C not a multiple of 32'),
    PCS(20000, 8, why='more than 16384 tiles: the 64-split cap (313 rows per split)'),
    # ---- folded BatchNorm parameter gradients
    BNF(128, 64, 0, ops=True, why='test_gpu_backward shape'),
    BNF(128, 64, 37, ops=True, why='test_gpu_backward shape'),
    BNF(64, 576, 1, why='K 576: three trips of the dot loop; one tile'),
    BNF(32, 4608, 300, why='K 4608; tiles > 256: second trip of the tile loop'),
    BNF(8, 576, 5000, why='tiles > 4096'),
    BNF(16, 100, 0, null=True, why='null dgamma / dbeta: the weight scaling alone'),
    # ---- elementwise helpers
    AXPBY(9_000_003, 0.75, -1.5, why='wraps (cap 8 388 608), not a multiple of 256'),
    AXPBY(100, 1.0, 1.0, ops=True, why='less than one block'),
    AXPBY(77777, -0.3, 0.0, why='beta 0'),
    PSA(2, 17, 15, 128, 2, 1, 0, 1, 0, why='odd map, shifted source window'),
    PSA(1, 3, 5, 4, 2, 1, 1, 0, 0, why='less than one block'),
    PSA(2, 132, 128, 1024, 1, 0, 0, 0, 0, why='wraps (8.65 M lanes)'),
    ZI(1, 5, 4, 8, 11, 10, 2, why='rows and columns past s * OH, s * OW stay zero; less than one block'),
    ZI(2, 9, 8, 64, 17, 15, 2, why='odd map'),
    ZI(2, 66, 64, 1024, 132, 128, 2, why='wraps (8.65 M lanes)'),
    # ---- max-pool 3x3 / 2 / 1
    POOL(2, 32, 48, 64, ops=True, why='test_gpu_kernels shape'),
    POOL(1, 33, 31, 64, rec=True, ops=True, why='test_gpu_kernels shape, odd sizes, recording'),
    POOL(2, 33, 31, 64, dt='bf16', ops=True, why='test_gpu_bf16 shape'),
    POOL(1, 3, 2, 4, why='two output pixels; less than one block'),
    POOL(1, 1, 2, 4, rec=True, why='H 1, W 2: one output pixel; less than one block'),
    POOL(2, 2, 1, 8, dt='bf16', rec=True, ops=True, why='H 2, W 1'),
    POOL(2, 17, 13, 32, rec=True, data='nonpos', why='no positive value: 255 wherever the maximum is 0'),
    POOL(2, 17, 13, 32, dt='bf16', rec=True, data='ties', why='planted ties: the first window position wins'),
    POOL(1, 9, 11, 16, rec=True, data='ties', why='planted ties, fp32'),
    POOL(2, 260, 260, 512, why='wraps (4.33 M > 4.19 M lanes)'),
    POOL(2, 260, 260, 512, rec=True, data='ties', why='wraps, recording'),
    POOL(2, 260, 260, 512, dt='bf16', why='wraps, bf16'),
    POOL(2, 260, 260, 512, dt='bf16', rec=True, why='wraps, bf16, recording'),
    # ---- layout kernels
    NHWC4(2, 3, 17, 23, ops=True, why='test_gpu_kernels shape'),
    NHWC4(1, 1, 5, 7, why='one channel; less than one block'),
    NHWC4(2, 4, 9, 9, why='four channels'),
    NHWC4(1, 3, 1500, 1400, why='wraps (2.1 M pixels > 8192 * 256)'),
    NCHW(2, 19, 21, 70, ops=True, why='test_gpu_kernels shape'),
    NCHW(1, 5, 3, 4, why='one ragged tile'),
]


def case_id(c):
    skip = ('op', 'why', 'ops')
    parts = []
    for k, v in c.items():
        if k in skip or v is None or v is False:
            continue
        if v is True:
            parts.append(k)
        elif isinstance(v, tuple):
            parts.append('%s%s' % (k, 'x'.join(str(i) for i in v)))
        else:
            parts.append('%s%s' % (k if not isinstance(v, str) else '', v))
    return c['op'] + '_' + '_'.join(parts)


def case_seed(c):
    return 1000 + CASES.index(c)


def slots_of(c):
    return c['P'] if c['P'] is not None else R.default_slots(c['H'] * c['W'])


# ---- operands (CPU, seeded: the host test regenerates them) --------------------------------------------------------
def make_x(N, H, W, C, G, ratio, gen, bf16):
    """NHWC map with per-channel scales and offsets whose groups sit at |mean| / std ~ ratio; image n is scaled by 1 + n / 4
    so that the per-image affines differ well beyond any bar."""
    sc = torch.rand(C, generator=gen) + 0.5
    sg = (sc * sc).view(G, C // G).mean(1).sqrt()
    sign = (torch.randint(0, 2, (G,), generator=gen) * 2 - 1).float()
    off = (sg * sign * ratio).repeat_interleave(C // G) + 0.1 * sc * torch.randn(C, generator=gen)
    x = torch.randn((N, H, W, C), generator=gen)
    x.mul_(sc).add_(off)
    for n in range(N):
        x[n].mul_(1 + 0.25 * n)
    return x.bfloat16() if bf16 else x


def make_affine(N, C, gen):
    sign = (torch.randint(0, 2, (N, C), generator=gen) * 2 - 1).float()
    return (torch.rand((N, C), generator=gen) + 0.5) * sign, torch.randn((N, C), generator=gen)


def make_gamma_beta(C, gen):
    sign = (torch.randint(0, 8, (C,), generator=gen) > 0).float() * 2 - 1          # one channel in eight has a negative gamma
    return (torch.rand(C, generator=gen) + 0.5) * sign, torch.randn(C, generator=gen)


def gnb_operands(c):
    """Everything cpr_gn_bwd* reads, on the CPU.  mean / rstd / a / b are the fp32 roundings of the fp64 statistics of x."""
    gen = torch.Generator().manual_seed(case_seed(c))
    N, H, W, C, G = c['N'], c['H'], c['W'], c['C'], c['G']
    x = make_x(N, H, W, C, G, c['ratio'], gen, c['entry'] != 'f32')
    dz = torch.randn((N, H, W, C), generator=gen)
    if c['entry'] == 'dz16':
        dz = dz.bfloat16()
    gamma, beta = make_gamma_beta(C, gen)
    xg = x.double().view(N, H * W, G, C // G)
    mean = xg.mean((1, 3))
    rstd = (((xg - mean.view(N, 1, G, 1)) ** 2).mean((1, 3)) + EPS) ** -0.5
    mean, rstd = mean.float(), rstd.float()
    a = rstd.repeat_interleave(C // G, dim=1) * gamma
    b = beta - mean.repeat_interleave(C // G, dim=1) * a
    base = torch.randn((2, C), generator=gen) * (H * W) ** 0.5
    return dict(x=x, dz=dz, gamma=gamma, beta=beta, mean=mean.contiguous(), rstd=rstd.contiguous(), a=a.contiguous(), b=b.contiguous(), base=base)


def gnb_reference(c, o=None):
    o = o or gnb_operands(c)
    N, HW, C = c['N'], c['H'] * c['W'], c['C']
    d = lambda t: t.double()
    return R.gn_bwd_ref(d(o['x']).view(N, HW, C), d(o['dz']).view(N, HW, C), d(o['a']), d(o['b']), d(o['mean']), d(o['rstd']),
                        d(o['gamma']), c['G'], slots_of(c), c['relu'])


# ---- plumbing ---------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    from pointtinybenchmark_amd import _lib
    return _lib.call(name, *[_ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], torch.cuda.current_stream().cuda_stream)


def nanf(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device='cuda')


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(name, o1, o2):
    for k in o1:
        if o1[k] is not None:
            assert torch.equal(bits(o1[k]), bits(o2[k])), '%s: %s differs between two runs / entry points' % (name, k)


def twice(name, fn):
    o1 = fn()
    torch.cuda.synchronize()
    o2 = fn()
    torch.cuda.synchronize()
    same_bits(name, o1, o2)
    return o1


def worst(name, key, got, ref, bar, out):
    q = R.ratio(got.detach().cpu().double().reshape(ref.shape), ref, bar)
    w = float(q.max()) if q.numel() else 0.0
    out[key] = w
    if not w <= 1.0:
        bad = torch.nonzero(~(q <= 1.0))
        i = tuple(bad[0].tolist())
        raise AssertionError('%s: %s: %d/%d over the bar, worst ratio %.3g; first at %s got %.9g ref %.9g bar %.3g' % (
            name, key, bad.shape[0], q.numel(), w, i, float(got.detach().cpu().double().reshape(ref.shape)[i]), float(ref[i]), float(bar[i])))


def pixel_rows(c, pixels_per_trip=None):
    """All pixel rows of a small map, else sampled rows: borders, either side of every wrap point (``pixels_per_trip``: the
    pixels one trip of the whole grid covers) and of every image boundary, random ones."""
    N, HW = c['N'], c['H'] * c['W']
    total = N * HW
    if total * c['C'] <= FULL_REF_ELEMS:
        return None
    marks = [n * HW for n in range(1, N)]
    if pixels_per_trip:
        marks += list(range(pixels_per_trip, total, pixels_per_trip))
    return torch.as_tensor(R.sample_rows(total, marks, seed=case_seed(c), edge=max(4, min(64, pixels_per_trip or 4) // 8)))


def take(t, rows, C):
    """Rows of an (.., C) device map as fp64 on the CPU."""
    t = t.reshape(-1, C)
    return (t if rows is None else t[rows.to(t.device)]).cpu().double()


def up_rows(c, up, rows):
    """The nearest-upsampled source row of each checked pixel row."""
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    UH, UW = c['up']
    r = torch.arange(N * H * W) if rows is None else rows
    n, rem = r // (H * W), r % (H * W)
    uy = torch.as_tensor(R.nearest_index(H, UH))[rem // W]
    ux = torch.as_tensor(R.nearest_index(W, UW))[rem % W]
    return take(up, (n * UH + uy) * UW + ux, C), n


def check_apply(name, c, x, a, b, up, y, out, key='y'):
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    bf = c['dt'] == 'bf16'
    if bf and R.bf16_wide(C, N * H * W):
        trip = R.GRID_CAPS['gn_apply_bf16_wide'] * (R.BLOCK // (C // 8))
    else:
        trip = R.GRID_CAPS['gn_apply_bf16' if bf else 'gn_apply'] * R.BLOCK // (C // 4)
    rows = pixel_rows(c, trip)
    xr = take(x, rows, C)
    r = torch.arange(N * H * W) if rows is None else rows
    n = r // (H * W)
    ar, br = a.cpu().double()[n], b.cpu().double()[n]
    ur = up_rows(c, up, rows)[0] if up is not None else None
    ref, bar = R.apply_ref(xr, ar, br, c['relu'], ur, bf)
    worst(name, key, take(y, rows, C), ref, bar, out)


# ---- runners ----------------------------------------------------------------------------------------------------
def run_gn(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(case_seed(c))
    N, H, W, C, G = c['N'], c['H'], c['W'], c['C'], c['G']
    HW, P, bf = H * W, slots_of(c), c['dt'] == 'bf16'
    sfx = '_bf16' if bf else ''
    x = make_x(N, H, W, C, G, c['ratio'], gen, bf)
    gamma, beta = make_gamma_beta(C, gen)
    up = None
    UH = UW = 0
    if c['up']:
        UH, UW = c['up']
        up = torch.randn((N, UH, UW, C), generator=gen)
        up = (up.bfloat16() if bf else up).cuda()
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()

    def once():
        part = nanf((N * P, C, 2))
        call('cpr_gn_stats' + sfx, xd, part, N, HW, C, P)
        a, b, mean, rstd = nanf((N, C)), nanf((N, C)), nanf((N, G)), nanf((N, G))
        call('cpr_gn_finalize', part, gd, bd, a, b, mean, rstd, N, P, C, G, HW, EPS)
        y = nanf(xd.shape, xd.dtype)
        call('cpr_gn_apply' + sfx, xd, a, b, up, y, N, H, W, C, UH, UW, int(c['relu']))
        return dict(part=part, a=a, b=b, mean=mean, rstd=rstd, y=y)

    o = twice(name, once)
    if c['ops']:
        part = ops.gn_stats(xd, slots=c['P'])
        a, b, mean, rstd = ops.gn_finalize(part, gd, bd, N, HW, G, EPS, want_stats=True)
        same_bits(name + ' ops', o, dict(part=part, a=a, b=b, mean=mean, rstd=rstd, y=ops.gn_apply(xd, a, b, relu=c['relu'], up=up)))
    x64 = x.double().view(N, HW, C)
    ref_p, bar_p = R.stats_slots(x64, P)
    worst(name, 'part', o['part'], ref_p, bar_p, out)
    fin = R.finalize_from_partials(o['part'].cpu().double().view(N, P, C, 2), gamma.double(), beta.double(), G, HW, EPS)
    e2e = R.groupnorm_end_to_end(x64, bar_p, gamma.double(), beta.double(), G, EPS)
    for k in ('mean', 'rstd', 'a', 'b'):
        worst(name, 'fin_' + k, o[k], fin[k][0], fin[k][1], out)
        worst(name, 'gn_' + k, o[k], e2e[k][0], e2e[k][1], out)
    out['group_ratio'] = e2e['ratio']
    out['rstd_rel_err'] = float(((o['rstd'].cpu().double() - e2e['rstd'][0]).abs() / e2e['rstd'][0]).max())
    check_apply(name, c, xd, o['a'], o['b'], up, o['y'], out)
    if not bf and up is None and N * HW * C <= 40_000_000:
        # printed, not asserted: the normalised output against fp64 GroupNorm, beside torch's fp32 group_norm on the same data
        R._threads()
        t64 = F.group_norm(x64.view(N, H, W, C).permute(0, 3, 1, 2), G, gamma.double(), beta.double(), EPS)
        t32 = F.group_norm(x.permute(0, 3, 1, 2), G, gamma, beta, EPS)
        if c['relu']:
            t64, t32 = t64.relu(), t32.relu()
        out['y_err_kernel'] = float((o['y'].cpu().double().permute(0, 3, 1, 2) - t64).abs().max())
        out['y_err_torch32'] = float((t32.double() - t64).abs().max())


def run_apply(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(case_seed(c))
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    bf = c['dt'] == 'bf16'
    x = torch.randn((N, H, W, C), generator=gen) * 1.5 + 0.25
    a, b = make_affine(N, C, gen)
    up, UH, UW = None, 0, 0
    if c['up']:
        UH, UW = c['up']
        up = torch.randn((N, UH, UW, C), generator=gen)
        up = (up.bfloat16() if bf else up).cuda()
    xd, ad, bd = (x.bfloat16() if bf else x).cuda(), a.cuda(), b.cuda()

    def once():
        y = nanf(xd.shape, xd.dtype)
        call('cpr_gn_apply' + ('_bf16' if bf else ''), xd, ad, bd, up, y, N, H, W, C, UH, UW, int(c['relu']))
        return dict(y=y)

    o = twice(name, once)
    if c['ops']:
        same_bits(name + ' ops', o, dict(y=ops.gn_apply(xd, ad, bd, relu=c['relu'], up=up)))
    check_apply(name, c, xd, ad, bd, up, o['y'], out)


def run_b8(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(case_seed(c))
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    x = torch.randn((N, H, W, C), generator=gen) * 1.5 + 0.25
    a, b = make_affine(N, C, gen)
    xb = x.view(N, H, W, C // 8, 8).permute(0, 3, 1, 2, 4).contiguous().cuda()
    ad, bd = (a.cuda(), b.cuda()) if c['affine'] else (None, None)

    def once():
        y = nanf((N, H, W, C))
        call('cpr_gn_apply_b8', xb, ad, bd, y, N, H, W, C, int(c['relu']))
        return dict(y=y)

    o = twice(name, once)
    if c['ops']:
        same_bits(name + ' ops', o, dict(y=ops.gn_apply_b8(xb, ad, bd, relu=c['relu'])))
    if c['affine']:
        n = torch.arange(N * H * W) // (H * W)
        ref, bar = R.apply_ref(x.double().view(-1, C), a.double()[n], b.double()[n], c['relu'])
        worst(name, 'y', o['y'], ref, bar, out)
    else:
        assert torch.equal(o['y'].cpu(), x.relu() if c['relu'] else x), name
        out['y'] = 0.0


def run_gnbwd(c, name, out):
    from pointtinybenchmark_amd import ops
    N, H, W, C, G = c['N'], c['H'], c['W'], c['C'], c['G']
    HW, P = H * W, slots_of(c)
    o = gnb_operands(c)
    dv = {k: v.cuda() for k, v in o.items()}
    want32, want16 = c['out'] in ('dx', 'both'), c['out'] in ('dx16', 'both')
    entry = {'f32': 'cpr_gn_bwd', 'bf16': 'cpr_gn_bwd_bf16', 'dz16': 'cpr_gn_bwd_bf16_dz16'}[c['entry']]

    def once():
        ws_part, ws_k = nanf((N * P * C * 2,)), nanf((2 * N * G + 2 * N * C,))
        dx = nanf((N, H, W, C)) if want32 else None
        dx16 = nanf((N, H, W, C), torch.bfloat16) if want16 else None
        dg, db = (dv['base'][0].clone(), dv['base'][1].clone()) if c['acc'] else (nanf((C,)), nanf((C,)))
        outs = (dx,) if c['entry'] == 'f32' else (dx, dx16)
        call(entry, dv['x'], dv['dz'], dv['a'], dv['b'], dv['mean'], dv['rstd'], dv['gamma'], *outs, dg, db, ws_part, ws_k, N, HW, C,
             G, P, int(c['relu']), int(c['acc']))
        return dict(part=ws_part, k=ws_k[:2 * N * G], dx=dx, dx16=dx16, dgamma=dg, dbeta=db)

    got = twice(name, once)
    if c['ops']:
        kw = dict(slots=c['P'])
        if c['acc']:
            kw.update(dgamma=dv['base'][0].clone(), dbeta=dv['base'][1].clone())
        if c['entry'] != 'f32':
            kw.update(want16=want16, want32=want32)
        r = ops.gn_bwd(dv['x'], dv['dz'], dv['a'], dv['b'], dv['mean'], dv['rstd'], dv['gamma'], c['relu'], **kw)
        same_bits(name + ' ops', dict(dx=got['dx'], dx16=got['dx16'], dgamma=got['dgamma'], dbeta=got['dbeta']),
                  dict(dx=r[0], dx16=r[3] if len(r) > 3 else None, dgamma=r[1], dbeta=r[2]))
    ref = gnb_reference(c, o)
    out['ambiguous'] = ref['amb_share']
    assert ref['amb_share'] <= R.AMBIG_CAP, (name, ref['amb_share'])
    worst(name, 'part', got['part'], *ref['part'], out)
    for i, k in enumerate(('dgamma', 'dbeta')):
        r, bar = ref[k]
        if c['acc']:
            r = o['base'][i].double() + r
            bar = bar + R.ULP32 * r.abs()
        worst(name, k, got[k], r, bar, out)
    k2, k3 = got['k'][:N * G].view(N, G), got['k'][N * G:].view(N, G)
    worst(name, 'k2', k2, *ref['k2'], out)
    worst(name, 'k3', k3, *ref['k3'], out)
    rows = pixel_rows(c, R.GRID_CAPS['gn_bwd_apply'] * R.BLOCK // (C // 4))
    r = torch.arange(N * HW) if rows is None else rows
    n = r // HW
    sel = lambda t: t.reshape(-1, C) if rows is None else t.reshape(-1, C)[rows]
    args = (sel(o['x']).double(), sel(o['dz']).double(), sel(ref['dy']), sel(ref['amb']), o['a'].double()[n],
            k2.cpu().double()[n], k3.cpu().double()[n], G)
    for key, bf in (('dx', False), ('dx16', True)):
        if got[key] is None:
            continue
        rr, bar, alt, bar_alt = R.gn_bwd_dx(*args, bf)
        g_ = take(got[key], rows, C)
        q = R.ratio2(g_, rr, bar, alt, bar_alt)
        out[key] = float(q.max())
        assert out[key] <= 1.0, '%s: %s worst ratio %.3g (%d over the bar)' % (name, key, out[key], int((~(q <= 1)).sum()))


def run_ups(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(case_seed(c))
    N, H, W, UH, UW, C = c['N'], c['H'], c['W'], c['UH'], c['UW'], c['C']
    d = torch.randn((N, H, W, C), generator=gen)
    base = torch.randn((N, UH, UW, C), generator=gen) * 2 if c['acc'] else None
    dd = d.cuda()

    def once():
        dc = base.cuda() if c['acc'] else nanf((N, UH, UW, C))
        call('cpr_upsample_add_bwd', dd, dc, N, H, W, UH, UW, C, int(c['acc']))
        return dict(dc=dc)

    o = twice(name, once)
    if c['ops']:
        same_bits(name + ' ops', o, dict(dc=ops.upsample_add_bwd(dd, base.cuda() if c['acc'] else (N, UH, UW, C))))
    R._threads()
    ref, bar = R.upsample_add_bwd_ref(d.double(), UH, UW, base.double() if c['acc'] else None)
    worst(name, 'dcoarse', o['dc'], ref, bar, out)


def run_rbc(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(case_seed(c))
    M, C = c['M'], c['C']
    dy = torch.randn((M, C), generator=gen)
    add = torch.randn((M, C), generator=gen) if c['add'] else None
    y = None
    if c['y']:
        y = torch.randn((M, C), generator=gen).clamp_min(0)
        y = y.bfloat16() if c['y'] == 'bf16' else y
    base = torch.randn(C, generator=gen) * M ** 0.5
    dyd, addd, yd = dy.cuda(), None if add is None else add.cuda(), None if y is None else y.cuda()
    ws_n = call_ws(M, C)

    def once():
        g_ = nanf((M, C)) if c['gout'] else None
        g16 = nanf((M, C), torch.bfloat16) if c['want16'] else None
        cs = base.cuda() if c['acc'] else nanf((C,))
        ws = nanf((ws_n,))
        call('cpr_relu_bwd_colsum', dyd, addd, yd, int(c['y'] == 'bf16'), g_, g16, cs, ws, M, C, int(c['acc']))
        return dict(g=g_, g16=g16, colsum=cs)

    o = twice(name, once)
    if c['ops']:
        r = ops.relu_bwd_colsum(dyd, yd, want_g=c['gout'], colsum=base.cuda() if c['acc'] else None, want16=c['want16'], add=addd)
        same_bits(name + ' ops', o, dict(g=r[0], g16=r[2] if c['want16'] else None, colsum=r[1]))
    gref = dy + add if c['add'] else dy                              # the torch expression: one fp32 add, the mask, then RNE
    if y is not None:
        gref = torch.where(y.float() > 0, gref, torch.zeros_like(gref))
    if c['gout']:
        assert torch.equal(o['g'].cpu(), gref), name + ': g'
    if c['want16']:
        assert torch.equal(o['g16'].cpu(), gref.bfloat16()), name + ': g16'
    out['g'] = 0.0
    R._threads()
    ref, bar = R.relu_colsum_ref(gref.double(), base.double() if c['acc'] else None)
    worst(name, 'colsum', o['colsum'], ref, bar, out)


def call_ws(M, C):
    from pointtinybenchmark_amd import _lib
    n = _lib.call('cpr_relu_bwd_colsum_ws', M, C, positive=True)
    assert n == R.relu_bwd_ws(M, C), (n, M, C)
    return n


def run_pcs(c, name, out):
    gen = torch.Generator().manual_seed(case_seed(c))
    tiles, C = c['tiles'], c['C']
    part = torch.randn((tiles, C, 2), generator=gen)
    pd = part.cuda()

    def once():
        o, ws = nanf((C,)), nanf((64 * C,))
        call('cpr_part_colsum', pd, o, ws, tiles, C)
        return dict(colsum=o)

    o = twice(name, once)
    worst(name, 'colsum', o['colsum'], *R.part_colsum_ref(part.double()), out)


def run_bnf(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(case_seed(c))
    Cout, K, tiles = c['Cout'], c['K'], c['tiles']
    Gw = torch.randn((Cout, K), generator=gen)
    Wt = torch.randn((Cout, K), generator=gen) / K ** 0.5
    gamma = torch.rand(Cout, generator=gen) + 0.5
    gamma[3] = 0.0
    inv_sigma = 1.0 / torch.sqrt(torch.rand(Cout, generator=gen) + 0.5)
    mean = torch.randn(Cout, generator=gen)
    scale = gamma * inv_sigma
    cs = torch.randn((tiles, Cout, 2), generator=gen) if tiles else torch.randn(Cout, generator=gen) * 30
    Wd, sd, md, isd, csd = Wt.cuda(), scale.cuda(), mean.cuda(), inv_sigma.cuda(), cs.cuda()

    def once():
        G_ = Gw.cuda()
        dg, db = (None, None) if c['null'] else (nanf((Cout,)), nanf((Cout,)))
        if tiles:
            call('cpr_bn_fold_bwd_part', G_, Wd, sd, md, isd, csd, tiles, dg, db, Cout, K)
        else:
            call('cpr_bn_fold_bwd', G_, Wd, sd, md, isd, csd, dg, db, Cout, K)
        return dict(dW=G_, dgamma=dg, dbeta=db)

    o = twice(name, once)
    if c['ops']:
        G_ = Gw.cuda()
        dg, db = ops.bn_fold_bwd(G_, Wd, sd, md, isd, ops.TilePartials(csd, tiles, Cout) if tiles else csd)
        same_bits(name + ' ops', o, dict(dW=G_, dgamma=dg, dbeta=db))
    assert torch.equal(o['dW'].cpu(), Gw * scale.view(-1, 1)), name + ': dW'
    assert float(o['dW'][3].abs().max()) == 0.0
    out['dW'] = 0.0
    if not c['null']:
        ref = R.bn_fold_bwd_ref(Gw.double(), Wt.double(), mean.double(), inv_sigma.double(),
                                None if tiles else cs.double(), cs.double() if tiles else None)
        for k in ('dgamma', 'dbeta'):
            worst(name, k, o[k], *ref[k], out)
        if not tiles:
            assert torch.equal(o['dbeta'].cpu(), cs), name + ': dbeta is the given column sum'


def run_axpby(c, name, out):
    from pointtinybenchmark_amd import _lib, ops
    gen = torch.Generator().manual_seed(case_seed(c))
    n = c['n']
    x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    xd = x.cuda()

    def once():
        yd = y.cuda()
        _lib.call('cpr_axpby', yd.data_ptr(), xd.data_ptr(), c['alpha'], c['beta'], n, torch.cuda.current_stream().cuda_stream)
        return dict(y=yd)

    o = twice(name, once)
    if c['ops']:
        same_bits(name + ' ops', o, dict(y=ops.axpby(y.cuda(), xd, c['alpha'], c['beta'])))
    worst(name, 'y', o['y'], *R.axpby_ref(y.double(), x.double(), c['alpha'], c['beta']), out)


def run_psa(c, name, out):
    gen = torch.Generator(device='cuda').manual_seed(case_seed(c))
    N, H, W, C, s, py, px, sh, sw = (c[k] for k in ('N', 'H', 'W', 'C', 's', 'py', 'px', 'sh', 'sw'))
    nh, nw = R.cdiv(H - py, s), R.cdiv(W - px, s)
    Hs, Ws = nh + sh + 1, nw + sw + 2
    src = torch.randn((N, Hs, Ws, C), generator=gen, device='cuda')
    dst0 = torch.randn((N, H, W, C), generator=gen, device='cuda')

    def once():
        dst = dst0.clone()
        call('cpr_phase_scatter_add', src, dst, N, Hs, Ws, C, H, W, py, px, sh, sw, s)
        return dict(dst=dst)

    o = twice(name, once)
    ref = dst0.clone()
    ref[:, py::s, px::s] += src[:, sh:sh + nh, sw:sw + nw]
    assert torch.equal(o['dst'], ref), name
    out['dst'] = 0.0


def run_zi(c, name, out):
    gen = torch.Generator(device='cuda').manual_seed(case_seed(c))
    N, OH, OW, C, H, W, s = (c[k] for k in ('N', 'OH', 'OW', 'C', 'H', 'W', 's'))
    dy = torch.randn((N, OH, OW, C), generator=gen, device='cuda')

    def once():
        o = nanf((N, H, W, C))
        call('cpr_zero_insert', dy, o, N, OH, OW, C, H, W, s)
        return dict(out=o)

    o = twice(name, once)
    ref = torch.zeros((N, H, W, C), device='cuda')
    oh, ow = min(OH, R.cdiv(H, s)), min(OW, R.cdiv(W, s))
    ref[:, 0:s * oh:s, 0:s * ow:s] = dy[:, :oh, :ow]
    assert torch.equal(o['out'], ref), name
    out['out'] = 0.0


def pool_data(c, device='cuda'):
    gen = torch.Generator(device=device).manual_seed(case_seed(c))
    shape = (c['N'], c['H'], c['W'], c['C'])
    if c['data'] == 'ties':
        x = torch.randint(-1, 3, shape, generator=gen, device=device).float()
    else:
        x = torch.randn(shape, generator=gen, device=device)
        if c['data'] == 'nonpos':
            x = -x.abs() * (torch.rand(shape, generator=gen, device=device) > 0.3)      # 30 % exact zeros, nothing positive
    return x.bfloat16() if c['dt'] == 'bf16' else x


def pool_reference(x):
    """The torch expression of the kernel: first window position of a tie wins, positions outside the map never win, 255 where
    the maximum is 0.  x (N, H, W, C) float -> (max (N, OH, OW, C), arg uint8)."""
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((N, 2 * OH + 1, 2 * OW + 1, C), float('-inf'), device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    m = torch.full((N, OH, OW, C), float('-inf'), device=x.device)
    arg = torch.zeros((N, OH, OW, C), dtype=torch.uint8, device=x.device)
    for k in range(9):
        v = xp[:, k // 3:k // 3 + 2 * OH:2, k % 3:k % 3 + 2 * OW:2]
        upd = v > m
        arg = torch.where(upd, torch.full_like(arg, k), arg)
        m = torch.where(upd, v, m)
    return m, torch.where(m == 0, torch.full_like(arg, 255), arg)


def run_pool(c, name, out):
    from pointtinybenchmark_amd import ops
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    x = pool_data(c)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    entry = 'cpr_maxpool3x3s2' + ('_bf16' if c['dt'] == 'bf16' else '') + ('_rec' if c['rec'] else '')

    def once():
        o = nanf((N, OH, OW, C), x.dtype)
        arg = torch.full((N, OH, OW, C), 0x7f, dtype=torch.uint8, device='cuda') if c['rec'] else None
        call(entry, x, o, *((arg,) if c['rec'] else ()), N, H, W, C)
        return dict(out=o, arg=arg)

    o = twice(name, once)
    if c['ops']:
        r = ops.maxpool3x3s2(x, record=c['rec'])
        same_bits(name + ' ops', o, dict(out=r[0], arg=r[1]) if c['rec'] else dict(out=r, arg=None))
    m, arg = pool_reference(x.float())
    assert torch.equal(o['out'].float(), m), name + ': values'
    if c['rec']:
        assert torch.equal(o['arg'], arg), name + ': argmax bytes (%d differ)' % int((o['arg'] != arg).sum())
        out['share_255'] = float((arg == 255).float().mean())
    out['out'] = 0.0


def run_nhwc4(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(case_seed(c))
    N, C, H, W = c['N'], c['C'], c['H'], c['W']
    x = torch.randn((N, C, H, W), generator=gen, device='cuda')

    def once():
        o = nanf((N, H, W, 4))
        call('cpr_nchw_to_nhwc4', x, o, N, C, H, W)
        return dict(out=o)

    o = twice(name, once)
    if c['ops']:
        same_bits(name + ' ops', o, dict(out=ops.nchw_to_nhwc(x)))
    ref = torch.zeros((N, H, W, 4), device='cuda')
    ref[..., :C] = x.permute(0, 2, 3, 1)
    assert torch.equal(o['out'], ref), name
    out['out'] = 0.0


def run_nchw(c, name, out):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(case_seed(c))
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    x = torch.randn((N, H, W, C), generator=gen, device='cuda')

    def once():
        o = nanf((N, C, H, W))
        call('cpr_nhwc_to_nchw', x, o, N, C, H, W)
        return dict(out=o)

    o = twice(name, once)
    if c['ops']:
        same_bits(name + ' ops', o, dict(out=ops.nhwc_to_nchw_dense(x)))
    assert torch.equal(o['out'], x.permute(0, 3, 1, 2).contiguous()), name
    out['out'] = 0.0


RUNNERS = dict(gn=run_gn, apply=run_apply, b8=run_b8, gnbwd=run_gnbwd, ups=run_ups, rbc=run_rbc, pcs=run_pcs, bnf=run_bnf,
               axpby=run_axpby, psa=run_psa, zi=run_zi, pool=run_pool, nhwc4=run_nhwc4, nchw=run_nchw)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_stream_instance(c):
    name = case_id(c)
    out = {}
    t0 = time.time()
    RUNNERS[c['op']](c, name, out)
    print('%s: %s  (%.2f s; %s)' % (name, ' '.join('%s=%.3g' % kv for kv in out.items()), time.time() - t0, c['why']))


def _group_ratios(record, run):
    """Largest per-group |mean| / std over every GroupNorm the run finalises: ops.gn_finalize is wrapped so that every call
    also returns the kernel's own mean / rstd (std^2 = 1 / rstd^2 - eps)."""
    from pointtinybenchmark_amd import ops
    real = ops.gn_finalize

    def spy(part, gamma, beta, N, HW, groups=32, eps=1e-5, want_stats=False):
        a, b, mean, rstd = real(part, gamma, beta, N, HW, groups, eps, want_stats=True)
        std = (1.0 / (rstd.double() * rstd.double()) - eps).clamp_min(1e-30).sqrt()
        record.append(float((mean.double().abs() / std).max()))
        return (a, b, mean, rstd) if want_stats else (a, b)

    ops.gn_finalize = spy
    try:
        with torch.no_grad():
            run()
            torch.cuda.synchronize()
    finally:
        ops.gn_finalize = real


def test_product_groupnorm_inputs_stay_inside_the_covered_ratio():
    """The bars on rstd grow with mean^2 / var (the E[x^2] - mean^2 form), so the table only speaks for the ratios it runs at.
    This measures the largest per-group |mean| / std over the GroupNorm inputs of the CPR head and the P2PNet head on the
    synthetic full-size models of tests/test_gpu_fullsize.py (synthetic weights: no trained checkpoint exists here) and
    asserts it is at most the largest ratio of the table."""
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    from tests.test_gpu_cpr_parity import build_hip_locator, to_cuda
    from tests.test_gpu_fullsize import CFG
    cpr, p2p = [], []
    m, _ = build_hip_locator(CFG)
    cb = to_cuda(synthetic.synthetic_batch(2, 640, 640, 32, 1, 0))
    _group_ratios(cpr, lambda: m.bbox_head(m.neck(m.backbone(cb['img']))))
    m2 = P.build_detector(p2p_model_cfg(50)).cuda()
    m2.load_state_dict(synthetic.locator_state_dict(50, 1, 0, 'p2p', 61, head_std=0.05), strict=True)
    m2.train()
    cb2 = to_cuda(synthetic.synthetic_batch(1, 640, 640, 32, 1, seed=61))
    _group_ratios(p2p, lambda: m2.bbox_head(m2.neck(m2.backbone(cb2['img']))))
    print('GroupNorm inputs, largest per-group |mean| / std: CPR %d layers max %.3f; P2PNet %d layers max %.3f; table covers %g'
          % (len(cpr), max(cpr, default=0.0), len(p2p), max(p2p, default=0.0), max(RATIOS)))
    assert cpr and p2p, 'no GroupNorm was finalised: the models changed, measure them another way'
    assert max(cpr + p2p) <= max(RATIOS), (max(cpr), max(p2p))
