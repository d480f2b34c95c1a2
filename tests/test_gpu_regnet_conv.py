"""-m gpu: the RegNet kernels.

  grouped 3x3 at a channel pitch (csrc/conv_group.hip; widths 24 / 40 / 48 / 56 and the PITCH instances): forward, data gradient and
      weight gradient through ops.conv2d / conv2d_dgrad / conv2d_wgrad on maps at pitch roundup(C, 32), against the fp64 references and
      per-element bars of tests/grouped_conv_ref.py.  Pad channels: written as bit-zero into a NaN-filled output, never read (NaN there
      changes no output bit, the weight gradient stays finite); exact group isolation; bit-repeatability; batch independence; one
      existing-width call keeps its variant.
  stem (csrc/stem_deep.hip launch A alone, csrc/stem3x3_bwd.hip): forward in both input layouts bit-equal and within the bar of
      tests/conv_fp64_ref.py; weight gradient within the bar of tests/wgrad_fp64_ref.py with zero-mean dy
  argument errors: C % cg, pitch < C, bf16 tensors"""
import functools

import numpy as np
import pytest
import torch

from tests import conv_fp64_ref as CF
from tests import grouped_conv_ref as G
from tests import wgrad_fp64_ref as WF
from tests.conv_fp64_ref import check

pytestmark = pytest.mark.gpu

# (N, H, W, C, cg, stride), each at pitch roundup(C, 32)
SHAPES = [
    (2, 7, 9, 72, 24, 1),          # pitch 96: a pad as wide as a group
    (1, 18, 23, 96, 48, 2),        # both reach 9 x 12: the data gradient must tell the input sizes apart; pitch == C
    (1, 17, 23, 96, 48, 2),
    (2, 9, 12, 432, 48, 1),        # 448
    (2, 5, 6, 1008, 48, 2),        # 1024, -> 3 x 3
    (2, 9, 12, 80, 40, 2),         # 96
    (2, 5, 6, 560, 40, 1),         # 576
    (2, 5, 6, 168, 56, 1),         # 192
    (1, 6, 6, 1624, 56, 1),        # 1632
    (2, 20, 20, 168, 24, 1),       # 192; an image boundary inside a pixel tile
    (3, 17, 24, 408, 24, 1),       # 416
]
IDS = [G.shape_id(s) for s in SHAPES]
NAN = float('nan')


def _ops():
    from pointtinybenchmark_amd import ops
    return ops


def pitch_of(shape):
    return (shape[3] + 31) // 32 * 32


def padded(t_nchw, Cp, fill):
    """CPU NCHW master -> device NHWC map at pitch Cp, pad channels = fill."""
    t = G.nhwc(t_nchw)
    out = torch.full(tuple(t.shape[:3]) + (Cp,), fill, dtype=torch.float32)
    out[..., :t.shape[3]] = t
    return out.cuda()


@functools.lru_cache(maxsize=None)
def case(shape):
    """The operands of one shape, CPU masters and their device copies, shared by every test and left unchanged."""
    c = G.make_case(shape, seed=7)
    Cp = pitch_of(shape)
    c['Cp'] = Cp
    c['xd'], c['xnan'] = padded(c['x'], Cp, 0.0), padded(c['x'], Cp, NAN)
    c['dyd'], c['dynan'] = padded(c['dy'], Cp, 0.0), padded(c['dy'], Cp, NAN)
    c['wd'], c['scaled'], c['biasd'] = c['w'].cuda(), c['scale'].cuda(), c['bias'].cuda()
    return c


def forward(c, x=None, w=None, affine=False, out=None):
    ops = _ops()
    pc = ops.PackedConv(c['wd'] if w is None else w, c['stride'], 1, groups=c['groups'], pitch=c['Cp'])
    assert pc.C == c['shape'][3] and pc.Cin == pc.Cout == c['Cp']
    x = c['xd'] if x is None else x
    if affine:
        return ops.conv2d(x, pc, scale=c['scaled'], bias=c['biasd'], relu=True, out=out)
    return ops.conv2d(x, pc, out=out)


def dgrad(c, dy=None, w=None, scaled=True):
    ops = _ops()
    H, W = c['shape'][1:3]
    pt = ops.dgrad_pack(c['wd'] if w is None else w, c['stride'], 1, scale=c['scaled'] if scaled else None, groups=c['groups'],
                        pitch=c['Cp'])
    assert isinstance(pt, ops.PackedConv) and pt.groups == c['groups'] and pt.Cin == c['Cp']
    return ops.conv2d_dgrad(c['dyd'] if dy is None else dy, pt, (H, W), c['stride'])


def wgrad(c, dy=None, x=None):
    return _ops().conv2d_wgrad(c['dyd'] if dy is None else dy, c['xd'] if x is None else x, tuple(c['w'].shape), c['stride'], 1,
                               groups=c['groups'])


def _flat(t):
    return t.reshape(-1, t.shape[-1])


def _pad_is_bit_zero(t, C):
    pad = t[..., C:]
    return pad.numel() == 0 or int(torch.count_nonzero(pad.contiguous().view(torch.int32))) == 0      # (+0.0: -0.0 has a bit set)


@pytest.mark.parametrize('affine', [False, True], ids=['raw', 'scale_bias_relu'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_within_bar_and_pad_written_as_zero(shape, affine):
    c = case(shape)
    C, Cp = shape[3], c['Cp']
    OH, OW = G.out_hw(shape[1], shape[2], shape[5])
    out = torch.full((shape[0], OH, OW, Cp), NAN, device='cuda')
    got = forward(c, affine=affine, out=out)
    assert got is out and _pad_is_bit_zero(got, C)
    ref, bar = G.fwd_ref(c['x'], c['w'], c['groups'], c['stride'], *((c['scale'], c['bias'], True) if affine else ()))
    assert tuple(got.shape) == tuple(ref.shape[:3]) + (Cp,)
    worst = check('grouped forward %s' % G.shape_id(shape), _flat(got[..., :C].cpu()), _flat(ref), _flat(bar))
    print('forward %s %s: worst |err| / bar = %.3g' % (G.shape_id(shape), 'affine' if affine else 'raw', worst))


@pytest.mark.parametrize('scaled', [False, True], ids=['raw', 'bn_scale'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_data_gradient_within_bar(shape, scaled):
    c = case(shape)
    H, W, C = shape[1], shape[2], shape[3]
    got = dgrad(c, scaled=scaled)
    assert tuple(got.shape) == (shape[0], H, W, c['Cp']) and _pad_is_bit_zero(got, C)
    ref, bar = G.dgrad_ref(c['dy'], c['w'], c['groups'], c['stride'], (H, W), c['scale'] if scaled else None)
    worst = check('grouped dgrad %s' % G.shape_id(shape), _flat(got[..., :C].cpu()), _flat(ref), _flat(bar))
    print('dgrad %s: worst |err| / bar = %.3g' % (G.shape_id(shape), worst))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_weight_gradient_within_bar(shape):
    c = case(shape)
    got = wgrad(c).cpu()
    ref, bar = G.wgrad_ref(c['dy'], c['x'], c['w'].shape, c['groups'], c['stride'])
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('grouped wgrad %s' % G.shape_id(shape), got.reshape(shape[3], -1), ref.reshape(shape[3], -1), bar.reshape(shape[3], -1))
    print('wgrad %s: worst |err| / bar = %.3g' % (G.shape_id(shape), worst))
    base = torch.randn(tuple(c['w'].shape), generator=torch.Generator().manual_seed(5))
    acc = base.cuda()
    _ops().conv2d_wgrad(c['dyd'], c['xd'], tuple(c['w'].shape), c['stride'], 1, grad=acc, groups=c['groups'])
    assert torch.equal(acc.cpu(), base + got)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_pad_channels_are_never_read(shape):
    """NaN in the pad channels of the inputs: the real outputs keep their bits, the pad outputs stay bit-zero, the weight gradient is
    the same finite tensor."""
    c = case(shape)
    C = shape[3]
    for affine in (False, True):
        a, b = forward(c, affine=affine), forward(c, x=c['xnan'], affine=affine)
        assert torch.equal(a[..., :C], b[..., :C]) and _pad_is_bit_zero(b, C) and bool(torch.isfinite(b).all())
    a, b = dgrad(c), dgrad(c, dy=c['dynan'])
    assert torch.equal(a[..., :C], b[..., :C]) and _pad_is_bit_zero(b, C) and bool(torch.isfinite(b).all())
    a, b = wgrad(c), wgrad(c, dy=c['dynan'], x=c['xnan'])
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_group_isolation_is_exact(shape):
    c = case(shape)
    N, H, W, C, cg, stride = shape
    groups = c['groups']
    k = groups // 3
    lo, hi = k * cg, (k + 1) * cg
    others = torch.zeros(c['Cp'], dtype=torch.bool)
    others[:C] = True
    others[lo:hi] = False
    others = others.cuda()
    xm, dym = c['xd'].clone(), c['dyd'].clone()
    xm[..., lo:hi] = xm[..., lo:hi] * 0.5 - 1.0
    dym[..., lo:hi] = -dym[..., lo:hi]
    y, y2 = forward(c, affine=True), forward(c, x=xm, affine=True)
    assert not torch.equal(y[..., lo:hi], y2[..., lo:hi])
    assert torch.equal(y[..., others], y2[..., others])
    dx, dx2 = dgrad(c), dgrad(c, dy=dym)
    assert not torch.equal(dx[..., lo:hi], dx2[..., lo:hi])
    assert torch.equal(dx[..., others], dx2[..., others])
    dw, dw2 = wgrad(c), wgrad(c, dy=dym, x=xm)
    assert not torch.equal(dw[lo:hi], dw2[lo:hi])
    assert torch.equal(dw[others[:C]], dw2[others[:C]])
    # input non-zero in one group's channels only, no bias: every output channel of every other group is exactly 0
    x1 = torch.zeros_like(c['xd'])
    x1[..., lo:hi] = c['xd'][..., lo:hi]
    pc = _ops().PackedConv(c['wd'], stride, 1, groups=groups, pitch=c['Cp'])
    y1 = _ops().conv2d(x1, pc, scale=c['scaled'])
    assert float(y1[..., lo:hi].abs().max()) > 0 and int(torch.count_nonzero(y1[..., others])) == 0


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_bit_repeatable_and_batch_independent(shape):
    c = case(shape)
    runs = [(forward(c, affine=True), forward(c), dgrad(c), wgrad(c)) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    y, _, dx, _ = runs[0]
    x0, dy0 = c['xd'][0:1].contiguous(), c['dyd'][0:1].contiguous()
    assert torch.equal(forward(c, x=x0, affine=True)[0], y[0])            # image 0 of the batch equals its single-image run
    assert torch.equal(dgrad(c, dy=dy0)[0], dx[0])


def test_existing_width_keeps_its_variant_and_bits():
    """(3, 17, 24, 256, 8, 1), pitch == C: the call traces ('group', 8) through the entry point it always took, and the pitched entry
    point given Cp == C launches the same kernel -- the same bits."""
    import ctypes
    from pointtinybenchmark_amd import _lib
    ops = _ops()
    shape = (3, 17, 24, 256, 8, 1)
    c = G.make_case(shape)
    x, w, scale, bias = G.nhwc(c['x']).cuda(), c['w'].cuda(), c['scale'].cuda(), c['bias'].cuda()
    pc = ops.PackedConv(w, 1, 1, groups=c['groups'])
    assert pc.C == pc.Cin == pc.Cout == 256
    calls = []
    real = _lib.call

    def spy(name, *args, **kw):
        calls.append(name)
        return real(name, *args, **kw)
    ops.TRACE_CONV_VARIANT[0], ops.TRACE_CONV_VARIANT[1] = True, None
    _lib.call = spy
    try:
        got = ops.conv2d(x, pc, scale=scale, bias=bias, relu=True)
    finally:
        _lib.call = real
        ops.TRACE_CONV_VARIANT[0] = False
    assert ops.TRACE_CONV_VARIANT[1] == ('group', 8) and calls == ['cpr_conv_group_fwd'], (ops.TRACE_CONV_VARIANT[1], calls)
    ref, bar = G.fwd_ref(c['x'], c['w'], c['groups'], 1, c['scale'], c['bias'], True)
    check('grouped forward cg 8', _flat(got.cpu()), _flat(ref), _flat(bar))
    want = torch.empty_like(got)
    P, st = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    real('cpr_conv_group_fwd_pitch', P(x), P(pc.w), P(want), P(scale), P(bias), 3, 17, 24, 256, 256, 8, 1, 1, st)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ stem
STEM = [(2, 7, 9), (1, 33, 66), (2, 70, 90), (1, 67, 93)]


@functools.lru_cache(maxsize=None)
def stem_case(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(300 + H)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn((B, 3, H, W), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) * (2.0 / 27) ** 0.5
    scale = (torch.rand((32,), generator=g) + 0.5) * torch.where(torch.rand((32,), generator=g) < 0.25, -1.0, 1.0)
    bias = torch.randn((32,), generator=g) * 0.3
    dy = torch.randn((B, OH, OW, 32), generator=g)            # zero-mean (tests/wgrad_fp64_ref.py says why)
    x4 = torch.zeros((B, H, W, 4))
    x4[..., :3] = x.permute(0, 2, 3, 1)
    return dict(x=x, x4=x4, w=w, scale=scale, bias=bias, dy=dy, OH=OH, OW=OW)


@pytest.mark.parametrize('shape', STEM, ids=['b%d_%dx%d' % s for s in STEM])
def test_stem_forward_both_layouts(shape):
    ops = _ops()
    c = stem_case(shape)
    pc = ops.PackedConv(c['w'].cuda(), 2, 1)
    s, b = c['scale'].cuda(), c['bias'].cuda()
    planar = ops.stem3x3s2(c['x'].cuda(), pc, s, b, planar=True)
    nhwc4 = ops.stem3x3s2(c['x4'].cuda(), pc, s, b, planar=False)
    assert tuple(planar.shape) == (shape[0], c['OH'], c['OW'], 32) and torch.equal(planar, nhwc4)
    m = np.arange(shape[0] * c['OH'] * c['OW'])
    r = CF.reference(c['x4'], c['w'], 2, 1, m, scale=c['scale'], bias=c['bias'], relu=True)
    assert r['out_hw'] == (c['OH'], c['OW'])
    worst = check('stem3x3s2 forward %s' % (shape,), _flat(planar.cpu()), r['ref'], CF.out_bar(r, False), m=m, OHW=r['out_hw'])
    print('stem forward %s: worst |err| / bar = %.3g' % (shape, worst))


@pytest.mark.parametrize('shape', STEM, ids=['b%d_%dx%d' % s for s in STEM])
def test_stem_weight_gradient_both_layouts(shape):
    ops = _ops()
    c = stem_case(shape)
    dy = c['dy'].cuda()
    a = ops.stem3x3s2_wgrad(dy, c['x'].cuda(), planar=True)
    b = ops.stem3x3s2_wgrad(dy, c['x4'].cuda(), planar=False)
    assert tuple(a.shape) == (32, 3, 3, 3) and torch.equal(a, b) and torch.equal(a, ops.stem3x3s2_wgrad(dy, c['x'].cuda(), planar=True))
    r = WF.reference(c['dy'], c['x4'][..., :3], 3, 2, 1)
    worst = check('stem3x3s2 wgrad %s' % (shape,), a.cpu().reshape(32, -1), r['ref'].reshape(32, -1), WF.bar_fp32(r).reshape(32, -1))
    print('stem wgrad %s: worst |err| / bar = %.3g' % (shape, worst))


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from pointtinybenchmark_amd import _lib
    ops = _ops()
    w = torch.zeros((96, 48, 3, 3), device='cuda')
    with pytest.raises(AssertionError, match='grouped conv'):
        ops.PackedConv(torch.zeros((100, 50, 3, 3), device='cuda'), 1, 1, groups=2)            # cg 50
    with pytest.raises(AssertionError, match='pitch'):
        ops.PackedConv(w, 1, 1, groups=2, pitch=64)                                             # pitch < C
    with pytest.raises(AssertionError, match='pitch'):
        ops.PackedConv(w, 1, 1, groups=2, pitch=98)
    with pytest.raises(NotImplementedError, match='groups=2'):
        ops.PackedConv(w, 1, 1, torch.bfloat16, groups=2, pitch=96)
    pc = ops.PackedConv(torch.zeros((72, 24, 3, 3), device='cuda'), 1, 1, groups=3, pitch=96)
    with pytest.raises(AssertionError):
        ops.conv2d(torch.zeros((1, 4, 4, 96), device='cuda', dtype=torch.bfloat16), pc)
    with pytest.raises(AssertionError):
        ops.conv2d(torch.zeros((1, 4, 4, 72), device='cuda'), pc)                                # the map is not at the pack's pitch
    with pytest.raises(AssertionError):
        ops.conv2d_wgrad(torch.zeros((1, 4, 4, 96), device='cuda', dtype=torch.bfloat16), torch.zeros((1, 4, 4, 96), device='cuda'),
                         (72, 24, 3, 3), 1, 1, groups=3)
    # the C ABI itself: C % cg, pitch < C, pitch % 4
    import ctypes
    P, st = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, o = torch.zeros((1, 4, 4, 96), device='cuda'), torch.zeros((1, 4, 4, 96), device='cuda')
    for C, Cp, cg in ((80, 96, 48), (72, 64, 24), (72, 74, 24), (72, 96, 12), (128, 128, 64)):
        with pytest.raises(_lib.CprHipError, match='invalid argument'):
            _lib.call('cpr_conv_group_fwd_pitch', P(x), P(pc.w), P(o), None, None, 1, 4, 4, C, Cp, cg, 1, 0, st)
        with pytest.raises(_lib.CprHipError, match='invalid argument'):
            _lib.call('cpr_conv_group_wgrad_pitch', P(x), P(x), P(o), P(o), 1, 4, 4, C, Cp, cg, 1, 0, st)
    with pytest.raises(AssertionError):
        ops.stem3x3s2_wgrad(torch.zeros((1, 4, 4, 64), device='cuda'), torch.zeros((1, 3, 8, 8), device='cuda'))
