"""-m gpu: the dilated 3x3 convolution kernels through ops.conv2d / conv2d_dgrad / conv2d_wgrad against the fp64 references and bars
of tests/dilated_conv_ref.py -- dense (cpr_conv2d_fwd_dil: every epilogue it takes, both tiles the launcher chooses;
cpr_conv2d_wgrad_dil: written, accumulated, many slabs) and grouped (cpr_conv_group_fwd_dil / _wgrad_dil: exact group isolation,
bit-repeatability, batch independence) -- every output element of the small maps; every new entry at dil = 1 against the old entry,
bit for bit; and the CPR_ERR_ARG cases, which return before any launch."""
import ctypes
import functools

import pytest
import torch

from tests import dilated_conv_ref as D
from tests.conv_fp64_ref import check, sample_pixels

pytestmark = pytest.mark.gpu

DENSE_IDS = [D.dense_id(s) for s in D.DENSE]
GROUPED_IDS = [D.grouped_id(s) for s in D.GROUPED]
ERR_ARG = -1001


def _ops():
    from pointtinybenchmark_amd import ops
    return ops


def _flat(t):
    return t.reshape(-1, t.shape[-1])


@functools.lru_cache(maxsize=None)
def dense(shape):
    """The operands of one dense shape, CPU masters and their device copies (NHWC maps), shared by every test and left unchanged."""
    c = D.make_dense(shape)
    for k in ('x', 'res', 'dy'):
        c[k + 'd'] = D.nhwc(c[k]).cuda()
    for k in ('w', 'scale', 'bias'):
        c[k + 'd'] = c[k].cuda()
    return c


@functools.lru_cache(maxsize=None)
def grouped(shape):
    c = D.make_grouped(shape)
    for k in ('x', 'dy'):
        c[k + 'd'] = D.nhwc(c[k]).cuda()
    for k in ('w', 'scale', 'bias'):
        c[k + 'd'] = c[k].cuda()
    return c


def _traced(fn):
    """fn() with the launched instance's variant word."""
    ops = _ops()
    ops.TRACE_CONV_VARIANT[0], ops.TRACE_CONV_VARIANT[1] = True, None
    try:
        out = fn()
        return out, ops.TRACE_CONV_VARIANT[1]
    finally:
        ops.TRACE_CONV_VARIANT[0] = False


# ---------------------------------------------------------------------------------------------------------------- dense forward
EPILOGUES = ['raw', 'scale_bias_relu', 'residual', 'mask_colsum']


@pytest.mark.parametrize('epi', EPILOGUES)
@pytest.mark.parametrize('shape', D.DENSE, ids=DENSE_IDS)
def test_dense_forward_within_bar(shape, epi):
    ops = _ops()
    c = dense(shape)
    d = c['d']
    pc = ops.PackedConv(c['wd'], 1, d, dilation=d)
    assert pc.dilation == d and not ops.wino_eligible(pc, shape[1], shape[2])
    if epi == 'raw':
        got, var = _traced(lambda: ops.conv2d(c['xd'], pc))
        ref, bar = D.dense_fwd_ref(c['x'], c['w'], d)
    elif epi == 'scale_bias_relu':
        got, var = _traced(lambda: ops.conv2d(c['xd'], pc, scale=c['scaled'], bias=c['biasd'], relu=True))
        ref, bar = D.dense_fwd_ref(c['x'], c['w'], d, c['scale'], c['bias'], relu=True)
    elif epi == 'residual':
        got, var = _traced(lambda: ops.conv2d(c['xd'], pc, scale=c['scaled'], bias=c['biasd'], residual=c['resd'], relu=True))
        ref, bar = D.dense_fwd_ref(c['x'], c['w'], d, c['scale'], c['bias'], c['res'], relu=True)
    else:
        (got, part), var = _traced(lambda: ops.conv2d(c['xd'], pc, scale=c['scaled'], residual=c['resd'], res_mask=True, colsum=True))
        ref, bar = D.dense_fwd_ref(c['x'], c['w'], d, c['scale'], None, c['res'], res_mask=True)
        cs_ref, cs_bar = D.colsum_ref(ref, bar)
        w = check('dilated colsum %s' % D.dense_id(shape), part.reduce().cpu().view(1, -1), cs_ref.view(1, -1), cs_bar.view(1, -1))
        print('colsum %s: worst |err| / bar = %.3g' % (D.dense_id(shape), w))
    assert var == ('fp32_dil', 64064001), var          # the tile rule sends every small launch to <64, 64>
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('dilated forward %s %s' % (D.dense_id(shape), epi), _flat(got.cpu()), _flat(ref), _flat(bar), bm=64,
                  OHW=(shape[1], shape[2]))
    print('forward %s %s: worst |err| / bar = %.3g' % (D.dense_id(shape), epi, worst))


def test_dense_forward_large_tile_within_bar():
    """The <128, 128> instance: long K, wide, 4096 tiles.  Sampled pixels: every border, the last tile, random ones."""
    ops = _ops()
    N, H, W, Cin, Cout, d = D.BIG_TILE
    g = torch.Generator().manual_seed(7)
    x = torch.randn((N, H, W, Cin), generator=g).cuda()
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (2.0 / (9 * Cin)) ** 0.5
    scale, bias = torch.rand((Cout,), generator=g) + 0.5, torch.randn((Cout,), generator=g) * 0.3
    pc = ops.PackedConv(w.cuda(), 1, d, dilation=d)
    got, var = _traced(lambda: ops.conv2d(x, pc, scale=scale.cuda(), bias=bias.cuda(), relu=True))
    assert var == ('fp32_dil', 128128001), var
    m, _ = sample_pixels(N, H, W, 128)
    ref, bar = D.sampled_fwd_ref(x, w, d, m, scale, bias, relu=True)
    worst = check('dilated forward <128,128>', _flat(got)[torch.as_tensor(m, device='cuda')].cpu(), ref, bar, m=m, bm=128, OHW=(H, W))
    print('forward <128,128> %s: worst |err| / bar = %.3g over %d pixels' % (D.dense_id(D.BIG_TILE), worst, len(m)))


# ---------------------------------------------------------------------------------------------------------- dense data gradient
@pytest.mark.parametrize('scaled', [False, True], ids=['raw', 'bn_scale'])
@pytest.mark.parametrize('shape', D.DENSE, ids=DENSE_IDS)
def test_dense_data_gradient_within_bar(shape, scaled):
    ops = _ops()
    c = dense(shape)
    N, H, W, Cin, Cout, d = shape
    pt = ops.dgrad_pack(c['wd'], 1, d, scale=c['scaled'] if scaled else None, dilation=d)
    assert isinstance(pt, ops.PackedConv) and pt.dilation == d and pt.padding == d and pt.stride == 1
    got = ops.conv2d_dgrad(c['dyd'], pt, (H, W), 1)
    ref, bar = D.dense_dgrad_ref(c['dy'], c['w'], d, c['scale'] if scaled else None)
    assert tuple(got.shape) == tuple(ref.shape) == (N, H, W, Cin)
    worst = check('dilated dgrad %s' % D.dense_id(shape), _flat(got.cpu()), _flat(ref), _flat(bar), bm=64, OHW=(H, W))
    print('dgrad %s %s: worst |err| / bar = %.3g' % (D.dense_id(shape), 'scaled' if scaled else 'raw', worst))


# -------------------------------------------------------------------------------------------------------- dense weight gradient
def _check_wgrad(name, c, shape):
    ops = _ops()
    N, H, W, Cin, Cout, d = shape
    got = ops.conv2d_wgrad(c['dyd'], c['xd'], (Cout, Cin, 3, 3), 1, d, dilation=d).cpu()
    ref, bar = D.wgrad_ref(c['dy'], c['x'], (Cout, Cin, 3, 3), d)
    worst = check(name, got.reshape(Cout, -1), ref.reshape(Cout, -1), bar.reshape(Cout, -1))
    print('%s: worst |err| / bar = %.3g' % (name, worst))
    # accumulated into an existing tensor: the same sum, one more rounded addition
    base = torch.randn((Cout, Cin, 3, 3), generator=torch.Generator().manual_seed(5))
    acc = base.cuda()
    ops.conv2d_wgrad(c['dyd'], c['xd'], (Cout, Cin, 3, 3), 1, d, grad=acc, dilation=d)
    assert torch.equal(acc.cpu(), base + got)
    # written into a given tensor
    out = torch.full((Cout, Cin, 3, 3), float('nan'), device='cuda')
    assert ops.conv2d_wgrad(c['dyd'], c['xd'], (Cout, Cin, 3, 3), 1, d, out=out, dilation=d) is out and torch.equal(out.cpu(), got)


@pytest.mark.parametrize('shape', D.DENSE, ids=DENSE_IDS)
def test_dense_weight_gradient_within_bar(shape):
    _check_wgrad('dilated wgrad %s' % D.dense_id(shape), dense(shape), shape)


def test_dense_weight_gradient_with_many_slabs():
    from pointtinybenchmark_amd import _lib
    N, H, W, Cin, Cout, d = D.WGRAD_SLABS
    floats = _lib.call('cpr_conv2d_wgrad_workspace', N, H, W, Cin, Cout, 3, 3, positive=True)
    slabs = floats // (Cout * 9 * Cin)
    chunks = N * H * W // 32
    assert slabs * Cout * 9 * Cin == floats and slabs > 1 and chunks > slabs, (floats, slabs, chunks)     # several chunks per slab
    _check_wgrad('dilated wgrad %s (%d slabs)' % (D.dense_id(D.WGRAD_SLABS), slabs), dense(D.WGRAD_SLABS), D.WGRAD_SLABS)


# --------------------------------------------------------------------------------------------------------------------- grouped
def g_forward(c, x=None, w=None, affine=False):
    ops = _ops()
    pc = ops.PackedConv(c['wd'] if w is None else w, 1, c['d'], groups=c['groups'], dilation=c['d'])
    x = c['xd'] if x is None else x
    return ops.conv2d(x, pc, scale=c['scaled'], bias=c['biasd'], relu=True) if affine else ops.conv2d(x, pc)


def g_dgrad(c, dy=None, w=None, scaled=True):
    ops = _ops()
    H, W = c['shape'][1:3]
    pt = ops.dgrad_pack(c['wd'] if w is None else w, 1, c['d'], scale=c['scaled'] if scaled else None, groups=c['groups'], dilation=c['d'])
    assert pt.groups == c['groups'] and pt.dilation == c['d'] and pt.padding == c['d']
    return ops.conv2d_dgrad(c['dyd'] if dy is None else dy, pt, (H, W), 1)


def g_wgrad(c, dy=None, x=None, **kw):
    return _ops().conv2d_wgrad(c['dyd'] if dy is None else dy, c['xd'] if x is None else x, tuple(c['w'].shape), 1, c['d'],
                               groups=c['groups'], dilation=c['d'], **kw)


@pytest.mark.parametrize('affine', [False, True], ids=['raw', 'scale_bias_relu'])
@pytest.mark.parametrize('shape', D.GROUPED, ids=GROUPED_IDS)
def test_grouped_forward_within_bar(shape, affine):
    c = grouped(shape)
    got = g_forward(c, affine=affine).cpu()
    ref, bar = D.grouped_fwd_ref(c['x'], c['w'], c['groups'], c['d'], *((c['scale'], c['bias'], True) if affine else ()))
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('dilated grouped forward %s' % D.grouped_id(shape), _flat(got), _flat(ref), _flat(bar))
    print('grouped forward %s %s: worst |err| / bar = %.3g' % (D.grouped_id(shape), 'affine' if affine else 'raw', worst))


@pytest.mark.parametrize('scaled', [False, True], ids=['raw', 'bn_scale'])
@pytest.mark.parametrize('shape', D.GROUPED, ids=GROUPED_IDS)
def test_grouped_data_gradient_within_bar(shape, scaled):
    c = grouped(shape)
    got = g_dgrad(c, scaled=scaled).cpu()
    ref, bar = D.grouped_dgrad_ref(c['dy'], c['w'], c['groups'], c['d'], c['scale'] if scaled else None)
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('dilated grouped dgrad %s' % D.grouped_id(shape), _flat(got), _flat(ref), _flat(bar))
    print('grouped dgrad %s: worst |err| / bar = %.3g' % (D.grouped_id(shape), worst))


@pytest.mark.parametrize('shape', D.GROUPED, ids=GROUPED_IDS)
def test_grouped_weight_gradient_within_bar(shape):
    c = grouped(shape)
    C = shape[3]
    got = g_wgrad(c).cpu()
    ref, bar = D.wgrad_ref(c['dy'], c['x'], c['w'].shape, c['d'], c['groups'])
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('dilated grouped wgrad %s' % D.grouped_id(shape), got.reshape(C, -1), ref.reshape(C, -1), bar.reshape(C, -1))
    print('grouped wgrad %s: worst |err| / bar = %.3g' % (D.grouped_id(shape), worst))
    base = torch.randn(tuple(c['w'].shape), generator=torch.Generator().manual_seed(5))
    acc = base.cuda()
    g_wgrad(c, grad=acc)
    assert torch.equal(acc.cpu(), base + got)


@pytest.mark.parametrize('shape', D.GROUPED, ids=GROUPED_IDS)
def test_grouped_isolation_repeatability_and_batch_independence(shape):
    c = grouped(shape)
    N, H, W, C, cg, d = shape
    k = c['groups'] // 3                                  # the group that is singled out
    lo, hi = k * cg, (k + 1) * cg
    others = torch.ones(C, dtype=torch.bool)
    others[lo:hi] = False
    others = others.cuda()
    # input / gradient non-zero in one group's channels only: every other group's results are exactly 0
    x1 = torch.zeros_like(c['xd'])
    x1[..., lo:hi] = c['xd'][..., lo:hi]
    dy1 = torch.zeros_like(c['dyd'])
    dy1[..., lo:hi] = c['dyd'][..., lo:hi]
    y1, dx1, dw1 = g_forward(c, x=x1), g_dgrad(c, dy=dy1), g_wgrad(c, dy=dy1)
    assert float(y1[..., lo:hi].abs().max()) > 0 and int(torch.count_nonzero(y1[..., others])) == 0
    assert float(dx1[..., lo:hi].abs().max()) > 0 and int(torch.count_nonzero(dx1[..., others])) == 0
    assert float(dw1[lo:hi].abs().max()) > 0 and int(torch.count_nonzero(dw1[others])) == 0
    # other weights in one group leave every other group's results bit-equal
    w2 = c['wd'].clone()
    w2[lo:hi] = w2[lo:hi] * 1.5 + 0.25
    y, y2 = g_forward(c, affine=True), g_forward(c, w=w2, affine=True)
    assert not torch.equal(y[..., lo:hi], y2[..., lo:hi]) and torch.equal(y[..., others], y2[..., others])
    dx, dx2 = g_dgrad(c), g_dgrad(c, w=w2)
    assert not torch.equal(dx[..., lo:hi], dx2[..., lo:hi]) and torch.equal(dx[..., others], dx2[..., others])
    # two runs are bit-equal; an image of a batch equals its single-image run
    dw = g_wgrad(c)
    assert torch.equal(y, g_forward(c, affine=True)) and torch.equal(dx, g_dgrad(c)) and torch.equal(dw, g_wgrad(c))
    n = N - 1
    xn, dyn = c['xd'][n:n + 1].contiguous(), c['dyd'][n:n + 1].contiguous()
    assert torch.equal(g_forward(c, x=xn, affine=True)[0], y[n])
    assert torch.equal(g_dgrad(c, dy=dyn)[0], dx[n])


# ------------------------------------------------------------------------------------------------- dil = 1: the old entries' bits
def _raw():
    from pointtinybenchmark_amd import _lib
    lib = _lib.load()
    P = (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None)
    return lib, P, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_dense_entries_at_dilation_1_equal_the_old_entries():
    ops = _ops()
    lib, P, st = _raw()
    N, H, W, Cin, Cout = 2, 13, 11, 64, 96
    g = torch.Generator().manual_seed(11)
    x = torch.randn((N, H, W, Cin), generator=g).cuda()
    dy = torch.randn((N, H, W, Cout), generator=g).cuda()
    res = torch.randn((N, H, W, Cout), generator=g).cuda()
    w = (torch.randn((Cout, Cin, 3, 3), generator=g) * 0.05).cuda()
    scale, bias = (torch.rand((Cout,), generator=g) + 0.5).cuda(), torch.randn((Cout,), generator=g).cuda()
    pc = ops.PackedConv(w, 1, 1)
    for flags, r in ((0, None), (1, res), (4 | 8, res)):
        a, b = torch.empty((N, H, W, Cout), device='cuda'), torch.empty((N, H, W, Cout), device='cuda')
        pa = pb = None
        if flags & 8:
            pa, pb = (torch.zeros(((N * H * W + 63) // 64, Cout, 2), device='cuda') for _ in range(2))
        va, vb = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.cpr_conv2d_fwd(P(x), P(pc.w), P(a), P(scale), P(bias), P(r), None, None, P(pa), N, H, W, Cin, Cout, 3, 3, 1, 1, pc.Kpad,
                                  flags, 0, ctypes.byref(va), st) == 0
        assert lib.cpr_conv2d_fwd_dil(P(x), P(pc.w), P(b), P(scale), P(bias), P(r), None, None, P(pb), N, H, W, Cin, Cout, 3, 3, 1, 1, 1,
                                      pc.Kpad, flags, 0, ctypes.byref(vb), st) == 0
        assert va.value == vb.value == 64064001 and torch.equal(a, b)
        assert pa is None or torch.equal(pa, pb)
    n = lib.cpr_conv2d_wgrad_workspace(N, H, W, Cin, Cout, 3, 3)
    ws = torch.empty((n,), device='cuda')
    ga, gb = torch.empty((Cout, Cin, 3, 3), device='cuda'), torch.empty((Cout, Cin, 3, 3), device='cuda')
    assert lib.cpr_conv2d_wgrad(P(dy), P(x), None, None, P(ga), P(ws), N, H, W, Cin, Cout, 3, 3, 1, 1, 0, 0, st) == 0
    assert lib.cpr_conv2d_wgrad_dil(P(dy), P(x), P(gb), P(ws), N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 0, st) == 0
    assert torch.equal(ga, gb)
    # ... and through ops: dilation=1 keeps the route (Winograd-eligible layers included) and the bits
    assert torch.equal(ops.conv2d_wgrad(dy, x, (Cout, Cin, 3, 3), 1, 1, dilation=1), ops.conv2d_wgrad(dy, x, (Cout, Cin, 3, 3), 1, 1))
    assert torch.equal(ops.conv2d(x, ops.PackedConv(w, 1, 1, dilation=1), scale=scale), ops.conv2d(x, pc, scale=scale))


def test_grouped_entries_at_dilation_1_equal_the_old_entries():
    ops = _ops()
    lib, P, st = _raw()
    N, H, W, C, cg = 2, 9, 12, 64, 16
    g = torch.Generator().manual_seed(12)
    x = torch.randn((N, H, W, C), generator=g).cuda()
    dy = torch.randn((N, H, W, C), generator=g).cuda()
    w = (torch.randn((C, cg, 3, 3), generator=g) * 0.1).cuda()
    scale, bias = (torch.rand((C,), generator=g) + 0.5).cuda(), torch.randn((C,), generator=g).cuda()
    pc = ops.PackedConv(w, 1, 1, groups=C // cg)
    a, b = torch.empty_like(x), torch.empty_like(x)
    assert lib.cpr_conv_group_fwd(P(x), P(pc.w), P(a), P(scale), P(bias), N, H, W, C, cg, 1, 1, st) == 0
    assert lib.cpr_conv_group_fwd_dil(P(x), P(pc.w), P(b), P(scale), P(bias), N, H, W, C, cg, 1, 1, st) == 0
    assert torch.equal(a, b)
    n = lib.cpr_conv_group_wgrad_workspace(N, H, W, C, cg)
    ws = torch.empty((n,), device='cuda')
    ga, gb = torch.empty_like(w), torch.empty_like(w)
    assert lib.cpr_conv_group_wgrad(P(dy), P(x), P(ga), P(ws), N, H, W, C, cg, 1, 0, st) == 0
    assert lib.cpr_conv_group_wgrad_dil(P(dy), P(x), P(gb), P(ws), N, H, W, C, cg, 1, 0, st) == 0
    assert torch.equal(ga, gb)


# --------------------------------------------------------------------------------------------------------------- CPR_ERR_ARG
def test_bad_arguments_return_err_arg_before_any_launch():
    """Geometry and operands the dilated entries have no instance for: the code comes back and the output buffer keeps its sentinel
    (nothing was launched)."""
    ops = _ops()
    lib, P, st = _raw()
    N, H, W, Cin, Cout, d = 1, 6, 6, 32, 32, 2
    x = torch.randn((N, H, W, Cin), device='cuda')
    w = torch.randn((Cout, Cin, 3, 3), device='cuda')
    pc = ops.PackedConv(w, 1, d, dilation=d)
    ab = torch.ones((N, Cin), device='cuda')
    part = torch.zeros((4, Cout, 2), device='cuda')
    out = torch.full((N, H, W, Cout), 7.0, device='cuda')

    def fwd(stride=1, pad=d, dil=d, flags=0, in_a=None, in_b=None, gn=None, in_relu=0, k=3, kpad=pc.Kpad):
        return lib.cpr_conv2d_fwd_dil(P(x), P(pc.w), P(out), None, None, None, P(in_a), P(in_b), P(gn), N, H, W, Cin, Cout, k, k, stride,
                                      pad, dil, kpad, flags, in_relu, None, st)
    bad = dict(stride=fwd(stride=2), pad=fwd(pad=1), pad0=fwd(pad=3), in_ab=fwd(in_a=ab, in_b=ab), in_relu=fwd(in_relu=1),
               gn_partials=fwd(gn=part), bf16_out=fwd(flags=2), colsum_without_slots=fwd(flags=8), mask_without_source=fwd(flags=4),
               dil0=fwd(dil=0, pad=0), k1=fwd(k=1, kpad=Cin), unknown_flag=fwd(flags=16))
    assert all(rc == ERR_ARG for rc in bad.values()), bad
    n = lib.cpr_conv2d_wgrad_workspace(N, H, W, Cin, Cout, 3, 3)
    ws = torch.empty((n,), device='cuda')
    gw = torch.full((Cout, Cin, 3, 3), 7.0, device='cuda')
    dy = torch.randn((N, H, W, Cout), device='cuda')
    assert lib.cpr_conv2d_wgrad_dil(P(dy), P(x), P(gw), P(ws), N, H, W, Cin, Cout, 3, 3, 1, d, 0, 0, st) == ERR_ARG
    assert lib.cpr_conv2d_wgrad_dil(P(dy), P(x), P(gw), P(ws), N, 2, 2, Cin, Cout, 3, 3, 1, 0, d, 0, st) == ERR_ARG      # no output pixel
    assert lib.cpr_conv2d_wgrad_dil(P(dy), P(x), None, P(ws), N, H, W, Cin, Cout, 3, 3, 1, d, d, 0, st) == ERR_ARG
    C, cg = 32, 4
    xg = torch.randn((N, H, W, C), device='cuda')
    wg = torch.randn((C, cg, 3, 3), device='cuda')
    pg = ops.PackedConv(wg, 1, d, groups=C // cg, dilation=d)
    og = torch.full((N, H, W, C), 7.0, device='cuda')
    assert lib.cpr_conv_group_fwd_dil(P(xg), P(pg.w), P(og), None, None, N, H, W, C, cg, 0, 0, st) == ERR_ARG
    assert lib.cpr_conv_group_fwd_dil(P(xg), P(pg.w), P(og), None, None, N, H, W, C, cg, d, 4, st) == ERR_ARG      # a flag beyond ReLU
    assert lib.cpr_conv_group_fwd_dil(P(xg), P(pg.w), P(og), None, None, N, H, W, C, 12, d, 0, st) == ERR_ARG      # no such group width
    gg = torch.full((C, cg, 3, 3), 7.0, device='cuda')
    wsg = torch.empty((lib.cpr_conv_group_wgrad_workspace(N, H, W, C, cg),), device='cuda')
    assert lib.cpr_conv_group_wgrad_dil(P(xg), P(xg), P(gg), P(wsg), N, H, W, C, cg, 0, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    for t in (out, gw, og, gg):
        assert bool((t == 7.0).all())
    # the Python layer refuses the same operands by name
    with pytest.raises(AssertionError, match='dilat'):
        ops.conv2d(x, pc, in_ab=(ab, ab))
    with pytest.raises(AssertionError, match='dilat'):
        ops.conv2d(x, pc, out_dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        ops.conv2d(x, pc, out_b8=True)
    with pytest.raises(AssertionError, match='dilat'):
        ops.conv2d(x, pc, gn_part=True)
