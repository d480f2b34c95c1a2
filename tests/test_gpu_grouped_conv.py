"""-m gpu: the grouped 3x3 convolution kernels (csrc/conv_group.hip) through ops.conv2d / conv2d_dgrad / conv2d_wgrad against the fp64
references and bars of tests/grouped_conv_ref.py, on the smallest shapes at which a tile edge, a group boundary or a stride can go
wrong; exact group isolation; bit-repeatability; batch independence; and the dense (groups == 1) dispatch left where it was."""
import functools

import pytest
import torch

from tests import grouped_conv_ref as G
from tests.conv_fp64_ref import check

pytestmark = pytest.mark.gpu

IDS = [G.shape_id(s) for s in G.SHAPES]


@functools.lru_cache(maxsize=None)
def case(shape):
    """The operands of one shape, CPU masters and their device copies (NHWC maps), shared by every test and left unchanged."""
    c = G.make_case(shape)
    dev = torch.device('cuda')
    c['xd'] = G.nhwc(c['x']).to(dev)
    c['dyd'] = G.nhwc(c['dy']).to(dev)
    c['wd'] = c['w'].to(dev)
    c['scaled'] = c['scale'].to(dev)
    c['biasd'] = c['bias'].to(dev)
    return c


def _ops():
    from pointtinybenchmark_amd import ops
    return ops


def forward(c, x=None, w=None, affine=False):
    ops = _ops()
    pc = ops.PackedConv(c['wd'] if w is None else w, c['stride'], 1, groups=c['groups'])
    x = c['xd'] if x is None else x
    if affine:
        return ops.conv2d(x, pc, scale=c['scaled'], bias=c['biasd'], relu=True)
    return ops.conv2d(x, pc)


def dgrad(c, dy=None, w=None, scaled=True):
    ops = _ops()
    H, W = c['shape'][1:3]
    pt = ops.dgrad_pack(c['wd'] if w is None else w, c['stride'], 1, scale=c['scaled'] if scaled else None, groups=c['groups'])
    assert isinstance(pt, ops.PackedConv) and pt.groups == c['groups']
    return ops.conv2d_dgrad(c['dyd'] if dy is None else dy, pt, (H, W), c['stride'])


def wgrad(c, dy=None, x=None):
    ops = _ops()
    return ops.conv2d_wgrad(c['dyd'] if dy is None else dy, c['xd'] if x is None else x, tuple(c['w'].shape), c['stride'], 1,
                            groups=c['groups'])


def _flat(t):
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize('affine', [False, True], ids=['raw', 'scale_bias_relu'])
@pytest.mark.parametrize('shape', G.SHAPES, ids=IDS)
def test_forward_within_bar(shape, affine):
    c = case(shape)
    got = forward(c, affine=affine).cpu()
    ref, bar = G.fwd_ref(c['x'], c['w'], c['groups'], c['stride'], *((c['scale'], c['bias'], True) if affine else ()))
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('grouped forward %s' % G.shape_id(shape), _flat(got), _flat(ref), _flat(bar))
    print('forward %s %s: worst |err| / bar = %.3g' % (G.shape_id(shape), 'affine' if affine else 'raw', worst))


@pytest.mark.parametrize('scaled', [False, True], ids=['raw', 'bn_scale'])
@pytest.mark.parametrize('shape', G.SHAPES, ids=IDS)
def test_data_gradient_within_bar(shape, scaled):
    c = case(shape)
    H, W = shape[1:3]
    got = dgrad(c, scaled=scaled).cpu()
    ref, bar = G.dgrad_ref(c['dy'], c['w'], c['groups'], c['stride'], (H, W), c['scale'] if scaled else None)
    assert tuple(got.shape) == tuple(ref.shape) == (shape[0], H, W, shape[3])
    worst = check('grouped dgrad %s' % G.shape_id(shape), _flat(got), _flat(ref), _flat(bar))
    print('dgrad %s: worst |err| / bar = %.3g' % (G.shape_id(shape), worst))


@pytest.mark.parametrize('shape', G.SHAPES, ids=IDS)
def test_weight_gradient_within_bar(shape):
    c = case(shape)
    got = wgrad(c).cpu()
    ref, bar = G.wgrad_ref(c['dy'], c['x'], c['w'].shape, c['groups'], c['stride'])
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('grouped wgrad %s' % G.shape_id(shape), got.reshape(shape[3], -1), ref.reshape(shape[3], -1), bar.reshape(shape[3], -1))
    print('wgrad %s: worst |err| / bar = %.3g' % (G.shape_id(shape), worst))
    # accumulation into an existing gradient: one more rounded addition
    base = torch.randn(tuple(c['w'].shape), generator=torch.Generator().manual_seed(5))
    acc = base.cuda()
    _ops().conv2d_wgrad(c['dyd'], c['xd'], tuple(c['w'].shape), c['stride'], 1, grad=acc, groups=c['groups'])
    assert torch.equal(acc.cpu(), base + got)


@pytest.mark.parametrize('shape', G.SHAPES, ids=IDS)
def test_group_isolation_is_exact(shape):
    c = case(shape)
    N, H, W, C, cg, stride = shape
    groups = c['groups']
    k = groups // 3                                  # the group that is singled out
    lo, hi = k * cg, (k + 1) * cg
    others = torch.ones(C, dtype=torch.bool)
    others[lo:hi] = False
    # (a) input non-zero in one group's channels only, no bias: every output channel of every other group is exactly 0
    x1 = torch.zeros_like(c['xd'])
    x1[..., lo:hi] = c['xd'][..., lo:hi]
    pc = _ops().PackedConv(c['wd'], stride, 1, groups=groups)
    y1 = _ops().conv2d(x1, pc, scale=c['scaled'])
    assert float(y1[..., lo:hi].abs().max()) > 0
    assert int(torch.count_nonzero(y1[..., others.cuda()])) == 0
    dy1 = torch.zeros_like(c['dyd'])
    dy1[..., lo:hi] = c['dyd'][..., lo:hi]
    dx1 = dgrad(c, dy=dy1)
    assert float(dx1[..., lo:hi].abs().max()) > 0
    assert int(torch.count_nonzero(dx1[..., others.cuda()])) == 0
    dw1 = wgrad(c, dy=dy1)
    assert float(dw1[lo:hi].abs().max()) > 0
    assert int(torch.count_nonzero(dw1[others.cuda()])) == 0
    # (b) another set of weights (maps) in one group leaves every other group's results bit-equal
    w2 = c['wd'].clone()
    w2[lo:hi] = w2[lo:hi] * 1.5 + 0.25
    y, y2 = forward(c, affine=True), forward(c, w=w2, affine=True)
    assert not torch.equal(y[..., lo:hi], y2[..., lo:hi])
    assert torch.equal(y[..., others.cuda()], y2[..., others.cuda()])
    dx, dx2 = dgrad(c), dgrad(c, w=w2)
    assert not torch.equal(dx[..., lo:hi], dx2[..., lo:hi])
    assert torch.equal(dx[..., others.cuda()], dx2[..., others.cuda()])
    xm, dym = c['xd'].clone(), c['dyd'].clone()
    xm[..., lo:hi] = xm[..., lo:hi] * 0.5 - 1.0
    dym[..., lo:hi] = -dym[..., lo:hi]
    dw, dw2 = wgrad(c), wgrad(c, dy=dym, x=xm)
    assert not torch.equal(dw[lo:hi], dw2[lo:hi])
    assert torch.equal(dw[others.cuda()], dw2[others.cuda()])


@pytest.mark.parametrize('shape', G.SHAPES, ids=IDS)
def test_bit_repeatable_and_batch_independent(shape):
    c = case(shape)
    N = shape[0]
    runs = [(forward(c, affine=True), forward(c), dgrad(c), wgrad(c)) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    if N >= 2:
        # image 1 of the batch equals its single-image run, forward and data gradient
        y, _, dx, _ = runs[0]
        x1, dy1 = c['xd'][1:2].contiguous(), c['dyd'][1:2].contiguous()
        assert torch.equal(forward(c, x=x1, affine=True)[0], y[1])
        assert torch.equal(dgrad(c, dy=dy1)[0], dx[1])


@pytest.mark.parametrize('dense', [(2, 40, 40, 64, 64, 3, 1, 1), (2, 20, 20, 128, 128, 3, 2, 1)], ids=['wino_3x3', 'direct_3x3_s2'])
def test_dense_calls_keep_their_path_and_bits(dense, monkeypatch):
    """groups == 1: ops.conv2d reaches the entry point it reached before the grouped kernels existed, with the arguments it passed
    then -- the result equals that entry point called directly -- and no grouped entry point is called."""
    import ctypes
    from pointtinybenchmark_amd import _lib
    ops = _ops()
    N, H, W, Cin, Cout, k, s, p = dense
    g = torch.Generator().manual_seed(3)
    x = torch.randn((N, H, W, Cin), generator=g).cuda()
    w = (torch.randn((Cout, Cin, k, k), generator=g) * 0.05).cuda()
    scale, bias = (torch.rand((Cout,), generator=g) + 0.5).cuda(), torch.randn((Cout,), generator=g).cuda()
    pc = ops.PackedConv(w, s, p)
    assert pc.groups == 1 and tuple(pc.w.shape) == (Cout, 9 * Cin)
    calls = []
    real = _lib.call

    def spy(name, *args, **kw):
        calls.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, 'call', spy)
    got = ops.conv2d(x, pc, scale=scale, bias=bias, relu=True)
    monkeypatch.setattr(_lib, 'call', real)
    assert not [n for n in calls if 'group' in n], calls
    OH, OW = pc.out_hw(H, W)
    want = torch.empty((N, OH, OW, Cout), device='cuda')
    P, st = (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if dense[5:] == (3, 1, 1):        # Winograd-eligible: the 8 x 16-region kernel on a 40 x 40 map (ops.WINO_AUTO)
        assert calls == ['cpr_wino32_pack_weights', 'cpr_conv3x3_wino32_fwd'], calls
        real('cpr_conv3x3_wino32_fwd', P(x), P(pc.wino32), P(want), P(scale), P(bias), None, None, None, N, H, W, Cin, Cout, 1, 0, 0, st)
    else:
        assert calls == ['cpr_conv2d_fwd'], calls
        real('cpr_conv2d_fwd', P(x), P(pc.w), P(want), P(scale), P(bias), None, None, None, None, N, H, W, Cin, Cout, k, k, s, p, pc.Kpad,
             1, 0, None, st)
    assert torch.equal(got, want)
    # and the dense pack is the image the dense pack kernel wrote
    ref_pack = torch.empty_like(pc.w)
    real('cpr_pack_weights', P(w), None, P(ref_pack), Cout, Cin, k, k, Cin, pc.Kpad, 0, st)
    assert torch.equal(pc.w, ref_pack)
