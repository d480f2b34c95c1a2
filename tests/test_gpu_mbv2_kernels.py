"""-m gpu: the MobileNetV2 kernels (csrc/mbv2.hip) through ops.DwPack / dw_conv / dw_dgrad / dw_wgrad / relu6_bwd_colsum / clamp6 on
maps at pitch roundup(C, 32), per element against the fp64 references and bars of tests/mobilenet_v2_ref.py.

  forward           raw and scale / bias / relu6, with and without in_clamp6
  data gradient     raw, scaled, mask6, add, colsum (the column sums at their own bar)
  weight gradient   plain (with and without in_clamp6) and accumulate: acc == base + got exactly
  relu6_bwd_colsum  and clamp6: exact against torch, the column sums at the bar
  pad channels      NaN in the pad of every input changes no output bit; the forward, the data gradient (every mode), the weight
                    gradient and relu6_bwd_colsum write into NaN-prefilled outputs (``out=``), which come back with every real element
                    written and every pad element bit-zero
  bit-repeatability, batch independence (image k of N equals its single-image run), argument errors (C % 8, stride 3, an undefined flag)
The worst |err| / bar per kernel is printed (DESIGN.md quotes it)."""
import functools

import pytest
import torch

from tests import mobilenet_v2_ref as M
from tests.conv_fp64_ref import check

pytestmark = pytest.mark.gpu

IDS = [M.shape_id(s) for s in M.SHAPES]
NAN = float('nan')
WORST = {}


def _ops():
    from pointtinybenchmark_amd import ops
    return ops


def note(kernel, worst):
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print('worst |err| / bar  %-18s %.3f' % (kernel, WORST[kernel]))


def padded(t_nchw, Cp, fill):
    """CPU NCHW master -> device NHWC map at pitch Cp, pad channels = fill."""
    t = M.nhwc(t_nchw)
    out = torch.full(tuple(t.shape[:3]) + (Cp,), fill, dtype=torch.float32)
    out[..., :t.shape[3]] = t
    return out.cuda()


@functools.lru_cache(maxsize=None)
def case(shape):
    """The operands of one shape, CPU masters and their device copies (NaN in the pad channels), shared by every test, left unchanged."""
    c = M.make_case(shape, seed=5)
    C = shape[3]
    c['C'], c['Cp'] = C, (C + 31) // 32 * 32
    for k in ('x', 'm', 'dy', 'g', 'add'):
        c[k + 'd'] = padded(c[k], c['Cp'], NAN)
    for k in ('w', 'scale', 'bias', 'base'):
        c[k + 'd'] = c[k].cuda()
    return c


def real(c, t):
    """The real channels of a device NHWC map as a CPU (P, C) matrix; the pad must be bit-zero."""
    C = c['C']
    pad = t[..., C:]
    assert pad.numel() == 0 or bool((pad.contiguous().view(torch.int32) == 0).all()), 'pad channels are not +0.0'
    r = t[..., :C].cpu()
    assert not bool(torch.isnan(r).any()), 'an element was not written (or read a pad channel)'
    return r.reshape(-1, C)


def flat(t):
    return t.reshape(-1, t.shape[-1])


def fwd(c, affine, clamp, x=None):
    ops = _ops()
    H, W = c['shape'][1:3]
    x = c['xd'] if x is None else x
    out = torch.full((x.shape[0],) + M.out_hw(H, W, c['stride']) + (c['Cp'],), NAN, dtype=torch.float32, device='cuda')
    pack = ops.DwPack(c['wd'])
    if affine:
        return ops.dw_conv(x, pack, c['stride'], scale=c['scaled'], bias=c['biasd'], in_clamp6=clamp, relu6=True, out=out)
    return ops.dw_conv(x, pack, c['stride'], in_clamp6=clamp, out=out)


@pytest.mark.parametrize('shape', M.SHAPES, ids=IDS)
@pytest.mark.parametrize('affine', [False, True], ids=['raw', 'bn_relu6'])
@pytest.mark.parametrize('clamp', [False, True], ids=['asis', 'in_clamp6'])
def test_forward(shape, affine, clamp):
    c = case(shape)
    got = fwd(c, affine, clamp)
    ref, bar = M.dw_fwd_ref(c['x'], c['w'], c['stride'], c['scale'] if affine else None, c['bias'] if affine else None, clamp, affine)
    note('dw3x3_fwd', check('forward', real(c, got), flat(ref), flat(bar)))
    assert torch.equal(got.view(torch.int32), fwd(c, affine, clamp).view(torch.int32)), 'not bit-repeatable'


@pytest.mark.parametrize('shape', M.SHAPES, ids=IDS)
@pytest.mark.parametrize('mode', ['raw', 'scaled', 'mask6', 'add', 'add_mask6_colsum'])
def test_data_gradient(shape, mode):
    ops = _ops()
    c = case(shape)
    H, W = shape[1:3]
    scaled = mode != 'raw'
    mask = 'mask6' in mode
    add = 'add' in mode
    colsum = 'colsum' in mode
    pack = ops.DwPack(c['wd'], c['scaled'] if scaled else None)

    def run(dy=c['dyd'], m=c['md'], a=c['addd']):
        out = torch.full((dy.shape[0], H, W, c['Cp']), NAN, dtype=torch.float32, device='cuda')      # real() finds what was not written
        r = ops.dw_dgrad(dy, pack, (H, W), c['stride'], mask6=m if mask else None, add=a if add else None, colsum=colsum, out=out)
        assert (r[0] if colsum else r) is out
        return r
    r = run()
    dx, cs = r if colsum else (r, None)
    ref, bar = M.dw_dgrad_ref(c['dy'], c['w'], c['stride'], (H, W), c['scale'] if scaled else None, c['m'] if mask else None,
                              c['add'] if add else None)
    note('dw3x3_dgrad', check('data gradient ' + mode, real(c, dx), flat(ref), flat(bar)))
    if mask:
        assert M.threshold_fraction(c['m']) <= 0.005
        keep = (M.nhwc(c['m']) > 0) & (M.nhwc(c['m']) < 6)
        assert 0.2 < float(keep.double().mean()) < 0.6 or keep.numel() < 64
        assert bool((real(c, dx).reshape(keep.shape)[~keep] == 0).all())
    if colsum:
        cref, cbar = M.colsum_ref(ref, bar)
        note('dw3x3_dgrad colsum', check('data gradient column sums', cs.cpu().view(1, -1), cref.view(1, -1), cbar.view(1, -1)))
    r2 = run()
    assert torch.equal((r2[0] if colsum else r2).view(torch.int32), dx.view(torch.int32)), 'not bit-repeatable'
    if colsum:
        assert torch.equal(r2[1], cs), 'column sums not bit-repeatable'
    N = shape[0]
    if N > 1:       # image k of the batch equals its single-image run
        k = N - 1
        one = run(c['dyd'][k:k + 1].contiguous(), c['md'][k:k + 1].contiguous(), c['addd'][k:k + 1].contiguous())
        one = one[0] if colsum else one
        assert torch.equal(one.view(torch.int32), dx[k:k + 1].view(torch.int32)), 'batch-dependent'
    plain = ops.dw_dgrad(c['dyd'], pack, (H, W), c['stride'], mask6=c['md'] if mask else None, add=c['addd'] if add else None)
    assert torch.equal(plain.view(torch.int32), dx.view(torch.int32)), 'out= changes the result'


@pytest.mark.parametrize('shape', M.SHAPES, ids=IDS)
@pytest.mark.parametrize('clamp', [False, True], ids=['asis', 'in_clamp6'])
def test_weight_gradient(shape, clamp):
    ops = _ops()
    c = case(shape)
    C = c['C']
    got = ops.dw_wgrad(c['dyd'], c['xd'], C, c['stride'], in_clamp6=clamp)
    ref, bar = M.dw_wgrad_ref(c['dy'], c['x'], c['stride'], clamp)
    assert not bool(torch.isnan(got).any())
    note('dw3x3_wgrad', check('weight gradient', got.cpu().view(C, 9), ref.view(C, 9), bar.view(C, 9)))
    assert torch.equal(ops.dw_wgrad(c['dyd'], c['xd'], C, c['stride'], in_clamp6=clamp), got), 'not bit-repeatable'
    acc = c['based'].clone()
    ops.dw_wgrad(c['dyd'], c['xd'], C, c['stride'], in_clamp6=clamp, grad=acc)
    assert torch.equal(acc, c['based'] + got), 'accumulate is not base + got'
    out = torch.full((C, 1, 3, 3), NAN, device='cuda')
    assert ops.dw_wgrad(c['dyd'], c['xd'], C, c['stride'], in_clamp6=clamp, out=out) is out and torch.equal(out, got)


BATCHED = [s for s in M.SHAPES if s[0] > 1]
PADDED = [s for s in M.SHAPES if s[3] % 32]


@pytest.mark.parametrize('shape', BATCHED, ids=[M.shape_id(s) for s in BATCHED])
def test_forward_batch_independence(shape):
    c = case(shape)
    N = shape[0]
    got = fwd(c, True, True)
    for k in range(N):
        one = fwd(c, True, True, x=c['xd'][k:k + 1].contiguous())
        assert torch.equal(one.view(torch.int32), got[k:k + 1].view(torch.int32)), 'image %d differs from its single-image run' % k


@pytest.mark.parametrize('shape', PADDED, ids=[M.shape_id(s) for s in PADDED])
def test_pad_channels_are_never_read(shape):
    """Every operand above carries NaN in its pad channels; here the same calls on zero-padded operands give the same bits."""
    ops = _ops()
    c = case(shape)
    H, W = shape[1:3]
    z = {k: padded(c[k], c['Cp'], 0.0) for k in ('x', 'm', 'dy', 'add')}
    assert torch.equal(fwd(c, True, True, x=z['x']).view(torch.int32), fwd(c, True, True).view(torch.int32))
    pack = ops.DwPack(c['wd'], c['scaled'])
    def nan_out():
        return torch.full((shape[0], H, W, c['Cp']), NAN, dtype=torch.float32, device='cuda')
    a = ops.dw_dgrad(z['dy'], pack, (H, W), c['stride'], mask6=z['m'], add=z['add'], colsum=True, out=nan_out())
    b = ops.dw_dgrad(c['dyd'], pack, (H, W), c['stride'], mask6=c['md'], add=c['addd'], colsum=True, out=nan_out())
    real(c, a[0]), real(c, b[0])                      # every real element written, every pad element bit-zero
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert torch.equal(ops.dw_wgrad(z['dy'], z['x'], c['C'], c['stride'], in_clamp6=True),
                       ops.dw_wgrad(c['dyd'], c['xd'], c['C'], c['stride'], in_clamp6=True))


@pytest.mark.parametrize('shape', M.SHAPES, ids=IDS)
def test_relu6_bwd_colsum_and_clamp6(shape):
    """On maps at the pitch with zero pad channels (what the block rule hands it; the pass runs over the whole pitch): exact against
    torch but for the column sums.  g goes into a NaN-prefilled buffer: every element is written, the pad as zero."""
    ops = _ops()
    c = case(shape)
    g, y, add = (padded(c[k], c['Cp'], 0.0) for k in ('g', 'm', 'add'))
    gc, yc, ac = g.cpu().double(), y.cpu().double(), add.cpu().double()
    keep = (yc > 0) & (yc < 6)
    for with_add in (False, True):
        buf = torch.full_like(g, NAN)
        got, cs = ops.relu6_bwd_colsum(g, y, add=add if with_add else None, out=buf)
        assert got is buf and not bool(torch.isnan(got).any()) and bool((got[..., c['C']:] == 0).all())
        want = torch.where(keep, (g.cpu() + add.cpu()) if with_add else g.cpu(), torch.zeros(()))
        assert torch.equal(got.cpu(), want)
        want64 = want.double()
        cref, cbar = M.colsum_ref(want64, torch.zeros_like(want64))
        note('relu6_bwd_colsum', check('relu6 column sums', cs.cpu().view(1, -1), cref.view(1, -1), cbar.view(1, -1)))
        assert torch.equal(ops.relu6_bwd_colsum(g, y, add=add if with_add else None)[1], cs), 'not bit-repeatable'
    # the clamped map decides as the ReLU(v) map does
    assert torch.equal(ops.relu6_bwd_colsum(g, y.clamp(max=6.0))[0], ops.relu6_bwd_colsum(g, y)[0])
    same, cs = ops.relu6_bwd_colsum(g)
    assert same is g
    cref, cbar = M.colsum_ref(gc, torch.zeros_like(gc))
    note('relu6_bwd_colsum', check('plain column sums', cs.cpu().view(1, -1), cref.view(1, -1), cbar.view(1, -1)))
    z = y.clone()
    assert ops.clamp6(z) is z and torch.equal(z, y.clamp(max=6.0))
    assert (float(z.max()) == 6.0 or z.numel() < 1024) and M.threshold_fraction(c['m']) <= 0.005


def test_argument_errors():
    from pointtinybenchmark_amd import _lib
    ops = _ops()
    err = _lib.CprHipError
    with pytest.raises(err, match='invalid argument'):
        ops.DwPack(torch.zeros((12, 1, 3, 3), device='cuda'))                   # C % 8
    pack = ops.DwPack(torch.zeros((32, 1, 3, 3), device='cuda'))
    x = torch.zeros((1, 6, 6, 32), device='cuda')
    with pytest.raises(err, match='invalid argument'):
        ops.dw_conv(x, pack, stride=3)
    with pytest.raises(err, match='invalid argument'):
        ops.dw_dgrad(torch.zeros((1, 2, 2, 32), device='cuda'), pack, (6, 6), stride=3)
    with pytest.raises(err, match='invalid argument'):
        ops.dw_wgrad(torch.zeros((1, 2, 2, 32), device='cuda'), x, 32, stride=3)
    y = torch.empty_like(x)
    s = ops._stream()
    with pytest.raises(err, match='invalid argument'):                          # a flag beyond the defined ones
        _lib.call('cpr_dw3x3_fwd', ops._ptr(x), ops._ptr(pack.w), None, None, ops._ptr(y), 1, 6, 6, 32, 1, 4, s)
    with pytest.raises(err, match='invalid argument'):
        _lib.call('cpr_dw3x3_wgrad', ops._ptr(y), ops._ptr(x), ops._ptr(pack.w), ops._ptr(y), 1, 6, 6, 32, 1, 2, 0, s)
    _lib.call('cpr_dw3x3_fwd', ops._ptr(x), ops._ptr(pack.w), None, None, ops._ptr(y), 1, 6, 6, 32, 1, 3, s)      # both defined flags
    torch.cuda.synchronize()
    assert bool((y == 0).all())
