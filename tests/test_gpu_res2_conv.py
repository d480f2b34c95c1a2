"""-m gpu: the Res2Net slice kernels (csrc/res2net.hip) through ops.res2_conv / res2_wgrad / res2_pool / res2_pool_bwd against the fp64
references and bars of tests/res2_conv_ref.py, on the smallest shapes at which a tile edge, a slice boundary or a stride can go wrong.
On every shape: the output map is pattern-filled before the launch and every channel outside the written slice comes back bit for
bit; the channels the kernel must not read hold NaN; two runs agree bit for bit; image 1 of a batch equals its single-image run; the
weight gradient is bit-repeatable.  The slice ReLU backward with its column sums.  And the argument errors of the C entry points."""
import ctypes
import functools

import pytest
import torch

from tests import res2_conv_ref as R
from tests.conv_fp64_ref import check

pytestmark = pytest.mark.gpu

IDS = [R.shape_id(s) for s in R.SHAPES]


def _ops():
    from pointtinybenchmark_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def case(shape):
    """The operands of one shape, CPU masters and their device maps (NaN outside the slices), shared by every test and left unchanged."""
    N, H, W, width, pitch, sl, stride, add = shape
    c = R.make_case(shape)
    xo, ao, oo = R.slices(shape)
    dev = torch.device('cuda')
    OH, OW = R.out_hw(H, W, stride)
    c.update(xo=xo, ao=ao, oo=oo, width=width, pitch=pitch, ohw=(OH, OW))
    c['xd'] = R.embed(c['x'], pitch, xo).to(dev)
    c['addd'] = R.embed(c['add'], pitch, ao).to(dev) if add else None
    c['dyd'] = R.embed(c['dy'], pitch, oo).to(dev)          # the gradient arrives where the forward wrote
    c['wd'], c['scaled'], c['biasd'] = c['w'].to(dev), c['scale'].to(dev), c['bias'].to(dev)
    c['pat_out'] = R.pattern(N, OH, OW, pitch).to(dev)
    c['pat_in'] = R.pattern(N, H, W, pitch, seed=8).to(dev)
    return c


def _only_slice_written(got, pat, off, width):
    keep = torch.ones(got.shape[-1], dtype=torch.bool, device=got.device)
    keep[off:off + width] = False
    assert torch.equal(got[..., keep], pat[..., keep]), 'channels outside the written slice changed'
    assert bool(torch.isfinite(got[..., off:off + width]).all()), 'the slice holds a non-finite value: a channel outside the slices was read'


def forward(c, x=None, add=None, affine=False):
    ops = _ops()
    x = c['xd'] if x is None else x
    add = c['addd'] if add is None else add
    out = c['pat_out'][:x.shape[0]].clone()
    pk = ops.Res2Pack(c['wd'])
    kw = dict(scale=c['scaled'], bias=c['biasd'], relu=True) if affine else {}
    ops.res2_conv(x, c['xo'], pk, out, c['oo'], stride=c['stride'], add=add, add_off=c['ao'], **kw)
    _only_slice_written(out, c['pat_out'][:x.shape[0]], c['oo'], c['width'])
    return out[..., c['oo']:c['oo'] + c['width']]


def dgrad(c, dy=None, scaled=True):
    """The data gradient, written to the input slice's place in a pattern-filled map of the layer's input size."""
    ops = _ops()
    dy = c['dyd'] if dy is None else dy
    out = c['pat_in'][:dy.shape[0]].clone()
    pk = ops.Res2Pack(c['wd'], scale=c['scaled'] if scaled else None, transpose=True)
    ops.res2_conv(dy, c['oo'], pk, out, c['xo'], stride=c['stride'], transposed=True)
    _only_slice_written(out, c['pat_in'][:dy.shape[0]], c['xo'], c['width'])
    return out[..., c['xo']:c['xo'] + c['width']]


def wgrad(c, **kw):
    return _ops().res2_wgrad(c['dyd'], c['oo'], c['xd'], c['xo'], c['width'], c['stride'], add=c['addd'], add_off=c['ao'], **kw)


def _flat(t):
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize('affine', [False, True], ids=['raw', 'scale_bias_relu'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=IDS)
def test_forward_within_bar(shape, affine):
    c = case(shape)
    got = forward(c, affine=affine).cpu()
    ref, bar = R.fwd_ref(c['xin'], c['w'], c['stride'], *((c['scale'], c['bias'], True) if affine else ()))
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('slice forward %s' % R.shape_id(shape), _flat(got), _flat(ref), _flat(bar))
    print('forward %s %s: worst |err| / bar = %.3g' % (R.shape_id(shape), 'affine' if affine else 'raw', worst))


@pytest.mark.parametrize('scaled', [False, True], ids=['raw', 'bn_scale'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=IDS)
def test_data_gradient_within_bar(shape, scaled):
    c = case(shape)
    H, W = shape[1:3]
    got = dgrad(c, scaled=scaled).cpu()
    ref, bar = R.dgrad_ref(c['dy'], c['w'], c['stride'], (H, W), c['scale'] if scaled else None)
    assert tuple(got.shape) == tuple(ref.shape) == (shape[0], H, W, shape[3])
    worst = check('slice dgrad %s' % R.shape_id(shape), _flat(got), _flat(ref), _flat(bar))
    print('dgrad %s: worst |err| / bar = %.3g' % (R.shape_id(shape), worst))


@pytest.mark.parametrize('shape', R.SHAPES, ids=IDS)
def test_weight_gradient_within_bar(shape):
    c = case(shape)
    width = c['width']
    got = wgrad(c)
    assert torch.equal(got, wgrad(c)), 'the weight gradient is not bit-repeatable'
    got = got.cpu()
    ref, bar = R.wgrad_ref(c['dy'], c['xin'], c['stride'])
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('slice wgrad %s' % R.shape_id(shape), got.reshape(width, -1), ref.reshape(width, -1), bar.reshape(width, -1))
    print('wgrad %s: worst |err| / bar = %.3g' % (R.shape_id(shape), worst))
    # accumulation into an existing gradient: one more rounded addition
    base = torch.randn(tuple(c['w'].shape), generator=torch.Generator().manual_seed(5))
    acc = base.cuda()
    wgrad(c, grad=acc)
    assert torch.equal(acc.cpu(), base + got)


@pytest.mark.parametrize('shape', R.SHAPES, ids=IDS)
def test_pool_and_its_backward_within_bar(shape):
    """The last slice at this shape's stride: the 3x3 / stride-2 average (divisor 9), or the copy."""
    c = case(shape)
    ops = _ops()
    N, H, W, width, pitch, sl, stride, add = shape
    out = c['pat_out'].clone()
    ops.res2_pool(c['xd'], c['xo'], out, c['oo'], width, stride)
    _only_slice_written(out, c['pat_out'], c['oo'], width)
    got = out[..., c['oo']:c['oo'] + width]
    ref, bar = R.pool_ref(c['x'], stride)
    assert tuple(got.shape) == tuple(ref.shape)
    worst = check('slice pool %s' % R.shape_id(shape), _flat(got.cpu()), _flat(ref), _flat(bar))
    dx = c['pat_in'].clone()
    ops.res2_pool_bwd(c['dyd'], c['oo'], dx, c['xo'], width, stride)
    _only_slice_written(dx, c['pat_in'], c['xo'], width)
    gdx = dx[..., c['xo']:c['xo'] + width]
    ref, bar = R.pool_bwd_ref(c['dy'], stride, (H, W))
    worst_b = check('slice pool backward %s' % R.shape_id(shape), _flat(gdx.cpu()), _flat(ref), _flat(bar))
    print('pool %s: worst |err| / bar = %.3g forward, %.3g backward' % (R.shape_id(shape), worst, worst_b))
    out2, dx2 = c['pat_out'].clone(), c['pat_in'].clone()
    ops.res2_pool(c['xd'], c['xo'], out2, c['oo'], width, stride)
    ops.res2_pool_bwd(c['dyd'], c['oo'], dx2, c['xo'], width, stride)
    assert torch.equal(out, out2) and torch.equal(dx, dx2)


@pytest.mark.parametrize('shape', R.SHAPES, ids=IDS)
def test_bit_repeatable_and_batch_independent(shape):
    c = case(shape)
    N = shape[0]
    runs = [(forward(c, affine=True), forward(c), dgrad(c)) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    if N >= 2:
        # image 1 of the batch equals its single-image run, forward and data gradient
        y, _, dx = runs[0]
        x1, dy1 = c['xd'][1:2].contiguous(), c['dyd'][1:2].contiguous()
        a1 = c['addd'][1:2].contiguous() if c['addd'] is not None else None
        assert torch.equal(forward(c, x=x1, add=a1, affine=True)[0], y[1])
        assert torch.equal(dgrad(c, dy=dy1)[0], dx[1])


@pytest.mark.parametrize('shape', R.SHAPES, ids=IDS)
def test_slice_relu_backward_and_column_sums(shape):
    """ops.res2_relu_bwd in place on the gradient slice: g = (dy + carry) * (y > 0) is the fp32 sum exactly (one rounding, torch's own
    fp32 add); the column sums against their fp64 sums within (M - 1) * 2^-24 * sum |g| (any order of M - 1 fp32 additions,
    tests/conv_fp64_ref.py); nothing outside the slice is written, NaN outside the slices is not read, two runs agree bit for bit."""
    from tests.conv_fp64_ref import U32
    c = case(shape)
    ops = _ops()
    width, oo = c['width'], c['oo']
    N, OH, OW = c['dyd'].shape[:3]
    g = torch.Generator().manual_seed(17)
    y = R.embed(torch.randn((N, width, OH, OW), generator=g).clamp_min(0), c['pitch'], oo).cuda()          # a ReLU output: half zeros
    carry_cpu = torch.randn((N, width, OH, OW), generator=g)
    carry = R.embed(carry_cpu, c['pitch'], c['ao']).cuda()
    for use_carry in (False, True):
        runs = []
        for _ in range(2):
            buf = c['dyd'].clone()
            cs = ops.res2_relu_bwd(buf, oo, y, oo, width, carry=carry if use_carry else None, carry_off=c['ao'])
            runs.append((buf, cs))
        assert torch.equal(runs[0][0][..., oo:oo + width], runs[1][0][..., oo:oo + width]) and torch.equal(runs[0][1], runs[1][1])
        buf, cs = runs[0]
        keep = torch.ones(c['pitch'], dtype=torch.bool)
        keep[oo:oo + width] = False
        assert bool(torch.isnan(buf[..., keep.cuda()]).all()), 'channels outside the slice were written'
        want = R.nhwc(c['dy'] + carry_cpu if use_carry else c['dy']) * (y[..., oo:oo + width].cpu() > 0)
        got = buf[..., oo:oo + width].cpu()
        assert torch.equal(got, want)
        flat = want.double().reshape(-1, width)
        ref, bar = flat.sum(0), (flat.shape[0] - 1) * U32 * flat.abs().sum(0)
        check('slice relu backward column sums %s' % R.shape_id(shape), cs.cpu().view(1, -1), ref.view(1, -1), bar.view(1, -1))
    from pointtinybenchmark_amd import _lib
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.res2_relu_bwd(c['dyd'].clone(), oo + 1, y, oo, width)
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.res2_relu_bwd(c['dyd'].clone(), oo, y, c['pitch'] - width + 2, width)


def test_padding_contributes_zero_to_the_sum():
    """x + add = 0 everywhere (add = -x): a kernel that formed the sum for a padding pixel from stale or out-of-range data would not
    return exactly bias at the borders."""
    ops = _ops()
    c = case(R.SHAPES[3])
    neg = torch.where(torch.isnan(c['addd']), c['addd'], torch.zeros_like(c['addd']))
    neg[..., c['ao']:c['ao'] + c['width']] = -c['xd'][..., c['xo']:c['xo'] + c['width']]
    out = c['pat_out'].clone()
    ops.res2_conv(c['xd'], c['xo'], ops.Res2Pack(c['wd']), out, c['oo'], add=neg, add_off=c['ao'], scale=c['scaled'], bias=c['biasd'])
    got = out[..., c['oo']:c['oo'] + c['width']]
    assert torch.equal(got, c['biasd'].expand_as(got))


def test_argument_errors_come_before_any_launch():
    """NULL maps, a slice that overruns its pitch, a misaligned offset, pitch or width, a stride other than 1 / 2 and an add operand at
    stride 2 are the argument error; sizes whose pixel index leaves int are the unsupported error -- none of them launches."""
    from pointtinybenchmark_amd import _lib
    ops = _ops()
    dev = torch.device('cuda')
    N, H, W, width, pitch = 1, 4, 4, 26, 128
    x = torch.zeros((N, H, W, pitch), device=dev)
    out = torch.full((N, H, W, pitch), 5.0, device=dev)
    half = torch.full((N, 2, 2, pitch), 5.0, device=dev)
    pk = ops.Res2Pack(torch.zeros((width, width, 3, 3), device=dev))
    bad = pytest.raises(_lib.CprHipError, match='invalid argument')
    with bad:
        ops.res2_conv(x, 104, pk, out, 0)                       # 104 + 26 > 128: the input slice overruns its pitch
    with bad:
        ops.res2_conv(x, 0, pk, out, 104)                       # ... the output slice
    with bad:
        ops.res2_conv(x, 0, pk, out, 26, add=x, add_off=104)    # ... the add slice
    with bad:
        ops.res2_conv(x, 1, pk, out, 0)                         # an odd offset breaks the 8-byte alignment of the float2 loads
    with bad:
        ops.res2_conv(x, 0, pk, out, 27)
    with bad:
        ops.res2_conv(x, -2, pk, out, 0)
    with bad:
        ops.res2_conv(x, 0, pk, out, 0, stride=3)
    with bad:
        ops.res2_conv(x, 0, pk, out, 0, stride=0)
    with bad:
        ops.res2_conv(x, 0, pk, half, 0, stride=2, add=x, add_off=26)       # add at stride 2
    with bad:
        ops.res2_conv(x, 0, pk, half, 0, stride=1)              # 4 x 4 -> 2 x 2 is not a stride-1 layer
    with bad:
        ops.res2_conv(half, 0, pk, out, 0, stride=1, transposed=True)
    odd = torch.zeros((N, H, W, 27), device=dev)
    with bad:
        ops.res2_conv(odd, 0, pk, out, 0)                       # an odd pitch
    with bad:
        ops.res2_wgrad(out, 104, x, 0, width)
    with bad:
        ops.res2_wgrad(out, 0, x, 3, width)
    with bad:
        ops.res2_wgrad(out, 0, x, 0, 25)                        # an odd width
    with bad:
        ops.res2_wgrad(half, 0, x, 0, width, stride=3)
    with bad:
        ops.res2_wgrad(half, 0, x, 0, width, stride=2, add=x, add_off=26)
    with bad:
        ops.res2_pool(x, 104, half, 0, width, 2)
    with bad:
        ops.res2_pool(x, 0, half, 1, width, 2)
    with bad:
        ops.res2_pool(x, 0, half, 0, width, 3)
    with bad:
        ops.res2_pool_bwd(half, 0, out, 104, width, 2)
    with bad:
        ops.res2_pool_bwd(half, 2, out, 1, width, 2)
    # NULL pointers and sizes past int, through the C ABI itself
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros((4096,), device=dev)
    gw = torch.zeros((width, width, 3, 3), device=dev)

    def conv(xp=x, wp=pk.w, op=out, n=N, h=H, w=W):
        return _lib.call('cpr_res2_conv_fwd', P(xp), pitch, 0, None, 0, 0, P(wp), P(op), pitch, 26, None, None, n, h, w, h, w, width, 1, 0,
                         0, st)
    for kw in (dict(xp=None), dict(wp=None), dict(op=None)):
        with bad:
            conv(**kw)
    big = pytest.raises(_lib.CprHipError, match='unsupported')
    with big:
        conv(n=1 << 20, h=64, w=64)                             # 2^32 pixels
    with bad:
        _lib.call('cpr_res2_pack_weights', None, None, P(pk.w), width, 0, st)
    with bad:
        _lib.call('cpr_res2_pack_weights', P(gw), None, P(pk.w), 27, 0, st)
    with bad:
        _lib.call('cpr_res2_conv_wgrad', None, pitch, 0, P(x), pitch, 0, None, 0, 0, P(gw), P(ws), N, H, W, width, 1, 0, st)
    with bad:
        _lib.call('cpr_res2_conv_wgrad', P(out), pitch, 0, P(x), pitch, 0, None, 0, 0, None, P(ws), N, H, W, width, 1, 0, st)
    with bad:
        _lib.call('cpr_res2_conv_wgrad', P(out), pitch, 0, P(x), pitch, 0, None, 0, 0, P(gw), None, N, H, W, width, 1, 0, st)
    with big:
        _lib.call('cpr_res2_conv_wgrad', P(out), pitch, 0, P(x), pitch, 0, None, 0, 0, P(gw), P(ws), 1 << 20, 64, 64, width, 1, 0, st)
    with big:
        _lib.call('cpr_res2_conv_wgrad_workspace', 1 << 20, 64, 64, 208)
    with bad:
        _lib.call('cpr_res2_pool_fwd', None, pitch, 0, P(half), pitch, 0, N, H, W, width, 2, st)
    with bad:
        _lib.call('cpr_res2_pool_bwd', P(half), pitch, 0, None, pitch, 0, N, H, W, width, 2, st)
    with big:
        _lib.call('cpr_res2_pool_fwd', P(x), pitch, 0, P(half), pitch, 0, 1 << 20, 64, 64, width, 2, st)
    with big:
        _lib.call('cpr_res2_pool_bwd', P(half), pitch, 0, P(out), pitch, 0, 1 << 20, 64, 64, width, 2, st)
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 5.0 and float(half.min()) == 5.0, 'a refused call wrote its output'
