"""csrc/deconv.hip on the device: the transposed convolution 4x4 / stride 2 / padding 1 (ops.deconv4x4s2, ops.DeconvPack) and its two
gradients on the dense-conv entries (ops.deconv4x4s2_dgrad_pack, ops.deconv4x4s2_wgrad), EVERY output element against fp64.

Bars.  Forward and data gradient: the per-element bar of tests/conv_fp64_ref.py -- ``ACC_REL * |scale| * sum |x w|`` plus one ``ULP32`` of
the intermediate per rounded epilogue operation.  Weight gradient: ``bar_fp32`` of tests/wgrad_fp64_ref.py, what
tests/test_gpu_wgrad_instances.py holds every weight-gradient kernel to.  Small-integer operands (|v| <= 4: every sum at K <= 1024 is
exact in fp32) must come out equal to the fp64 reference bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_fp64_ref as WR
from tests.conv_fp64_ref import ACC_REL, ULP32, _threads, ratio

# (N, H, W, Cin, Cout): odd sizes with an M tile across the image boundary; H = 1 (both row taps of a class fall off the map); a ragged
# Cout tile; a ragged last M tile; the real first stage at one 640^2 image (K = 1024)
SHAPES = [(2, 5, 7, 32, 64), (3, 1, 9, 64, 32), (1, 8, 8, 32, 96), (2, 13, 11, 64, 128), (1, 20, 20, 256, 256)]
VARIANT = 64 * 1000000 + 64 * 1000 + 1          # the launcher has one tile instance: 64 x 64, interleaved K loop
_REF = {}


def _ids(s):
    return 'x'.join(map(str, s))


def _operands(shape, integer=False):
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    if integer:
        x = torch.randint(-4, 5, (N, H, W, Cin), generator=g).float()
        w = torch.randint(-4, 5, (Cin, Cout, 4, 4), generator=g).float()
    else:
        x = torch.randn((N, H, W, Cin), generator=g)
        w = torch.randn((Cin, Cout, 4, 4), generator=g) * (4 * Cin) ** -0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    bias = torch.randn(Cout, generator=g)
    return x, w, scale * torch.where(torch.arange(Cout) % 3 == 0, -1.0, 1.0), bias


def _reference(shape, integer=False):
    """fp64 F.conv_transpose2d of the operands (NHWC) and the magnitude sum |x| |w| per output element; computed once per shape."""
    key = (shape, integer)
    if key not in _REF:
        _threads()
        x, w, _, _ = _operands(shape, integer)
        xd, wd = x.double().permute(0, 3, 1, 2), w.double()
        _REF[key] = (F.conv_transpose2d(xd, wd, None, 2, 1).permute(0, 2, 3, 1).contiguous(),
                     F.conv_transpose2d(xd.abs(), wd.abs(), None, 2, 1).permute(0, 2, 3, 1).contiguous())
    return _REF[key]


def _epilogue(t, mag, scale=None, bias=None, relu=False):
    """(reference, bar) after the kernel's epilogue, in its order (tests/conv_fp64_ref.reference)."""
    bar = ACC_REL * mag
    if scale is not None:
        t = t * scale.double()
        bar = bar * scale.double().abs() + ULP32 * t.abs()
    if bias is not None:
        t = t + bias.double()
        bar = bar + ULP32 * t.abs()
    if relu:
        t = t.clamp_min(0)
    return t, bar


def _worst(name, got, ref, bar):
    q = ratio(got.cpu(), ref, bar)
    worst = float(q.max())
    assert worst <= 1.0, '%s: %d / %d elements over the bar, worst ratio %.3g at %s' % (
        name, int((q > 1).sum()), q.numel(), worst, tuple(torch.nonzero(q == q.max())[0].tolist()))
    return worst


def composed(x, w):
    """The route the project had before: per output-parity class a 2x2 / padding 1 sub-convolution (PackedConv) over x, scattered to the
    strided positions by cpr_phase_scatter_add, as ops.PhasedDgrad assembles a stride-2 data gradient."""
    from pointtinybenchmark_amd import _lib, ops
    N, H, W, Cin = x.shape
    Cout = w.shape[1]
    y = torch.zeros((N, 2 * H, 2 * W, Cout), device=x.device, dtype=torch.float32)
    for a in range(2):
        for b in range(2):
            # out[i', j'] = sum_{r, s} x[i' - 1 + r, j' - 1 + s] g[r, s] with g[r, s] = w[.., 1 - a + 2 (1 - r), 1 - b + 2 (1 - s)]; class (a, b) is out[i + a, j + b]
            sub = w[:, :, [3 - a, 1 - a]][:, :, :, [3 - b, 1 - b]].permute(1, 0, 2, 3).contiguous()
            o = ops.conv2d(x, ops.PackedConv(sub, 1, 1))
            _lib.call('cpr_phase_scatter_add', ops._ptr(o), ops._ptr(y), N, H + 1, W + 1, Cout, 2 * H, 2 * W, a, b, a, b, 2, ops._stream())
    return y


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_forward_vs_fp64_raw_and_with_epilogue(shape):
    from pointtinybenchmark_amd import ops
    x, w, scale, bias = _operands(shape)
    t, mag = _reference(shape)
    xd, pack = x.cuda(), ops.DeconvPack(w.cuda())
    ops.TRACE_CONV_VARIANT[0] = True
    try:
        raw = ops.deconv4x4s2(xd, pack)
        assert ops.TRACE_CONV_VARIANT[1] == ('deconv', VARIANT), ops.TRACE_CONV_VARIANT[1]
    finally:
        ops.TRACE_CONV_VARIANT[0] = False
    assert tuple(raw.shape) == tuple(t.shape)
    w_raw = _worst('raw', raw, *_epilogue(t, mag))
    full = ops.deconv4x4s2(xd, pack, scale=scale.cuda(), bias=bias.cuda(), relu=True)
    ref, bar = _epilogue(t, mag, scale, bias, True)
    w_full = _worst('scale + bias + ReLU', full, ref, bar)
    assert bool((full >= 0).all()) and 0.2 < float((full == 0).float().mean()) < 0.8, 'the ReLU cuts about half'
    w_sc = _worst('scale only', ops.deconv4x4s2(xd, pack, scale=scale.cuda()), *_epilogue(t, mag, scale))
    print('\nDECONV %s worst |err| / bar: raw %.4f  scale+bias+relu %.4f  scale %.4f' % (_ids(shape), w_raw, w_full, w_sc))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_small_integers_are_exact_repeatable_and_the_pack_layout(shape):
    from pointtinybenchmark_amd import ops
    N, H, W, Cin, Cout = shape
    x, w, _, _ = _operands(shape, integer=True)
    t, _ = _reference(shape, integer=True)
    pack = ops.DeconvPack(w.cuda())
    want = ops.deconv_pack_image(w)
    assert float(want[3, 1, 2 * Cin + 5]) == float(w[5, 1, 2, 0]), 'class (1, 1), tap (1, 0): w[ci, co, 1 - 1 + 2, 1 - 1 + 0]'
    assert torch.equal(pack.w.cpu(), want), 'the pack is [class][Cout][(tap row, tap column, cin)]'
    y = ops.deconv4x4s2(x.cuda(), pack)
    assert torch.equal(y.cpu().double(), t), 'integer operands: every sum is exact, any tap / parity / border slip shows'
    again = ops.deconv4x4s2(x.cuda(), pack)
    assert torch.equal(y.view(torch.int32), again.view(torch.int32)), 'two launches differ'


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 5, 7, 32, 64), (3, 1, 9, 64, 32), (3, 13, 11, 64, 128)], ids=_ids)
def test_batch_independence(shape):
    """Image 1 of an N = 3 launch -- its rows start inside an M tile and straddle the next -- equals the same image launched alone."""
    from pointtinybenchmark_amd import ops
    x, w, scale, bias = _operands(shape)
    xd, pack = x.cuda(), ops.DeconvPack(w.cuda())
    for kw in (dict(), dict(scale=scale.cuda(), bias=bias.cuda(), relu=True)):
        whole = ops.deconv4x4s2(xd, pack, **kw)
        alone = ops.deconv4x4s2(xd[1:2].contiguous(), pack, **kw)
        assert torch.equal(whole[1:2].view(torch.int32), alone.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_composed_route_meets_the_same_bar(shape):
    x, w, _, _ = _operands(shape)
    t, mag = _reference(shape)
    # (one more rounding than the fused kernel: the scatter adds the sub-convolution's value to the zeroed map, exactly)
    worst = _worst('composed', composed(x.cuda(), w.cuda()), *_epilogue(t, mag))
    print('\nDECONV composed %s worst |err| / bar %.4f' % (_ids(shape), worst))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_data_gradient_vs_fp64_adjoint(shape):
    """dx = conv2d(dy, w read as (out = Cin, in = Cout, 4, 4), stride 2, padding 1): the adjoint of the forward, under the forward bar."""
    from pointtinybenchmark_amd import ops
    _threads()
    N, H, W, Cin, Cout = shape
    _, w, _, _ = _operands(shape)
    g = torch.Generator().manual_seed(7 + sum(shape))
    dy = torch.randn((N, 2 * H, 2 * W, Cout), generator=g)
    dyd, wd = dy.double().permute(0, 3, 1, 2), w.double()
    ref = F.conv2d(dyd, wd, None, 2, 1).permute(0, 2, 3, 1)
    mag = F.conv2d(dyd.abs(), wd.abs(), None, 2, 1).permute(0, 2, 3, 1)
    xx = torch.zeros((N, Cin, H, W), dtype=torch.float64, requires_grad=True)
    (F.conv_transpose2d(xx, wd, None, 2, 1) * dyd).sum().backward()
    assert float((xx.grad.permute(0, 2, 3, 1) - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), 'the identity itself, by autograd'
    pc = ops.deconv4x4s2_dgrad_pack(w.cuda())
    assert (pc.Cout, pc.Cin, pc.KH, pc.KW, pc.stride, pc.padding) == (Cin, Cout, 4, 4, 2, 1)
    dx = ops.conv2d(dy.cuda(), pc)
    assert tuple(dx.shape) == (N, H, W, Cin)
    worst = _worst('data gradient', dx, *_epilogue(ref, mag))
    print('\nDECONV dgrad %s worst |err| / bar %.4f' % (_ids(shape), worst))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_weight_gradient_written_and_accumulated(shape):
    """dw (Cin, Cout, 4, 4) = the dense conv's weight gradient with the maps' roles swapped, at the bar of the weight-gradient tests."""
    from pointtinybenchmark_amd import ops
    N, H, W, Cin, Cout = shape
    x, w, _, _ = _operands(shape)
    g = torch.Generator().manual_seed(11 + sum(shape))
    dy = torch.randn((N, 2 * H, 2 * W, Cout), generator=g)
    base = torch.randn((Cin, Cout, 4, 4), generator=g)
    xd, dyd = x.cuda(), dy.cuda()
    r = WR.reference(xd, dyd, 4, 2, 1)          # the 'conv' reads dy (its input) and writes x's shape (its output gradient)
    ww = w.double().clone().requires_grad_(True)
    (F.conv_transpose2d(x.double().permute(0, 3, 1, 2), ww, None, 2, 1) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    assert float((ww.grad - r['ref']).abs().max()) <= 1e-12 * float(r['ref'].abs().max()), 'the identity itself, by autograd'
    got = ops.deconv4x4s2_wgrad(dyd, xd, (Cin, Cout, 4, 4))
    worst = WR.check('written', got.cpu().double(), r['ref'], WR.bar_fp32(r))
    out = torch.full((Cin, Cout, 4, 4), float('nan'), device='cuda')
    assert ops.deconv4x4s2_wgrad(dyd, xd, (Cin, Cout, 4, 4), out=out) is out and torch.equal(out.view(torch.int32), got.view(torch.int32))
    acc = base.cuda()
    ops.deconv4x4s2_wgrad(dyd, xd, (Cin, Cout, 4, 4), grad=acc)
    worst_acc = WR.check('accumulated', acc.cpu().double(), r['ref'] + base.double(), WR.bar_fp32(r, base.double()))
    print('\nDECONV wgrad %s worst |err| / bar: written %.4f accumulated %.4f' % (_ids(shape), worst, worst_acc))


@pytest.mark.gpu
def test_argument_errors_return_before_any_launch():
    from pointtinybenchmark_amd import _lib, ops
    lib = _lib.load()
    x = torch.randn((1, 2, 2, 64), device='cuda')
    wgt = torch.randn((4, 64, 256), device='cuda')
    out = torch.full((1, 4, 4, 64), 7.0, device='cuda')
    s = ops._stream()

    def fwd(i, w, o, Cin=64, Cout=64, flags=0, N=1, H=2, W=2):
        return lib.cpr_deconv4x4s2_fwd(ops._ptr(i), ops._ptr(w), ops._ptr(o), None, None, N, H, W, Cin, Cout, flags, None, s)
    assert fwd(x, wgt, out) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    out.fill_(7.0)
    for rc in (fwd(x, wgt, out, Cin=48), fwd(x, wgt, out, Cout=40), fwd(None, wgt, out), fwd(x, None, out), fwd(x, wgt, None),
               fwd(x, wgt, out, flags=2), fwd(x, wgt, out, N=0), fwd(x, wgt, out, H=0)):
        assert rc == -1001, rc
    w = torch.randn((64, 64, 4, 4), device='cuda')
    pk = torch.full((4, 64, 256), 7.0, device='cuda')
    for rc in (lib.cpr_pack_weights_deconv(ops._ptr(w), ops._ptr(pk), 48, 64, s), lib.cpr_pack_weights_deconv(ops._ptr(w), ops._ptr(pk), 64, 40, s),
               lib.cpr_pack_weights_deconv(None, ops._ptr(pk), 64, 64, s), lib.cpr_pack_weights_deconv(ops._ptr(w), None, 64, 64, s)):
        assert rc == -1001, rc
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((pk == 7.0).all()), 'a refused call wrote nothing'
