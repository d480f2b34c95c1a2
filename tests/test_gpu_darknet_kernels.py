"""-m gpu: the Darknet kernels (csrc/darknet.hip) one by one.

  leaky_fwd          bit-equal to torch's CPU fp32 F.leaky_relu(z, slope) (+ res): with and without the shortcut, in place and out of
                     place, slopes 0.1 and 0.2, on values that include +-0.0, denormals, +-inf and NaN
  leaky_bwd_colsum   g bit-equal to torch's CPU autograd of F.leaky_relu at z (with and without ``add``, the mask read from z and from
                     leaky(z)); the column sums against the fp64 sums within gamma_M * sum|g|, gamma_M = M u / (1 - M u), u = 2^-24 --
                     the worst case of ANY summation order of M fp32 terms (Higham, Accuracy and Stability, (4.4)), so the bound is
                     derived from the format alone; two runs bit-equal; each image's rows of g equal its single-image run
  stem3x3s1_wgrad    against fp64 torch.nn.grad.conv2d_weight within gamma_n * conv(|dy|, |x|), n = N H W (the same bound: every
                     output is a sum of at most n products, each rounded once or fused); both image layouts; two runs bit-equal.  At
                     5 x 7 one missing border tap exceeds the bound by orders of magnitude (asserted on the reference itself)
  argument errors    C % 4 != 0 and bf16 tensors through the ops wrappers"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _gamma(n):
    return n * U / (1 - n * U)


def _bits_equal(a, b):
    """Bit for bit, except that any NaN matches any NaN (torch's CPU kernels and the device may differ in a NaN's payload)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    nan = torch.isnan(a) & torch.isnan(b)
    return a.shape == b.shape and bool(((a.view(torch.int32) == b.view(torch.int32)) | nan).all())


def _values(n, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    if special:
        sp = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, float('inf'), float('-inf'), float('nan'), -3.0e38, 3.0e38, 1.17549435e-38])
        k = min(n, sp.numel())
        v[:k] = sp[:k]
        if n > 64:      # and scattered through the map, so that every lane position of a quad sees them
            idx = torch.randperm(n, generator=g)[:48]
            v[idx] = sp[torch.arange(48) % sp.numel()]
    return v


# ------------------------------------------------------------------------------------------------ leaky_fwd
@pytest.mark.parametrize('n', [4, 28, 4 * 257, 4 * 65537])
@pytest.mark.parametrize('slope', [0.1, 0.2])
def test_leaky_fwd_bit_equal(n, slope):
    from pointtinybenchmark_amd import ops
    z, res = _values(n, 11 + n), _values(n, 12 + n)
    for with_res in (False, True):
        ref = F.leaky_relu(z, slope)
        if with_res:
            ref = ref + res
        r = res.cuda() if with_res else None
        out = torch.full((n,), 7.0, device='cuda')
        zc = z.cuda()
        got = ops.leaky(zc, slope, res=r, out=out)
        assert got is out and _bits_equal(out, ref), (n, slope, with_res, 'out of place')
        assert _bits_equal(zc, z), 'the out-of-place form wrote its input'
        got = ops.leaky(zc, slope, res=r)
        assert got is zc and _bits_equal(zc, ref), (n, slope, with_res, 'in place')


def test_leaky_fwd_signed_zero_and_nan():
    from pointtinybenchmark_amd import ops
    z = torch.tensor([-0.0, 0.0, float('nan'), -1e-45], device='cuda')
    out = ops.leaky(z.clone(), 0.1).cpu()
    assert out[0].item() == 0 and torch.signbit(out[0]) and not torch.signbit(out[1]) and torch.isnan(out[2])
    assert _bits_equal(out, F.leaky_relu(z.cpu(), 0.1))


# ------------------------------------------------------------------------------------------------ leaky_bwd_colsum
def _bwd_case(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g)
    z.view(-1)[::7] = 0.0                     # y == 0 takes the slope
    z.view(-1)[3::11] = -0.0
    dy, add = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    return z, dy, add


# (53, 32): rows per workgroup is 16 for a small map, so three full partials and a ragged tail of 5 rows
@pytest.mark.parametrize('M,C', [(1, 32), (7, 64), (257, 32), (4099, 1024), (53, 32)])
@pytest.mark.parametrize('slope', [0.1, 0.2])
def test_leaky_bwd_colsum(M, C, slope):
    from pointtinybenchmark_amd import ops
    z, dy, add = _bwd_case(M, C, 100 + M + C)
    for with_add in (False, True):
        s = (dy + add) if with_add else dy
        zz = z.clone().requires_grad_(True)
        F.leaky_relu(zz, slope).backward(s)
        ref = zz.grad
        for y in (z, F.leaky_relu(z, slope)):      # the pre-activation and the activated map: the same predicate
            g, cs = ops.leaky_bwd_colsum(dy.cuda(), y.cuda(), slope, add=add.cuda() if with_add else None)
            assert _bits_equal(g, ref), (M, C, slope, with_add)
            ref64 = ref.double().sum(0)
            bound = _gamma(M) * ref.double().abs().sum(0)
            err = (cs.double().cpu() - ref64).abs()
            print('leaky_bwd_colsum M=%d C=%d worst err / bound %.3g' % (M, C, float((err / bound.clamp_min(1e-300)).max())))
            assert bool((err <= bound).all()), (M, C, float((err - bound).max()))
            g2, cs2 = ops.leaky_bwd_colsum(dy.cuda(), y.cuda(), slope, add=add.cuda() if with_add else None)
            assert _bits_equal(g2, g) and _bits_equal(cs2, cs), 'two runs differ'
            none, cs3 = ops.leaky_bwd_colsum(dy.cuda(), y.cuda(), slope, add=add.cuda() if with_add else None, want_g=False)
            assert none is None and _bits_equal(cs3, cs), 'the sums depend on whether g is written'


def test_leaky_bwd_rows_do_not_depend_on_batch():
    from pointtinybenchmark_amd import ops
    N, HW, C = 2, 37, 64
    z, dy, add = _bwd_case(N * HW, C, 77)
    g, _ = ops.leaky_bwd_colsum(dy.cuda(), z.cuda(), 0.1, add=add.cuda())
    for n in range(N):
        sl = slice(n * HW, (n + 1) * HW)
        g1, _ = ops.leaky_bwd_colsum(dy[sl].contiguous().cuda(), z[sl].contiguous().cuda(), 0.1, add=add[sl].contiguous().cuda())
        assert _bits_equal(g[sl], g1), n


# ------------------------------------------------------------------------------------------------ stem3x3s1_wgrad
def _wgrad_ref(dy_nhwc, x_nchw):
    """fp64 conv2d_weight and the bound's scale conv(|dy|, |x|), both (32, 3, 3, 3)."""
    dy = dy_nhwc.double().permute(0, 3, 1, 2).contiguous()
    x = x_nchw.double()
    ref = torch.nn.grad.conv2d_weight(x, (32, 3, 3, 3), dy, stride=1, padding=1)
    scale = torch.nn.grad.conv2d_weight(x.abs(), (32, 3, 3, 3), dy.abs(), stride=1, padding=1)
    return ref, scale


@pytest.mark.parametrize('N,H,W', [(1, 1, 1), (2, 5, 7), (2, 33, 40)])
def test_stem3x3s1_wgrad(N, H, W):
    from pointtinybenchmark_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    x = torch.randn(N, 3, H, W, generator=g)
    dy = torch.randn(N, H, W, 32, generator=g)
    ref, scale = _wgrad_ref(dy, x)
    bound = _gamma(N * H * W) * scale
    x4 = torch.cat([x, torch.full((N, 1, H, W), 9.0)], 1).permute(0, 2, 3, 1).contiguous()      # (the 4th channel is ignored)
    outs = []
    for img, planar in ((x4, False), (x, True)):
        gw = ops.stem3x3s1_wgrad(dy.cuda(), img.cuda(), planar=planar)
        err = (gw.double().cpu() - ref).abs()
        print('stem3x3s1_wgrad %dx%dx%d planar=%s worst err / bound %.3g' % (N, H, W, planar, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (N, H, W, planar, float((err - bound).max()))
        again = ops.stem3x3s1_wgrad(dy.cuda(), img.cuda(), planar=planar, out=torch.empty((32, 3, 3, 3), device='cuda'))
        assert _bits_equal(again, gw), 'two runs differ'
        outs.append(gw)
    assert _bits_equal(outs[0], outs[1]), 'the two image layouts give different bits'
    if (H, W) == (5, 7):
        # the bound sees a single missing border tap: drop tap (0, 0) of output pixel (1, 1), which reads the image corner (0, 0)
        wrong = ref.clone()
        wrong[:, :, 0, 0] -= dy[0, 1, 1, :, None].double() * x[0, :, 0, 0][None].double()
        over = ((wrong - ref).abs() / bound.clamp_min(1e-300)).max()
        assert float(over) > 1e3, float(over)


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from pointtinybenchmark_amd import _lib, ops
    dy, y = torch.zeros(8, 6, device='cuda'), torch.zeros(8, 6, device='cuda')
    with pytest.raises(_lib.CprHipError):
        ops.leaky_bwd_colsum(dy, y, 0.1)                       # C % 4 != 0
    with pytest.raises(_lib.CprHipError):
        ops.leaky(torch.zeros(6, device='cuda'), 0.1)          # n % 4 != 0
    z16 = torch.zeros(8, 32, device='cuda', dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        ops.leaky(z16, 0.1)
    with pytest.raises(AssertionError):
        ops.leaky_bwd_colsum(z16, z16, 0.1)
    with pytest.raises(AssertionError):
        ops.stem3x3s1_wgrad(torch.zeros(1, 4, 4, 32, device='cuda', dtype=torch.bfloat16), torch.zeros(1, 4, 4, 4, device='cuda'))
    with pytest.raises(AssertionError):
        ops.stem3x3s1_wgrad(torch.zeros(1, 4, 4, 32, device='cuda'), torch.zeros(1, 4, 4, 4, device='cuda', dtype=torch.bfloat16))
