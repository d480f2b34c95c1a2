"""-m gpu: the HRFPN neck (csrc/hrfpn.hip, necks/hrfpn.py).

  shapes     level 0 of 8x8 with 4 inputs (the coarsest level is 1x1: both taps clamp onto one pixel), 24x40 (3x5 coarsest, 24 // 16 = 1
             drops 8 rows), 72x104 (crosses the workgroup tiles of every kernel in both directions, a multiple of none; 72 // 16 = 4 drops
             8 rows and 8 columns); N = 1 and 3; C = 32 and 256; 1..4 inputs, 1..5 outputs
  exact      inputs and gradients on a grid of multiples of 2^-4 with |v| <= 2, grid-valued bias: bilinear weights are dyadic with
             denominator <= 256 and every sum has fewer than 2^11 terms, so every product and sum of hrfpn_fuse, hrfpn_pool,
             hrfpn_pool_bwd and hrfpn_fuse_bwd is exact in fp32 and the kernels EQUAL fp64 torch / autograd, border rows and dropped pool
             rows included; bf16: the exact result rounded once
  random     forward fp32 |err| <= 1e-5 max|want|, bf16 |err| <= 2^-8 |want| + 1e-5 max|want|; backward kernels rel-L2 <= 1e-5 per tensor
             against fp64 autograd
  repeat     an image of a batch of 3 bit-equal to its single-image run; a second run bit-equal to the first
  refusals   wrong channel multiple, mismatched level sizes, an empty level: the kernels' own argument checks
  neck       per fixture case each output <= 2e-4 max|level|; forward_lazy equals forward; the bf16 compute mode; a padded-pitch input
             read in place gives the bits of its copy; gradients of every parameter and input against the fixture <= 2e-3 on norm and on
             sample, the reduction weight's per column slice
  locators   R18 128x160: P2PHead (the 4-point grid, C = 2) over num_outs=3 and CPRHead over num_outs=1 -- losses within 3e-4 of fp64
             autograd over tests/hrfpn_ref + the oracle, gradients <= 2e-3 rel-L2 per tensor; the bridge bit-equal to the native trainer;
             steps repeat bit for bit; three SGD steps lower the loss; bucket ready points; CprTrainer refuses num_outs=2; mixed precision
             at the bars of tests/test_gpu_bfp.py's mixed test"""
import pytest
import torch

from oracle import cpr_oracle as O
from oracle import p2p_options_oracle as PO
from pointtinybenchmark_amd import synthetic
from tests import hrfpn_ref as HR
from tests.ready_point_check import checked
from tests.test_gpu_fpn_extra import GRID4, _cells, _data, _NeckOnly, _record_assignments

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (24, 40), (72, 104)]
NC = [(1, 32), (3, 256)]
DT = {torch.float32: 'fp32', torch.bfloat16: 'bf16'}


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _grid(shape, g, dtype=torch.float32):
    """Multiples of 2^-4 in [-2, 2]: exact in fp32 and in bf16."""
    return (torch.randint(-32, 33, shape, generator=g).float() * 2.0 ** -4).to(dtype).cuda()


def _levels(hw, n_in, N, C, g, dtype, grid):
    H0, W0 = hw
    mk = (lambda s: _grid(s, g, dtype)) if grid else (lambda s: torch.randn(s, generator=g).to(dtype).cuda())
    return [mk((N, H0 >> i, W0 >> i, C)) for i in range(n_in)]


def _fuse64(ys, bias):
    out = bias.double().cpu()[None, :, None, None] + _nchw64(ys[0])
    for i in range(1, len(ys)):
        out = out + HR.upsample(_nchw64(ys[i]), i)
    return out


def _max_outs(hw):
    return min(5, min(hw).bit_length())        # the largest num_outs with no empty level


def _bar(want, dtype):
    return 1e-5 * want.abs().max() + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0.0)


def _check(tag, got, want, dtype):
    err = (_nchw64(got) - want).abs()
    bar = _bar(want, dtype)
    print('ERR %-44s max err %.3e  max err / bar %.3f' % (tag, float(err.max()), float((err / bar).max())), flush=True)
    assert bool((err <= bar).all()), (tag, float((err / bar).max()))


def _rel_l2(tag, got, want):
    e = float((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-300))
    print('REL %-44s rel-L2 %.3e' % (tag, e), flush=True)
    return e


# ------------------------------------------------------------------------------------------------ forward kernels
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=DT.get)
@pytest.mark.parametrize('N,C', NC)
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: '%dx%d' % s)
def test_fuse_and_pool_are_exact_on_the_grid(hw, N, C, dtype):
    from pointtinybenchmark_amd import ops
    g = torch.Generator().manual_seed(hw[0] * 7 + C)
    bias = _grid((C,), g)
    for n_in in range(1, 5):
        ys = _levels(hw, n_in, N, C, g, dtype, grid=True)
        out = ops.hrfpn_fuse(ys, bias)
        want = _fuse64(ys, bias)
        assert out.dtype == dtype and out.shape == ys[0].shape
        assert torch.equal(_nchw64(out), want.float().to(dtype).double()), ('fuse', hw, n_in, float((_nchw64(out) - want).abs().max()))
    assert torch.equal(_nchw64(ops.hrfpn_fuse(ys[:1], None)), _nchw64(ys[0])), 'one input, no bias: the identity'
    x = _grid((N,) + hw + (C,), g, dtype)
    for num_outs in range(1, _max_outs(hw) + 1):
        levels = ops.hrfpn_pool(x, num_outs)
        want = HR.pools(_nchw64(x), num_outs)[1:]
        assert len(levels) == num_outs - 1
        for k, (lv, w) in enumerate(zip(levels, want)):
            assert lv.dtype == dtype and tuple(lv.shape) == (N, hw[0] >> (k + 1), hw[1] >> (k + 1), C)
            assert torch.equal(_nchw64(lv), w.float().to(dtype).double()), ('pool', hw, num_outs, k + 1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=DT.get)
@pytest.mark.parametrize('hw,N,C', [((24, 40), 3, 32), ((72, 104), 1, 256)], ids=['24x40', '72x104'])
def test_fuse_and_pool_vs_fp64_on_random_data(hw, N, C, dtype):
    from pointtinybenchmark_amd import ops
    g = torch.Generator().manual_seed(5)
    bias = torch.randn((C,), generator=g).cuda()
    for n_in in (2, 4):
        ys = _levels(hw, n_in, N, C, g, dtype, grid=False)
        out = ops.hrfpn_fuse(ys, bias)
        _check('fuse %dx%d in=%d %s' % (hw + (n_in, DT[dtype])), out, _fuse64(ys, bias), dtype)
    levels = ops.hrfpn_pool(out, _max_outs(hw))
    for k, (lv, w) in enumerate(zip(levels, HR.pools(_nchw64(out), _max_outs(hw))[1:])):
        _check('pool %dx%d level %d %s' % (hw + (k + 1, DT[dtype])), lv, w, dtype)


# ------------------------------------------------------------------------------------------------ backward kernels
def _pool_bwd64(gs):
    out = torch.zeros_like(_nchw64(gs[0])).requires_grad_(True)
    sum((o * _nchw64(gk)).sum() for o, gk in zip(HR.pools(out, len(gs)), gs)).backward()
    return out.grad


def _fuse_bwd64(d_out, sizes):
    N, _, _, C = d_out.shape
    ys = [torch.zeros((N, C) + tuple(s), dtype=torch.float64, requires_grad=True) for s in sizes]
    (sum(HR.upsample(y, i + 1) for i, y in enumerate(ys)) * _nchw64(d_out)).sum().backward()
    return [y.grad for y in ys]


@pytest.mark.parametrize('N,C', NC)
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: '%dx%d' % s)
def test_backward_kernels_are_exact_on_the_grid(hw, N, C):
    from pointtinybenchmark_amd import ops
    g = torch.Generator().manual_seed(hw[1] * 3 + N)
    for K in range(1, _max_outs(hw) + 1):
        gs = [_grid((N, hw[0] >> k, hw[1] >> k, C), g) for k in range(K)]
        d_out, part = ops.hrfpn_pool_bwd(gs)
        want = _pool_bwd64(gs)
        assert torch.equal(_nchw64(d_out), want), ('pool_bwd', hw, K, float((_nchw64(d_out) - want).abs().max()))
        if K > 1 and hw[0] % (1 << (K - 1)):       # rows the coarsest pool drops: that level adds exactly +0.0, the rest is exact too
            rows = (hw[0] >> (K - 1)) << (K - 1)
            sub = _pool_bwd64(gs[:K - 1]) if K > 2 else _nchw64(gs[0])
            assert torch.equal(_nchw64(d_out)[:, :, rows:], sub[:, :, rows:])
        cs = part.reduce().double().cpu()
        wcs = want.sum((0, 2, 3))
        assert float((cs - wcs).abs().max()) <= 1e-6 * float(wcs.abs().max()), ('pool_bwd column sums', hw, K)
    d_out = _grid((N,) + hw + (C,), g)
    for n_in in range(2, 5):
        sizes = [(hw[0] >> i, hw[1] >> i) for i in range(1, n_in)]
        dys = ops.hrfpn_fuse_bwd(d_out, sizes)
        for i, (dy, w) in enumerate(zip(dys, _fuse_bwd64(d_out, sizes))):
            assert tuple(dy.shape) == (N,) + sizes[i] + (C,)
            assert torch.equal(_nchw64(dy), w), ('fuse_bwd', hw, n_in, i + 1, float((_nchw64(dy) - w).abs().max()))
    assert ops.hrfpn_fuse_bwd(d_out, []) == []


@pytest.mark.parametrize('hw,N,C', [((24, 40), 3, 32), ((72, 104), 1, 256)], ids=['24x40', '72x104'])
def test_backward_kernels_vs_fp64_autograd_on_random_data(hw, N, C):
    from pointtinybenchmark_amd import ops
    g = torch.Generator().manual_seed(9)
    K = _max_outs(hw)
    gs = [torch.randn((N, hw[0] >> k, hw[1] >> k, C), generator=g).cuda() for k in range(K)]
    d_out, part = ops.hrfpn_pool_bwd(gs)
    want = _pool_bwd64(gs)
    assert _rel_l2('pool_bwd %dx%d' % hw, _nchw64(d_out), want) <= 1e-5
    assert _rel_l2('pool_bwd column sums %dx%d' % hw, part.reduce(), want.sum((0, 2, 3))) <= 1e-5
    sizes = [(hw[0] >> i, hw[1] >> i) for i in range(1, 4)]
    for i, (dy, w) in enumerate(zip(ops.hrfpn_fuse_bwd(d_out, sizes), _fuse_bwd64(d_out, sizes))):
        assert _rel_l2('fuse_bwd %dx%d level %d' % (hw + (i + 1,)), _nchw64(dy), w) <= 1e-5


# ------------------------------------------------------------------------------------------------ repeatability
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=DT.get)
def test_kernels_repeat_and_do_not_depend_on_the_batch(dtype):
    from pointtinybenchmark_amd import ops
    hw, N, C = (24, 40), 3, 64
    g = torch.Generator().manual_seed(21)
    ys = _levels(hw, 4, N, C, g, dtype, grid=False)
    bias = torch.randn((C,), generator=g).cuda()
    out = ops.hrfpn_fuse(ys, bias)
    levels = ops.hrfpn_pool(out, 5)
    assert torch.equal(out, ops.hrfpn_fuse(ys, bias)) and all(torch.equal(a, b) for a, b in zip(levels, ops.hrfpn_pool(out, 5)))
    one = ops.hrfpn_fuse([y[1:2].contiguous() for y in ys], bias)
    assert torch.equal(one, out[1:2])
    assert all(torch.equal(a, b[1:2]) for a, b in zip(ops.hrfpn_pool(one, 5), levels))
    if dtype == torch.bfloat16:
        return
    gs = [torch.randn(lv.shape, generator=g).cuda() for lv in [out] + levels]
    d_out, part = ops.hrfpn_pool_bwd(gs)
    d_out2, part2 = ops.hrfpn_pool_bwd(gs)
    assert torch.equal(d_out, d_out2) and torch.equal(part.reduce(), part2.reduce())
    sizes = [tuple(y.shape[1:3]) for y in ys[1:]]
    dys = ops.hrfpn_fuse_bwd(d_out, sizes)
    assert all(torch.equal(a, b) for a, b in zip(dys, ops.hrfpn_fuse_bwd(d_out, sizes)))
    d1, _ = ops.hrfpn_pool_bwd([t[1:2].contiguous() for t in gs])
    assert torch.equal(d1, d_out[1:2])
    assert all(torch.equal(a, b[1:2]) for a, b in zip(ops.hrfpn_fuse_bwd(d1, sizes), dys))


# ------------------------------------------------------------------------------------------------ refusals
def test_kernels_refuse_bad_arguments():
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd._lib import CprHipError
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt).cuda()      # noqa: E731
    with pytest.raises(CprHipError, match='cpr_hrfpn_fuse: invalid argument'):      # fp32 takes channels in fours
        ops.hrfpn_fuse([z(1, 8, 8, 6), z(1, 4, 4, 6)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_fuse_bf16: invalid argument'):  # bf16 in eights
        ops.hrfpn_fuse([z(1, 8, 8, 12, dt=torch.bfloat16)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_pool: invalid argument'):
        ops.hrfpn_pool(z(1, 8, 8, 6), 2)
    for bad in ((5, 4), (4, 3), (3, 4)):        # level 1 of an 8x8 map is 4x4 and nothing else; 7x8 has no level 1
        with pytest.raises(CprHipError, match='cpr_hrfpn_fuse: invalid argument'):
            ops.hrfpn_fuse([z(1, 8, 8, 8), z(1, *bad, 8)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_fuse: invalid argument'):
        ops.hrfpn_fuse([z(1, 7, 8, 8), z(1, 3, 4, 8)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_fuse: invalid argument'):      # five inputs
        ops.hrfpn_fuse([z(1, 16 >> i, 16 >> i, 8) for i in range(5)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_pool: invalid argument'):      # 8 >> 4 = 0: an empty level
        ops.hrfpn_pool(z(1, 8, 8, 8), 5)
    with pytest.raises(CprHipError, match='cpr_hrfpn_pool_bwd: invalid argument'):
        ops.hrfpn_pool_bwd([z(1, 8, 8, 8), z(1, 4, 3, 8)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_pool_bwd: invalid argument'):
        ops.hrfpn_pool_bwd([z(1, 8, 8, 6)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_fuse_bwd: invalid argument'):
        ops.hrfpn_fuse_bwd(z(1, 8, 8, 8), [(4, 4), (2, 1)])
    with pytest.raises(CprHipError, match='cpr_hrfpn_fuse_bwd: invalid argument'):
        ops.hrfpn_fuse_bwd(z(1, 8, 8, 8), [(4, 4), (2, 2), (1, 1), (0, 0)])


# ------------------------------------------------------------------------------------------------ the neck
def _neck(cfg):
    import pointtinybenchmark_amd as P
    neck = P.build_neck(dict(type='HRFPN', **HR.neck_kwargs(cfg)))
    neck.load_state_dict(HR.case_state_dict(cfg, torch.float32), strict=True)
    return neck.cuda()


@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_neck_forward_vs_the_reference_fixture(name):
    from pointtinybenchmark_amd import ops
    cfg = HR.cases()[name]
    neck = _neck(cfg)
    xs = [x.cuda() for x in HR.case_inputs(cfg, torch.float32)]
    with torch.no_grad():
        outs = neck(xs)
        tape = []
        lazy = neck.forward_lazy(xs, tape=tape)
    assert len(outs) == cfg['num_outs'] == len(lazy)
    for l, o in enumerate(outs):
        err = HR.output_error(name, l, o)
        print('ERR %s out%d %.3e' % (name, l, err), flush=True)
        assert err <= 2e-4, (name, l, err)
        assert torch.is_tensor(lazy[l]) and torch.equal(ops.as_nchw(lazy[l]), o), 'the lazy form is the materialised map'
    rin, rout = tape
    assert rin['kind'] == 'hrfpn_in' and len(rin['xs']) == len(xs) and rin['sizes'] == [tuple(x.shape[2:]) for x in xs]
    assert rout['kind'] == 'hrfpn_out' and len(rout['levels']) == cfg['num_outs'] and rout['levels'][0] is rout['out']


def test_neck_refuses_sizes_the_reference_cannot_concatenate_and_empty_levels():
    cfg = HR.cases()['i2_o2']
    neck = _neck(cfg)
    a, b = [x.cuda() for x in HR.case_inputs(cfg, torch.float32)]
    with torch.no_grad():
        with pytest.raises(ValueError, match=r'\(10, 14\).*\(5, 6\)'):
            neck([a, b[..., :6].contiguous()])
    cfg = HR.cases()['i1_o2']
    neck = _neck(cfg)
    x, = [x.cuda() for x in HR.case_inputs(cfg, torch.float32)]
    with torch.no_grad():
        with pytest.raises(ValueError, match='1 x 9 level 0 leaves output level 1 empty'):
            neck([x[:, :, :1].contiguous()])


def test_neck_bf16_compute_mode_tracks_fp32():
    """bf16 inputs run the bf16 1x1 and 3x3 kernels; y_i, the fused map and the pooled levels are bf16 and the fuse / pool kernels round
    once on store.  Against the fp64 restatement every stage adds one rounding of relative size <= 2^-9 (inputs, weights, y_i, the fused
    map, a pooled level, the output): rel-L2 <= 6 * 2^-9 < 2^-6 per level."""
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import synthetic
    cfg = dict(in_channels=[64, 128, 256, 512], out_channels=64, num_outs=3, stride=1)
    neck = P.build_neck(dict(type='HRFPN', **cfg))
    sd = synthetic.hrfpn_state_dict(cfg['in_channels'], 64, 3, seed=4, prefix='')
    neck.load_state_dict(sd, strict=True)
    neck = neck.cuda()
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn((2, c, 24 >> i, 40 >> i), generator=g) for i, c in enumerate(cfg['in_channels'])]
    with torch.no_grad():
        outs = neck([x.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for x in xs])
    want = HR.hrfpn_forward({k: v.double() for k, v in sd.items()}, [x.double() for x in xs], 3)
    for l, (o, w) in enumerate(zip(outs, want)):
        assert o.dtype == torch.bfloat16 and o.shape == w.shape
        assert _rel_l2('bf16 neck level %d' % l, o, w) <= 2.0 ** -6


def test_padded_pitch_input_is_read_in_place_and_gives_the_bits_of_its_copy():
    """A MobileNetV2 stage map (24 channels at pitch 32, zeros behind them) handed over as the backbone's view: the level's 1x1 pack has
    zero columns in the pad and reads the buffer in place; a copy of the view takes ops.neck_input's copying route.  Same bits."""
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import ops
    torch.manual_seed(3)
    neck = P.build_neck(dict(type='HRFPN', in_channels=[24, 32], out_channels=32, num_outs=2)).cuda()
    buf = torch.zeros((2, 10, 14, 32)).cuda()
    buf[..., :24] = torch.randn((2, 10, 14, 24)).cuda()
    x1 = torch.randn((2, 32, 5, 7)).cuda()
    view = ops.as_nchw_padded(buf, 24)
    copies = ops.NECK_INPUT_COPIES[0]
    with torch.no_grad():
        a = neck([view, x1])
        assert ops.NECK_INPUT_COPIES[0] == copies, 'the view was copied'
        b = neck([view.clone(), x1])
        assert ops.NECK_INPUT_COPIES[0] == copies + 1
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    want = HR.hrfpn_forward({k: v.detach().double().cpu() for k, v in neck.state_dict().items()},
                            [view.double().cpu(), x1.double().cpu()], 2)
    for l, (o, w) in enumerate(zip(a, want)):
        assert float((o.double().cpu() - w).abs().max()) <= 2e-4 * float(w.abs().max()), l


# ------------------------------------------------------------------------------------------------ the neck's backward
@pytest.mark.parametrize('name', HR.CASE_NAMES)
def test_neck_backward_vs_reference_gradients(name):
    """The recorded forward + BackwardEngine._backward_neck on the fixture's linear functional (dz of level l = w_l) against the reference
    class's fp64 autograd: rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample; the reduction weight per column slice."""
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg = HR.cases()[name]
    neck = _neck(cfg)
    xs = [x.cuda() for x in HR.case_inputs(cfg, torch.float32)]
    eng = BackwardEngine(_NeckOnly(neck))
    eng._sink = {}
    eng.begin_step()
    tape = []
    outs = neck.forward_lazy(xs, tape=tape)
    dzs = [HR.functional_weight(cfg, l, (o.shape[0], o.shape[3], o.shape[1], o.shape[2]), torch.float32).permute(0, 2, 3, 1).contiguous().cuda()
           for l, o in enumerate(outs)]
    d_stage = eng._backward_neck(neck, tape, dzs)
    params = dict(neck.named_parameters())
    grads = dict(zip(params, eng.collect(list(params.values()))))
    torch.cuda.synchronize()
    assert sorted(d_stage) == list(range(len(xs)))
    for i, d in d_stage.items():
        grads['in%d' % i] = d.permute(0, 3, 1, 2)
    lo = 0
    for i, c in enumerate(cfg['in_channels']):
        grads['reduction_slice%d' % i] = grads['reduction_conv.conv.weight'][:, lo:lo + c]
        lo += c
    assert set(grads) == set(HR.grad_names(name))
    failed = []
    for k in sorted(grads):
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        en, es = HR.grad_errors(name, k, grads[k])
        print('ERR backward %-10s %-28s norm %.2e  sample rel-L2 %.2e (bar 2e-3)' % (name, k, en, es), flush=True)
        if not (en <= 2e-3 and es <= 2e-3):
            failed.append((k, en, es))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ the whole locator
NUM_OUTS = {'p2p': 3, 'cpr': 1}
STRIDES = {'p2p': [4, 8, 16], 'cpr': [4]}


def build_locator(head, C=2, seed=3, depth=18, num_outs=None):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    n = NUM_OUTS[head] if num_outs is None else num_outs
    cfg = p2p_model_cfg(depth, C) if head == 'p2p' else model_cfg(depth, C)
    cfg['neck'] = dict(type='HRFPN', in_channels=synthetic.backbone_out_channels(depth), out_channels=256, num_outs=n)
    if head == 'p2p':
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4 << k for k in range(n)], point_anchor=list(GRID4))
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, C, 0, head, seed, **(dict(head_std=0.05, num_points=4) if head == 'p2p' else dict(head_std=0.3)))
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.hrfpn_state_dict(synthetic.backbone_out_channels(depth), 256, n, seed + 1))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m, sd


def _trainer(head):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    return P2PTrainer if head == 'p2p' else CprTrainer


def _ref_losses(head, m, sd64, batch, gt_inds):
    """fp64: the oracle backbone -> tests/hrfpn_ref -> the oracle head and loss (P2P: on the device's own assignment) -> (names, values)."""
    feats = O.resnet_forward(sd64, batch['img'].double(), depth=18)
    outs = HR.hrfpn_forward(sd64, list(feats), NUM_OUTS[head], prefix='neck.')
    assert [tuple(o.shape[2:]) for o in outs] == _cells(STRIDES[head])
    if head == 'cpr':
        cls_feat, _ = O.cpr_head_forward(sd64, outs)
        losses, _ = O.cpr_loss(sd64, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'], 4, 5, 2)
        names = [k for k in losses if 'loss' in k]
        return names, torch.stack([losses[k] for k in names])
    hd = m.bbox_head
    co, po = O.p2p_head_forward(sd64, outs)
    pred, cls = PO.get_pred_points(co, po, STRIDES[head], GRID4, hd.pts_gamma, 2)
    ctr = [(b[:, :2] + b[:, 2:]) / 2 for b in batch['gt_bboxes']]
    counts = [len(c) for c in ctr]
    rc, rp = PO.p2p_loss_from_assignment(cls, pred, gt_inds, torch.cat(ctr).double(), torch.cat(list(batch['gt_labels'])),
                                         torch.tensor([0] + counts[:-1]).cumsum(0), 0.25, 2.0, 1.0 / 9.0, 1.0, 1.0, hd.reg_norm,
                                         1.0, 0.5, 0, 0)
    return ['loss_cls', 'loss_pts'], torch.stack([rc, rp], 1)


@pytest.mark.parametrize('head', ['p2p', 'cpr'])
def test_locator_gradients_vs_fp64_autograd(head):
    """The native trainer's forward_backward on BasicLocator(R18, HRFPN, head) against fp64 autograd of the oracle backbone -> the fp64
    neck restatement -> the oracle head / loss: losses within 3e-4, gradients <= 2e-3 relative L2 per parameter tensor (the bars of
    tests/test_gpu_bfp.py and tests/test_gpu_pafpn.py)."""
    m, sd = build_locator(head)
    batch, data = _data(seed=8)
    rec = _record_assignments(m.bbox_head) if head == 'p2p' else None
    tr = _trainer(head)(m, lr=1e-3)
    losses = tr.forward_backward(**data)
    torch.cuda.synchronize()
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    assert {'neck.reduction_conv.conv.weight', 'neck.reduction_conv.conv.bias', 'neck.fpn_convs.0.conv.bias'} <= trainable
    sd64 = {k: v.double().requires_grad_(k in trainable) for k, v in sd.items()}
    names, ref = _ref_losses(head, m, sd64, batch, rec[-1].cpu() if rec else None)
    if head == 'p2p':
        got = torch.tensor([[float(losses[k][b]) for k in names] for b in range(2)], dtype=torch.float64)
    else:
        got = torch.tensor([float(losses[k]) for k in names], dtype=torch.float64)
    ref_l = ref.detach()
    print('ERR locator %s losses max|diff| %.2e (bar 3e-4 * %.3f)' % (head, float((got - ref_l).abs().max()), max(1.0, float(ref_l.abs().max()))),
          flush=True)
    assert float((got - ref_l).abs().max()) <= 3e-4 * max(1.0, float(ref_l.abs().max())), (got, ref_l)
    ref.sum().backward()
    gmax = max(float(sd64[k].grad.norm()) for k in trainable)
    params = dict(m.named_parameters())
    failed = []
    for k in sorted(trainable):
        gr, rf = params[k].grad.detach().double().cpu().flatten(), sd64[k].grad.flatten()
        rel = float((gr - rf).norm()) / max(float(rf.norm()), 1e-5 * gmax)
        print('ERR locator %s %-44s rel %.2e |g|/gmax %.1e (bar 2e-3)' % (head, k, rel, float(rf.norm()) / gmax), flush=True)
        if not rel <= 2e-3:
            failed.append((k, rel))
    assert not failed, failed


@pytest.mark.parametrize('head', ['p2p', 'cpr'])
def test_bridge_is_bit_equal_to_the_trainer_and_steps_repeat(head):
    from pointtinybenchmark_amd import autograd_bridge
    _, data = _data(seed=8)
    ma, _ = build_locator(head)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr = _trainer(head)(ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb, _ = build_locator(head)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    la_total = float(sum((sum(v) if isinstance(v, (list, tuple)) else v) for k, v in la.items() if 'loss' in k))
    assert abs(out['log_vars']['loss'] - la_total) <= 1e-6 * max(1.0, abs(la_total))
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
    mc, _ = build_locator(head)
    trc = _trainer(head)(mc)
    for _ in range(2):
        tr.forward_backward(**data)
        tr.step()
        trc.forward_backward(**data)
        trc.step()
        torch.cuda.synchronize()
        assert torch.equal(tr.flat_g, trc.flat_g)
    pa, pc = dict(ma.named_parameters()), dict(mc.named_parameters())
    for k in pa:
        assert torch.equal(pa[k], pc[k]), k


@pytest.mark.parametrize('head', ['p2p', 'cpr'])
def test_three_sgd_steps_lower_the_loss_and_ready_points_cover_the_neck(head):
    from pointtinybenchmark_amd import training
    m, _ = build_locator(head)
    _, data = _data()
    with torch.no_grad():
        ref = m.forward_train(**data)
        ref_total = sum(float(v) for k, vs in ref.items() if 'loss' in k for v in (vs if isinstance(vs, (list, tuple)) else [vs]))
    Checked, seen = checked(_trainer(head))
    tr = Checked(m, lr=2e-4, momentum=0.9, weight_decay=1e-4, max_norm=35.0)
    tr.flat_g.fill_(float('nan'))
    convs = [m.neck.reduction_conv.conv] + [cm.conv for cm in m.neck.fpn_convs]
    w0 = [(c.weight.detach().clone(), c.bias.detach().clone()) for c in convs]
    totals = []
    for _ in range(3):
        out = tr.train_step(dict(data))
        tr.check = False
        assert out['log_vars']['loss'] == out['log_vars']['loss'] and abs(out['log_vars']['loss']) < float('inf')
        totals.append(out['log_vars']['loss'])
    print('ERR steps %s totals %s (forward-only %.6f)' % (head, totals, ref_total), flush=True)
    assert seen and max(seen) == tr.flat_g.numel() and seen == sorted(seen)
    # (flat order: per output conv weight then bias, then the reduction conv's bias then weight -- the last of each is declared)
    assert {tr.offset[id(convs[0].weight)][1]} | {tr.offset[id(c.bias)][1] for c in convs[1:]} <= set(seen), \
        'every HRFPN module declares its gradients final'
    assert abs(totals[0] - ref_total) <= 1e-4 * max(1.0, abs(ref_total)), (totals[0], ref_total)
    assert totals[2] < totals[0], totals
    for c, (w, b) in zip(convs, w0):
        assert float((c.weight - w).abs().max()) > 0 and float((c.bias - b).abs().max()) > 0, 'every HRFPN conv and bias trains'


def test_cpr_trainer_and_bridge_refuse_two_levels_naming_the_count():
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import CprTrainer
    m, _ = build_locator('cpr', num_outs=2)
    with pytest.raises(NotImplementedError, match='one pyramid level.*HRFPN has 2 output levels'):
        CprTrainer(m)
    assert 'HRFPN has 2 output levels' in autograd_bridge.unsupported_reason(m)


def test_mixed_precision_step_tracks_the_fp32_step():
    """The bf16 compute mode on the P2P locator with the decomposition and the bars of tests/test_gpu_bfp.py's mixed test, unchanged: worst
    large head / neck tensor <= 0.25, worst large backbone tensor <= 0.5, losses within 5e-2, bf16 gradient kernels against the fp32 ones
    behind the same bf16 forward <= 0.02; the new module's own tensors (reduction_conv.*, fpn_convs.*), same comparison, <= 0.03.  Then the
    bridge, bit-equal to the native mixed step."""
    from pointtinybenchmark_amd import training
    m, _ = build_locator('p2p')
    _, data = _data(seed=22)
    rec = _record_assignments(m.bbox_head)
    tr = training.P2PTrainer(m, lr=1e-3)
    l32 = tr.forward_backward(**data)
    torch.cuda.synchronize()
    g32, inds32 = tr.flat_g.clone(), rec[-1]
    rec16 = _record_assignments(m.bbox_head, force=inds32)
    m.set_compute_dtype('bf16')
    l16 = tr.forward_backward(**data)
    torch.cuda.synchronize()
    g16 = tr.flat_g.clone()
    assert torch.equal(rec16[-1], inds32) and torch.isfinite(g16).all()
    training.MIXED_BF16.update(wgrad=False, dgrad=False)
    try:
        tr.forward_backward(**data)
        torch.cuda.synchronize()
    finally:
        training.MIXED_BF16.update(wgrad=True, dgrad=True)
    gk = tr.flat_g.clone()
    gmax = max(float(p.grad.norm()) for p in m.parameters() if p.requires_grad)
    names = {id(p): k for k, p in m.named_parameters()}
    rows, off, worst_k, worst_new = [], 0, 0.0, 0.0
    for p_ in tr.params:
        n, k = p_.numel(), names[id(p_)]
        a, b, c = g16[off:off + n].double(), g32[off:off + n].double(), gk[off:off + n].double()
        off += n
        rows.append((float((a - b).norm() / max(float(b.norm()), 1e-30)), float(b.norm()) / gmax, k))
        relk = float((a - c).norm() / max(float(c.norm()), 1e-30))
        if k.startswith('neck.'):
            print('ERR mixed new %-36s bf16 vs fp32 backward %.3e (bar 0.03)  vs fp32 step %.3e  |g|/gmax %.2e' % (k, relk, rows[-1][0], rows[-1][1]),
                  flush=True)
            worst_new = max(worst_new, relk)
        elif float(c.norm()) >= 1e-2 * gmax:
            worst_k = max(worst_k, relk)
    for r in sorted(rows, reverse=True)[:8]:
        print('ERR mixed %-44s rel %.3e  |g|/gmax %.2e' % (r[2], r[0], r[1]), flush=True)
    big = [r for r in rows if r[1] >= 1e-2]
    worst_hn = max(r[0] for r in big if not r[2].startswith('backbone.'))
    worst_bb = max([r[0] for r in big if r[2].startswith('backbone.')] or [0.0])
    print('ERR mixed head+neck worst %.4f | backbone worst %.4f | kernels worst %.4f | HRFPN tensors worst %.4f'
          % (worst_hn, worst_bb, worst_k, worst_new), flush=True)
    assert worst_new <= 0.03, 'HRFPN tensors: bf16 backward against the fp32 backward behind the same bf16 forward: %.4f' % worst_new
    assert worst_k <= 0.02, 'bf16 gradient kernels against fp32 ones behind the same bf16 forward: %.4f' % worst_k
    for k in ('loss_cls', 'loss_pts'):
        x, y = sum(float(v) for v in l16[k]), sum(float(v) for v in l32[k])
        assert abs(x - y) <= 5e-2 * max(1.0, abs(y)), (k, x, y)
    assert worst_hn <= 0.25, 'mixed-precision gradient, worst relative L2 over the large head / neck tensors: %.3f' % worst_hn
    assert worst_bb <= 0.5, 'mixed-precision gradient, worst relative L2 over the large backbone tensors: %.3f' % worst_bb
    mb, _ = build_locator('p2p')
    mb.set_compute_dtype('bf16')
    _record_assignments(mb.bbox_head, force=inds32)
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}
    out = mb.train_step(dict(data))
    out['loss'].backward()
    torch.cuda.synchronize()
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
