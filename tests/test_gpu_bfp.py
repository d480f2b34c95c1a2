"""-m gpu: the BFP neck (Balanced Feature Pyramid), forward and training.

  kernels    ops.bfp_gather / bfp_scatter (csrc/bfp.hip) against fp64 torch on two odd pyramids, every refine_level, levels materialised
             and raw under affines of both signs: fp32 |err| <= 1e-5 max|want|, bf16 |err| <= 2^-8 |want| + 1e-5 max|want| (one bf16
             rounding of an fp32 result); two runs bit-equal; an image of a batch of 3 bit-equal to its single-image run
  exact      inputs on a grid of multiples of 2^-6 (|.| <= 4, quantised so that many windows tie), a power-of-two level count: a*x+b, the
             sums and the division are exact in fp32, so values and gradients EQUAL fp64 autograd -- first-maximum routing, negative-a
             routing, overlapping windows, the 6 <-> 74 / 2 <-> 82 axes of the float nearest rule (windows of 41 cells: 16-bit codes)
  backward   bfp_scatter_bwd / bfp_gather_bwd against fp64 autograd per tensor by rel-L2 <= 1e-5 on selection-safe data (values and
             affines exact in fp32, so no argmax can differ; the sums have at most ~50 fp32 terms: <= 50 * 2^-24 = 3e-6 relative)
  neck       per fixture case each output <= 2e-4 max|level| (the a3 bar); the lazy form materialised equals forward; neck gradients
             against the fixture rel-L2 <= 2e-3 on norms and samples (the reference-golden bar)
  locator    R18 128x160, the 4-point grid, C = 2: [FPN, BFP(conv)] on strides [4, 8, 16, 32] and [PAFPN, BFP(None)] on start_level=1,
             num_outs=5: P2PTrainer against fp64 autograd of tests/bfp_ref + the oracle at the bars of test_gpu_pafpn; the bridge bit-equal
             to the trainer, repeatable; three SGD steps lower the loss; bucket ready points; mixed precision; inference; refusals"""
import pytest
import torch
import torch.nn.functional as F

from oracle import cpr_oracle as O
from oracle import p2p_options_oracle as PO
from pointtinybenchmark_amd import synthetic
from tests import bfp_ref as BR
from tests import pafpn_ref as PR
from tests.fpn_extra_ref import fpn_forward
from tests.ready_point_check import run_checked_backward
from tests.test_gpu_fpn_extra import GRID4, _cells, _data, _NeckOnly, _record_assignments

pytestmark = pytest.mark.gpu

PYRAMIDS = {'p5': ([(26, 38), (13, 19), (7, 10), (4, 5), (2, 3)], 64, 2), 'p3': ([(25, 42), (13, 21), (7, 11)], 256, 2)}
PYR_R = [('p5', r) for r in range(5)] + [('p3', r) for r in range(3)]
DT = {torch.float32: 'fp32', torch.bfloat16: 'bf16'}


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2)


def _mat64(x, ab):
    """The fp64 NCHW map a level stands for: x, or x*a + b."""
    y = x.detach().double().cpu()
    if ab is not None:
        y = y * ab[0].double().cpu()[:, None, None, :] + ab[1].double().cpu()[:, None, None, :]
    return y.permute(0, 3, 1, 2).contiguous()


def _bar(want, dtype):
    return 1e-5 * want.abs().max() + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0.0)


def _check(tag, got, want, dtype):
    err = (_nchw64(got) - want).abs()
    bar = _bar(want, dtype)
    print('ERR %-44s max err %.3e  max err / bar %.3f' % (tag, float(err.max()), float((err / bar).max())), flush=True)
    assert bool((err <= bar).all()), (tag, float((err / bar).max()))


def _random_levels(sizes, C, N, dtype, affine, seed):
    """-> (levels as the ops take them, [(x, ab | None)]): normal maps; affines with a of both signs."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for hw in sizes:
        x = torch.randn((N,) + hw + (C,), generator=g).to(dtype).cuda()
        ab = None
        if affine:
            a = (torch.randn((N, C), generator=g) * 0.5 + 1.0) * (torch.randint(0, 2, (N, C), generator=g) * 2 - 1).float()
            ab = (a.cuda(), torch.randn((N, C), generator=g).cuda())
        out.append((x, ab))
    return [x if ab is None else (x, ab) for x, ab in out], out


def _grid_levels(sizes, C, N, dtype, affine, seed, step=2.0 ** -6, pow2_a=False):
    """Values on a grid: x multiples of ``step`` in [-4, 4] quantised to few distinct values (many windows tie); a, b multiples of 2^-6
    in [-4, 4] with a of both signs (pow2_a: a in +-{0.5, 1, 2}), so a*x + b is exact in fp32 (and x exact in bf16 for step 2^-4)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for hw in sizes:
        x = (torch.randint(-4, 5, (N,) + hw + (C,), generator=g).float() * (16 * step)).clamp(-4, 4).to(dtype).cuda()
        ab = None
        if affine:
            sign = (torch.randint(0, 2, (N, C), generator=g) * 2 - 1).float()
            a = sign * (2.0 ** torch.randint(-1, 2, (N, C), generator=g).float() if pow2_a else
                        torch.randint(1, 257, (N, C), generator=g).float() * 2.0 ** -6)
            ab = (a.cuda(), (torch.randint(-256, 257, (N, C), generator=g).float() * 2.0 ** -6).cuda())
        out.append((x, ab))
    return [x if ab is None else (x, ab) for x, ab in out], out


def _grid_grads(sizes, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(-256, 257, (N,) + hw + (C,), generator=g).float() * 2.0 ** -6).cuda() for hw in sizes]


def _autograd64(pairs, r, gs, ref=None):
    """fp64 autograd of the gather (ref None: the scatter reads the gathered map) or of the scatter alone on a given refined map
    ``ref`` (NCHW fp64): -> (bsf | None, outs, d_levels, d_ref | None), all NCHW fp64."""
    xs = [_mat64(x, ab).requires_grad_(True) for x, ab in pairs]
    bsf = None
    if ref is None:
        bsf = BR.bfp_gather(xs, r)
        mid = bsf
    else:
        mid = ref.clone().requires_grad_(True)
    outs = BR.bfp_scatter(xs, r, mid)
    sum((o * _nchw64(g)).sum() for o, g in zip(outs, gs)).backward()
    return bsf, outs, [x.grad for x in xs], (None if ref is None else mid.grad)


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=DT.get)
@pytest.mark.parametrize('affine', [False, True], ids=['materialised', 'raw_affine'])
@pytest.mark.parametrize('pyr,r', PYR_R)
def test_gather_and_scatter_vs_fp64(pyr, r, affine, dtype):
    from pointtinybenchmark_amd import ops
    sizes, C, N = PYRAMIDS[pyr]
    levels, pairs = _random_levels(sizes, C, N, dtype, affine, seed=10 + r)
    bsf = ops.bfp_gather(levels, r)
    bsf_rec, gargs = ops.bfp_gather(levels, r, record=True)
    xs = [_mat64(x, ab) for x, ab in pairs]
    _check('gather %s r=%d %s %s' % (pyr, r, 'raw' if affine else 'mat', DT[dtype]), bsf, BR.bfp_gather(xs, r), dtype)
    assert bsf.dtype == dtype and torch.equal(bsf, bsf_rec) and torch.equal(bsf, ops.bfp_gather(levels, r)), 'gather: runs differ'
    assert [a is not None for a in gargs] == [i < r for i in range(len(sizes))]
    # the refined map: materialised, or raw under an affine of both signs and ReLU
    g = torch.Generator().manual_seed(99 + r)
    h, w = sizes[r]
    ref = torch.randn((N, h, w, C), generator=g).to(dtype).cuda()
    ref_ab, ref64 = None, _mat64(ref, None)
    if affine:
        ref_ab = ((torch.randn((N, C), generator=g) + 0.2).cuda(), (torch.randn((N, C), generator=g) * 0.3).cuda())
        ref64 = _mat64(ref, ref_ab).clamp_min(0)
    outs = ops.bfp_scatter(levels, r, ref, ref_ab)
    outs_rec, sargs = ops.bfp_scatter(levels, r, ref, ref_ab, record=True)
    again = ops.bfp_scatter(levels, r, ref, ref_ab)
    torch.cuda.synchronize()
    for i, (o, want) in enumerate(zip(outs, BR.bfp_scatter(xs, r, ref64))):
        assert o.dtype == dtype and o.shape == pairs[i][0].shape
        _check('scatter %s r=%d level %d %s %s' % (pyr, r, i, 'raw' if affine else 'mat', DT[dtype]), o, want, dtype)
        assert torch.equal(o, outs_rec[i]) and torch.equal(o, again[i]), 'scatter: runs differ'
    assert [a is not None for a in sargs] == [i > r for i in range(len(sizes))]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=DT.get)
def test_an_image_of_a_batch_equals_its_single_image_run(dtype):
    from pointtinybenchmark_amd import ops
    sizes, C, _ = PYRAMIDS['p5']
    r = 2
    levels, pairs = _random_levels(sizes, C, 3, dtype, True, seed=5)
    one = [(x[1:2].contiguous(), (ab[0][1:2].contiguous(), ab[1][1:2].contiguous())) for x, ab in pairs]
    gs = [torch.randn(x.shape, generator=torch.Generator().manual_seed(7 + i)).cuda() for i, (x, _) in enumerate(pairs)]

    def run(lv, g):
        bsf, ga = ops.bfp_gather(lv, r, record=True)
        outs, sa = ops.bfp_scatter(lv, r, bsf, record=True)
        d = ops.bfp_scatter_bwd(g, r, sa)
        return [bsf] + outs + [d] + ops.bfp_gather_bwd(g, r, d, ga)
    full, single = run(levels, gs), run(one, [g[1:2].contiguous() for g in gs])
    torch.cuda.synchronize()
    for a, b in zip(full, single):
        assert torch.equal(a[1:2], b)


def _exact_case(sizes, C, N, r, seed, dtype=torch.float32):
    """Grid data through gather -> scatter (no refine) and the scatter alone on a raw refined map under affine + ReLU; fp32: everything
    equals fp64 autograd exactly."""
    from pointtinybenchmark_amd import ops
    assert len(sizes) in (1, 2, 4, 8), 'a power-of-two level count keeps the division by L exact'
    levels, pairs = _grid_levels(sizes, C, N, dtype, True, seed, step=2.0 ** -6 if dtype == torch.float32 else 2.0 ** -4)
    gs = _grid_grads(sizes, C, N, seed + 1)
    bsf, gargs = ops.bfp_gather(levels, r, record=True)
    outs, sargs = ops.bfp_scatter(levels, r, bsf, record=True)
    d_ref = ops.bfp_scatter_bwd(gs, r, sargs)
    d_lv = ops.bfp_gather_bwd(gs, r, d_ref, gargs)
    want_bsf, want_outs, want_dlv, _ = _autograd64(pairs, r, gs)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        assert torch.equal(_nchw64(bsf), want_bsf.detach()), 'gather values'
        for i in range(len(sizes)):
            assert torch.equal(_nchw64(outs[i]), want_outs[i].detach()), 'scatter values, level %d' % i
            assert torch.equal(_nchw64(d_lv[i]), want_dlv[i]), 'gradient of level %d' % i
    else:
        _check('exact-grid gather bf16', bsf, want_bsf.detach(), dtype)
    # the scatter on a raw refined map: ReLU(ra * x + rb) on load, its gradient wrt the refined (activated) map
    (ref,), ((_, ref_ab),) = _grid_levels([sizes[r]], C, N, dtype, True, seed + 2, step=2.0 ** -6 if dtype == torch.float32 else 2.0 ** -4)
    ref, ref_ab = ref[0], ref_ab
    ref64 = _mat64(ref, ref_ab).clamp_min(0)
    outs2, sargs2 = ops.bfp_scatter(levels, r, ref, ref_ab, record=True)
    d_ref2 = ops.bfp_scatter_bwd(gs, r, sargs2)
    _, want_outs2, _, want_dref2 = _autograd64(pairs, r, gs, ref=ref64)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        for i in range(len(sizes)):
            assert torch.equal(_nchw64(outs2[i]), want_outs2[i].detach()), 'scatter on the raw refined map, level %d' % i
    else:
        for i in range(len(sizes)):
            _check('exact-grid scatter bf16 level %d' % i, outs2[i], want_outs2[i].detach(), dtype)
    assert torch.equal(_nchw64(d_ref2), want_dref2), 'gradient of the refined map'


@pytest.mark.parametrize('r', range(4))
def test_exact_values_and_gradients_equal_fp64_autograd(r):
    _exact_case(PYRAMIDS['p5'][0][:4], 64, 2, r, seed=20 + r)


@pytest.mark.parametrize('r', range(2))
def test_exact_case_bf16_keeps_the_one_rounding_bar_and_routes_exactly(r):
    _exact_case(PYRAMIDS['p3'][0][:2], 256, 2, r, seed=30 + r, dtype=torch.bfloat16)


@pytest.mark.parametrize('r', range(2))
def test_float_nearest_rule_on_the_6_74_and_2_82_axes(r):
    """(74, 82) <-> (6, 2): r = 1 resizes the refined (6, 2) map to (74, 82) by nearest in the scatter and pools (74, 82) to (6, 2) in
    the gather; r = 0 the other way round.  The integer rule dst * in // out differs from torch on both axes; windows of 41 cells take
    the 16-bit argmax codes.  Values and gradients equal fp64 autograd exactly."""
    from pointtinybenchmark_amd import ops
    assert ops.nearest_index(6, 74).tolist() != [d * 6 // 74 for d in range(74)]
    assert ops.nearest_index(2, 82).tolist() != [d * 2 // 82 for d in range(82)]
    _exact_case([(74, 82), (6, 2)], 8, 2, r, seed=40 + r)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=DT.get)
@pytest.mark.parametrize('pyr,r', PYR_R)
def test_backward_kernels_vs_fp64_autograd(pyr, r, dtype):
    """Selection-safe data (x on a grid, a in +-{0.5, 1, 2}: a*x + b exact in fp32, x exact in bf16) with normal upstream gradients
    and any level count: every gradient tensor within rel-L2 1e-5 of fp64 autograd."""
    from pointtinybenchmark_amd import ops
    sizes, C, N = PYRAMIDS[pyr]
    levels, pairs = _grid_levels(sizes, C, N, dtype, True, seed=50 + r, step=2.0 ** -4, pow2_a=True)
    gs = [torch.randn(x.shape, generator=torch.Generator().manual_seed(60 + i)).cuda() for i, (x, _) in enumerate(pairs)]
    (ref,), ((_, ref_ab),) = _grid_levels([sizes[r]], C, N, dtype, True, seed=70 + r, step=2.0 ** -4, pow2_a=True)
    ref = ref[0]
    _, gargs = ops.bfp_gather(levels, r, record=True)
    _, sargs = ops.bfp_scatter(levels, r, ref, ref_ab, record=True)
    d_ref = ops.bfp_scatter_bwd(gs, r, sargs)
    d_bsf = torch.randn(d_ref.shape, generator=torch.Generator().manual_seed(80)).cuda()
    d_lv = ops.bfp_gather_bwd(gs, r, d_bsf, gargs)
    again = ops.bfp_gather_bwd(gs, r, d_bsf, gargs)
    torch.cuda.synchronize()
    assert torch.equal(d_ref, ops.bfp_scatter_bwd(gs, r, sargs)) and all(torch.equal(a, b) for a, b in zip(d_lv, again))
    _, _, _, want_dref = _autograd64(pairs, r, gs, ref=_mat64(ref, ref_ab).clamp_min(0))
    xs = [_mat64(x, ab).requires_grad_(True) for x, ab in pairs]
    (BR.bfp_gather(xs, r) * _nchw64(d_bsf)).sum().backward()
    rows = [('d_ref', _nchw64(d_ref), want_dref)] + [('d_level%d' % i, _nchw64(d), x.grad + _nchw64(g))
                                                     for i, (d, x, g) in enumerate(zip(d_lv, xs, gs))]
    for k, got, want in rows:
        rel = float((got - want).norm() / want.norm())
        print('ERR backward %s r=%d %s %-9s rel-L2 %.2e (bar 1e-5)' % (pyr, r, DT[dtype], k, rel), flush=True)
        assert rel <= 1e-5, (k, rel)


def test_kernels_refuse_what_they_cannot_run():
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd._lib import CprHipError
    x = torch.zeros((1, 2, 2, 6), device='cuda')
    with pytest.raises(CprHipError):
        ops.bfp_gather([x], 0)                              # C % 4 != 0
    with pytest.raises(CprHipError):
        ops.bfp_gather([torch.zeros((1, 2, 2, 12), device='cuda', dtype=torch.bfloat16)], 0)     # bf16: C % 8 != 0
    with pytest.raises(AssertionError):
        ops.bfp_gather([torch.zeros((1, 2, 2, 8), device='cuda'), torch.zeros((1, 1, 1, 16), device='cuda')], 0)
    with pytest.raises(AssertionError):
        ops.bfp_gather([torch.zeros((1, 1, 1, 8), device='cuda')] * 9, 0)


# ------------------------------------------------------------------------------------------------ the neck against the reference
def _neck(name, dtype=torch.float32):
    import pointtinybenchmark_amd as P
    cfg = BR.cases()[name]
    neck = P.build_neck(dict(type='BFP', **BR.neck_kwargs(cfg))).cuda()
    neck.load_state_dict(BR.case_state_dict(cfg, torch.float32), strict=True)
    xs = [x.cuda().to(dtype).contiguous(memory_format=torch.channels_last) for x in BR.case_inputs(cfg, torch.float32)]
    return cfg, neck, xs


@pytest.mark.parametrize('name', BR.CASE_NAMES)
def test_bfp_forward_vs_reference(name):
    from pointtinybenchmark_amd import ops
    cfg, neck, xs = _neck(name)
    with torch.no_grad():
        outs = neck(xs)
        # the lazy form: every level as a raw map under a pending affine (a = 2, b = -1 on half the map's values), materialised by BFP
        N, C = xs[0].shape[:2]
        a, b = torch.full((N, C), 2.0, device='cuda'), torch.full((N, C), -1.0, device='cuda')
        lazy = neck.run([((ops.from_nchw(x) + 1.0) * 0.5, (a, b)) for x in xs])
    torch.cuda.synchronize()
    assert isinstance(outs, tuple) and len(outs) == len(lazy) == cfg['num_levels']
    failed = []
    for l, o in enumerate(outs):
        e = BR.output_error(name, l, o)
        e_lazy = BR.output_error(name, l, ops.as_nchw(lazy[l]))
        print('ERR forward %-14s level %d %-10s max|diff|/max|level| %.2e  lazy %.2e (bar 2e-4)' % (name, l, tuple(o.shape[2:]), e, e_lazy),
              flush=True)
        if not (e <= 2e-4 and e_lazy <= 2e-4):
            failed.append((l, e, e_lazy))
    assert not failed, failed


@pytest.mark.parametrize('inner', ['FPN', 'PAFPN'])
def test_list_neck_lazy_form_materialised_equals_forward(inner):
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd import ops
    gn = dict(type='GN', num_groups=32)
    neck = P.build_neck([dict(type=inner, in_channels=[64, 128, 256, 512], out_channels=64, start_level=1, num_outs=5,
                              add_extra_convs='on_input', norm_cfg=gn),
                         dict(type='BFP', in_channels=64, num_levels=5, refine_level=1, refine_type='conv', norm_cfg=gn)]).cuda()
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn((2, c) + hw, generator=g).cuda().contiguous(memory_format=torch.channels_last)
          for c, hw in zip([64, 128, 256, 512], [(50, 84), (25, 42), (13, 21), (7, 11)])]
    with torch.no_grad():
        outs = neck(xs)
        tape = []
        lazy, taped = neck.forward_lazy(xs), neck.forward_lazy(xs, tape=tape)
        two_step = neck.bfp(neck.inner(xs))          # the reference's Sequential: BFP on the materialised FPN outputs
    torch.cuda.synchronize()
    assert [tuple(o.shape[2:]) for o in outs] == [(25, 42), (13, 21), (7, 11), (4, 6), (2, 3)]
    for o, l, t, s in zip(outs, lazy, taped, two_step):
        assert torch.equal(o, ops.as_nchw(l)), 'forward_lazy != forward'
        assert float((ops.as_nchw(t) - o).abs().max()) <= 2e-4 * float(o.abs().max()), 'the recorded forward'
        assert float((s - o).abs().max()) <= 2e-4 * float(o.abs().max()), 'levels applied on load != levels materialised first'
    assert [r['kind'] for r in tape][-3:] == ['bfp_gather', 'bfp_refine', 'bfp_scatter']


@pytest.mark.parametrize('name', BR.CASE_NAMES)
def test_neck_backward_vs_reference_gradients(name):
    """The recorded forward + BackwardEngine._backward_bfp on the fixture's linear functional (dz of level l = w_l) against the
    reference class's fp64 autograd: rel-L2 <= 2e-3 per tensor, on the norm and on the strided sample."""
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.training import BackwardEngine
    cfg, neck, xs = _neck(name)
    eng = BackwardEngine(_NeckOnly(neck))
    eng._sink = {}
    eng.begin_step()
    tape = []
    outs = neck.run([ops.from_nchw(x) for x in xs], tape)
    dzs = [BR.functional_weight(cfg, l, (o.shape[0], o.shape[3], o.shape[1], o.shape[2]), torch.float32).permute(0, 2, 3, 1).contiguous().cuda()
           for l, o in enumerate(outs)]
    d_in = eng._backward_bfp(neck, tape, dzs)
    params = dict(neck.named_parameters())
    grads = dict(zip(params, eng.collect(list(params.values()))))
    torch.cuda.synchronize()
    for i, d in enumerate(d_in):
        grads['in%d' % i] = d.permute(0, 3, 1, 2)
    assert set(grads) == set(BR.grad_names(name))
    failed = []
    for k in sorted(grads):
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        en, es = BR.grad_errors(name, k, grads[k])
        print('ERR backward %-14s %-22s norm %.2e  sample rel-L2 %.2e (bar 2e-3)' % (name, k, en, es), flush=True)
        if not (en <= 2e-3 and es <= 2e-3):
            failed.append((k, en, es))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ the whole locator
LOCATORS = {
    #             inner neck, start_level, num_outs, add_extra_convs, strides, refine_level, refine_type
    'fpn_conv':   ('FPN', 0, 4, False, [4, 8, 16, 32], 1, 'conv'),
    'pafpn_none': ('PAFPN', 1, 5, 'on_input', [8, 16, 32, 64, 128], 2, None),
}
# admitted by tools/bfp_locator_conditioning.py: fpn_conv 194 (fp32 vs fp64 1.7e-5, kink exposure 1.8e-3; seeds 1-300 scanned),
# pafpn_none 18 (8.2e-6, 1.1e-3; seeds 1-40)
GRAD_SEED = {'fpn_conv': 194, 'pafpn_none': 18}


def _neck_cfg(kind, base):
    inner, start, num_outs, extra, _, r, refine = LOCATORS[kind]
    return [dict(base, type=inner, start_level=start, num_outs=num_outs, add_extra_convs=extra),
            dict(type='BFP', in_channels=256, num_levels=num_outs, refine_level=r, refine_type=refine, norm_cfg=dict(type='GN', num_groups=32))]


def build_locator(kind, C=2, seed=3, depth=18):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    inner, start, num_outs, extra, strides, _, refine = LOCATORS[kind]
    cfg = p2p_model_cfg(depth, C)
    cfg['neck'] = _neck_cfg(kind, cfg['neck'])
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=strides, point_anchor=list(GRID4))
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, C, start, 'p2p', seed, head_std=0.05, num_points=4)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    make = synthetic.pafpn_state_dict if inner == 'PAFPN' else synthetic.fpn_state_dict
    sd.update(make(synthetic.backbone_out_channels(depth), 256, start, num_outs, seed + 1, prefix='neck.0.', add_extra_convs=extra))
    sd.update(synthetic.bfp_state_dict(256, refine, seed + 2, prefix='neck.1.'))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m, sd


def _ref_neck(kind, sd64, feats):
    inner, start, num_outs, extra, _, r, refine = LOCATORS[kind]
    mid = (PR.pafpn_forward if inner == 'PAFPN' else fpn_forward)(sd64, list(feats), num_outs, start, extra, prefix='neck.0.')
    return BR.bfp_forward(sd64, list(mid), r, refine, prefix='neck.1.')


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_locator_gradients_vs_fp64_autograd(kind):
    """P2PTrainer.forward_backward on BasicLocator(R18, [FPN | PAFPN, BFP], P2PHead, the 4-point grid, C=2) against fp64 autograd of the
    oracle backbone -> the fp64 neck restatements (tests/fpn_extra_ref / pafpn_ref, then tests/bfp_ref.bfp_forward) -> oracle head / loss,
    on the device's own assignment: losses within 3e-4, gradients <= 2e-3 relative L2 per parameter tensor (the bars of
    tests/test_gpu_pafpn.py).  The data seed is admitted by the reference alone (tools/bfp_locator_conditioning.py: the oracle network in
    fp32 against its fp64 run within a quarter of the bar, and a head-tower kink exposure below the bar)."""
    from pointtinybenchmark_amd.training import P2PTrainer
    strides = LOCATORS[kind][4]
    m, sd = build_locator(kind)
    batch, data = _data(seed=GRAD_SEED[kind])
    rec = _record_assignments(m.bbox_head)
    tr = P2PTrainer(m, lr=1e-3)
    losses = tr.forward_backward(**data)
    torch.cuda.synchronize()
    gt_inds = rec[-1].cpu()
    assert int((gt_inds > 0).sum()) > 0 and gt_inds.shape[1] == sum(h * w * 4 for h, w in _cells(strides))
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    assert any(k.startswith('neck.0.') for k in trainable) and (LOCATORS[kind][6] is None or 'neck.1.refine.conv.weight' in trainable)
    sd64 = {k: v.double().requires_grad_(k in trainable) for k, v in sd.items()}
    head = m.bbox_head
    feats = O.resnet_forward(sd64, batch['img'].double(), depth=18)
    outs = _ref_neck(kind, sd64, feats)
    assert [tuple(o.shape[2:]) for o in outs] == _cells(strides)
    co, po = O.p2p_head_forward(sd64, outs)
    pred, cls = PO.get_pred_points(co, po, strides, GRID4, head.pts_gamma, 2)
    ctr = [(b[:, :2] + b[:, 2:]) / 2 for b in batch['gt_bboxes']]
    counts = [len(c) for c in ctr]
    rc, rp = PO.p2p_loss_from_assignment(cls, pred, gt_inds, torch.cat(ctr).double(), torch.cat(list(batch['gt_labels'])),
                                         torch.tensor([0] + counts[:-1]).cumsum(0), 0.25, 2.0, 1.0 / 9.0, 1.0, 1.0, head.reg_norm,
                                         1.0, 0.5, 0, 0)
    got_l = torch.tensor([[float(losses['loss_cls'][b]), float(losses['loss_pts'][b])] for b in range(2)], dtype=torch.float64)
    ref_l = torch.stack([rc, rp], 1).detach()
    print('ERR locator %-12s losses max|diff| %.2e (bar 3e-4 * %.3f)' % (kind, float((got_l - ref_l).abs().max()),
                                                                        max(1.0, float(ref_l.abs().max()))), flush=True)
    assert float((got_l - ref_l).abs().max()) <= 3e-4 * max(1.0, float(ref_l.abs().max())), (got_l, ref_l)
    (rc.sum() + rp.sum()).backward()
    gmax = max(float(sd64[k].grad.norm()) for k in trainable)
    params = dict(m.named_parameters())
    failed = []
    for k in sorted(trainable):
        gr, ref = params[k].grad.detach().double().cpu().flatten(), sd64[k].grad.flatten()
        rel = float((gr - ref).norm()) / max(float(ref.norm()), 1e-5 * gmax)
        print('ERR locator %-12s %-44s rel %.2e |g|/gmax %.1e (bar 2e-3)' % (kind, k, rel, float(ref.norm()) / gmax), flush=True)
        if not rel <= 2e-3:
            failed.append((k, rel))
    assert not failed, failed


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_bridge_is_bit_equal_to_the_trainer_and_steps_repeat(kind):
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import P2PTrainer
    _, data = _data(seed=8)
    ma, _ = build_locator(kind)
    assert autograd_bridge.unsupported_reason(ma, data['gt_bboxes'], data['gt_labels']) is None
    tr = P2PTrainer(ma)
    la = tr.forward_backward(**data)
    torch.cuda.synchronize()
    want = {k: p.grad.clone() for k, p in ma.named_parameters() if p.requires_grad}
    mb, _ = build_locator(kind)
    out = mb.train_step(dict(data))
    assert out['loss'].requires_grad and out['loss'].grad_fn is not None
    out['loss'].backward()
    torch.cuda.synchronize()
    la_total = float(sum(sum(v) for k, v in la.items() if 'loss' in k))
    assert abs(out['log_vars']['loss'] - la_total) <= 1e-6 * max(1.0, abs(la_total))
    for k, p in mb.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, want[k]), k
    mc, _ = build_locator(kind)
    trc = P2PTrainer(mc)
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


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_three_sgd_steps_lower_the_loss(kind):
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = build_locator(kind)
    _, data = _data()
    with torch.no_grad():
        ref = m.forward_train(**data)
        ref_total = sum(float(v) for vs in ref.values() for v in vs)
    tr = P2PTrainer(m, lr=2e-4, momentum=0.9, weight_decay=1e-4, max_norm=35.0)
    mods = list(m.neck.inner.fpn_convs) + ([m.neck.bfp.refine] if m.neck.bfp.refine_type else [])
    w0 = [cm.conv.weight.detach().clone() for cm in mods]
    totals = []
    for _ in range(3):
        out = tr.train_step(dict(data))
        assert out['log_vars']['loss'] == out['log_vars']['loss'] and abs(out['log_vars']['loss']) < float('inf')
        totals.append(out['log_vars']['loss'])
    print('ERR steps %-12s totals %s (forward-only %.6f)' % (kind, totals, ref_total), flush=True)
    assert abs(totals[0] - ref_total) <= 1e-4 * max(1.0, abs(ref_total)), (totals[0], ref_total)
    assert totals[2] < totals[0], totals
    for cm, w in zip(mods, w0):
        assert float((cm.conv.weight - w).abs().max()) > 0, 'every neck conv, the refine layer included, trains'


@pytest.mark.parametrize('kind', list(LOCATORS))
def test_bucket_ready_points_cover_the_refine_conv(kind):
    from pointtinybenchmark_amd import training
    m, _ = build_locator(kind)
    _, data = _data(seed=8)
    tr, seen = run_checked_backward(training.P2PTrainer, m, data)
    mods = list(m.neck.inner.fpn_convs) + ([m.neck.bfp.refine] if m.neck.bfp.refine_type else [])
    assert {tr.offset[id(cm.conv.weight)][1] for cm in mods} <= set(seen), 'every neck conv, the refine conv included, declares its gradients final'


def test_mixed_precision_step_tracks_the_fp32_step():
    """The bf16 compute mode on the 'fpn_conv' locator with the bars of tests/test_gpu_pafpn.py's mixed test, unchanged: worst large head /
    neck tensor <= 0.25, worst large backbone tensor <= 0.5, losses within 5e-2, bf16 gradient kernels against the fp32 ones behind the same
    bf16 forward <= 0.02; the new module's own tensors (the refine layer), same comparison, <= 0.03.  Then the bridge, bit-equal to the
    native mixed step."""
    from pointtinybenchmark_amd import training
    from pointtinybenchmark_amd.training import P2PTrainer
    m, _ = build_locator('fpn_conv')
    _, data = _data(seed=22)
    rec = _record_assignments(m.bbox_head)
    tr = P2PTrainer(m, lr=1e-3)
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
        if k.startswith('neck.1.'):
            print('ERR mixed new %-30s bf16 vs fp32 backward %.3e (bar 0.03)  vs fp32 step %.3e  |g|/gmax %.2e' % (k, relk, rows[-1][0], rows[-1][1]),
                  flush=True)
            worst_new = max(worst_new, relk)
        elif float(c.norm()) >= 1e-2 * gmax:
            worst_k = max(worst_k, relk)
    for r in sorted(rows, reverse=True)[:8]:
        print('ERR mixed %-44s rel %.3e  |g|/gmax %.2e' % (r[2], r[0], r[1]), flush=True)
    big = [r for r in rows if r[1] >= 1e-2]
    worst_hn = max(r[0] for r in big if not r[2].startswith('backbone.'))
    worst_bb = max([r[0] for r in big if r[2].startswith('backbone.')] or [0.0])
    print('ERR mixed head+neck worst %.4f | backbone worst %.4f | kernels worst %.4f | refine layer worst %.4f'
          % (worst_hn, worst_bb, worst_k, worst_new), flush=True)
    assert worst_new <= 0.03, 'refine layer: bf16 backward against the fp32 backward behind the same bf16 forward: %.4f' % worst_new
    assert worst_k <= 0.02, 'bf16 gradient kernels against fp32 ones behind the same bf16 forward: %.4f' % worst_k
    for k in ('loss_cls', 'loss_pts'):
        x, y = sum(float(v) for v in l16[k]), sum(float(v) for v in l32[k])
        assert abs(x - y) <= 5e-2 * max(1.0, abs(y)), (k, x, y)
    assert worst_hn <= 0.25, 'mixed-precision gradient, worst relative L2 over the large head / neck tensors: %.3f' % worst_hn
    assert worst_bb <= 0.5, 'mixed-precision gradient, worst relative L2 over the large backbone tensors: %.3f' % worst_bb
    mb, _ = build_locator('fpn_conv')
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


# ------------------------------------------------------------------------------------------------ inference, refusals
def test_extract_feat_returns_the_levels():
    for kind, want in (('fpn_conv', [(32, 40), (16, 20), (8, 10), (4, 5)]), ('pafpn_none', [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)])):
        m, _ = build_locator(kind)
        m.eval()
        _, data = _data()
        with torch.no_grad():
            feats = m.extract_feat(data['img'])
            # (the reference cuts the concatenated proposals into len(strides) equal chunks, p2p_head.py:357: 1700 cells over four levels do)
            res = m.simple_test(data['img'], data['img_metas']) if kind == 'fpn_conv' else [None, None]
        torch.cuda.synchronize()
        assert [tuple(f.shape) for f in feats] == [(2, 256) + hw for hw in want]
        assert all(bool(torch.isfinite(f).all()) for f in feats) and len(res) == 2


def test_a_one_element_list_is_refused_and_a_dict_neck_is_what_it_was():
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    cfg = p2p_model_cfg(18, 2)
    base = dict(cfg['neck'], start_level=0, num_outs=4)
    with pytest.raises(NotImplementedError, match='FPN'):
        P.build_detector(dict(cfg, neck=[base]))
    # the FPN of a dict-valued neck and the FPN inside the list are the same class running the same code: bit-equal levels
    strides = dict(cfg['bbox_head'], strides=[4, 8, 16, 32], point_anchor=list(GRID4))
    md = P.build_detector(dict(cfg, neck=base, bbox_head=strides)).cuda().eval()
    ml, _ = build_locator('fpn_conv')
    ml.eval()
    assert type(md.neck).__name__ == 'FPN' and type(ml.neck.inner) is type(md.neck)
    md.backbone.load_state_dict(ml.backbone.state_dict())
    md.neck.load_state_dict(ml.neck.inner.state_dict())
    _, data = _data()
    with torch.no_grad():
        feats = md.backbone(data['img'])
        a, b = md.neck(feats), ml.neck.inner(feats)
        c = md.extract_feat(data['img'])
    torch.cuda.synchronize()
    assert len(a) == 4 and all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
