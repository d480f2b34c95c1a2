"""-m gpu: the six split-attention kernels (csrc/splat.hip) against fp64 torch and its autograd adjoints (tests/splat_ref.py).

  shapes     w in {64, 96, 512}, inter in {32, 48, 256}, N in {1, 3}, maps 1x1, 7x9, 17x23, 18x24 (both pool to 9x12), 40x40 -- one to
             ten pixel chunks per image, w / 4 = 24 lanes per pixel leaves an idle tail in the workgroup
  bar        rel-L2 <= 1e-5 per output (tests/splat_ref.BAR); the fp32 torch restatement alone stays within a quarter of it on these
             inputs (tests/test_resnest_host.py)
  further    logits of +-60 stay finite and match fp64; output and scratch buffers pre-filled with NaN come back fully written;
             (one, two and seven chunks per image); bit-repeatable; image k of a batch of 3 equals its solo run bit for bit; 17x23 and 18x24
             inputs are told apart under the same pooled gradient; w % 4 != 0 is the argument error of every entry point"""
import ctypes

import pytest
import torch

from tests import splat_ref as SR

pytestmark = pytest.mark.gpu
POOLS = [False, True]


def _dev(d):
    return {k: v.cuda().contiguous() for k, v in d.items()}


def _fold(d):
    """(scale, shift, inv_sigma) of the eval BatchNorm, fp32 on the device, from fp64 arithmetic rounded once."""
    inv = 1.0 / torch.sqrt(d['bn_var'].double() + 1e-5)
    s = d['bn_w'].double() * inv
    return s.float().cuda(), (d['bn_b'].double() - d['bn_mean'].double() * s).float().cuda(), inv.float().cuda()


def _check(tag, got, want):
    e = SR.rel_l2(got, want)
    print('ERR splat %-34s rel-L2 %.2e (bar 1e-5)' % (tag, e), flush=True)
    assert e <= SR.BAR, (tag, e)


_REF = {}


def _ref(shape, pool):
    """The fp64 reference of one (shape, pool), computed once and left unchanged."""
    key = (shape, pool)
    if key not in _REF:
        d = SR.inputs(shape)
        f = SR.forward(d, torch.float64, pool)
        att_in = torch.softmax(torch.randn(d['datt'].shape, generator=torch.Generator().manual_seed(3)).double(), 1)
        datt, du, cs = SR.map_backward(d, att_in, torch.float64, pool)
        _REF[key] = dict(d=d, fwd=f, att_in=att_in, datt=datt, du=du, cs=cs)
    return _REF[key]


@pytest.mark.parametrize('shape', SR.SHAPES, ids=SR.IDS)
def test_forward_chain_vs_fp64(shape):
    """splat_gap, splat_attn (att and the recorded z) and splat_apply with and without the pool, each on the fp64 reference's input."""
    from pointtinybenchmark_amd import ops
    for pool in POOLS:
        r = _ref(shape, pool)
        d, f = _dev(r['d']), r['fwd']
        s, t, _ = _fold(r['d'])
        if not pool:
            g = ops.splat_gap(d['u'])
            _check('gap %s' % (shape,), g, f['g'])
            att, z = ops.splat_attn(f['g'].float().cuda(), d['fc1_w'], d['fc1_b'], s, t, d['fc2_w'], d['fc2_b'], record=True)
            _check('attn att %s' % (shape,), att, f['att'])
            _check('attn z %s' % (shape,), z, f['z'])
            assert torch.equal(att, ops.splat_attn(f['g'].float().cuda(), d['fc1_w'], d['fc1_b'], s, t, d['fc2_w'], d['fc2_b']))
        out = ops.splat_apply(d['u'], f['att'].float().cuda(), pool=pool)
        assert tuple(out.shape) == (shape[2],) + SR.pooled(shape[3], shape[4], pool) + (shape[0],)
        _check('apply pool=%d %s' % (pool, shape), out, f['out'])


@pytest.mark.parametrize('shape', SR.SHAPES, ids=SR.IDS)
def test_map_backward_vs_fp64_autograd(shape):
    """splat_attn_grad and splat_apply_bwd (du and its column sums) against the autograd adjoints, with and without the pool."""
    from pointtinybenchmark_amd import ops
    for pool in POOLS:
        r = _ref(shape, pool)
        d = _dev(r['d'])
        att = r['att_in'].float().cuda()
        dout = d['dout_pool' if pool else 'dout']
        _check('attn_grad pool=%d %s' % (pool, shape), ops.splat_attn_grad(dout, d['u'], pool=pool), r['datt'])
        du, cs = ops.splat_apply_bwd(dout, d['u'], att, d['dg'], pool=pool)
        _check('apply_bwd du pool=%d %s' % (pool, shape), du, r['du'])
        _check('apply_bwd colsum pool=%d %s' % (pool, shape), cs, r['cs'])
        assert int(torch.count_nonzero(du[d['u'] == 0])) == 0


@pytest.mark.parametrize('shape', SR.SHAPES[:4], ids=SR.IDS[:4])
def test_attention_backward_vs_fp64_autograd(shape):
    """splat_attn_bwd: dg and the six parameter gradients (images added up) against fp64 autograd with the recorded ReLU pattern."""
    from pointtinybenchmark_amd import ops
    d0 = SR.inputs(shape)
    att64, z64 = SR.attention_from(d0, torch.float64)
    want = SR.attn_backward(d0, z64, torch.float64)
    d = _dev(d0)
    s, _, inv = _fold(d0)
    w, inter = shape[0], shape[1]
    grads = dict(fc1_w=torch.empty(inter, w, 1, 1), fc1_b=torch.empty(inter), bn_w=torch.empty(inter), bn_b=torch.empty(inter),
                 fc2_w=torch.empty(2 * w, inter, 1, 1), fc2_b=torch.empty(2 * w))
    grads = {k: v.cuda() for k, v in grads.items()}
    dg = ops.splat_attn_bwd(att64.float().cuda(), d['datt'], z64.float().cuda(), d['gvec'], d['fc1_w'], d['fc1_b'], s, d['bn_mean'], inv,
                            d['fc2_w'], grads=grads)
    _check('attn_bwd dg %s' % (shape,), dg, want['dg'])
    for k, g in grads.items():
        _check('attn_bwd %s %s' % (k, shape), g, want[k])
    # no gradient buffers: dg alone, the same bits
    assert torch.equal(dg, ops.splat_attn_bwd(att64.float().cuda(), d['datt'], z64.float().cuda(), d['gvec'], d['fc1_w'], d['fc1_b'], s,
                                              d['bn_mean'], inv, d['fc2_w']))


def test_logits_of_sixty_stay_finite_and_match_fp64():
    from pointtinybenchmark_amd import ops
    shape = (64, 32, 3, 7, 9)
    d0 = SR.inputs(shape)
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    d0['fc2_w'] = d0['fc2_w'] * 0.01
    d0['fc2_b'] = torch.cat([60.0 * sign, -60.0 * sign])
    att64, _ = SR.attention_from(d0, torch.float64)
    d = _dev(d0)
    s, t, _ = _fold(d0)
    att = ops.splat_attn(d['gvec'], d['fc1_w'], d['fc1_b'], s, t, d['fc2_w'], d['fc2_b'])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(att).all()) and float(att.min()) >= 0.0 and float(att.max()) <= 1.0
    assert float((att.sum(1) - 1).abs().max()) <= 1e-6
    _check('attn logits +-60', att, att64)
    assert float((att.double().cpu() - att64).abs().max()) <= 1e-6


def _raw(name, *args):
    from pointtinybenchmark_amd import _lib
    _lib.call(name, *[ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args],
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize('shape,chunks', [((96, 48, 3, 7, 9), 1), ((512, 256, 3, 7, 9), 2), ((64, 32, 3, 40, 40), 7)], ids=['k1', 'k2', 'k7'])
@pytest.mark.parametrize('pool', POOLS)
def test_nan_filled_outputs_and_scratch_come_back_written(pool, shape, chunks):
    """Every entry point on caller-allocated NaN-filled outputs and workspaces: the outputs are fully written and equal the wrappers'
    bits, so no kernel reads scratch it did not write -- with one, two and seven pixel chunks per image (the ws[n][k][...] layout and
    the per-image tail of apply_bwd's workspace)."""
    from pointtinybenchmark_amd import _lib, ops
    w, inter, N, H, W = shape
    d0 = SR.inputs(shape)
    d = _dev(d0)
    s, t, inv = _fold(d0)
    K = _lib.call('cpr_splat_chunks', H, W, w, positive=True)
    assert K == 1 + (H * W - 1) // (16 * (256 // (w // 4))) == chunks

    def nan(*sh):
        return torch.full(sh, float('nan'), device='cuda')
    g, ws = nan(N, w), nan(N * K * w)
    _raw('cpr_splat_gap', d['u'], g, ws, N, H, W, w)
    assert torch.equal(g, ops.splat_gap(d['u']))
    att, z = nan(N, 2, w), nan(N, inter)
    _raw('cpr_splat_attn', g, d['fc1_w'], d['fc1_b'], s, t, d['fc2_w'], d['fc2_b'], att, z, N, w, inter)
    a2, z2 = ops.splat_attn(g, d['fc1_w'], d['fc1_b'], s, t, d['fc2_w'], d['fc2_b'], record=True)
    assert torch.equal(att, a2) and torch.equal(z, z2)
    OH, OW = SR.pooled(H, W, pool)
    out = nan(N, OH, OW, w)
    _raw('cpr_splat_apply', d['u'], att, out, N, H, W, w, int(pool))
    assert torch.equal(out, ops.splat_apply(d['u'], att, pool=pool))
    dout = d['dout_pool' if pool else 'dout']
    datt, ws = nan(N, 2, w), nan(N * K * 2 * w)
    _raw('cpr_splat_attn_grad', dout, d['u'], datt, ws, N, H, W, w, int(pool))
    assert torch.equal(datt, ops.splat_attn_grad(dout, d['u'], pool=pool))
    dg, ws = nan(N, w), nan(N * (2 * w + 3 * inter))
    pg = [nan(inter * w), nan(inter), nan(inter), nan(inter), nan(2 * w * inter), nan(2 * w)]
    _raw('cpr_splat_attn_bwd', att, datt, z, g, d['fc1_w'], d['fc1_b'], s, d['bn_mean'], inv, d['fc2_w'], dg, ws, *pg, N, w, inter)
    keys = ('fc1_w', 'fc1_b', 'bn_w', 'bn_b', 'fc2_w', 'fc2_b')
    want = {k: torch.empty_like(v) for k, v in zip(keys, pg)}
    assert torch.equal(dg, ops.splat_attn_bwd(att, datt, z, g, d['fc1_w'], d['fc1_b'], s, d['bn_mean'], inv, d['fc2_w'], grads=want))
    for k, v in zip(keys, pg):
        assert torch.equal(v, want[k]), k
    du, cs, ws = nan(N, H, W, 2 * w), nan(2 * w), nan(N * K * 2 * w + N * 2 * w)
    _raw('cpr_splat_apply_bwd', dout, d['u'], att, dg, du, cs, ws, N, H, W, w, int(pool))
    du2, cs2 = ops.splat_apply_bwd(dout, d['u'], att, dg, pool=pool)
    assert torch.equal(du, du2) and torch.equal(cs, cs2)
    torch.cuda.synchronize()
    for name, v in [('g', g), ('att', att), ('z', z), ('out', out), ('datt', datt), ('dg', dg), ('du', du), ('cs', cs)] + list(zip(keys, pg)):
        assert bool(torch.isfinite(v).all()), name


def _all_outputs(d, fold, pool):
    from pointtinybenchmark_amd import ops
    s, t, inv = fold
    g = ops.splat_gap(d['u'])
    att, z = ops.splat_attn(g, d['fc1_w'], d['fc1_b'], s, t, d['fc2_w'], d['fc2_b'], record=True)
    out = ops.splat_apply(d['u'], att, pool=pool)
    dout = d['dout_pool' if pool else 'dout']
    datt = ops.splat_attn_grad(dout, d['u'], pool=pool)
    dg = ops.splat_attn_bwd(att, datt, z, g, d['fc1_w'], d['fc1_b'], s, d['bn_mean'], inv, d['fc2_w'])
    du, cs = ops.splat_apply_bwd(dout, d['u'], att, dg, pool=pool)
    return dict(g=g, att=att, z=z, out=out, datt=datt, dg=dg, du=du), cs


@pytest.mark.parametrize('shape', [SR.SHAPES[1], SR.SHAPES[6]], ids=[SR.IDS[1], SR.IDS[6]])
@pytest.mark.parametrize('pool', POOLS)
def test_bit_repeatable_and_batch_independent(shape, pool):
    """The whole chain twice: the same bits; and image k of the batch of 3 equals the chain run on that image alone, bit for bit."""
    d0 = SR.inputs(shape)
    d, fold = _dev(d0), _fold(d0)
    a, cs_a = _all_outputs(d, fold, pool)
    b, cs_b = _all_outputs(d, fold, pool)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(cs_a, cs_b)
    per_image = ('u', 'dout', 'dout_pool', 'gvec', 'dg', 'datt')
    for n in range(shape[2]):
        solo, _ = _all_outputs({k: (v[n:n + 1].contiguous() if k in per_image else v) for k, v in d.items()}, fold, pool)
        for k in a:
            assert torch.equal(a[k][n:n + 1], solo[k]), (k, n)


def test_17x23_and_18x24_are_told_apart_under_the_same_pooled_gradient():
    from pointtinybenchmark_amd import ops
    w, N = 64, 2
    g = torch.Generator().manual_seed(9)
    dout = torch.randn((N, 9, 12, w), generator=g)
    att = torch.softmax(torch.randn((N, 2, w), generator=g), 1)
    dg = torch.randn((N, w), generator=g)
    res = {}
    for hw in ((17, 23), (18, 24)):
        u = torch.relu(torch.randn((N,) + hw + (2 * w,), generator=g))
        d = dict(u=u, dout_pool=dout, dg=dg)
        datt, du, cs = SR.map_backward(d, att.double(), torch.float64, True)
        got_datt = ops.splat_attn_grad(dout.cuda(), u.cuda(), pool=True)
        got_du, got_cs = ops.splat_apply_bwd(dout.cuda(), u.cuda(), att.cuda(), dg.cuda(), pool=True)
        assert tuple(got_du.shape) == (N,) + hw + (2 * w,)
        _check('attn_grad %dx%d' % hw, got_datt, datt)
        _check('apply_bwd %dx%d' % hw, got_du, du)
        _check('apply_bwd colsum %dx%d' % hw, got_cs, cs)
        res[hw] = got_du
    # row 17 / column 23 of the larger map lie in the last windows alone: they exist only there
    assert float(res[(18, 24)][:, 17].abs().max()) > 0 and float(res[(18, 24)][:, :, 23].abs().max()) > 0


def test_width_not_a_multiple_of_four_is_the_argument_error():
    from pointtinybenchmark_amd import _lib, ops
    u = torch.zeros((1, 3, 3, 2 * 6), device='cuda')
    att = torch.full((1, 2, 6), 0.5, device='cuda')
    dout = torch.zeros((1, 3, 3, 6), device='cuda')
    vec = torch.zeros((1, 6), device='cuda')
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.splat_gap(u)
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.splat_apply(u, att)
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.splat_attn_grad(dout, u)
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.splat_apply_bwd(dout, u, att, vec)
    p = dict(fc1_w=torch.zeros((32, 6, 1, 1), device='cuda'), b=torch.zeros(32, device='cuda'), fc2_w=torch.zeros((12, 32, 1, 1), device='cuda'),
             fc2_b=torch.zeros(12, device='cuda'))
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.splat_attn(vec, p['fc1_w'], p['b'], p['b'], p['b'], p['fc2_w'], p['fc2_b'])
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        ops.splat_attn_bwd(att, att, torch.zeros((1, 32), device='cuda'), vec, p['fc1_w'], p['b'], p['b'], p['b'], p['b'], p['fc2_w'])
    # the wrappers of the three reductions raise from their workspace query: the entry points' own check, called directly
    ws, out = torch.zeros(4096, device='cuda'), torch.zeros((1, 3, 3, 12), device='cuda')
    for name, args in (('cpr_splat_gap', (u, vec, ws, 1, 3, 3, 6)), ('cpr_splat_attn_grad', (dout, u, att, ws, 1, 3, 3, 6, 0)),
                       ('cpr_splat_apply_bwd', (dout, u, att, vec, out, torch.zeros(12, device='cuda'), ws, 1, 3, 3, 6, 0)),
                       ('cpr_splat_apply', (u, att, out, 1, 3, 3, 6, 0))):
        with pytest.raises(_lib.CprHipError, match='%s: invalid argument' % name):
            _raw(name, *args)
    assert _lib.load().cpr_splat_chunks(3, 3, 6) == -1001
