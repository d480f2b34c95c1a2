"""-m gpu: the two-pass reduction entries through their C entry points, on every case of tests/reduce_plan_ref.py -- one kernel writes
per-workgroup partials into a caller-allocated workspace, a second adds them in a fixed order:

  cpr_leaky_bwd_colsum, cpr_relu6_bwd_colsum, cpr_res2_relu_bwd_colsum                      the column-sum passes
  cpr_res2_conv_wgrad, cpr_conv_group_wgrad[_pitch|_dil], cpr_dw3x3_wgrad,
  cpr_stem3x3s1_wgrad, cpr_stem3x3s2_wgrad                                                  the weight gradients
  cpr_dw3x3_dgrad with column sums                                                          a data gradient that leaves partials
  cpr_hrnet_fuse_bwd, cpr_hrfpn_pool_bwd                                                    partials the later cpr_part_colsum adds

Every case runs three times:
  A   outputs and workspace are slices of an arena of 0xFF bytes (NaN as fp32) with 64 guard elements on either side; the workspace is
      exactly the floats the entry's own query returns (which must be the number tests/reduce_plan_ref.py restates)
  B   the same with the workspace pre-filled with 3e38 and the outputs with -7.25
  C   the ``ops`` wrapper, as the product calls it
and must return status 0, leave every guard byte 0xFF, write every output element (no 0xFFFFFFFF left from run A), keep the channels
outside a written slice of a pitched map at their prefill bits, give the same bits in A, B and C -- so nothing a workspace held before
the call reaches a result: a slot the second kernel reads and the first did not write would bring NaN into A and 3e38 into B -- and
stay within the family's existing bar of the fp64 reference (tests/reduce_plan_ref.py lists the bars).  accumulate = 1 must equal
base + got exactly.  The operands sit between NaN bytes too, so a read past their end does not find zeros.  Each entry also gets a
refused call (a bad size, a misaligned slice or workspace): the documented error code, and outputs that keep their prefill.

tests/test_reduce_instances_host.py holds the restated plans to the source text and to the queries, asserts the tables' coverage and
shows on the references alone that each bar sees one left-out pixel.  The file prints its wall time and the worst |err| / bar per
family when its last test is done (pytest -s shows it); CHANGELOG.md records them."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import reduce_plan_ref as P

pytestmark = pytest.mark.gpu

INPUT_GUARD_BYTES = 4096
ERR_ARG = -1001
T0 = [None]
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _wall_time():
    T0[0] = time.perf_counter()
    yield
    torch.cuda.synchronize()
    for fam in sorted(WORST):
        print('\n%-28s worst |err| / bar = %.3g' % (fam, WORST[fam]), end='')
    print('\ntests/test_gpu_reduce_instances.py: %.1f s wall time' % (time.perf_counter() - T0[0]))


def note(fam, ratio):
    WORST[fam] = max(WORST.get(fam, 0.0), float(ratio))
    return ratio


# ---- plumbing ----------------------------------------------------------------------------------------------------
def _lib():
    from pointtinybenchmark_amd import _lib
    return _lib


def _ops():
    from pointtinybenchmark_amd import ops
    return ops


def _args(args):
    out = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    return out + [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]


def call(name, *args):
    """The C entry through _lib.call: 0, or CprHipError."""
    return _lib().call(name, *_args(args))


def status(name, *args):
    """The C entry's own return value."""
    return getattr(_lib().load(), name)(*_args(args))


def query(name, *args):
    return _lib().call(name, *args, positive=True)


def dev(t):
    """An operand on the device in the middle of 0xFF bytes: a read past its end finds NaN, not what the allocator left there."""
    if t is None:
        return None
    t = t.contiguous()
    nbytes = t.numel() * 4
    buf = torch.full((2 * INPUT_GUARD_BYTES + (nbytes + 255) // 256 * 256,), 0xFF, dtype=torch.uint8, device='cuda')
    view = buf[INPUT_GUARD_BYTES:INPUT_GUARD_BYTES + nbytes].view(torch.float32).view(t.shape)
    view.copy_(t)
    return view


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(name, a, b):
    a, b = bits(a).reshape(-1), bits(b.to(a.device)).reshape(-1)
    assert a.numel() == b.numel(), (name, a.numel(), b.numel())
    ne = torch.nonzero(a != b)
    assert ne.numel() == 0, '%s: %d of %d elements differ, the first at %d: 0x%08X != 0x%08X' % (
        name, ne.numel(), a.numel(), int(ne[0]), int(a[ne[0]]) & 0xFFFFFFFF, int(b[ne[0]]) & 0xFFFFFFFF)


def within(name, fam, got, ref, bar):
    got, ref, bar = (torch.as_tensor(v).detach().double().cpu().reshape(-1) for v in (got, ref, bar))
    assert bool(torch.isfinite(got).all()), '%s: a non-finite result' % name
    err = (got - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bar).max())
    print('%s: worst |err| / bar = %.3g' % (name, ratio))
    note(fam, ratio)
    assert ratio <= 1.0, '%s: %d of %d over the bar, worst ratio %.3g' % (name, int((err > bar).sum()), err.numel(), ratio)


def arena_runs(name, specs, launch, init=None):
    """Runs A and B of one case.  specs: [(slice, floats, 'out' | 'ws')]; init(arena, run) writes what the entry reads from its own
    outputs (an accumulated gradient, an in-place map) after the prefill; launch(arena) -> status.  Yields (run, arena) after the
    launch, with the status and the guards already checked."""
    for run in 'AB':
        a = P.Arena([(n, k) for n, k, _ in specs])
        if run == 'B':
            for n, _, role in specs:
                a[n].fill_(P.POISON_WS if role == 'ws' else P.POISON_OUT)
        if init is not None:
            init(a, run)
        assert launch(a) == 0, '%s run %s: status' % (name, run)
        torch.cuda.synchronize()
        a.intact('%s run %s' % (name, run))
        yield run, a


def all_written(name, a, slices):
    for n in slices:
        assert a.unwritten(n) == 0, '%s: %d elements of %s were not written' % (name, a.unwritten(n), n)
        assert not bool(torch.isnan(a[n]).any()), '%s: NaN in %s' % (name, n)


def prefill_bits(run):
    return -1 if run == 'A' else int(np.float32(P.POISON_OUT).view(np.int32))


# ---- the column-sum passes: leaky, relu6 -----------------------------------------------------------------------------------
@pytest.mark.parametrize('c', P.COLSUM_CASES, ids=P.case_id)
def test_colsum_pass(c):
    ops = _ops()
    kind, M, C, name = c['kind'], c['M'], c['C'], P.case_id(c)
    entry = 'cpr_%s_bwd_colsum' % kind
    d = P.colsum_data(c)
    n_ws = query(entry + '_ws', M, C)
    assert n_ws == P.colsum_ws(kind, M, C) == P.cdiv(M, P.rows_per_block(M, P.colsum_rule(kind))) * C
    dy, add, y, want = dev(d['dy']), dev(d['add']), dev(d['y']), d['g'].cuda()
    write_g = c['want_g'] and y is not None
    specs = ([('g', M * C, 'out')] if write_g else []) + [('cs', C, 'out'), ('ws', n_ws, 'ws')]
    tail = [P.SLOPE] if kind == 'leaky' else []

    def launch(a):
        return call(entry, dy, add, y, a['g'] if write_g else None, a['cs'], a['ws'], M, C, *tail)
    res = {}
    for run, a in arena_runs(name, specs, launch):
        all_written(name + ' run ' + run, a, [n for n, _, _ in specs])          # the workspace too: exactly the floats the plan writes
        res[run] = (a['g'].clone() if write_g else None, a['cs'].clone())
    if kind == 'leaky':
        res['C'] = ops.leaky_bwd_colsum(dy, y, P.SLOPE, add=add, want_g=c['want_g'])
    else:
        g, cs = ops.relu6_bwd_colsum(dy, y, add=add, want_g=c['want_g'])
        res['C'] = (g if y is not None else None, cs)
    for run in 'ABC':
        g, cs = res[run]
        assert (g is not None) == write_g, (name, run)
        if write_g:
            same_bits('%s run %s g' % (name, run), g, want)
        same_bits('%s run %s column sums against run A' % (name, run), cs, res['A'][1])
    within(name + ' column sums', '%s_bwd_colsum' % kind, res['A'][1], d['cs'], d['cs_bar'])


# ---- res2_relu_bwd_colsum: in place on a channel slice of a pitched map ----------------------------------------------------------------
def _carry_off(c):
    return c['off'] + c['width'] if c['off'] + 2 * c['width'] <= c['pitch'] else 0


@pytest.mark.parametrize('c', P.RES2CS_CASES, ids=P.case_id)
def test_res2_relu_bwd_colsum(c):
    ops = _ops()
    name = P.case_id(c)
    N, H, W, width, pitch, off = (c[k] for k in ('N', 'H', 'W', 'width', 'pitch', 'off'))
    M, co = N * H * W, _carry_off(c)
    d = P.res2cs_data(c)
    n_ws = query('cpr_res2_relu_bwd_colsum_ws', M, width)
    assert n_ws == P.res2_cs_ws(M, width) == (M + 255) // 256 * width
    ymap = dev(P.embed_nhwc(d['y'], pitch, off))
    cmap = dev(P.embed_nhwc(d['carry'], pitch, co)) if c['carry'] else None
    dyd, want = d['dy'].cuda(), d['g'].cuda()
    specs = [('gmap', M * pitch, 'out'), ('cs', width, 'out'), ('ws', n_ws, 'ws')]

    def init(a, run):
        a['gmap'].view(N, H, W, pitch)[..., off:off + width] = dyd

    def launch(a):
        return call('cpr_res2_relu_bwd_colsum', a['gmap'], pitch, off, cmap, pitch if c['carry'] else 0, co, ymap, pitch, off, a['cs'], a['ws'],
                    M, width)
    outside = torch.ones(pitch, dtype=torch.bool, device='cuda')
    outside[off:off + width] = False
    res = {}
    for run, a in arena_runs(name, specs, launch, init):
        all_written(name + ' run ' + run, a, ['cs', 'ws'])
        gmap = a['gmap'].view(N, H, W, pitch)
        assert bool((bits(gmap)[..., outside] == prefill_bits(run)).all()), '%s run %s: channels outside the slice were written' % (name, run)
        res[run] = (gmap[..., off:off + width].clone(), a['cs'].clone())
    gmap = dev(P.embed_nhwc(d['dy'], pitch, off))
    cs = ops.res2_relu_bwd(gmap, off, ymap, off, width, carry=cmap, carry_off=co)
    assert bool(torch.isnan(gmap[..., outside]).all())
    res['C'] = (gmap[..., off:off + width], cs)
    for run in 'ABC':
        same_bits('%s run %s g' % (name, run), res[run][0], want)
        same_bits('%s run %s column sums against run A' % (name, run), res[run][1], res['A'][1])
    within(name + ' column sums', 'res2_relu_bwd_colsum', res['A'][1], d['cs'], d['cs_bar'])


# ---- the weight gradients ----------------------------------------------------------------------------------------------
def _res2_slices(c):
    """(x, add, dy) channel offsets, as tests/res2_conv_ref.slices lays a Bottle2neck's maps out."""
    n = c['pitch'] // c['width']
    return c['sl'] * c['width'], (c['sl'] + n - 1) % n * c['width'], (c['sl'] + 1) % n * c['width']


def _pad_nan(t, pitch):
    return t if t.shape[-1] == pitch else P.embed_nhwc(t, pitch, 0)


def wgrad_setup(c, d):
    """-> (query value, launch(grad_w, ws, acc) -> status, wrapper(grad or None) -> tensor)."""
    ops = _ops()
    fam, N, H, W, stride = c['fam'], c['N'], c['H'], c['W'], c['stride']
    M, OH, OW = P.wgrad_pixels(c)
    if fam == 'res2':
        width, pitch = c['width'], c['pitch']
        xo, ao, oo = _res2_slices(c)
        x, dy = dev(P.embed_nhwc(d['x'], pitch, xo)), dev(P.embed_nhwc(d['dy'], pitch, oo))
        add = dev(P.embed_nhwc(d['add'], pitch, ao)) if d['add'] is not None else None
        n_ws = query('cpr_res2_conv_wgrad_workspace', N, OH, OW, width)

        def launch(gw, ws, acc):
            return call('cpr_res2_conv_wgrad', dy, pitch, oo, x, pitch, xo, add, pitch if add is not None else 0, ao, gw, ws, N, H, W, width,
                        stride, acc)

        def wrapper(grad):
            return ops.res2_wgrad(dy, oo, x, xo, width, stride, add=add, add_off=ao, grad=grad)
    elif fam.startswith('group'):
        C, cg, Cp, dil = c['C'], c['cg'], c.get('Cp', c['C']), c.get('dil', 1)
        x, dy = dev(_pad_nan(d['x'], Cp)), dev(_pad_nan(d['dy'], Cp))          # the pad channels of a pitched map are never read
        n_ws = query('cpr_conv_group_wgrad_workspace', N, OH, OW, C, cg)

        def launch(gw, ws, acc):
            if fam == 'group':
                return call('cpr_conv_group_wgrad', dy, x, gw, ws, N, H, W, C, cg, stride, acc)
            if fam == 'group_pitch':
                return call('cpr_conv_group_wgrad_pitch', dy, x, gw, ws, N, H, W, C, Cp, cg, stride, acc)
            return call('cpr_conv_group_wgrad_dil', dy, x, gw, ws, N, H, W, C, cg, dil, acc)

        def wrapper(grad):
            return ops.conv2d_wgrad(dy, x, (C, cg, 3, 3), stride, dil, grad=grad, groups=C // cg, dilation=dil)
    elif fam == 'dw':
        C, Cp = c['C'], P.pad32(c['C'])
        x, dy = dev(_pad_nan(d['x'], Cp)), dev(_pad_nan(d['dy'], Cp))
        n_ws = query('cpr_dw3x3_wgrad_workspace', N, H, W, C, stride)

        def launch(gw, ws, acc):
            return call('cpr_dw3x3_wgrad', dy, x, gw, ws, N, H, W, C, stride, c['clamp'], acc)

        def wrapper(grad):
            return ops.dw_wgrad(dy, x, C, stride, in_clamp6=bool(c['clamp']), grad=grad)
    else:
        sfx = 's1' if fam == 'stem_s1' else 's2'
        x = dev(d['x'] if c['layout'] == 0 else P.nchw(d['x'][..., :3]))
        dy = dev(d['dy'])
        n_ws = query('cpr_stem3x3%s_wgrad_workspace' % sfx, N, H, W)

        def launch(gw, ws, acc):
            assert acc == 0
            return call('cpr_stem3x3%s_wgrad' % sfx, dy, x, gw, ws, N, H, W, c['layout'])

        def wrapper(grad):
            assert grad is None
            return getattr(ops, 'stem3x3%s_wgrad' % sfx)(dy, x, planar=bool(c['layout']))
    return n_ws, launch, wrapper


@pytest.mark.parametrize('c', P.WGRAD_CASES, ids=P.case_id)
def test_weight_gradient(c):
    name = P.case_id(c)
    d = P.wgrad_data(c)
    n_ws, launch, wrapper = wgrad_setup(c, d)
    assert n_ws == P.wgrad_ws(c), (name, n_ws, P.wgrad_ws(c))
    n_out = int(np.prod(d['shape']))
    specs = [('gw', n_out, 'out'), ('ws', n_ws, 'ws')]
    res = {}
    for run, a in arena_runs(name, specs, lambda a: launch(a['gw'], a['ws'], 0)):
        all_written(name + ' run ' + run, a, ['gw', 'ws'])
        res[run] = a['gw'].clone()
    res['C'] = wrapper(None)
    assert tuple(res['C'].shape) == tuple(d['shape'])
    for run in 'BC':
        same_bits('%s run %s against run A' % (name, run), res[run], res['A'])
    within(name, P.wgrad_family(c) + ' wgrad', res['A'], d['ref'], d['bar'])
    if c['acc']:
        base = d['base'].cuda()
        want = base + res['A'].view(d['shape'])                    # one more rounded addition
        for run, a in arena_runs(name + ' accumulate', specs, lambda a: launch(a['gw'], a['ws'], 1),
                                 lambda a, run: a['gw'].copy_(base.reshape(-1))):
            all_written(name + ' accumulate run ' + run, a, ['ws'])
            same_bits('%s accumulate run %s' % (name, run), a['gw'], want)
        same_bits(name + ' accumulate run C', wrapper(base.clone()), want)


# ---- dw3x3 data gradient with column sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', P.DWDGRAD_CASES, ids=P.case_id)
def test_dw3x3_dgrad_column_sums(c):
    ops = _ops()
    name = P.case_id(c)
    N, H, W, C, stride = (c[k] for k in ('N', 'H', 'W', 'C', 'stride'))
    Cp = P.pad32(C)
    d = P.dwdgrad_data(c)
    n_ws = query('cpr_dw3x3_dgrad_workspace', N, H, W, C)
    assert n_ws == P.dw_dgrad_ws(N, H, W, C)
    pack = ops.DwPack(d['w'].cuda(), d['scale'].cuda())
    ops.pack_ready(pack)
    dy = dev(_pad_nan(d['dy'], Cp))                            # the pad channels of an input are never read
    mask = dev(_pad_nan(d['mask'], Cp)) if c['mask'] else None
    add = dev(_pad_nan(d['add'], Cp)) if c['add'] else None
    specs = [('dx', N * H * W * Cp, 'out'), ('cs', C, 'out'), ('ws', n_ws, 'ws')]
    res = {}
    for run, a in arena_runs(name, specs, lambda a: call('cpr_dw3x3_dgrad', dy, pack.w, add, mask, a['dx'], a['cs'], a['ws'], N, H, W, C, stride)):
        all_written(name + ' run ' + run, a, ['dx', 'cs', 'ws'])
        res[run] = (a['dx'].view(N, H, W, Cp).clone(), a['cs'].clone())
    res['C'] = ops.dw_dgrad(dy, pack, (H, W), stride, mask6=mask, add=add, colsum=True)
    for run in 'BC':
        same_bits('%s run %s dx against run A' % (name, run), res[run][0], res['A'][0])
        same_bits('%s run %s column sums against run A' % (name, run), res[run][1], res['A'][1])
    dx, cs = res['A']
    assert bool((bits(dx[..., C:]) == 0).all()), name + ': a pad channel of dx is not +0.0'
    within(name + ' dx', 'dw3x3_dgrad', dx[..., :C], d['ref'], d['bar'])
    within(name + ' column sums', 'dw3x3_dgrad column sums', cs, d['cs'], d['cs_bar'])


# ---- the two HR entries: the partials are an output, sized by the *_blocks query -----------------------------------------------------
def _part_sum(part, C):
    """fp64 sums over the blocks of element 0 of a [blocks][C][2] partials slice."""
    return part.view(-1, C, 2)[..., 0].double().sum(0)


@pytest.mark.parametrize('c', [c for c in P.HR_CASES if c['fam'] == 'hrnet'], ids=P.case_id)
def test_hrnet_fuse_bwd(c):
    ops = _ops()
    name = P.case_id(c)
    N, H, W, C, K = (c[k] for k in ('N', 'H', 'W', 'C', 'K'))
    d = P.hr_data(c)
    tiles = query('cpr_hrnet_fuse_bwd_blocks', N, H, W, C, K)
    assert tiles == P.hrnet_bwd_blocks(N, H, W, C, K)
    dy, y = dev(d['dy']), dev(d['y'])
    names = ['g'] + ['pool%d' % k for k in range(1, K + 1)] + ['part']
    specs = [('g', N * H * W * C, 'out')] + [('pool%d' % k, N * (H >> k) * (W >> k) * C, 'out') for k in range(1, K + 1)] + \
            [('part', tiles * C * 2, 'ws')]
    wants = [torch.from_numpy(d['g'])] + [torch.from_numpy(p) for p in d['pools']]

    def launch(a):
        table = (ctypes.c_void_p * max(1, K))(*[a['pool%d' % k].data_ptr() for k in range(1, K + 1)])
        return call('cpr_hrnet_fuse_bwd', dy, y, a['g'], table, K, a['part'], N, H, W, C)
    res = {}
    for run, a in arena_runs(name, specs, launch):
        all_written(name + ' run ' + run, a, names)
        res[run] = [a[n].clone() for n in names]
    g, pools, tp = ops.hrnet_fuse_bwd(dy, y, K)
    res['C'] = [g] + list(pools) + [tp.part]
    assert tp.tiles == tiles
    for run in 'ABC':
        for n, got, want in zip(names, res[run], wants):
            same_bits('%s run %s %s' % (name, run, n), got, want)
        same_bits('%s run %s partials against run A' % (name, run), res[run][-1], res['A'][-1])
    part = res['A'][-1].view(tiles, C, 2)
    assert bool((bits(part[..., 1]) == 0).all()), name + ': element 1 of a partial is not +0.0'
    within(name + ' column sums of the partials', 'hrnet_fuse_bwd', _part_sum(part, C), d['cs'], d['cs_bar'])
    within(name + ' reduced column sums', 'hrnet_fuse_bwd', tp.reduce(), d['cs'], d['cs_bar'])


@pytest.mark.parametrize('c', [c for c in P.HR_CASES if c['fam'] == 'hrfpn'], ids=P.case_id)
def test_hrfpn_pool_bwd(c):
    ops = _ops()
    name = P.case_id(c)
    N, H, W, C, K = (c[k] for k in ('N', 'H', 'W', 'C', 'K'))
    d = P.hr_data(c)
    tiles = query('cpr_hrfpn_pool_bwd_blocks', N, H, W)
    assert tiles == P.hrfpn_pool_bwd_blocks(N, H, W)
    gs = [dev(t) for t in d['gs']]
    specs = [('d_out', N * H * W * C, 'out'), ('part', tiles * C * 2, 'ws')]

    def launch(a):
        return call('cpr_hrfpn_pool_bwd', ops._hrfpn_table(gs), K, a['d_out'], a['part'], N, C)
    res = {}
    for run, a in arena_runs(name, specs, launch):
        all_written(name + ' run ' + run, a, ['d_out', 'part'])
        res[run] = (a['d_out'].clone(), a['part'].clone())
    d_out, tp = ops.hrfpn_pool_bwd(gs)
    res['C'] = (d_out, tp.part)
    for run in 'BC':
        same_bits('%s run %s d_out against run A' % (name, run), res[run][0], res['A'][0])
        same_bits('%s run %s partials against run A' % (name, run), res[run][1], res['A'][1])
    part = res['A'][1].view(tiles, C, 2)
    assert bool((bits(part[..., 1]) == 0).all()), name + ': element 1 of a partial is not +0.0'

    def rel_l2(tag, got, want):
        e = float((got.double().cpu().reshape(-1) - want.reshape(-1)).norm() / want.norm())
        print('%s %s: rel-L2 %.3g, / bar = %.3g' % (name, tag, e, e / 1e-5))
        note('hrfpn_pool_bwd', e / 1e-5)
        assert e <= 1e-5, (name, tag, e)
    rel_l2('d_out', res['A'][0], d['d_out'])
    rel_l2('column sums of the partials', _part_sum(part, C), d['cs'])
    rel_l2('reduced column sums', tp.reduce(), d['cs'])


# ---- refused calls launch nothing -----------------------------------------------------------------------------------------------
def test_refused_calls_return_the_error_code_and_write_nothing():
    """One refusal per entry (the queries' own refusals are host code: tests/test_reduce_instances_host.py): a non-positive size, a
    channel count or width the kernels do not take, a misaligned slice or workspace -> CPR_ERR_ARG, and outputs and workspace keep the
    prefill."""
    ops = _ops()
    a = P.Arena([('out', 4096), ('cs', 64), ('ws', 4096)])
    for n in ('out', 'cs', 'ws'):
        a[n].fill_(P.POISON_OUT)
    out, cs, ws = a['out'], a['cs'], a['ws']
    src = dev(torch.randn(8192))
    odd = ws[1:]                                              # 4 bytes past an 8-byte boundary
    refused = [
        ('cpr_leaky_bwd_colsum', (src, None, src, out, cs, ws, 0, 32, P.SLOPE)),
        ('cpr_leaky_bwd_colsum', (src, None, src, out, cs, ws, 16, 6, P.SLOPE)),
        ('cpr_relu6_bwd_colsum', (src, None, src, out, cs, ws, -1, 32)),
        ('cpr_relu6_bwd_colsum', (src, src, None, out, cs, ws, 16, 32)),              # add without y
        ('cpr_res2_relu_bwd_colsum', (out, 32, 3, None, 0, 0, src, 32, 2, cs, ws, 16, 26)),      # an odd slice offset
        ('cpr_res2_relu_bwd_colsum', (out, 32, 2, None, 0, 0, src, 32, 2, cs, odd, 16, 26)),     # a workspace off the 8-byte grid
        ('cpr_res2_relu_bwd_colsum', (out, 32, 8, None, 0, 0, src, 32, 2, cs, ws, 16, 26)),      # the slice ends past the pitch
        ('cpr_res2_conv_wgrad', (src, 32, 0, src, 32, 0, None, 0, 0, out, odd, 1, 4, 4, 26, 1, 0)),
        ('cpr_res2_conv_wgrad', (src, 32, 0, src, 32, 0, None, 0, 0, out, ws, 1, 4, 4, 26, 3, 0)),
        ('cpr_conv_group_wgrad', (src, src, out, ws, 1, 4, 4, 16, 12, 1, 0)),
        ('cpr_conv_group_wgrad', (src, src, out, ws, 0, 4, 4, 16, 4, 1, 0)),
        ('cpr_conv_group_wgrad_pitch', (src, src, out, ws, 1, 4, 4, 24, 16, 8, 1, 0)),   # pitch below C
        ('cpr_conv_group_wgrad_dil', (src, src, out, ws, 1, 4, 4, 16, 4, 0, 0)),
        ('cpr_dw3x3_wgrad', (src, src, out, ws, 1, 4, 4, 12, 1, 0, 0)),
        ('cpr_dw3x3_wgrad', (src, src, out, ws, 1, 4, 4, 32, 3, 0, 0)),
        ('cpr_dw3x3_dgrad', (src, src, None, None, out, cs, ws, 1, 4, 4, 12, 1)),
        ('cpr_dw3x3_dgrad', (src, src, None, None, out, cs, None, 1, 4, 4, 32, 1)),        # column sums without a workspace
        ('cpr_stem3x3s1_wgrad', (src, src, out, ws, 1, 4, 4, 2)),
        ('cpr_stem3x3s2_wgrad', (src, src, out, ws, 0, 4, 4, 0)),
        ('cpr_hrnet_fuse_bwd', (src, src, out, (ctypes.c_void_p * 1)(ws.data_ptr()), 1, cs, 1, 5, 4, 32)),      # H % 2^K != 0
        ('cpr_hrfpn_pool_bwd', (ops._hrfpn_table([src.view(1, 8, 8, 128)[..., :32], src.view(1, 8, 8, 128)[:, :4, :3, :32]]), 2, out, ws, 1, 32)),
    ]
    for entry, args in refused:
        assert status(entry, *args) == ERR_ARG, entry
    torch.cuda.synchronize()
    a.intact('refused calls')
    for n in ('out', 'cs', 'ws'):
        assert bool((bits(a[n]) == prefill_bits('B')).all()), 'a refused call wrote its %s' % n
    assert {e for e, _ in refused} == {'cpr_leaky_bwd_colsum', 'cpr_relu6_bwd_colsum', 'cpr_res2_relu_bwd_colsum', 'cpr_res2_conv_wgrad',
                                       'cpr_conv_group_wgrad', 'cpr_conv_group_wgrad_pitch', 'cpr_conv_group_wgrad_dil', 'cpr_dw3x3_wgrad', 'cpr_dw3x3_dgrad',
                                       'cpr_stem3x3s1_wgrad', 'cpr_stem3x3s2_wgrad', 'cpr_hrnet_fuse_bwd', 'cpr_hrfpn_pool_bwd'}
