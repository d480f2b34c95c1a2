"""-m gpu: the small-J head output kernels through their C entry points -- ``cpr_logit_project`` (csrc/project.hip, 32 instances
<J, KC>), ``cpr_p2p_out_bf16_fwd`` / ``_dgrad`` / ``_wgrad`` (csrc/p2p_out_bf16.hip) and ``cpr_tap_sum3x3`` (csrc/postproc.hip) -- stage by
stage and element by element against the fp64 references and the derived bars of tests/head_out_fp64_ref.py, at the instances
tests/test_gpu_project.py and tests/test_gpu_p2p_bf16.py (Cin 256 only, J in {1, 2, 3, 8}, one global bar per tensor) never launch:
every (J, Cin) pair of every kernel, both dgrad output types, ldd in {J, max(4, J), J + 3} with NaN in the pad channels, image
boundaries inside a block, a wave and a range, one-row, one-column and one-pixel maps, a second grid-stride pass of logit_project,
and weight-gradient plans with R = 1, R = 32 and with empty ranges on both G branches.

Every output and every workspace is a slice in the middle of a larger buffer of 0xFF bytes (NaN in fp32 and bf16); workspaces have
exactly the size the query reports.  Per case: the guards are intact, every element is written and finite, every stage meets its bar
on the operands that stage read (the taps, the range partials and the bias partials are read back), the ``ops`` wrapper and a second
run give the same bits, and the last image of a batch equals its single-image run bit for bit (forward, dgrad, logit_project).  The
worst |err| / bar of every stage is printed.  ``coverage()`` names each state and the cases that reach it;
tests/test_head_out_instances_host.py asserts without a GPU that the tables reach them, that fp32 emulations in the kernels' own
order sit below half of every bar and that wrong emulations fail.  The argument refusals need no launch and also run without a GPU.

Measured on an MI355X: see CHANGELOG.md (wall time and the worst ratio per stage)."""
import collections
import time

import pytest
import torch

from tests import head_out_fp64_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                    # guard elements either side of every output and workspace
WORST = {}

# ---- tables ----------------------------------------------------------------------------------------------------------
BASE = (3, 5, 7)                                                            # 105 pixels: image boundaries inside a block, a wave, a range
PAIRS = [(J, Cin) for J in R.JS for Cin in R.CINS]
PROJ_PAIRS = [(2, 256), (5, 64), (8, 192)]
PROJ_VARIANTS = ('affine_norelu', 'plain_relu_flag', 'one_pixel')
PROJ_STRIDE = [(1, 64, (2, 120, 120)), (6, 64, (2, 120, 120))]
SHAPE_PAIRS = [(1, 64), (4, 192), (8, 256), (5, 128)]
SHAPES = [(1, 17, 19), (2, 1, 9), (2, 9, 1), (1, 1, 1)]
LDD_SHAPE = (1, 17, 19)
WGRAD_SHAPES = [(1, 5, 7), (1, 1, 1), (2, 33, 31)]
WGRAD_BIG = [(1, 64, (1, 363, 362)), (3, 64, (1, 363, 362)), (5, 128, (1, 264, 250))]
TAPSUM_CASES = [(J, s, bias) for J in (1, 2, 15) for s in ((2, 5, 7), (1, 1, 4)) for bias in (True, False)]


def ldds(J):
    return sorted({J, max(4, J), J + 3})


def cid(J, Cin, shape, ldd=None):
    return 'j%d_c%d_%dx%dx%d' % ((J, Cin) + tuple(shape)) + ('' if ldd is None else '_ldd%d' % ldd)


def wgrad_cases():
    return ([(J, Cin, BASE) for J, Cin in PAIRS] + [(J, Cin, s) for J, Cin in SHAPE_PAIRS for s in WGRAD_SHAPES] + WGRAD_BIG)


def coverage():
    """state -> ids of the cases that reach it, from the integer launch rules alone (no GPU)."""
    cov = {}
    add = lambda k, i: cov.setdefault(k, []).append(i)         # noqa: E731
    for J, Cin in PAIRS:
        i = cid(J, Cin, BASE)
        for kern in ('logit_project', 'taps', 'dgrad fp32', 'dgrad bf16', 'wgrad'):
            add('%s J %d Cin %d' % (kern, J, Cin), i)
        KW, G = R.groups(Cin, J)
        add('dgrad / wgrad KW %d G %d, J %s 4' % (KW, G, '<=' if J <= 4 else '>'), i)
    N, H, W = BASE
    if N * H * W < R.FWD_THREADS and N > 1:
        add('image boundary inside a block', 'every pair on %dx%dx%d' % BASE)
    if any(p // (H * W) != (p + R.DGRAD_PPW - 1) // (H * W) for p in range(0, N * H * W - R.DGRAD_PPW, R.DGRAD_PPW)):
        add('image boundary inside a dgrad wave', 'every pair on %dx%dx%d' % BASE)
    for J, Cin, s in wgrad_cases():
        npix, i = s[0] * s[1] * s[2], cid(J, Cin, s)
        G, Rn, ppw = R.wgrad_plan(npix, Cin, J)
        if R.straddling_ranges(npix, s[1] * s[2], Cin, J):
            add('wgrad range straddling an image', i)
        if Rn == 1:
            add('wgrad R 1', i)
        if Rn == 32 and ppw == 64:
            add('wgrad R 32 ppw 64', i)
        if R.empty_ranges(npix, Cin, J):
            add('wgrad empty ranges, G %s 1' % ('==' if G == 1 else '>'), i)
        if Rn == R.WGRAD_WAVES // G:
            add('wgrad range cap 2048 / G, G %d' % G, i)
    for J, Cin, s in PROJ_STRIDE:
        if R.proj_passes(s[0] * s[1] * s[2]) == 2:
            add('logit_project second grid-stride pass', cid(J, Cin, s))
    for J, Cin in PROJ_PAIRS:
        for v in PROJ_VARIANTS:
            add('logit_project ' + v, 'j%d_c%d' % (J, Cin))
    for J, Cin in SHAPE_PAIRS:
        for s in SHAPES:
            npix, i = s[0] * s[1] * s[2], cid(J, Cin, s)
            if npix > R.FWD_THREADS and npix % R.FWD_THREADS:
                add('forward: a second, ragged block', i)
            if npix % R.DGRAD_PPW and npix > R.DGRAD_PPW:
                add('dgrad: ragged last range', i)
            if s[1] > 2 and s[2] > 2:
                add('interior pixels', i)
            if s[1] == 1 and s[2] > 1:
                add('single-row map', i)
            if s[2] == 1 and s[1] > 1:
                add('single-column map', i)
            if npix == 1:
                add('one-pixel map', i)
        for ldd in ldds(J):
            add('dgrad ldd %s' % ('== J' if ldd == J else '> J'), cid(J, Cin, LDD_SHAPE, ldd))
    for J, s, bias in TAPSUM_CASES:
        add('tap_sum alone J %d bias %d' % (J, bias), 'x'.join(map(str, s)))
    return cov


WANTED = (['%s J %d Cin %d' % (k, J, Cin) for k in ('logit_project', 'taps', 'dgrad fp32', 'dgrad bf16', 'wgrad') for J, Cin in PAIRS]
          + ['dgrad / wgrad KW %d G 1, J <= 4' % k for k in (1, 2, 3, 4)] + ['dgrad / wgrad KW 1 G %d, J > 4' % k for k in (1, 2, 3, 4)]
          + ['image boundary inside a block', 'image boundary inside a dgrad wave', 'wgrad range straddling an image', 'wgrad R 1',
             'wgrad R 32 ppw 64', 'wgrad empty ranges, G == 1', 'wgrad empty ranges, G > 1', 'wgrad range cap 2048 / G, G 1',
             'wgrad range cap 2048 / G, G 2', 'logit_project second grid-stride pass', 'forward: a second, ragged block',
             'dgrad: ragged last range', 'interior pixels', 'single-row map', 'single-column map', 'one-pixel map', 'dgrad ldd == J',
             'dgrad ldd > J'] + ['logit_project ' + v for v in PROJ_VARIANTS]
          + ['tap_sum alone J %d bias %d' % (J, b) for J in (1, 2, 15) for b in (0, 1)])


# ---- operands (CPU, seeded: the host test regenerates them) --------------------------------------------------------
def operands(J, Cin, shape, ldd=None):
    """x32 (fp32 map of logit_project), x (the same map rounded to bf16), a / b (per image, ~20 % of a negative), w (J, Cin, 3, 3),
    wp (J, Cin), bias, dout (N, H, W, ldd) with NaN in channels [J, ldd)."""
    N, H, W = shape
    ldd = J + 3 if ldd is None else ldd
    gen = torch.Generator().manual_seed((((J * 8 + Cin // 64) * 16 + ldd) * 512 + N * 7 + H) * 512 + W)
    rn = lambda *s: torch.randn(s, generator=gen)         # noqa: E731
    x32 = 2 * rn(N, H, W, Cin)
    a = (torch.rand((N, Cin), generator=gen) + 0.25) * torch.where(torch.rand((N, Cin), generator=gen) < 0.2, -1.0, 1.0)
    dout = rn(N, H, W, ldd)
    dout[..., J:] = float('nan')
    return dict(x32=x32, x=x32.bfloat16(), a=a, b=0.5 * rn(N, Cin), w=0.02 * rn(J, Cin, 3, 3), wp=0.02 * rn(J, Cin), bias=rn(J), dout=dout)


def image(o, n):
    """The operands of image n alone."""
    return {k: (v[n:n + 1] if k in ('x32', 'x', 'a', 'b', 'dout') else v) for k, v in o.items()}


def f64(o):
    return {k: v.double() for k, v in o.items()}


# ---- plumbing ----------------------------------------------------------------------------------------------------
class Buf:
    """n elements inside a buffer whose every byte is 0xFF (a NaN in fp32 and in bf16), PAD elements either side."""

    def __init__(self, n, dtype=torch.float32):
        sz = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * PAD) * sz,), 0xFF, dtype=torch.uint8, device='cuda')
        self.v = self.raw.view(dtype)[PAD:PAD + n]
        self.lo, self.hi = self.raw[:PAD * sz], self.raw[(PAD + n) * sz:]

    def intact(self):
        return bool((self.lo == 0xFF).all()) and bool((self.hi == 0xFF).all())


def call(name, *args):
    from pointtinybenchmark_amd import _lib
    conv = lambda a: a.v.data_ptr() if isinstance(a, Buf) else a.data_ptr() if isinstance(a, torch.Tensor) else a      # noqa: E731
    return _lib.call(name, *[conv(a) for a in args], torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(name, a, b):
    assert a.numel() == b.numel() and a.dtype == b.dtype and torch.equal(bits(a).flatten(), bits(b).flatten()), '%s: the bits differ' % name


def settled(name, bufs):
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), '%s: guard bytes around %s were written' % (name, k)
        assert bool(torch.isfinite(b.v).all()), '%s: %s has unwritten or non-finite elements' % (name, k)


def judge(name, stage, got, ref, bar):
    C = ref.shape[-1]
    q = R.check('%s %s' % (name, stage), got.double().reshape(-1, C), ref.reshape(-1, C), bar.expand_as(ref).reshape(-1, C))
    WORST[stage] = max(WORST.get(stage, 0.0), q)
    return q


def dev(o):
    return {k: v.cuda().contiguous() for k, v in o.items()}


def vals(B):
    return {k: b.v for k, b in B.items()}


# ---- logit_project -----------------------------------------------------------------------------------------------
def run_project(o, J, Cin, shape, affine=True, in_relu=1):
    N, H, W = shape
    B = dict(out=Buf(N * H * W * J))
    call('cpr_logit_project', o['x32'], o['wp'], o['bias'], o['a'] if affine else None, o['b'] if affine else None, B['out'], N, H * W, Cin, J,
         in_relu)
    settled('logit_project ' + cid(J, Cin, shape), B)
    return B


def judge_project(name, o, out, J, shape, affine=True, in_relu=1):
    d = f64(o)
    ref, bar = R.project_ref(d['x32'], d['wp'], d['bias'], d['a'] if affine else None, d['b'] if affine else None, in_relu)
    return {'logit_project': judge(name, 'logit_project', out.view(shape + (J,)), ref, bar)}


def project_all(J, Cin, shape, affine=True, in_relu=1):
    from pointtinybenchmark_amd import ops
    name = 'logit_project %s affine=%d relu=%d' % (cid(J, Cin, shape), affine, in_relu)
    N = shape[0]
    o = dev(operands(J, Cin, shape))
    B = run_project(o, J, Cin, shape, affine, in_relu)
    qs = judge_project(name, o, B['out'].v, J, shape, affine, in_relu)
    same(name + ' ops', ops.logit_project(o['x32'], o['wp'], o['bias'], (o['a'], o['b']) if affine else None, bool(in_relu)), B['out'].v)
    same(name + ' second run', run_project(o, J, Cin, shape, affine, in_relu)['out'].v, B['out'].v)
    S = run_project(image(o, N - 1), J, Cin, (1,) + shape[1:], affine, in_relu)
    same(name + ' last image alone', S['out'].v, B['out'].v.view(N, -1)[N - 1])
    return qs


# ---- p2p_out forward ---------------------------------------------------------------------------------------------
def run_fwd(o, J, Cin, shape):
    N, H, W = shape
    B = collections.OrderedDict(taps=Buf(N * H * W * 9 * J), out=Buf(N * H * W * J))
    call('cpr_p2p_out_bf16_fwd', o['x'], o['a'], o['b'], o['w'], o['bias'], B['taps'], B['out'], N, H, W, Cin, J)
    settled('p2p_out forward ' + cid(J, Cin, shape), B)
    return B


def judge_fwd(name, o, B, J, shape):
    d = f64(o)
    act, ba = R.act_ref(d['x'], d['a'], d['b'])
    tref, tbar = R.taps_ref(act, ba, d['w'])
    taps, out = B['taps'].view(shape + (9 * J,)), B['out'].view(shape + (J,))
    qs = collections.OrderedDict()
    qs['taps'] = judge(name, 'taps', taps, tref, tbar)
    qs['tap_sum'] = judge(name, 'tap_sum', out, *R.tap_sum_ref(taps.double(), d['bias'], J))
    _, ebar = R.tap_sum_ref(tref, d['bias'], J, bar_R=tbar)
    qs['forward end to end'] = judge(name, 'forward end to end', out, R.conv_ref(act, d['w'], d['bias']).to(out.device), ebar)
    return qs


def fwd_all(J, Cin, shape):
    from pointtinybenchmark_amd import ops
    name = 'p2p_out ' + cid(J, Cin, shape)
    N = shape[0]
    o = dev(operands(J, Cin, shape))
    B = run_fwd(o, J, Cin, shape)
    qs = judge_fwd(name, o, vals(B), J, shape)
    same(name + ' ops forward', ops.p2p_out_bf16(o['x'], (o['a'], o['b']), o['w'], o['bias']), B['out'].v)
    same(name + ' ops tap_sum', ops.tap_sum3x3(B['taps'].v.view(shape + (9 * J,)), o['bias'], J), B['out'].v)
    B2 = run_fwd(o, J, Cin, shape)
    S = run_fwd(image(o, N - 1), J, Cin, (1,) + shape[1:])
    for k in B:
        same('%s second run %s' % (name, k), B2[k].v, B[k].v)
        same('%s last image alone: %s' % (name, k), S[k].v, B[k].v.view(N, -1)[N - 1])
    return qs


# ---- p2p_out dgrad -----------------------------------------------------------------------------------------------
def run_dgrad(o, J, Cin, shape, out16):
    N, H, W = shape
    B = dict(dx=Buf(N * H * W * Cin, torch.bfloat16 if out16 else torch.float32))
    call('cpr_p2p_out_bf16_dgrad', o['dout'], o['dout'].shape[-1], o['w'], B['dx'], int(out16), N, H, W, Cin, J)
    settled('p2p_out dgrad %s bf16=%d' % (cid(J, Cin, shape, o['dout'].shape[-1]), out16), B)
    return B


def judge_dgrad(name, o, dx, dx16, J, Cin, shape):
    d = f64(o)
    q = judge(name, 'dgrad', dx.view(shape + (Cin,)), *R.dgrad_ref(d['dout'][..., :J], d['w']))
    same(name + ': the bf16 output is the round-to-nearest-even of the fp32 output', dx16, R.bf16_rne(dx))
    return {'dgrad': q}


def dgrad_all(J, Cin, shape, ldd=None):
    from pointtinybenchmark_amd import ops
    o = dev(operands(J, Cin, shape, ldd))
    name = 'p2p_out dgrad ' + cid(J, Cin, shape, o['dout'].shape[-1])
    N = shape[0]
    B = {t: run_dgrad(o, J, Cin, shape, t)['dx'] for t in (False, True)}
    qs = judge_dgrad(name, o, B[False].v, B[True].v, J, Cin, shape)
    o1 = image(o, N - 1)
    for t, dt in ((False, torch.float32), (True, torch.bfloat16)):
        same('%s ops bf16=%d' % (name, t), ops.p2p_out_bf16_dgrad(o['dout'], o['w'], shape + (Cin,), dt), B[t].v)
        same('%s second run bf16=%d' % (name, t), run_dgrad(o, J, Cin, shape, t)['dx'].v, B[t].v)
        same('%s last image alone bf16=%d' % (name, t), run_dgrad(o1, J, Cin, (1,) + shape[1:], t)['dx'].v, B[t].v.view(N, -1)[N - 1])
    return qs


# ---- p2p_out wgrad -----------------------------------------------------------------------------------------------
def run_wgrad(o, J, Cin, shape):
    from pointtinybenchmark_amd import _lib
    N, H, W = shape
    n_ws = _lib.call('cpr_p2p_out_bf16_wgrad_ws', N, H, W, Cin, J, positive=True)
    assert n_ws == R.wgrad_ws(N * H * W, Cin, J)
    B = collections.OrderedDict(gw=Buf(J * Cin * 9), gb=Buf(J), ws=Buf(n_ws))
    call('cpr_p2p_out_bf16_wgrad', o['x'], o['a'], o['b'], o['dout'], o['dout'].shape[-1], B['gw'], B['gb'], B['ws'], N, H, W, Cin, J)
    settled('p2p_out wgrad ' + cid(J, Cin, shape), B)
    return B


def judge_wgrad(name, o, B, J, Cin, shape):
    d = f64(o)
    npix = shape[0] * shape[1] * shape[2]
    _, Rn, _ = R.wgrad_plan(npix, Cin, J)
    act, ba = R.act_ref(d['x'], d['a'], d['b'])
    dlive = d['dout'][..., :J]
    wref, wbar, bref, bbar, cnt = R.wgrad_partial_ref(act, ba, dlive, Cin, J)
    E = Rn * Cin * 9 * J
    ws, wsb = B['ws'][:E].view(Rn, Cin, 9 * J), B['ws'][E:].view(Rn, J)
    qs = collections.OrderedDict()
    qs['wgrad partial'] = judge(name, 'wgrad partial', ws, wref, wbar)
    qs['wgrad bias partial'] = judge(name, 'wgrad bias partial', wsb, bref, bbar)
    empty = cnt == 0
    assert int(empty.sum()) == R.empty_ranges(npix, Cin, J)
    assert R.positive_zero(ws[empty]) and R.positive_zero(wsb[empty]), name + ': an empty range is not +0.0'
    gw, gb = B['gw'].view(J, Cin, 3, 3), B['gb'].view(1, J)
    fw, fwb, fb, fbb = R.finalize_ref(ws.double().view(Rn, Cin, 9, J), wsb.double())
    qs['finalize gw'] = judge(name, 'finalize gw', gw, fw, fwb)
    qs['finalize gb'] = judge(name, 'finalize gb', gb, fb.view(1, J), fbb.view(1, J))
    _, agw, agb = R.conv_grads_ref(act, d['w'], dlive)
    ew, eb = R.wgrad_end_to_end_bars(wref, wbar, bref, bbar)
    qs['gw end to end'] = judge(name, 'gw end to end', gw, agw.to(gw.device), ew)
    qs['gb end to end'] = judge(name, 'gb end to end', gb, agb.to(gw.device).view(1, J), eb.view(1, J))
    return qs


def wgrad_all(J, Cin, shape, ldd=None):
    from pointtinybenchmark_amd import ops
    o = dev(operands(J, Cin, shape, ldd))
    name = 'p2p_out wgrad ' + cid(J, Cin, shape, o['dout'].shape[-1])
    B = run_wgrad(o, J, Cin, shape)
    qs = judge_wgrad(name, o, vals(B), J, Cin, shape)
    gw, gb = ops.p2p_out_bf16_wgrad(o['dout'], o['x'], (o['a'], o['b']), (J, Cin, 3, 3))
    same(name + ' ops gw', gw, B['gw'].v)
    same(name + ' ops gb', gb, B['gb'].v)
    B2 = run_wgrad(o, J, Cin, shape)
    for k in B:
        same('%s second run %s' % (name, k), B2[k].v, B[k].v)
    return qs


def report(name, t0, *qss):
    print('\nHEADOUT %s  %s  %.2f s' % (name, '  '.join('%s %.3f' % kv for qs in qss for kv in qs.items()), time.time() - t0))


# ---- the tests ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('J,Cin', PAIRS, ids=lambda v: str(v))
def test_every_instance_on_three_small_images(J, Cin):
    """logit_project with affine and ReLU, the forward, both dgrad output types and the wgrad (R = 2, ppw = 53: both ranges straddle an
    image boundary) of every (J, Cin) pair."""
    t0 = time.time()
    assert R.wgrad_plan(105, Cin, J)[1:] == (2, 53)
    report(cid(J, Cin, BASE), t0, project_all(J, Cin, BASE), fwd_all(J, Cin, BASE), dgrad_all(J, Cin, BASE), wgrad_all(J, Cin, BASE))


@pytest.mark.parametrize('J,Cin', PROJ_PAIRS, ids=lambda v: str(v))
def test_logit_project_variants(J, Cin):
    t0 = time.time()
    report('logit_project variants j%d_c%d' % (J, Cin), t0, project_all(J, Cin, BASE, affine=True, in_relu=0),
           project_all(J, Cin, BASE, affine=False, in_relu=1), project_all(J, Cin, (1, 1, 1)))


@pytest.mark.parametrize('J,Cin,shape', PROJ_STRIDE, ids=lambda v: str(v).replace(' ', ''))
def test_logit_project_second_grid_stride_pass(J, Cin, shape):
    t0 = time.time()
    npix = shape[0] * shape[1] * shape[2]
    assert (npix, R.proj_slots(npix), R.proj_passes(npix)) == (28800, 28672, 2)
    report('logit_project ' + cid(J, Cin, shape), t0, project_all(J, Cin, shape))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('J,Cin', SHAPE_PAIRS, ids=lambda v: str(v))
def test_forward_and_dgrad_shapes(J, Cin, shape):
    t0 = time.time()
    qd = [dgrad_all(J, Cin, shape, ldd) for ldd in (ldds(J) if shape == LDD_SHAPE else [J + 3])]
    report(cid(J, Cin, shape), t0, fwd_all(J, Cin, shape), *qd)


@pytest.mark.parametrize('shape', WGRAD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('J,Cin', SHAPE_PAIRS, ids=lambda v: str(v))
def test_wgrad_plans(J, Cin, shape):
    t0 = time.time()
    report('wgrad ' + cid(J, Cin, shape), t0, wgrad_all(J, Cin, shape, ldd=max(4, J)))


@pytest.mark.parametrize('J,Cin,shape', WGRAD_BIG, ids=lambda v: str(v).replace(' ', ''))
def test_wgrad_empty_ranges_are_written_as_zeros(J, Cin, shape):
    t0 = time.time()
    npix = shape[0] * shape[1] * shape[2]
    G, Rn, ppw = R.wgrad_plan(npix, Cin, J)
    assert Rn == R.WGRAD_WAVES // G and ppw == 65 and (Rn - 1) * ppw >= npix and R.empty_ranges(npix, Cin, J) == (26 if G == 1 else 8)
    report('wgrad ' + cid(J, Cin, shape), t0, wgrad_all(J, Cin, shape, ldd=max(4, J)))


def tapsum_operands(J, shape, bias):
    gen = torch.Generator().manual_seed(4000 + 100 * J + 10 * shape[2] + int(bias))
    return torch.randn(shape + (9 * J,), generator=gen), (torch.randn(J, generator=gen) if bias else None)


def judge_tapsum(name, Rm, bias, out, J):
    return {'tap_sum alone': judge(name, 'tap_sum alone', out.view(Rm.shape[:3] + (J,)), *R.tap_sum_ref(Rm.double(), None if bias is None else bias.double(), J))}


@pytest.mark.parametrize('J,shape,bias', TAPSUM_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_tap_sum_alone_on_random_responses(J, shape, bias):
    from pointtinybenchmark_amd import ops
    t0 = time.time()
    name = 'tap_sum j%d %s bias=%d' % (J, shape, bias)
    Rm, bv = tapsum_operands(J, shape, bias)
    Rm, bv = Rm.cuda(), (bv.cuda() if bias else None)
    N, H, W = shape

    def run(Rm, n):
        B = dict(out=Buf(n * H * W * J))
        call('cpr_tap_sum3x3', Rm, bv, B['out'], n, H, W, J)
        settled(name, B)
        return B['out'].v
    out = run(Rm, N)
    qs = judge_tapsum(name, Rm, bv, out, J)
    same(name + ' ops', ops.tap_sum3x3(Rm, bv, J), out)
    same(name + ' second run', run(Rm, N), out)
    same(name + ' last image alone', run(Rm[N - 1:].contiguous(), 1), out.view(N, -1)[N - 1])
    report(name, t0, qs)


def test_worst_ratio_per_stage():
    for k in sorted(WORST):
        print('HEADOUT worst |err| / bar  %-22s %.4f' % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())


# ---- argument refusals (no launch, so no GPU needed) ---------------------------------------------------------------------
def entry_arguments(pin, pout):
    """entry -> ordered [(parameter, value)] of one valid call, the stream last: J = 8, Cin = 256, ldd = 16 on a 3x3 map, so an entry
    that fails to refuse a probe stays inside the two buffers."""
    dims = [('N', 1), ('H', 3), ('W', 3), ('Cin', 256), ('J', 8)]
    P = lambda p, *names: [(n, p) for n in names]         # noqa: E731
    end = [('stream', None)]
    return collections.OrderedDict(
        cpr_logit_project=P(pin, 'x', 'w', 'bias', 'in_a', 'in_b') + P(pout, 'out') + [('N', 1), ('HW', 9), ('Cin', 256), ('J', 8), ('in_relu', 1)] + end,
        cpr_p2p_out_bf16_fwd=P(pin, 'x', 'a', 'b', 'w', 'bias') + P(pout, 'taps', 'out') + dims + end,
        cpr_p2p_out_bf16_dgrad=P(pin, 'dout') + [('ldd', 16)] + P(pin, 'w') + P(pout, 'dx') + [('out_bf16', 0)] + dims + end,
        cpr_p2p_out_bf16_wgrad=P(pin, 'x', 'a', 'b', 'dout') + [('ldd', 16)] + P(pout, 'gw', 'gb', 'ws') + dims + end,
        cpr_p2p_out_bf16_wgrad_ws=dims,
        cpr_tap_sum3x3=P(pin, 'R', 'bias') + P(pout, 'out') + [('N', 1), ('H', 3), ('W', 3), ('J', 8)] + end)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from pointtinybenchmark_amd import _lib
    where = 'cuda' if torch.cuda.is_available() else 'cpu'
    bin_, bout = torch.zeros(1 << 20, device=where), torch.zeros(1 << 20, device=where)
    L = _lib.load()
    ARG, UNS, EITHER = (R.ERR_ARG,), (R.ERR_UNSUPPORTED,), (R.ERR_ARG, R.ERR_UNSUPPORTED)
    count = 0
    for name, args in entry_arguments(bin_.data_ptr(), bout.data_ptr()).items():
        def refused(codes, **bad):
            a = collections.OrderedDict(args)
            assert set(bad) <= set(a)
            a.update(bad)
            rc = getattr(L, name)(*a.values())
            assert rc in codes, (name, bad, rc)
            return 1
        keys = [k for k, _ in args]
        query = name == 'cpr_p2p_out_bf16_wgrad_ws'
        count += refused(EITHER, J=0)                              # the header names only the upper end as "unsupported"
        if name != 'cpr_tap_sum3x3':                               # the tap sum takes any J > 0 and has no Cin
            count += refused(UNS, J=9)
            for cin in (0, -64, 32, 96, 320):
                count += refused(UNS, Cin=cin)
        for k in ('N', 'H', 'W', 'HW'):
            if k in keys:
                count += refused(EITHER if query else ARG, **{k: 0})
        if 'ldd' in keys:
            count += refused(ARG, ldd=7) + refused(ARG, ldd=0)
        for k, v in args:
            if isinstance(v, int) and v in (bin_.data_ptr(), bout.data_ptr()) and k not in ('in_a', 'in_b') and (name, k) != ('cpr_tap_sum3x3', 'bias'):
                count += refused(ARG, **{k: None})                  # every required pointer
        if name == 'cpr_logit_project':
            count += refused(ARG, in_a=None) + refused(ARG, in_b=None)
    if where == 'cuda':
        torch.cuda.synchronize()
        assert float(bout.abs().max()) == 0.0, 'a refused call wrote to its output'
    assert count == 6 + 5 + 25 + 17 + 4 + 23 + 2, count          # J 0, J 9, Cin, N / H / W, ldd, required pointers, in_a / in_b
