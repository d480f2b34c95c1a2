"""-m gpu: the nine split-attention kernels of csrc/splat.hip through their seven C entry points, stage by stage and element by element
against the fp64 references and the derived bars of tests/splat_fp64_ref.py, at the launch states tests/test_gpu_splat.py (one rel-L2
per tensor, w in {64, 96, 512}) never reaches: every product width 64 / 128 / 256 / 512 and both ends of the accepted range (w 4 and
1024, inter 1 and 1024, N 65535), lane layouts with idle threads (w 24, 96, 1000), chunks of exactly CH, CH + 1, CH - 1 pixels and a
one-pixel tail, all four parities of the pooled map, one-row and one-column maps, the grid-stride loop of splat_apply with its
attention reload at an image change, idle waves of the 1024-lane MLP kernels, saturated and tied logits, an all-zero ReLU, and every
subset class of the six parameter-gradient pointers.

Every output and every workspace is a slice in the middle of a larger buffer of 0xFF bytes (NaN in fp32).  Per case: the guards are
intact, every element is written and finite, every stage meets its bar on the operands that stage read (chunk partials, per-image sums
and the da | dh' | dh | xhat records are read back from the workspace), the ``ops`` wrapper and a second run give the same bits, and image
N - 1 of the batch equals its single-image run bit for bit (for ``colsum``: the per-image workspace rows).  The worst |err| / bar of every
stage is printed.  ``coverage()`` names each state and the cases that reach it; tests/test_splat_instances_host.py asserts without a
GPU that the tables reach them, that fp32 emulations of the kernels' own order sit below half of every bar and that wrong emulations
fail.  The argument refusals need no launch and also run without a GPU.

Measured on an MI355X: see CHANGELOG.md (wall time, worst ratios per stage, the two grid-stride cases)."""
import collections
import time

import pytest
import torch

from tests import splat_fp64_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                    # guard elements either side of every output and workspace
POOLS = (False, True)
ERR_ARG = -1001
GRADS = ('fc1_w', 'fc1_b', 'bn_w', 'bn_b', 'fc2_w', 'fc2_b')           # the order of the six pointers of cpr_splat_attn_bwd
WORST = {}

# ---- tables: (w, N, H, W) -----------------------------------------------------------------------------------------
MAP_CASES = [(4, 2, 1, 1), (4, 1, 64, 65), (24, 3, 13, 13), (64, 3, 16, 16), (64, 2, 1, 257), (64, 1, 255, 1), (96, 2, 40, 40),
             (128, 3, 17, 23), (128, 3, 18, 24), (128, 2, 17, 24), (128, 2, 18, 23), (256, 3, 5, 13), (256, 1, 1, 2), (256, 1, 2, 1),
             (256, 2, 2, 2), (256, 1, 3, 3), (512, 2, 9, 7), (1000, 1, 7, 9), (1024, 2, 40, 40), (4, 65535, 1, 1)]
STRIDE_PLAIN = (1024, 2, 182, 182)
STRIDE_POOL = (1024, 4, 257, 257)
# (w, inter, N)
MLP_CASES = [(4, 1, 1), (4, 32, 2), (64, 32, 3), (96, 48, 3), (128, 64, 2), (256, 128, 2), (512, 256, 2), (1000, 17, 2), (1024, 15, 2),
             (64, 1024, 1), (1024, 1024, 1)]
VARIANT_SHAPE = (64, 32, 3)
VARIANTS = ('tie', 'pm60', 'pm200', 'spread60', 'zeroz')
MLP_RUNS = [(s, None) for s in MLP_CASES] + [(VARIANT_SHAPE, v) for v in VARIANTS]
SUBSETS = [GRADS, ()] + [(k,) for k in GRADS]


def map_id(c):
    return 'w%d_n%d_%dx%d' % c


def mlp_id(r):
    return 'w%d_i%d_n%d' % r[0] + ('_' + r[1] if r[1] else '')


def coverage():
    """state -> ids of the cases that reach it, from the integer launch rules alone (no GPU)."""
    cov = {}
    add = lambda k, i: cov.setdefault(k, []).append(i)         # noqa: E731
    for c in MAP_CASES:
        w, N, H, W = c
        HW, P, CH, i = H * W, R.pp(w), R.chunk(w), map_id(c)
        cnt = R.chunk_counts(HW, w)
        add('width %d: WV %d PP %d' % (w, R.wv(w), P), i)
        if R.idle_lanes(w):
            add('idle lanes at WV %d' % R.wv(w), i)
        if HW == 1 and P == 256:
            add('one pixel, 255 empty row lanes', i)
        if len(cnt) == 2 and cnt[-1] < P:
            add('K 2, row lanes past the tail empty', i)
        if any(n > P and n % P for n in cnt):
            add('walks of unequal length', i)
        for d in (-1, 0, 1):
            if HW == CH + d:
                add('HW == CH %+d' % d, i)
        if H == 1 and W > 2:
            add('H 1: one row of pool taps', i)
        if W == 1 and H > 2:
            add('W 1: one column of pool taps', i)
        if len(cnt) >= 10:
            add('K >= 10 at PP %d' % P, i)
        if len(cnt) > 1 and cnt[-1] == 1:
            add('last chunk of one pixel', i)
        if HW <= 9:
            add('tiny map %dx%d' % (H, W), i)
        if H > 2 and W > 2:
            add('pool parity H %s W %s' % ('even' if H % 2 == 0 else 'odd', 'even' if W % 2 == 0 else 'odd'), i)
        if H % 2 == 0:
            add('adjoint window clipped at OH', i)
        if W % 2 == 0:
            add('adjoint window clipped at OW', i)
        if N == R.N_CAP:
            add('N at the gridDim.y cap', i)
        if N > 1:
            add('batch: image N - 1 against its solo run', i)
    for c, pool in ((STRIDE_PLAIN, False), (STRIDE_POOL, True)):
        w, N, H, W = c
        OH, OW = R.pooled(H, W, pool)
        if R.apply_strides(N * OH * OW, w) > 1:
            add('splat_apply grid stride, pool %d' % pool, map_id(c))
        if R.apply_reloads(N, OH * OW, w):
            add('attention reload at an image change, pool %d' % pool, map_id(c))
    for s, v in MLP_RUNS:
        w, inter, N = s
        i = mlp_id((s, v))
        add('mlp width %d' % w, i)
        add('mlp inter %d' % inter, i)
        if inter < R.ATTN_THREADS // 64:
            add('idle waves: inter < 16', i)
        if w % 64:
            add('dot product tail: w % 64 != 0', i)
        if inter % 64:
            add('dot product tail: inter % 64 != 0', i)
        if w > R.ATTN_THREADS // 64 * 64 or 2 * w > R.ATTN_THREADS:
            add('a lane takes a second channel', i)
        if v:
            add('variant ' + v, i)
    add('z null', 'every mlp case')
    add('gradient pointer subsets', 'every mlp case')
    return cov


WANTED = (['width %d: WV %d PP %d' % t for t in ((4, 1, 256), (24, 6, 42), (64, 16, 16), (96, 24, 10), (128, 32, 8), (256, 64, 4), (512, 128, 2),
                                                 (1000, 250, 1), (1024, 256, 1))]
          + ['idle lanes at WV %d' % v for v in (6, 24, 250)]
          + ['one pixel, 255 empty row lanes', 'K 2, row lanes past the tail empty', 'walks of unequal length', 'HW == CH -1', 'HW == CH +0',
             'HW == CH +1', 'H 1: one row of pool taps', 'W 1: one column of pool taps', 'K >= 10 at PP 10', 'K >= 10 at PP 1',
             'last chunk of one pixel', 'N at the gridDim.y cap', 'batch: image N - 1 against its solo run', 'adjoint window clipped at OH',
             'adjoint window clipped at OW']
          + ['tiny map %dx%d' % t for t in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3))]
          + ['pool parity H %s W %s' % t for t in (('odd', 'odd'), ('even', 'even'), ('odd', 'even'), ('even', 'odd'))]
          + ['splat_apply grid stride, pool 0', 'splat_apply grid stride, pool 1', 'attention reload at an image change, pool 0',
             'attention reload at an image change, pool 1']
          + ['mlp width %d' % w for w in (4, 64, 96, 128, 256, 512, 1000, 1024)] + ['mlp inter %d' % i for i in (1, 15, 17, 32, 1024)]
          + ['idle waves: inter < 16', 'dot product tail: w % 64 != 0', 'dot product tail: inter % 64 != 0', 'a lane takes a second channel',
             'z null', 'gradient pointer subsets'] + ['variant ' + v for v in VARIANTS])


# ---- operands (CPU, seeded: the host test regenerates them) --------------------------------------------------------
def map_operands(c, pool):
    w, N, H, W = c
    gen = torch.Generator().manual_seed(9000 + 2 * MAP_CASES.index(c) + int(pool))
    OH, OW = R.pooled(H, W, pool)
    return dict(u=torch.relu(torch.randn((N, H, W, 2 * w), generator=gen)), dout=torch.randn((N, OH, OW, w), generator=gen),
                att=torch.softmax(torch.randn((N, 2, w), generator=gen), 1), dg=torch.randn((N, w), generator=gen))


def mlp_operands(shape, variant=None):
    """fp32 operands of the two MLP entries; the eval BatchNorm is folded in fp64 and rounded once."""
    w, inter, N = shape
    gen = torch.Generator().manual_seed(9500 + MLP_CASES.index(shape) + 50 * (1 + VARIANTS.index(variant) if variant else 0))
    rn = lambda *s: torch.randn(s, generator=gen)         # noqa: E731
    o = dict(g=torch.rand((N, w), generator=gen) + 0.25, fc1_w=rn(inter, w) * (2.0 / w) ** 0.5, fc1_b=rn(inter) * 0.1,
             fc2_w=rn(2 * w, inter) * (2.0 / inter) ** 0.5, fc2_b=rn(2 * w) * 0.1, datt=rn(N, 2, w))
    bn_w, bn_b = torch.rand(inter, generator=gen) * 0.5 + 0.5, rn(inter) * 0.1
    mean, var = rn(inter) * 0.1, torch.rand(inter, generator=gen) + 0.5
    inv = 1.0 / torch.sqrt(var.double() + 1e-5)
    s = bn_w.double() * inv
    o.update(s1=s.float(), t1=(bn_b.double() - mean.double() * s).float(), mean=mean, inv=inv.float())
    sign = torch.where(torch.arange(w) % 2 == 0, 1.0, -1.0)
    if variant == 'tie':
        o['fc2_w'][w:] = o['fc2_w'][:w]
        o['fc2_b'][w:] = o['fc2_b'][:w]
    elif variant in ('pm60', 'pm200'):
        x = 60.0 if variant == 'pm60' else 200.0
        o['fc2_w'] *= 0.01
        o['fc2_b'] = torch.cat([x * sign, -x * sign])
    elif variant == 'spread60':
        o['fc2_w'] *= 0.01
        o['fc2_b'] = 60.0 * rn(2 * w).clamp(-0.65, 0.65)          # |a0 - a1| <= 78: att stays a normal fp32 number for attn_bwd
    elif variant == 'zeroz':
        o['t1'] = torch.full((inter,), -1e3)
    return o


# ---- plumbing ----------------------------------------------------------------------------------------------------
class Buf:
    """n floats inside a buffer whose every byte is 0xFF (a NaN in fp32), PAD elements either side."""

    def __init__(self, n):
        self.raw = torch.full(((n + 2 * PAD) * 4,), 0xFF, dtype=torch.uint8, device='cuda')
        self.v = self.raw.view(torch.float32)[PAD:PAD + n]
        self.lo, self.hi = self.raw[:PAD * 4], self.raw[(PAD + n) * 4:]

    def intact(self):
        return bool((self.lo == 0xFF).all()) and bool((self.hi == 0xFF).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


def call(name, *args):
    from pointtinybenchmark_amd import _lib
    conv = lambda a: a.v.data_ptr() if isinstance(a, Buf) else a.data_ptr() if isinstance(a, torch.Tensor) else a      # noqa: E731
    return _lib.call(name, *[conv(a) for a in args], torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(name, a, b):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), '%s: the bits differ' % name


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


def vals(B):
    return {k: b.v for k, b in B.items()}


def dev(o):
    return {k: v.cuda().contiguous() for k, v in o.items()}


# ---- the four map entries ----------------------------------------------------------------------------------------------
def run_map(o, c, pool):
    """gap, apply, attn_grad, apply_bwd on device operands ``o`` of shape c -> {name: Buf}."""
    w, N, H, W = c
    HW, K = H * W, R.chunks(H * W, w)
    OH, OW = R.pooled(H, W, pool)
    B = collections.OrderedDict(g=Buf(N * w), ws_gap=Buf(R.ws_gap(N, HW, w)), out=Buf(N * OH * OW * w), datt=Buf(N * 2 * w),
                                ws_ag=Buf(R.ws_attn_grad(N, HW, w)), du=Buf(N * HW * 2 * w), cs=Buf(2 * w), ws_ab=Buf(R.ws_apply_bwd(N, HW, w)))
    call('cpr_splat_gap', o['u'], B['g'], B['ws_gap'], N, H, W, w)
    call('cpr_splat_apply', o['u'], o['att'], B['out'], N, H, W, w, int(pool))
    call('cpr_splat_attn_grad', o['dout'], o['u'], B['datt'], B['ws_ag'], N, H, W, w, int(pool))
    call('cpr_splat_apply_bwd', o['dout'], o['u'], o['att'], o['dg'], B['du'], B['cs'], B['ws_ab'], N, H, W, w, int(pool))
    settled('%s pool=%d' % (map_id(c), pool), B)
    assert K == R.chunks(HW, w)
    return B


def judge_map(name, o, B, c, pool):
    w, N, H, W = c
    HW, K = H * W, R.chunks(H * W, w)
    d = {k: v.double() for k, v in o.items()}
    uf = d['u'].view(N, HW, 2 * w)
    qs = collections.OrderedDict()
    part = B['ws_gap'].view(N, K, w).double()
    qs['gap partial'] = judge(name, 'gap partial', part, *R.gap_partial_ref(uf, w))
    qs['gap final'] = judge(name, 'gap final', B['g'].view(N, w), *R.gap_final_ref(part, HW))
    qs['gap end to end'] = judge(name, 'gap end to end', B['g'].view(N, w), *R.gap_end_to_end(uf, w))
    stage = 'apply pooled' if pool else 'apply'
    ref, bar = R.apply_ref(d['u'], d['att'], pool)
    qs[stage] = judge(name, stage, B['out'], ref, bar)
    tag = ' pooled' if pool else ''
    part = B['ws_ag'].view(N, K, 2 * w).double()
    qs['attn_grad partial' + tag] = judge(name, 'attn_grad partial' + tag, part, *R.attn_grad_partial_ref(d['dout'], d['u'], pool))
    qs['attn_grad final'] = judge(name, 'attn_grad final', B['datt'].view(N, 2 * w), *R.rows_sum_ref(part))
    ref, bar, keep = R.du_ref(d['dout'], d['u'], d['att'], d['dg'], pool)
    du = B['du'].view(N, HW, 2 * w)
    qs['apply_bwd du' + tag] = judge(name, 'apply_bwd du' + tag, du, ref, bar)
    assert R.positive_zero(du[~keep]), '%s: a masked-out element of du is not +0.0' % name
    nk = N * K * 2 * w
    part = B['ws_ab'][:nk].view(N, K, 2 * w).double()
    qs['apply_bwd chunk sums'] = judge(name, 'apply_bwd chunk sums', part, *R.du_partial_ref(du.double(), w))
    per = B['ws_ab'][nk:].view(N, 2 * w).double()
    qs['apply_bwd per image'] = judge(name, 'apply_bwd per image', per, *R.rows_sum_ref(part))
    qs['apply_bwd colsum'] = judge(name, 'apply_bwd colsum', B['cs'].view(1, 2 * w), *R.rows_sum_ref(per.view(1, N, 2 * w)))
    return qs


@pytest.mark.parametrize('pool', POOLS, ids=['plain', 'pool'])
@pytest.mark.parametrize('c', MAP_CASES, ids=map_id)
def test_map_entries(c, pool):
    from pointtinybenchmark_amd import ops
    t0 = time.time()
    w, N, H, W = c
    HW, K = H * W, R.chunks(H * W, w)
    name = '%s pool=%d' % (map_id(c), pool)
    o = dev(map_operands(c, pool))
    B = run_map(o, c, pool)
    qs = judge_map(name, o, vals(B), c, pool)
    # the wrappers, a second run, the last image alone: the same bits
    same(name + ' ops gap', ops.splat_gap(o['u']).flatten(), B['g'].v)
    same(name + ' ops apply', ops.splat_apply(o['u'], o['att'], pool=pool).flatten(), B['out'].v)
    same(name + ' ops attn_grad', ops.splat_attn_grad(o['dout'], o['u'], pool=pool).flatten(), B['datt'].v)
    du, cs = ops.splat_apply_bwd(o['dout'], o['u'], o['att'], o['dg'], pool=pool)
    same(name + ' ops du', du.flatten(), B['du'].v)
    same(name + ' ops colsum', cs, B['cs'].v)
    B2 = run_map(o, c, pool)
    for k in B:
        same('%s second run %s' % (name, k), B2[k].v, B[k].v)
    S = run_map({k: v[N - 1:] for k, v in o.items()}, (w, 1, H, W), pool)
    nk = N * K * 2 * w
    for k, rows in (('g', N), ('ws_gap', N), ('out', N), ('datt', N), ('ws_ag', N), ('du', N)):
        same('%s image %d alone: %s' % (name, N - 1, k), S[k].v, B[k].v.view(rows, -1)[N - 1])
    same(name + ' alone: chunk sums', S['ws_ab'].v[:K * 2 * w], B['ws_ab'].v[:nk].view(N, -1)[N - 1])
    same(name + ' alone: per-image sums', S['ws_ab'].v[K * 2 * w:], B['ws_ab'].v[nk:].view(N, -1)[N - 1])
    same(name + ' alone: colsum is its per-image row', S['cs'].v, S['ws_ab'].v[K * 2 * w:])
    print('\nSPLAT %s  %s  %.2f s' % (name, '  '.join('%s %.3f' % kv for kv in qs.items()), time.time() - t0))


# ---- splat_apply's grid-stride loop ------------------------------------------------------------------------------------
def _stride_operands(c, seed):
    w, N, H, W = c
    gen = torch.Generator(device='cuda').manual_seed(seed)
    u = torch.randn((N, H, W, 2 * w), generator=gen, device='cuda').relu_()
    return u, torch.softmax(torch.randn((N, 2, w), generator=gen, device='cuda'), 1)


def _apply_into_buf(u, att, pool):
    N, H, W, w2 = u.shape
    OH, OW = R.pooled(H, W, pool)
    out = Buf(N * OH * OW * (w2 // 2))
    call('cpr_splat_apply', u, att, out, N, H, W, w2 // 2, int(pool))
    settled('apply %s pool=%d' % (tuple(u.shape), pool), dict(out=out))
    return out


@pytest.mark.parametrize('c,pool', [(STRIDE_PLAIN, False), (STRIDE_POOL, True)], ids=['plain', 'pool'])
def test_apply_grid_stride_and_reload_at_an_image_change(c, pool):
    """More than 65536 PP output pixels: some lanes take a second pixel, and it lies in a later image.  The batch equals its
    single-image runs (which take no stride) bit for bit; per element against fp64: the whole batch (unpooled), the last image (pooled)."""
    from pointtinybenchmark_amd import ops
    t0 = time.time()
    w, N, H, W = c
    OH, OW = R.pooled(H, W, pool)
    assert R.apply_strides(N * OH * OW, w) == 2 and R.apply_strides(OH * OW, w) == 1 and R.apply_reloads(N, OH * OW, w) > 0
    u, att = _stride_operands(c, 77 + int(pool))
    out = _apply_into_buf(u, att, pool)
    tk = time.time()
    got = out.v.view(N, OH, OW, w)
    same('stride ops', ops.splat_apply(u, att, pool=pool), got)
    same('stride second run', _apply_into_buf(u, att, pool).v, out.v)
    for n in range(N):
        same('stride image %d alone' % n, _apply_into_buf(u[n:n + 1], att[n:n + 1], pool).v, got[n].flatten())
    stage = 'apply pooled (grid stride)' if pool else 'apply (grid stride)'
    sel = slice(N - 1, N) if pool else slice(0, N)
    ref, bar = R.apply_ref(u[sel].double(), att[sel].double(), pool)
    q = judge(map_id(c), stage, got[sel], ref, bar)
    print('\nSPLAT %s %s worst |err| / bar %.3f  %.3f s (operands, first launch and its checks %.3f s)' % (map_id(c), stage, q, time.time() - t0, tk - t0))


# ---- the two MLP entries -----------------------------------------------------------------------------------------------
def run_attn(o, shape, record=True):
    w, inter, N = shape
    B = collections.OrderedDict(att=Buf(N * 2 * w))
    if record:
        B['z'] = Buf(N * inter)
    call('cpr_splat_attn', o['g'], o['fc1_w'], o['fc1_b'], o['s1'], o['t1'], o['fc2_w'], o['fc2_b'], B['att'], B.get('z'), N, w, inter)
    settled('attn %s' % (shape,), B)
    return B


def run_attn_bwd(o, att, z, shape, subset):
    w, inter, N = shape
    sizes = dict(fc1_w=inter * w, fc1_b=inter, bn_w=inter, bn_b=inter, fc2_w=2 * w * inter, fc2_b=2 * w)
    B = collections.OrderedDict(dg=Buf(N * w), ws=Buf(R.ws_attn_bwd(N, w, inter)))
    for k in subset:
        B[k] = Buf(sizes[k])
    call('cpr_splat_attn_bwd', att, o['datt'], z, o['g'], o['fc1_w'], o['fc1_b'], o['s1'], o['mean'], o['inv'], o['fc2_w'], B['dg'], B['ws'],
         *[B.get(k) for k in GRADS], N, w, inter)
    settled('attn_bwd %s %s' % (shape, subset), B)
    return B


def judge_attn(name, o, A, shape, variant):
    w, inter, N = shape
    d = {k: v.double() for k, v in o.items()}
    qs = collections.OrderedDict()
    z = A['z'].view(N, inter)
    qs['attn z'] = judge(name, 'attn z', z, *R.attn_z_ref(d['g'], d['fc1_w'], d['fc1_b'], d['s1'], d['t1']))
    a, bar_a = R.logits_ref(z.double(), d['fc2_w'], d['fc2_b'])
    assert float(bar_a.max()) <= R.BAR_A_MAX, (name, float(bar_a.max()))
    att = A['att'].view(N, 2, w)
    qs['attn att'] = judge(name, 'attn att', att, *R.softmax_ref(a, bar_a))
    ref, bar, ba = R.attn_end_to_end(d['g'], d['fc1_w'], d['fc1_b'], d['s1'], d['t1'], d['fc2_w'], d['fc2_b'])
    assert float(ba.max()) <= 1e-2, (name, float(ba.max()))
    qs['attn end to end'] = judge(name, 'attn end to end', att, ref, bar)
    assert float(att.min()) >= 0.0 and float(att.max()) <= 1.0
    if variant == 'tie':
        assert bool((att == 0.5).all()), name + ': identical fc2 rows must give exactly 0.5'
    if variant == 'pm200':
        big = (o['fc2_b'].view(2, w) > 0).unsqueeze(0).expand(N, 2, w)
        assert bool((att[big] == 1.0).all()) and R.positive_zero(att[~big]), name + ': logits of +-200 must give exactly 1.0 and +0.0'
    if variant == 'zeroz':
        assert R.positive_zero(z), name + ': z must be +0.0 everywhere'
        a0 = d['fc2_b'].view(1, 2 * w).expand(N, 2 * w)
        qs['attn att, a == b2'] = judge(name, 'attn att, a == b2', att, *R.softmax_ref(a0, torch.zeros_like(a0)))
    return qs


def judge_attn_bwd(name, o, att, z, Bw, shape):
    w, inter, N = shape
    d = {k: v.double() for k, v in o.items()}
    rec = Bw['ws'].view(N, 2 * w + 3 * inter).double()
    da, dhp, dh, xh = rec[:, :2 * w], rec[:, 2 * w:2 * w + inter], rec[:, 2 * w + inter:2 * w + 2 * inter], rec[:, 2 * w + 2 * inter:]
    qs = collections.OrderedDict()
    qs['attn_bwd da'] = judge(name, 'attn_bwd da', da, *R.da_ref(att.double().view(N, 2, w), d['datt']))
    qs['attn_bwd xhat'] = judge(name, 'attn_bwd xhat', xh, *R.xhat_ref(d['g'], d['fc1_w'], d['fc1_b'], d['mean'], d['inv']))
    ref, bar, keep = R.dhp_ref(da, d['fc2_w'], z.double())
    qs["attn_bwd dh'"] = judge(name, "attn_bwd dh'", dhp, ref, bar)
    raw = Bw['ws'].view(N, 2 * w + 3 * inter)[:, 2 * w:2 * w + inter]
    assert R.positive_zero(raw[~keep]), "%s: a masked-out element of dh' is not +0.0" % name
    qs['attn_bwd dh'] = judge(name, 'attn_bwd dh', dh, *R.dh_ref(ref, bar, d['s1']))
    qs['attn_bwd dg'] = judge(name, 'attn_bwd dg', Bw['dg'].view(N, w), *R.dg_ref(dh, d['fc1_w']))
    for k, (ref, bar) in R.param_refs(rec, z.double(), d['g'], w, inter).items():
        qs['attn_bwd d' + k] = judge(name, 'attn_bwd d' + k, Bw[k], ref, bar)
    return qs


@pytest.mark.parametrize('run', MLP_RUNS, ids=mlp_id)
def test_mlp_entries(run):
    from pointtinybenchmark_amd import ops
    t0 = time.time()
    shape, variant = run
    w, inter, N = shape
    name = mlp_id(run)
    o = dev(mlp_operands(shape, variant))
    A = run_attn(o, shape)
    qs = judge_attn(name, o, vals(A), shape, variant)
    att, z = A['att'].v.view(N, 2, w), A['z'].v.view(N, inter)
    same(name + ' z null: att', run_attn(o, shape, record=False)['att'].v, A['att'].v)
    a2, z2 = ops.splat_attn(o['g'], o['fc1_w'], o['fc1_b'], o['s1'], o['t1'], o['fc2_w'], o['fc2_b'], record=True)
    same(name + ' ops att', a2, att)
    same(name + ' ops z', z2, z)
    same(name + ' ops att, z not recorded', ops.splat_attn(o['g'], o['fc1_w'], o['fc1_b'], o['s1'], o['t1'], o['fc2_w'], o['fc2_b']), att)
    A2 = run_attn(o, shape)
    for k in A:
        same('%s second run %s' % (name, k), A2[k].v, A[k].v)
    if variant == 'zeroz':                       # a == b2 whatever g and fc2.weight are
        o2 = dict(o, g=o['g'] * 3 + 1, fc2_w=torch.zeros_like(o['fc2_w']))
        same(name + ' att does not depend on g or fc2.weight', run_attn(o2, shape)['att'].v, A['att'].v)
    runs = {s: run_attn_bwd(o, att, z, shape, s) for s in SUBSETS}
    full = runs[GRADS]
    qs.update(judge_attn_bwd(name, o, att, z, vals(full), shape))
    assert list(runs[()]) == ['dg', 'ws']                   # with no gradient pointer only dg and the workspace exist to be written
    for s, Bw in runs.items():
        for k in Bw:
            same('%s subset %s: %s' % (name, s, k), Bw[k].v, full[k].v)
    grads = {k: torch.empty_like(full[k].v) for k in GRADS}
    same(name + ' ops dg', ops.splat_attn_bwd(att, o['datt'], z, o['g'], o['fc1_w'], o['fc1_b'], o['s1'], o['mean'], o['inv'], o['fc2_w'],
                                              grads=grads).flatten(), full['dg'].v)
    for k in GRADS:
        same('%s ops d%s' % (name, k), grads[k], full[k].v)
    B2 = run_attn_bwd(o, att, z, shape, GRADS)
    for k in full:
        same('%s attn_bwd second run %s' % (name, k), B2[k].v, full[k].v)
    # image N - 1 alone: the same per-image bits (the parameter sums are over the batch, so not compared)
    per = ('g', 'datt')
    o1 = {k: (v[N - 1:] if k in per else v) for k, v in o.items()}
    s1 = (w, inter, 1)
    A1 = run_attn(o1, s1)
    same(name + ' alone: att', A1['att'].v, att[N - 1].flatten())
    same(name + ' alone: z', A1['z'].v, z[N - 1])
    W1 = run_attn_bwd(o1, att[N - 1:], z[N - 1:], s1, ())
    same(name + ' alone: dg', W1['dg'].v, full['dg'].v.view(N, w)[N - 1])
    same(name + ' alone: records', W1['ws'].v, full['ws'].v.view(N, -1)[N - 1])
    print('\nSPLAT %s  %s  %.2f s' % (name, '  '.join('%s %.3f' % kv for kv in qs.items()), time.time() - t0))


def test_worst_ratio_per_stage():
    for k in sorted(WORST):
        print('SPLAT worst |err| / bar  %-28s %.4f' % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())


# ---- argument refusals (no launch, so no GPU needed) ---------------------------------------------------------------------
def entry_arguments(p):
    """entry -> ordered [(parameter, value)] of one valid call on the buffer pointer p, the stream last."""
    dims = [('N', 1), ('H', 3), ('W', 3), ('w', 8)]
    mlp = [('N', 1), ('w', 8), ('inter', 4)]
    P = lambda *names: [(n, p) for n in names]         # noqa: E731
    opt = [(k, None) for k in ('gfc1w', 'gfc1b', 'gbnw', 'gbnb', 'gfc2w', 'gfc2b')]
    end = [('stream', None)]
    return collections.OrderedDict(
        cpr_splat_gap=P('u', 'g', 'ws') + dims + end,
        cpr_splat_attn=P('g', 'fc1w', 'fc1b', 's1', 't1', 'fc2w', 'fc2b', 'att') + [('z', None)] + mlp + end,
        cpr_splat_apply=P('u', 'att', 'out') + dims + [('pool', 0)] + end,
        cpr_splat_attn_grad=P('dout', 'u', 'datt', 'ws') + dims + [('pool', 0)] + end,
        cpr_splat_attn_bwd=P('att', 'datt', 'z', 'g', 'fc1w', 'fc1b', 's1', 'mean', 'inv_sigma', 'fc2w', 'dg', 'ws') + opt + mlp + end,
        cpr_splat_apply_bwd=P('dout', 'u', 'att', 'dg', 'du', 'colsum', 'ws') + dims + [('pool', 0)] + end)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from pointtinybenchmark_amd import _lib
    buf = torch.zeros(1 << 16, device='cuda' if torch.cuda.is_available() else 'cpu')
    L = _lib.load()
    count = 0
    for name, args in entry_arguments(buf.data_ptr()).items():
        def refused(**bad):
            a = collections.OrderedDict(args)
            assert set(bad) <= set(a)
            a.update(bad)
            assert getattr(L, name)(*a.values()) == ERR_ARG, (name, bad)
            return 1
        keys = [k for k, _ in args]
        for wbad in (0, 6, 1028, -4):
            count += refused(w=wbad)
        for k in ('N', 'H', 'W'):
            if k in keys:
                count += refused(**{k: 0}) + refused(**{k: -1})
        if 'inter' in keys:
            count += refused(inter=0) + refused(inter=1025)
        if name in ('cpr_splat_gap', 'cpr_splat_attn_grad', 'cpr_splat_apply_bwd'):
            count += refused(N=65536)
        if 'pool' in keys:
            count += refused(pool=2) + refused(pool=-1)
        for k, v in args:
            if v == buf.data_ptr():                   # every required pointer
                count += refused(**{k: None})
    assert L.cpr_splat_chunks(3, 3, 6) == ERR_ARG and L.cpr_splat_chunks(0, 3, 8) == ERR_ARG and L.cpr_splat_chunks(3, 3, 1028) == ERR_ARG
    assert count >= 90
