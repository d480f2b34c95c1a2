"""-m gpu: the batch-statistics BatchNorm kernels of csrc/bn_train.hip, bn_fold / bn_fold_multi of csrc/pack.hip and the clip-norm
and SGD kernels of csrc/backward.hip through their C entry points, stage by stage against the fp64 references and the derived bars
of tests/bn_fp64_ref.py, at the launch states the shape-level tests never reach: lane layouts with idle threads, unequal channel
groups in one launch, rows_per_block > 64, one-row blocks, exactly 16 / 17 row blocks, partial trips of the 4-row unroll, null
argument forms, degenerate channels, and the grid caps of the optimiser kernels.

Every output, the workspace included, is a slice of a larger buffer pre-filled with bytes that read as NaN (0xA5 for integers);
per case the guards must be intact, every element written and finite, every bar met (the worst error / bar of every stage is
printed), a second run bit-equal and the ops.* wrapper bit-equal to the direct call.  The fp64 references
run in plain torch on the device.  tests/test_bn_instances_host.py asserts without a GPU that the tables reach the states
``coverage()`` names and that the bars are sharp.

Measured on an MI355X: see CHANGELOG.md (wall time, worst ratios per stage, the bn_fold bit-difference count)."""
import pytest
import torch

from tests import bn_fp64_ref as R

pytestmark = pytest.mark.gpu

EPS = 1e-5
PAD = 64                    # guard elements either side of every output


# ---- tables ----------------------------------------------------------------------------------------------------------
def BN(M, C, kind='normal', nulls=False, forms=False, mom=0.1, ops=True, why=''):
    """One single-rank chain stats -> apply -> backward on an (M, C) map.  kind: normal | far (offset 1e3 sigma) | const (channel 5
    constant, channel 9 constant except one row) | outlier0 (row 0, the kernel's shift, at 32 sigma).  nulls: also the forms with
    scale / shift / center / running buffers / nbt / z / dgamma / dbeta null.  forms: also the residual and two-input apply.
    mom: momentum (None: 1 / num_batches_tracked)."""
    return dict(op='bn', M=M, C=C, kind=kind, nulls=nulls, forms=forms, mom=mom, ops=ops, why=why)


def SYNC(rows, C, variant=0.0, ops=True, why=''):
    """One process plays len(rows) ranks; variant: 0.0 | 1e3 | 'split' (chunks alternate between +1e3 and -1e3 sigma)."""
    return dict(op='sync', rows=tuple(rows), C=C, variant=variant, ops=ops, why=why)


LAYOUT_C = (192, 320, 448, 576, 1088, 1280, 2240)
EDGE_M = (2, 3, 63, 64, 65, 961, 1031, 2112)
BIG = ((131327, 64), (135170, 192))

CASES = (
    [BN(700, C, nulls=C in (448, 1088), forms=C == 320, why='lane layout / group split at M 700') for C in LAYOUT_C]
    + [BN(M, C, nulls=(M, C) in ((65, 192), (2, 64)), forms=(M, C) == (3, 64), mom=None if M == 1031 else 0.1,
          why='row edge at rows_per_block 64') for M in EDGE_M for C in (64, 192)]
    + [BN(961, 320, why='16 blocks, last of one row, PP 3: stride 12 through 64 rows')]
    + [BN(M, C, why='rows_per_block > 64') for M, C in BIG]
    + [BN(700, 192, kind='const', why='M2 exactly 0: rstd = 1 / sqrt(eps); a channel constant except one row'),
       BN(700, 64, kind='outlier0', nulls=True, why='the shift row is an outlier at 32 sigma'),
       BN(700, 320, kind='far', why='far mean, 16 idle lanes'),
       BN(65, 64, kind='far', mom=None, why='far mean at the one-row second block')]
)

SYNC_CASES = [
    SYNC((700,), 64, why='R 1'),
    SYNC((189, 63), 64, why='R 2, uneven'),
    SYNC((1, 6), 64, variant=1e3, why='a one-row rank'),
    SYNC((1, 1), 64, why='two one-row ranks alone: global count 2'),
    SYNC((65, 1, 130), 192, variant='split', why='R 3, uneven, a one-row rank, chunks at +-1e3 sigma, PP 5'),
    SYNC((70, 64), 1088, variant='split', why='C 1088: merge threads take a second channel; unequal channel groups'),
    SYNC((3, 64, 1, 65, 2, 100, 17, 129), 64, variant='split', why='R 8'),
    SYNC((961, 1031), 320, variant=1e3, why='16 and 17 blocks per rank, PP 3'),
]

FOLD_C = (1, 3, 64, 255, 256, 257, 2048)
FOLD_MULTI = ((64, 'scale shift inv'), (257, 'scale shift'), (2048, 'shift'), (1, 'inv'), (64, 'scale inv'))
SUMSQ_N = (1, 255, 1024, 1025, 1048576, 1048577, 3000001)
SGD_N = (1, 257, 2097152, 2097155)
SGD_FORMS = [
    dict(name='clip_active', max_norm=0.5, mu=0.9, wd=1e-4, first=0, gs=1.0),
    dict(name='clip_inactive', max_norm=1e9, mu=0.9, wd=1e-4, first=0, gs=1.0),
    dict(name='noclip_null_norm2', max_norm=0.0, mu=0.9, wd=1e-4, first=0, gs=1.0),
    dict(name='neg_max_norm_null_norm2_first', max_norm=-1.0, mu=0.9, wd=1e-4, first=1, gs=0.125),
    dict(name='mu0_null_buf', max_norm=0.5, mu=0.0, wd=1e-4, first=0, gs=1.0),
    dict(name='wd0_gs8', max_norm=0.5, mu=0.9, wd=0.0, first=0, gs=0.125),
    dict(name='first_clip', max_norm=0.5, mu=0.9, wd=0.0, first=1, gs=1.0),
]


def case_id(c):
    if c['op'] == 'sync':
        return 'sync_%s_C%d_%s' % ('+'.join(map(str, c['rows'])), c['C'], c['variant'])
    flags = ''.join('_' + k for k in ('nulls', 'forms') if c[k]) + ('_momNone' if c['mom'] is None else '')
    return 'bn_M%d_C%d_%s%s' % (c['M'], c['C'], c['kind'], flags)


def coverage():
    """state -> ids of the cases that reach it, from the launch rules alone (no GPU).  Every state of the issue's gap list."""
    cov = {}
    add = lambda k, c: cov.setdefault(k, []).append(case_id(c) if isinstance(c, dict) else c)         # noqa: E731
    for c in CASES:
        M, C = c['M'], c['C']
        lay = R.lane_layout(C)
        rpb, nb, rows = R.rows_per_block(M, C), R.blocks(M, C), R.block_rows(M, C)
        for _, _, Q, PP, idle in lay:
            if idle:
                add('idle lanes Q %d PP %d' % (Q, PP), c)
            if any(R.tail_trips(n, PP) for n in set(rows)):
                add('unroll tail PP %d' % PP, c)
        if len({Q for _, _, Q, _, _ in lay}) > 1:
            add('unequal channel groups C %d' % C, c)
        if rpb > 64:
            add('rows_per_block > 64', c)
        if rpb == 64 and M in EDGE_M:
            add('row edge M %d' % M, c)
        if nb == 16 and rows[-1] == 1:
            add('16 blocks, last of one row', c)
        if nb == 17:
            add('17 blocks: slice 0 gets two', c)
        if nb > 1 and rows[-1] == 1 and any(PP > 1 for _, _, _, PP, _ in lay):
            add('a block where most threads count zero rows', c)
        if c['kind'] != 'normal':
            add('input ' + c['kind'], c)
        if c['nulls']:
            for k in ('scale/shift null', 'center null in stats, apply, backward', 'dgamma/dbeta null', 'z null', 'running buffers and nbt null'):
                add(k, c)
        if c['forms']:
            add('residual and two-input apply', c)
        if c['mom'] is None:
            add('momentum < 0: 1 / nbt', c)
        if c['ops']:
            add('ops wrapper, single rank', c)
    for c in SYNC_CASES:
        R_ = len(c['rows'])
        add('sync R %d' % R_, c)
        if 1 in c['rows'] and R_ > 1:
            add('sync one-row rank', c)
        if c['rows'] == (1, 1):
            add('sync global count 2', c)
        if len(set(c['rows'])) > 1:
            add('sync uneven chunks', c)
        if c['C'] > R.MERGE_THREADS:
            add('sync merge threads take a second channel', c)
        if c['variant'] == 'split':
            add('sync chunks at +-1e3 sigma', c)
        if c['ops']:
            add('ops wrapper, sync', c)
    for C in FOLD_C:
        add('bn_fold C %d' % C, 'fold_%d' % C)
    for C, outs in FOLD_MULTI:
        if len(outs.split()) < 3:
            add('bn_fold_multi null outputs', 'fold_multi')
    add('bn_fold_multi jobs of different C', 'fold_multi')
    for n in SUMSQ_N:
        if n > R.SUMSQ_CAP * R.SUMSQ_PER_BLOCK:
            add('sumsq grid cap 1024 wraps', 'sumsq_%d' % n)
        if n < 256:
            add('sumsq less than one block', 'sumsq_%d' % n)
    for n in SGD_N:
        if n > R.SGD_CAP * R.BLOCK:
            add('sgd grid cap 8192 wraps', 'sgd_%d' % n)
        if n == R.SGD_CAP * R.BLOCK:
            add('sgd exactly the cap', 'sgd_%d' % n)
    for f in SGD_FORMS:
        for k, on in (('sgd mu == 0, null buf', f['mu'] == 0), ('sgd wd == 0', f['wd'] == 0), ('sgd max_norm <= 0, null norm2', f['max_norm'] <= 0),
                      ('sgd grad_scale != 1', f['gs'] != 1), ('sgd first', f['first'] == 1), ('sgd clip active', f['name'] == 'clip_active'),
                      ('sgd clip inactive', f['name'] == 'clip_inactive')):
            if on:
                add(k, f['name'])
    add('sumsq accumulate', 'acc1')
    return cov


WANTED = (['idle lanes Q %d PP %d' % qp for qp in ((48, 5), (80, 3), (112, 2), (144, 1))]
          + ['unequal channel groups C %d' % C for C in (1088, 1280, 2240)]
          + ['rows_per_block > 64', '16 blocks, last of one row', '17 blocks: slice 0 gets two', 'a block where most threads count zero rows',
             'unroll tail PP 5', 'unroll tail PP 3']
          + ['row edge M %d' % M for M in EDGE_M]
          + ['input const', 'input outlier0', 'input far', 'scale/shift null', 'center null in stats, apply, backward', 'dgamma/dbeta null',
             'z null', 'running buffers and nbt null', 'residual and two-input apply', 'momentum < 0: 1 / nbt', 'ops wrapper, single rank']
          + ['sync R %d' % r for r in (1, 2, 3, 8)]
          + ['sync one-row rank', 'sync global count 2', 'sync uneven chunks', 'sync merge threads take a second channel',
             'sync chunks at +-1e3 sigma', 'ops wrapper, sync']
          + ['bn_fold C %d' % C for C in FOLD_C] + ['bn_fold_multi null outputs', 'bn_fold_multi jobs of different C']
          + ['sumsq grid cap 1024 wraps', 'sumsq less than one block', 'sumsq accumulate', 'sgd grid cap 8192 wraps', 'sgd exactly the cap',
             'sgd mu == 0, null buf', 'sgd wd == 0', 'sgd max_norm <= 0, null norm2', 'sgd grad_scale != 1', 'sgd first', 'sgd clip active',
             'sgd clip inactive'])


# ---- operands (CPU, seeded: the host test regenerates them) ------------------------------------------------------------
def case_seed(c):
    return 7000 + (CASES.index(c) if c['op'] == 'bn' else 500 + SYNC_CASES.index(c))


def make_map(M, C, kind, gen, offset=0.0):
    std = 1.0 + torch.rand(C, generator=gen)
    off = 1e3 if kind == 'far' else offset
    y = torch.randn((M, C), generator=gen)
    y.mul_(std).add_(off * std + 0.3 * torch.randn(C, generator=gen))
    if kind == 'const':
        y[:, 5] = 2.5
        y[:, 9] = -1.25
        y[M // 2, 9] = 3.0
    if kind == 'outlier0':
        y[0] += 32 * std
    return y.contiguous()


def make_params(C, gen):
    sign = (torch.randint(0, 8, (C,), generator=gen) > 0).float() * 2 - 1            # one channel in eight has a negative gamma
    return dict(gamma=(1.0 + 0.4 * torch.rand(C, generator=gen)) * sign, beta=0.5 * torch.randn(C, generator=gen),
                rm=0.1 * torch.randn(C, generator=gen), rv=1.0 + torch.rand(C, generator=gen))


def bn_operands(c):
    gen = torch.Generator().manual_seed(case_seed(c))
    M, C = c['M'], c['C']
    o = dict(y=make_map(M, C, c['kind'], gen), dout=torch.randn((M, C), generator=gen), **make_params(C, gen))
    if c['forms']:
        o.update(res=torch.randn((M, C), generator=gen), y2=make_map(M, C, 'normal', gen), **{k + '2': v for k, v in make_params(C, gen).items()})
    return o


def sync_operands(c):
    gen = torch.Generator().manual_seed(case_seed(c))
    C = c['C']
    ys = []
    for r, M in enumerate(c['rows']):
        off = (1e3 if r % 2 == 0 else -1e3) if c['variant'] == 'split' else c['variant']
        ys.append(make_map(M, C, 'normal', gen, offset=off))
    return dict(ys=ys, douts=[torch.randn(y.shape, generator=gen) for y in ys], **make_params(C, gen))


# ---- plumbing --------------------------------------------------------------------------------------------------------
class Buf:
    """n elements inside a buffer whose every byte is 0xFF (a NaN in fp32 and fp64) or 0xA5 (integers), PAD elements either side."""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.fill = 0xA5 if dtype == torch.int64 else 0xFF
        size = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * PAD) * size,), self.fill, dtype=torch.uint8, device='cuda')
        self.v = self.raw.view(dtype)[PAD:PAD + n]
        self.lo, self.hi = self.raw[:PAD * size], self.raw[(PAD + n) * size:]
        if init is not None:
            self.v.copy_(init)

    def intact(self):
        return bool((self.lo == self.fill).all()) and bool((self.hi == self.fill).all())

    def untouched(self, lo=0, hi=None):
        size = self.v.element_size()
        hi = self.v.numel() if hi is None else hi
        return bool((self.raw[(PAD + lo) * size:(PAD + hi) * size] == self.fill).all())


def call(name, *args):
    from pointtinybenchmark_amd import _lib
    conv = lambda a: a.v.data_ptr() if isinstance(a, Buf) else a.data_ptr() if isinstance(a, torch.Tensor) else a      # noqa: E731
    return _lib.call(name, *[conv(a) for a in args], torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(name, a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), '%s: %s differs between two runs / entry points' % (name, k)


def finish(name, bufs, outs):
    """Guards intact, every output written and finite -> {key: tensor}."""
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), '%s: guard of %s overwritten' % (name, k)
    for k, t in outs.items():
        assert bool(torch.isfinite(t).all()) if t.is_floating_point() else True, '%s: %s has unwritten or non-finite elements' % (name, k)
    return outs


def worst(name, key, got, ref, bar, log):
    """Records the worst error / bar of a stage; a stage over its bar is reported by ``report`` once every stage has been judged."""
    q = R.ratio(got.double().reshape(ref.shape), ref, bar)
    w = float(q.max()) if q.numel() else 0.0
    log[key] = max(log.get(key, 0.0), w)
    if not w <= 1.0:
        bad = torch.nonzero(~(q <= 1.0))
        i = tuple(bad[0].tolist())
        log.setdefault('_failed', []).append('%s: %s: %d/%d over the bar, worst ratio %.3g; first at %s got %.9g ref %.9g bar %.3g' % (
            name, key, bad.shape[0], q.numel(), w, i, float(got.double().reshape(ref.shape)[i]), float(ref[i]), float(bar[i])))


def dd(t):
    return None if t is None else t.double()


def report(name, log):
    failed = log.pop('_failed', [])
    print('%s: worst |err| / bar: %s' % (name, ', '.join('%s %.3g' % kv for kv in sorted(log.items()))))
    assert not failed, '\n'.join(failed)


# ---- single rank -----------------------------------------------------------------------------------------------------
VEC = ('mean', 'rstd', 'scale', 'shift', 'center', 'cmean', 'cshift')


def chain(c, o, full=True):
    """stats -> apply -> backward through the C entries into guarded buffers.  full: the product's form (every vector, running
    buffers, nbt, centred apply with ReLU, masked backward); else every optional pointer null (mean / rstd only, plain apply
    without ReLU from the given scale / shift, backward without z, center, dgamma, dbeta)."""
    M, C = c['M'], c['C']
    name = case_id(c) + ('' if full else '/nulls')
    nbk = R.blocks(M, C)
    wsn = R.ws_floats(M, C)
    b = {k: Buf(C) for k in (VEC if full else VEC[:2])}
    b['ws_stats'], b['ws_bwd'], b['z'], b['dy'] = Buf(wsn), Buf(wsn), Buf(M * C), Buf(M * C)
    mom = -1.0 if c['mom'] is None else c['mom']
    if full:
        b.update(rm=Buf(C, init=o['rm']), rv=Buf(C, init=o['rv']), nbt=Buf(1, torch.int64, init=torch.tensor([3])), dgamma=Buf(C), dbeta=Buf(C))
        call('cpr_bn_batch_stats', o['y'], o['gamma'], o['beta'], b['rm'], b['rv'], b['nbt'], mom, EPS, *[b[k] for k in VEC], b['ws_stats'], M, C)
    else:
        call('cpr_bn_batch_stats', o['y'], o['gamma'], o['beta'], None, None, None, 0.1, EPS, b['mean'], b['rstd'], *[None] * 5, b['ws_stats'], M, C)
    torch.cuda.synchronize()
    assert b['ws_stats'].untouched(nbk * C * 2), name + ': the statistics launch wrote into the coef part of the workspace'
    outs = {k: b[k].v for k in b if k not in ('ws_stats', 'ws_bwd')}
    outs['part'] = b['ws_stats'].v[:nbk * C * 2].view(nbk, C, 2)
    if full:
        call('cpr_bn_apply', o['y'], b['center'], b['scale'], b['cshift'], None, None, None, None, None, b['z'], M, C, 1)
        call('cpr_bn_train_bwd', o['dout'], b['z'], o['y'], b['center'], b['cmean'], b['rstd'], o['gamma'], b['dy'], b['dgamma'], b['dbeta'],
             b['ws_bwd'], M, C)
    else:
        call('cpr_bn_apply', o['y'], None, o['scale'], o['shift'], None, None, None, None, None, b['z'], M, C, 0)
        call('cpr_bn_train_bwd', o['dout'], None, o['y'], None, b['mean'], b['rstd'], o['gamma'], b['dy'], None, None, b['ws_bwd'], M, C)
    outs['bpart'] = b['ws_bwd'].v[:nbk * C * 2].view(nbk, C, 2)
    outs['coef'] = b['ws_bwd'].v[nbk * C * 2:].view(C, 4)
    return finish(name, b, outs)


def check_chain(c, o, k, full, log):
    """Every stage of one chain run against its reference, judged on what that stage read."""
    M, C = c['M'], c['C']
    name = case_id(c) + ('' if full else '/nulls')
    y, yd, dout = o['y'], o['y'].double(), o['dout'].double()
    gamma, beta = dd(o['gamma']), dd(o['beta'])
    ref, bar = R.stats_part_ref(y)
    worst(name, 'stats_part.mean', k['part'][..., 0], ref[..., 0], bar[..., 0], log)
    worst(name, 'stats_part.M2', k['part'][..., 1], ref[..., 1], bar[..., 1], log)
    part_bar = bar
    nbt_after = 4 if full else None
    fin = R.finalize_ref(dd(k['part']), yd[0], M, gamma, beta, EPS, dd(o['rm']) if full else None, dd(o['rv']) if full else None,
                         -1.0 if c['mom'] is None else c['mom'], nbt_after)
    for key in (VEC if full else VEC[:2]):
        if key == 'center':
            assert torch.equal(bits(k['center']), bits(y[0])), name + ': center is not y[0] bit for bit'
        else:
            worst(name, 'finalize.' + key, k[key], *fin[key], log)
    if full:
        worst(name, 'finalize.running_mean', k['rm'], *fin['running_mean'], log)
        worst(name, 'finalize.running_var', k['rv'], *fin['running_var'], log)
        assert int(k['nbt'][0]) == 4, name + ': nbt incremented %d times' % (int(k['nbt'][0]) - 3)
        ce, sc, sh, mu, zmask = k['center'], k['scale'], k['cshift'], k['cmean'], k['z']
    else:
        ce, sc, sh, mu, zmask = None, o['scale'], o['shift'], k['mean'], None
    worst(name, 'apply', k['z'].view(M, C), *R.apply_ref(yd, dd(ce), dd(sc), dd(sh), full), log)
    zm = None if zmask is None else zmask.view(M, C)
    ref, bar = R.bwd_part_ref(dout, zm, yd, dd(ce), dd(mu))
    worst(name, 'bwd_part.sum_g', k['bpart'][..., 0], ref[..., 0], bar[..., 0], log)
    worst(name, 'bwd_part.sum_gx', k['bpart'][..., 1], ref[..., 1], bar[..., 1], log)
    bf = R.bwd_finalize_ref(dd(k['bpart']), M, dd(mu), dd(k['rstd']), gamma)
    worst(name, 'bwd_finalize.coef', k['coef'], *bf['coef'], log)
    assert torch.equal(bits(k['coef'][:, 3]), bits(mu)), name + ': coef[3] is not the mean bit for bit'
    if full:
        worst(name, 'bwd_finalize.dgamma', k['dgamma'], *bf['dgamma'], log)
        worst(name, 'bwd_finalize.dbeta', k['dbeta'], *bf['dbeta'], log)
    worst(name, 'bwd_apply', k['dy'].view(M, C), *R.bwd_apply_ref(dout, zm, yd, dd(k['coef']), dd(ce)), log)
    # end to end against fp64 F.batch_norm and its autograd
    e = R.end_to_end(y, gamma, beta, EPS, full, zm, dout, part_bar, lambda off: R.bwd_part_ref(dout, zm, yd, yd[0] if full else None, off)[1], full)
    worst(name, 'e2e.mean', k['mean'], *e['mean'], log)
    worst(name, 'e2e.rstd', k['rstd'], *e['rstd'], log)
    if full:                                                                    # the null form applies a scale / shift it was handed
        worst(name, 'e2e.z', k['z'].view(M, C), *e['z'], log)
        worst(name, 'e2e.dgamma', k['dgamma'], *e['dgamma'], log)
        worst(name, 'e2e.dbeta', k['dbeta'], *e['dbeta'], log)
    worst(name, 'e2e.dy', k['dy'].view(M, C), *e['dy'], log)
    for key in ('dgamma', 'dbeta'):                                             # the reference formulas are autograd's
        a = e[key + '_autograd']
        assert float((e[key][0] - a).abs().max()) <= 1e-9 * max(1.0, float(a.abs().max()))


def check_forms(c, o, k, log):
    """The residual and the two-input apply (center2 given and null) from the vectors of the chain."""
    M, C = c['M'], c['C']
    name = case_id(c) + '/forms'
    yd, y2d, resd = o['y'].double(), o['y2'].double(), o['res'].double()
    sc2, sh2, ce2 = o['gamma2'], o['beta2'], o['rm2']
    for key, relu, kw_k, kw_r in (
            ('apply.residual', 1, (o['res'], None, None, None, None), dict(residual=resd)),
            ('apply.two_input', 1, (None, o['y2'], ce2, sc2, sh2), dict(y2=y2d, ce2=dd(ce2), sc2=dd(sc2), sh2=dd(sh2))),
            ('apply.two_input_center2_null', 0, (None, o['y2'], None, sc2, sh2), dict(y2=y2d, ce2=None, sc2=dd(sc2), sh2=dd(sh2)))):
        def run():
            out = Buf(M * C)
            call('cpr_bn_apply', o['y'], k['center'], k['scale'], k['cshift'], *kw_k, out, M, C, relu)
            return finish(name, dict(out=out), dict(out=out.v))
        r1, r2 = run(), run()
        same_bits(name + ' ' + key, r1, r2)
        worst(name, key, r1['out'].view(M, C), *R.apply_ref(yd, dd(k['center']), dd(k['scale']), dd(k['cshift']), bool(relu), **kw_r), log)


def check_ops(c, o, k):
    """The ops wrappers give the bits of the direct calls."""
    from pointtinybenchmark_amd import ops
    name = case_id(c) + '/ops'
    rm, rv = o['rm'].clone(), o['rv'].clone()
    nbt = torch.full((), 3, device='cuda', dtype=torch.int64)
    st = ops.bn_batch_stats(o['y'], o['gamma'], o['beta'], rm, rv, nbt, c['mom'], EPS)
    z = ops.bn_apply(o['y'], st.scale, st.cshift, center=st.center, relu=True)
    dy, dg, db = ops.bn_train_bwd(o['dout'], o['y'], st.cmean, st.rstd, o['gamma'], mask=z, center=st.center)
    torch.cuda.synchronize()
    got = dict(zip(VEC, st), rm=rm, rv=rv, nbt=nbt.view(1), z=z.view(-1), dy=dy.view(-1), dgamma=dg, dbeta=db)
    same_bits(name, got, {key: k[key] for key in got})


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_bn_chain(c):
    o = {key: v.cuda() for key, v in bn_operands(c).items()}
    log = {}
    k = chain(c, o)
    same_bits(case_id(c), k, chain(c, o))
    check_chain(c, o, k, True, log)
    if c['nulls']:
        o2 = dict(o, scale=k['scale'], shift=k['shift'])
        k2 = chain(c, o2, full=False)
        same_bits(case_id(c) + '/nulls', k2, chain(c, o2, full=False))
        same_bits(case_id(c) + '/nulls vs full', {key: k2[key] for key in ('mean', 'rstd', 'part')}, {key: k[key] for key in ('mean', 'rstd', 'part')})
        check_chain(c, o2, k2, False, log)
    if c['forms']:
        check_forms(c, o, k, log)
    if c['ops']:
        check_ops(c, o, k)
    report(case_id(c), log)


# ---- SyncBN: one process plays the ranks --------------------------------------------------------------------------------
def play(c, o):
    C, rows = c['C'], c['rows']
    name = case_id(c)
    ranks = [dict() for _ in rows]
    bufs = {}
    for r, (M, y) in enumerate(zip(rows, o['ys'])):
        rec, ws = Buf(2 * C + 1, torch.float64), Buf(R.ws_floats(M, C))
        call('cpr_bn_sync_stats_local', y, rec, ws, M, C)
        bufs.update({'rec%d' % r: rec, 'ws%d' % r: ws})
        nbk = R.blocks(M, C)
        torch.cuda.synchronize()
        assert ws.untouched(nbk * C * 2), name + ': the local statistics launch wrote into the coef part of the workspace'
        ranks[r].update(rec=rec.v, part=ws.v[:nbk * C * 2].view(nbk, C, 2))
    recs = torch.stack([k['rec'] for k in ranks]).contiguous()
    for r, (M, y, dout) in enumerate(zip(rows, o['ys'], o['douts'])):
        b = {key: Buf(C) for key in VEC + ('dgamma', 'dbeta')}
        b.update(rm=Buf(C, init=o['rm']), rv=Buf(C, init=o['rv']), nbt=Buf(1, torch.int64, init=torch.tensor([3])), count=Buf(1, torch.float64),
                 z=Buf(M * C))
        call('cpr_bn_sync_stats_merge', recs, len(rows), y, o['gamma'], o['beta'], b['rm'], b['rv'], b['nbt'], 0.1, EPS, *[b[key] for key in VEC],
             b['count'], C)
        call('cpr_bn_apply', y, b['center'], b['scale'], b['cshift'], None, None, None, None, None, b['z'], M, C, 1)
        brec, ws = Buf(2 * C, torch.float64), Buf(R.ws_floats(M, C))
        call('cpr_bn_sync_bwd_local', dout, b['z'], y, b['center'], b['cmean'], b['rstd'], b['dgamma'], b['dbeta'], brec, ws, M, C)
        nbk = R.blocks(M, C)
        ranks[r].update({key: b[key].v for key in b}, brec=brec.v, bpart=ws.v[:nbk * C * 2].view(nbk, C, 2), ws=ws)
        bufs.update({'%s%d' % (key, r): v for key, v in b.items()}, **{'brec%d' % r: brec, 'wsb%d' % r: ws})
    torch.cuda.synchronize()
    brecs = torch.stack([k['brec'] for k in ranks]).contiguous()
    for r, (M, y, dout) in enumerate(zip(rows, o['ys'], o['douts'])):
        k = ranks[r]
        ws = k.pop('ws')
        assert ws.untouched(R.blocks(M, C) * C * 2), name + ': the local backward launch wrote into the coef part of the workspace'
        dy = Buf(M * C)
        call('cpr_bn_sync_bwd_merge', brecs, len(rows), k['count'], dout, k['z'], y, k['center'], k['cmean'], k['rstd'], o['gamma'], dy, ws, M, C)
        bufs['dy%d' % r] = dy
        k.update(dy=dy.v, coef=ws.v[R.blocks(M, C) * C * 2:].view(C, 4))
    flat = {'%s%d' % (key, r): v for r, k in enumerate(ranks) for key, v in k.items()}
    finish(name, bufs, flat)
    return recs, brecs, ranks, flat


@pytest.mark.parametrize('c', SYNC_CASES, ids=case_id)
def test_syncbn_ranks(c):
    o = sync_operands(c)
    o = {key: [t.cuda() for t in v] if isinstance(v, list) else v.cuda() for key, v in o.items()}
    C, rows, name = c['C'], c['rows'], case_id(c)
    log = {}
    recs, brecs, ranks, flat = play(c, o)
    same_bits(name, flat, play(c, o)[3])
    gamma, beta = dd(o['gamma']), dd(o['beta'])
    for r, (M, y, dout, k) in enumerate(zip(rows, o['ys'], o['douts'], ranks)):
        yd = y.double()
        ref, bar = R.stats_part_ref(y)
        worst(name, 'stats_part.mean', k['part'][..., 0], ref[..., 0], bar[..., 0], log)
        worst(name, 'stats_part.M2', k['part'][..., 1], ref[..., 1], bar[..., 1], log)
        worst(name, 'local.record', k['rec'], *R.local_record_ref(dd(k['part']), yd[0], M), log)
        assert float(k['rec'][2 * C]) == float(M)                                # the count travels as an exact integer value
        mg, Mg = R.merge_ref(recs, yd[0], gamma, beta, EPS, dd(o['rm']), dd(o['rv']), 0.1, 4)
        assert Mg == float(sum(rows)) and float(k['count'][0]) == Mg
        for key in VEC:
            if key == 'center':
                assert torch.equal(bits(k['center']), bits(y[0])), name + ': center is not this rank\'s y[0]'
            else:
                worst(name, 'merge.' + key, k[key], *mg[key], log)
        worst(name, 'merge.running_mean', k['rm'], *mg['running_mean'], log)
        worst(name, 'merge.running_var', k['rv'], *mg['running_var'], log)
        assert int(k['nbt'][0]) == 4
        for key in ('mean', 'rstd', 'scale', 'shift', 'rm', 'rv'):              # the same bits on every rank
            assert torch.equal(bits(k[key]), bits(ranks[0][key])), '%s: %s differs between ranks 0 and %d' % (name, key, r)
        zm = k['z'].view(M, C)
        worst(name, 'apply', zm, *R.apply_ref(yd, dd(k['center']), dd(k['scale']), dd(k['cshift']), True), log)
        ref, bar = R.bwd_part_ref(dout.double(), zm, yd, dd(k['center']), dd(k['cmean']))
        worst(name, 'bwd_part.sum_g', k['bpart'][..., 0], ref[..., 0], bar[..., 0], log)
        worst(name, 'bwd_part.sum_gx', k['bpart'][..., 1], ref[..., 1], bar[..., 1], log)
        worst(name, 'bwd_local.record', k['brec'], *R.bwd_local_record_ref(dd(k['bpart'])), log)
        bf = R.bwd_finalize_ref(dd(k['bpart']), M, dd(k['cmean']), dd(k['rstd']), gamma)
        worst(name, 'bwd_local.dgamma', k['dgamma'], *bf['dgamma'], log)
        worst(name, 'bwd_local.dbeta', k['dbeta'], *bf['dbeta'], log)
        worst(name, 'bwd_merge.coef', k['coef'], *R.bwd_merge_ref(brecs, Mg, dd(k['cmean']), dd(k['rstd']), gamma), log)
        assert torch.equal(bits(k['coef'][:, 3]), bits(k['cmean'])), name + ': coef[3] is not the mean bit for bit'
        worst(name, 'bwd_apply', k['dy'].view(M, C), *R.bwd_apply_ref(dout.double(), zm, yd, dd(k['coef']), dd(k['center'])), log)
    if c['ops']:
        from pointtinybenchmark_amd import ops
        lrecs = torch.stack([ops.bn_sync_local_stats(y)[0] for y in o['ys']])
        assert torch.equal(bits(lrecs), bits(recs))
        for r, (y, dout, k) in enumerate(zip(o['ys'], o['douts'], ranks)):
            rm, rv = o['rm'].clone(), o['rv'].clone()
            nbt = torch.full((), 3, device='cuda', dtype=torch.int64)
            st = ops.bn_sync_merge_stats(lrecs, y, o['gamma'], o['beta'], rm, rv, nbt, 0.1, EPS)
            z = ops.bn_apply(y, st.scale, st.cshift, center=st.center, relu=True)
            brec, ws, dg, db = ops.bn_sync_local_bwd(dout, y, st.cmean, st.rstd, mask=z, center=st.center)
            dy = ops.bn_sync_merge_bwd(brecs, ws, st.count, dout, y, st.cmean, st.rstd, o['gamma'], mask=z, center=st.center)
            torch.cuda.synchronize()
            got = dict(zip(VEC, st), rm=rm, rv=rv, nbt=nbt.view(1), count=st.count, z=z.view(-1), brec=brec, dgamma=dg, dbeta=db, dy=dy.view(-1))
            same_bits(name + '/ops rank %d' % r, got, {key: k[key] for key in got})
    report(name, log)


# ---- bn_fold / bn_fold_multi -----------------------------------------------------------------------------------------
def fold_operands(C, seed):
    gen = torch.Generator().manual_seed(seed)
    p = make_params(C, gen)
    var = torch.rand(C, generator=gen) * torch.tensor([1.0, 1e-3, 1e-6, 10.0])[torch.arange(C) % 4]
    var[::5] = 0.0                                                               # var down to 0: 1 / sqrt(eps)
    if C > 2:
        p['gamma'][2] = 0.0
    return dict(gamma=p['gamma'], beta=p['beta'], mean=10 * p['rm'], var=var)


FOLD_DIFFS = {}


@pytest.mark.parametrize('want_inv', [False, True], ids=['noinv', 'inv'])
@pytest.mark.parametrize('C', FOLD_C)
def test_bn_fold(C, want_inv):
    from pointtinybenchmark_amd import ops
    cpu = fold_operands(C, 8000 + C)
    o = {k: v.cuda() for k, v in cpu.items()}
    name = 'bn_fold C %d' % C

    def run():
        b = dict(scale=Buf(C), shift=Buf(C), inv_sigma=Buf(C))
        call('cpr_bn_fold', o['gamma'], o['beta'], o['mean'], o['var'], EPS, b['scale'], b['shift'], b['inv_sigma'] if want_inv else None, C)
        torch.cuda.synchronize()
        if not want_inv:
            assert b['inv_sigma'].untouched(), name + ': something wrote an inv_sigma nobody asked for'
        return finish(name, b, {k: b[k].v for k in b if want_inv or k != 'inv_sigma'})
    k = run()
    same_bits(name, k, run())
    ref = R.bn_fold_ref(*[dd(o[key]) for key in ('gamma', 'beta', 'mean', 'var')], EPS)
    log = {}
    for key in k:
        worst(name, key, k[key], *ref[key], log)
    sc, sh, inv = ops.bn_fold(o['gamma'], o['beta'], o['mean'], o['var'], EPS, want_inv)
    torch.cuda.synchronize()
    same_bits(name + '/ops', dict(scale=sc, shift=sh, **(dict(inv_sigma=inv) if want_inv else {})), k)
    # reported, not asserted: outputs whose bits differ from the fp32 torch expression of layers.folded_bn evaluated on the CPU
    scale_t = (cpu['gamma'] / torch.sqrt(cpu['var'] + EPS)).float()
    shift_t = (cpu['beta'] - cpu['mean'] * scale_t).float()
    diff = int((bits(k['scale'].cpu()) != bits(scale_t)).sum()) + int((bits(k['shift'].cpu()) != bits(shift_t)).sum())
    FOLD_DIFFS[(C, want_inv)] = diff
    report(name, log)
    print('%s: %d of %d scale / shift outputs differ in bits from the fp32 torch expression on the CPU (total so far %d of %d)' % (
        name, diff, 2 * C, sum(FOLD_DIFFS.values()), 2 * sum(cc for cc, _ in FOLD_DIFFS)))


def test_bn_fold_multi_is_bn_fold_job_by_job():
    """A job table built the way layers._PackCache.refresh_all builds it (FoldJob rows, one uint8 device tensor), jobs of different C
    and mixed null outputs; every output of every job lives in ONE guarded arena, so the slot of a null output must stay untouched."""
    from pointtinybenchmark_amd import layers
    jobs = [dict(C=C, outs=outs.split(), o={k: v.cuda() for k, v in fold_operands(C, 8100 + i).items()}) for i, (C, outs) in enumerate(FOLD_MULTI)]
    slot = lambda C: (C + 63) // 64 * 64                                        # noqa: E731
    total = sum(3 * slot(j['C']) for j in jobs)

    def run():
        arena = Buf(total)
        rows, off, views = [], 0, []
        for j in jobs:
            ptr, v = {}, {}
            for key in ('scale', 'shift', 'inv'):
                v[key] = arena.v[off:off + j['C']]
                ptr[key] = v[key].data_ptr() if key in j['outs'] else 0
                off += slot(j['C'])
            o = j['o']
            rows.append(layers.FoldJob._ROW.pack(o['gamma'].data_ptr(), o['beta'].data_ptr(), o['mean'].data_ptr(), o['var'].data_ptr(),
                                                 ptr['scale'], ptr['shift'], ptr['inv'], j['C'], EPS))
            views.append(v)
        assert all(len(r) == 64 for r in rows)
        table = torch.frombuffer(bytearray(b''.join(rows)), dtype=torch.uint8).cuda()
        call('cpr_bn_fold_multi', table, len(jobs), max(j['C'] for j in jobs))
        torch.cuda.synchronize()
        assert arena.intact(), 'bn_fold_multi: arena guard overwritten'
        return arena, views
    arena, views = run()
    arena2, _ = run()
    assert torch.equal(bits(arena.v), bits(arena2.v)), 'bn_fold_multi: two runs differ'
    written = torch.zeros(total, dtype=torch.bool, device='cuda')
    off = 0
    for j, v in zip(jobs, views):
        C, o = j['C'], j['o']
        b = dict(scale=Buf(C), shift=Buf(C), inv=Buf(C))
        call('cpr_bn_fold', o['gamma'], o['beta'], o['mean'], o['var'], EPS, b['scale'], b['shift'], b['inv'], C)
        torch.cuda.synchronize()
        for key in ('scale', 'shift', 'inv'):
            if key in j['outs']:
                assert torch.equal(bits(v[key]), bits(b[key].v)), 'bn_fold_multi: job C %d: %s is not bn_fold bit for bit' % (C, key)
                written[off:off + C] = True
            off += slot(C)
    raw = arena.v.view(torch.int32)
    assert bool((raw[~written] == -1).all()), 'bn_fold_multi: wrote through a null output pointer or past a job\'s C'


# ---- clip norm and SGD -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('acc', [0, 1], ids=['acc0', 'acc1'])
@pytest.mark.parametrize('n', SUMSQ_N)
def test_grad_sumsq(n, acc):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(9000 + n % 1000)
    gr = (torch.randn(n, generator=gen) * (1 + 9 * torch.rand(n, generator=gen))).cuda()
    base = 1234.5678
    name = 'sumsq n %d acc %d' % (n, acc)
    grid = R.sumsq_grid(n)

    def run(via_ops=False):
        ws, out = Buf(R.SUMSQ_CAP, torch.float64), Buf(1, torch.float64, init=torch.tensor([base], dtype=torch.float64) if acc else None)
        if via_ops:
            ops.grad_sumsq(gr, out.v, ws.v, acc)
        else:
            call('cpr_grad_sumsq', gr, n, ws, out, acc)
        torch.cuda.synchronize()
        assert ws.untouched(grid), name + ': partials past the grid were written'
        return finish(name, dict(ws=ws, out=out), dict(out=out.v, partials=ws.v[:grid]))
    k = run()
    same_bits(name, k, run())
    same_bits(name + '/ops', k, run(True))
    ref, bar = R.sumsq_ref(gr.double(), base if acc else None)
    err = abs(float(k['out'][0]) - ref)
    print('%s: worst |err| / bar: out %.3g' % (name, err / bar))
    assert err <= bar, (name, float(k['out'][0]), ref, bar)
    # each partial is its block's own elements: block b takes i with (i // 256) % grid == b
    idx = (torch.arange(n, device='cuda') // R.BLOCK) % grid
    pref = torch.zeros(grid, dtype=torch.float64, device='cuda').index_add_(0, idx, gr.double() ** 2)
    assert bool(((k['partials'] - pref).abs() <= (R.D64 + R.U64) * pref).all()), name + ': a partial is not its block\'s sum'


@pytest.mark.parametrize('form', SGD_FORMS, ids=[f['name'] for f in SGD_FORMS])
@pytest.mark.parametrize('n', SGD_N)
def test_sgd_step(n, form):
    from pointtinybenchmark_amd import ops
    gen = torch.Generator().manual_seed(9500 + n % 1000)
    p0, g0, m0 = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    g0 = torch.where(g0 >= 0, 3 * g0 + 8, 3 * g0 - 8)                           # |g| >= 8: max_norm 0.5 clips at every n and grad_scale
    lr = 0.02
    name = 'sgd n %d %s' % (n, form['name'])
    norm2 = float((g0.double() ** 2).sum()) if form['max_norm'] > 0 else None
    n2 = torch.tensor([norm2], dtype=torch.float64, device='cuda') if norm2 is not None else None
    coef, crel = R.sgd_coef_ref(norm2, form['max_norm'], form['gs'])
    clipped = form['max_norm'] > 0 and coef < R.f32(form['gs'])
    assert clipped == (form['max_norm'] == 0.5), 'the table\'s clip forms are not what they say'
    use_buf = form['mu'] != 0

    def run(via_ops=False):
        p, buf = Buf(n, init=p0), Buf(n, init=m0 if use_buf else None)
        args = (lr, form['mu'], form['wd'], form['max_norm'], form['gs'], form['first'])
        if via_ops:
            ops.sgd_step(p.v, g0, buf.v if use_buf else None, n2, *args)
        else:
            call('cpr_sgd_step', p, g0, buf if use_buf else None, n2, n, *args)
        torch.cuda.synchronize()
        if not use_buf:
            assert buf.untouched(), name + ': mu == 0 touched a momentum buffer'
        return finish(name, dict(p=p, buf=buf), dict(p=p.v, **(dict(buf=buf.v) if use_buf else {})))
    k = run()
    same_bits(name, k, run())
    same_bits(name + '/ops', k, run(True))
    ref = R.sgd_ref(p0.double(), g0.double(), m0.double() if use_buf else None, coef, crel, lr, form['mu'], form['wd'], form['first'])
    log = {}
    worst(name, 'p', k['p'], *ref['p'], log)
    if use_buf:
        worst(name, 'buf', k['buf'], *ref['buf'], log)
    report(name, log)
