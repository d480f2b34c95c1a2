"""CPU only: the table of tests/test_gpu_stream_instances.py meets its coverage conditions, the launch rules it restates are
the library's, the bars of tests/stream_fp64_ref.py pass fp32 emulations of the kernels and catch the faults they are there
for, the float32 index rules of the nearest upsample hold, and the entry points refuse arguments that would reach a launch
with an empty grid or a division by zero."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stream_fp64_ref as R
from tests.test_gpu_stream_instances import (CASES, EXISTING, RATIOS, case_id, gnb_reference, make_x, slots_of)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
ERR_ARG = -1001


def of(op):
    return [c for c in CASES if c['op'] == op]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _lib():
    from pointtinybenchmark_amd import _lib
    return _lib.load()


def _body(text, entry):
    """Source text of one extern "C" entry point or static launcher, up to its closing brace at column 0."""
    i = text.index(entry + '(')
    return text[i:text.index('\n}', i)]


# ---- launch rules ----------------------------------------------------------------------------------------------
def test_grid_caps_are_the_constants_in_the_source():
    npool, bwd = _src('norm_pool.hip'), _src('backward.hip')
    where = dict(gn_apply=(npool, 'int cpr_gn_apply'), maxpool=(npool, 'int maxpool3x3s2_launch'), maxpool_bf16=(npool, 'int maxpool3x3s2_bf16_launch'),
                 nchw_to_nhwc4=(npool, 'int cpr_nchw_to_nhwc4'), gn_bwd_apply=(bwd, 'int gn_bwd_launch'),
                 upsample_add_bwd=(bwd, 'int cpr_upsample_add_bwd'), axpby=(bwd, 'int cpr_axpby'),
                 zero_insert=(bwd, 'int cpr_zero_insert'), phase_scatter_add=(bwd, 'int cpr_phase_scatter_add'))
    for k, (text, entry) in where.items():
        m = re.findall(r'cdivll\(\w+, 256\) < (\d+) \? cdivll\(\w+, 256\) : (\d+)', _body(text, entry))
        assert m and all(int(a) == int(b) == R.GRID_CAPS[k] for a, b in m), (k, m)
    body = _body(npool, 'int cpr_gn_apply_bf16')
    assert re.search(r'blocks < (\d+) \? blocks : \1', body).group(1) == str(R.GRID_CAPS['gn_apply_bf16_wide'])
    assert re.findall(r'cdivll\(total, 256\) < (\d+)', body) == [str(R.GRID_CAPS['gn_apply_bf16'])]
    assert 'C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0 && np < (1ll << 31)' in body           # R.bf16_wide
    assert len(re.findall(r'dim3\(256\)', npool)) >= 10 and R.BLOCK == 256


def test_colsum_and_slot_rules_are_the_source():
    bwd, npool = _src('backward.hip'), _src('norm_pool.hip')
    body = _body(bwd, 'static int relu_bwd_rows_per_block')
    assert re.search(r'int rows = (\d+);', body).group(1) == '128'
    assert re.search(r'while \(rows > (\d+) && cdivll\(M, rows\) < (\d+)\) rows >>= 1;', body).groups() == ('16', '2048')
    body = _body(bwd, 'static void launch_colsum')
    assert re.search(r'int nsplit = \(rows \+ 255\) / (\d+);', body).group(1) == str(R.COLSUM_SPLIT_ROWS)
    assert re.search(r'if \(nsplit > (\d+)\) nsplit = \1;', body).group(1) == str(R.COLSUM_MAX_SPLITS)
    assert 'const int c0 = blockIdx.y * 1024;' in bwd and R.RELU_COL_GROUP == 1024
    for text in (bwd, npool):
        assert 'const int per = (HW + P - 1) / P;' in text and 'const int p0 = slot * per, p1 = min(HW, p0 + per);' in text
    ops = open(os.path.join(os.path.dirname(CSRC), 'ops.py')).read()
    assert ops.count('slots = max(1, min(256, HW // 256))') == 2                                   # R.default_slots
    assert [R.rows_per_block(m) for m in (1, 65504, 65505, 131008, 131009, 262016, 262017)] == [16, 16, 32, 32, 64, 64, 128]
    assert (R.colsum_plan(256), R.colsum_plan(257), R.colsum_plan(20000)) == ((1, 256), (2, 129), (64, 313))
    assert R.slot_extents(100, 30)[24:27] == [(96, 100), (100, 100), (100, 100)] and R.slot_extents(1600, 6)[-1] == (1335, 1600)


def test_workspace_query_agrees_with_the_restated_rule():
    L = _lib()
    rng = np.random.default_rng(0)
    ms = [c['M'] for c in of('rbc')] + [int(v) for v in rng.integers(1, 600000, size=200)] + [2048 * r + d for r in (16, 32, 64, 128) for d in (-1, 0, 1)]
    for M in ms:
        for C in (4, 160, 1028):
            assert L.cpr_relu_bwd_colsum_ws(ctypes.c_longlong(M), C) == R.relu_bwd_ws(M, C), (M, C)
    assert {R.rows_per_block(m) for m in ms} == {16, 32, 64, 128}


# ---- coverage --------------------------------------------------------------------------------------------------
def _lanes(c):
    """(kernel, lanes of its grid-stride loop) of every grid-stride launch a case makes."""
    op = c['op']
    if op in ('gn', 'apply'):
        npix = c['N'] * c['H'] * c['W']
        if c['dt'] == 'bf16' and R.bf16_wide(c['C'], npix):
            return [('gn_apply_bf16_wide', R.cdiv(npix, 256 // (c['C'] // 8)) * 256)]         # blocks, in units of 256 lanes
        return [('gn_apply_bf16' if c['dt'] == 'bf16' else 'gn_apply', npix * c['C'] // 4)]
    if op == 'gnbwd':
        return [('gn_bwd_apply', c['N'] * c['H'] * c['W'] * c['C'] // 4)]
    if op == 'ups':
        return [('upsample_add_bwd', c['N'] * c['UH'] * c['UW'] * c['C'] // 4)]
    if op == 'axpby':
        return [('axpby', c['n'])]
    if op == 'zi':
        return [('zero_insert', c['N'] * c['H'] * c['W'] * c['C'] // 4)]
    if op == 'psa':
        return [('phase_scatter_add', c['N'] * R.cdiv(c['H'] - c['py'], c['s']) * R.cdiv(c['W'] - c['px'], c['s']) * c['C'] // 4)]
    if op == 'pool':
        k = 'maxpool_bf16' if c['dt'] == 'bf16' else 'maxpool'
        return [(k + ('_rec' if c['rec'] else ''), c['N'] * ((c['H'] - 1) // 2 + 1) * ((c['W'] - 1) // 2 + 1) * c['C'] // 4)]
    if op == 'nhwc4':
        return [('nchw_to_nhwc4', c['N'] * c['H'] * c['W'])]
    return []


def test_every_grid_stride_kernel_wraps_is_ragged_and_is_tiny_somewhere():
    seen = {}
    for c in CASES:
        for k, lanes in _lanes(c):
            cap = R.GRID_CAPS[k.replace('_rec', '')]
            s = seen.setdefault(k, set())
            if R.wraps(lanes, cap):
                s.add('wraps')
            if lanes % 256:
                s.add('ragged')
            if lanes < 256:
                s.add('tiny')
    want = {'gn_apply', 'gn_apply_bf16', 'gn_bwd_apply', 'upsample_add_bwd', 'axpby', 'zero_insert', 'phase_scatter_add',
            'maxpool', 'maxpool_rec', 'maxpool_bf16', 'maxpool_bf16_rec', 'nchw_to_nhwc4'}
    for k in want:
        need = {'wraps', 'ragged', 'tiny'} if not k.startswith('maxpool_') else {'wraps'}
        assert need <= seen.get(k, set()), (k, seen.get(k))
    assert 'wraps' in seen['gn_apply_bf16_wide']
    pools = of('pool')
    assert {(c['dt'], c['rec']) for c in pools} == {('f32', False), ('f32', True), ('bf16', False), ('bf16', True)}
    assert {1, 2} <= {c['H'] for c in pools} | {c['W'] for c in pools} and any(c['H'] % 2 and c['W'] % 2 for c in pools)
    assert any(c['data'] == 'nonpos' and c['rec'] for c in pools) and any(c['data'] == 'ties' and c['rec'] for c in pools)
    for c in CASES:
        dims = [c[k] for k in ('N', 'H', 'W', 'C') if k in c]
        assert int(np.prod(dims or [1])) * 4 < (1 << 30) and c.get('M', 1) * c.get('C', 1) * 4 < (1 << 30), case_id(c)


def test_wide_and_generic_bf16_apply_coverage():
    wide, gen = [], []
    for c in of('gn') + of('apply'):
        if c['dt'] == 'bf16':
            (wide if R.bf16_wide(c['C'], c['N'] * c['H'] * c['W']) else gen).append(c)
    blocks = lambda c: R.cdiv(c['N'] * c['H'] * c['W'], 256 // (c['C'] // 8))
    assert any(blocks(c) > R.GRID_CAPS['gn_apply_bf16_wide'] and c['N'] >= 3 for c in wide)
    assert any((c['H'] * c['W']) % (256 // (c['C'] // 8)) != 0 and c['N'] > 1 for c in wide)
    assert {(bool(c['up']), c['relu']) for c in wide} >= {(True, True), (False, False)}
    assert {bool(c['up']) for c in wide} == {True, False} == {c['relu'] for c in wide}
    assert any(c['C'] % 8 != 0 for c in gen) and any(c['C'] % 8 == 0 and 256 % (c['C'] // 8) != 0 for c in gen)


@pytest.mark.parametrize('op', ['gn', 'gnbwd'])
def test_groupnorm_statistics_coverage(op):
    cs = of(op)
    assert {64, 128, 256, 512, 1024} <= {c['C'] for c in cs}
    assert {1, 32} <= {c['G'] for c in cs} and any(c['G'] == c['C'] for c in cs)
    assert any(c['C'] // c['G'] == 2 for c in cs)                                   # a thread's four channels span two groups
    ext = [R.slot_extents(c['H'] * c['W'], slots_of(c)) for c in cs]
    assert any(len(e) == 1 for e in ext) and any(len(e) == 256 for e in ext) and any(c['P'] is None for c in cs)
    assert any(0 < e[-1][1] - e[-1][0] < e[0][1] - e[0][0] for e in ext), 'no ragged last slot'
    assert any(e[-1][1] == e[-1][0] for e in ext), 'no empty last slot'
    assert any(c['H'] * c['W'] < 256 // (c['C'] // 4) for c in cs), 'no map below one pass of the block'
    assert {c['ratio'] for c in cs} == set(RATIOS)
    assert all(R.lanes_ok(c['C']) and c['C'] % c['G'] == 0 for c in cs)
    if op == 'gn':
        assert any(c['P'] == c['H'] * c['W'] // 128 for c in cs), 'no conv-epilogue slot count'
        assert all(c['C'] // c['G'] <= 256 for c in cs)
    else:
        assert {(c['entry'], c['out']) for c in cs} >= {('f32', 'dx'), ('bf16', 'dx'), ('bf16', 'dx16'), ('bf16', 'both'),
                                                          ('dz16', 'dx'), ('dz16', 'dx16'), ('dz16', 'both')}
        assert {c['acc'] for c in cs} == {True, False} == {c['relu'] for c in cs}


def test_column_sum_and_bn_fold_coverage():
    rbc = of('rbc')
    assert {R.rows_per_block(c['M']) for c in rbc} == {16, 32, 64, 128}
    blocks = [R.cdiv(c['M'], R.rows_per_block(c['M'])) for c in rbc]
    assert min(blocks) <= 256 < max(blocks)
    assert {4, 64, 160, 1024, 1028, 2048} <= {c['C'] for c in rbc}
    assert any(c['C'] > 1024 and R.cdiv(c['M'], R.rows_per_block(c['M'])) > 256 for c in rbc)
    assert {c['y'] for c in rbc} == {None, 'f32', 'bf16'}
    assert all(any(c[k] for c in rbc) for k in ('add', 'want16', 'acc')) and any(not c['gout'] for c in rbc)
    assert any(c['tiles'] > 16384 and R.colsum_plan(c['tiles'])[0] == 64 for c in of('pcs'))
    assert {R.colsum_plan(c['tiles'])[0] > 1 for c in of('pcs')} == {True, False}
    bnf = of('bnf')
    ks, ts = {c['K'] for c in bnf}, {c['tiles'] for c in bnf}
    assert {576, 4608} <= ks and min(ks) < 256
    assert {1, 37} <= ts and any(256 < t <= 4096 for t in ts) and any(t > 4096 for t in ts) and 0 in ts
    assert any(c['null'] for c in bnf) and all(c['Cout'] > 3 for c in bnf)             # channel 3 carries the zero gamma


def test_upsample_size_pairs_cover_both_kernels():
    fwd = [(c['H'], c['W']) + c['up'] for c in of('gn') + of('apply') if c['up']]
    bwd = [(c['H'], c['W'], c['UH'], c['UW']) for c in of('ups')]
    for name, pairs in (('gn_apply', fwd), ('upsample_add_bwd', bwd)):
        one = [(h, u) for h, w, u, v in pairs] + [(w, v) for h, w, u, v in pairs]
        assert any(h == 2 * u for h, u in one), name
        assert any(h == 2 * u - 1 and u > 1 for h, u in one), name
        assert (25, 13) in one and (8, 7) in one, name
        assert any(u == 1 and h > 1 for h, u in one) and any(h == u for h, u in one), name
        assert any(h * v != w * u for h, w, u, v in pairs), name
    assert {c['acc'] for c in of('ups')} == {True, False}


def test_every_shape_of_the_existing_kernel_tests_is_in_the_table():
    def has(op, **kw):
        return any(all(c.get(k) == v for k, v in kw.items()) for c in of(op))
    for N, H, W, C, up in EXISTING['gn']:
        assert has('gn', N=N, H=H, W=W, C=C, G=32, P=None, dt='f32', up=up), (N, H, W, C)
    for N, H, W, C, up in EXISTING['gn_bf16']:
        assert has('gn', N=N, H=H, W=W, C=C, G=32, P=None, dt='bf16', up=up, relu=True)
    for N, H, W, C in EXISTING['apply']:
        assert has('apply', N=N, H=H, W=W, C=C, dt='f32')
    for N, H, W, C in EXISTING['b8']:
        assert has('b8', N=N, H=H, W=W, C=C)
    for N, H, W, C in EXISTING['gnbwd']:
        assert has('gnbwd', N=N, H=H, W=W, C=C, G=32, P=None, entry='f32')
    for N, H, W, C in EXISTING['gnbwd_bf16']:
        assert has('gnbwd', N=N, H=H, W=W, C=C, G=32, P=None, entry='bf16', out='both') and has('gnbwd', N=N, H=H, W=W, C=C, entry='dz16', out='both')
    for N, H, W, UH, UW, C in EXISTING['ups']:
        assert has('ups', N=N, H=H, W=W, UH=UH, UW=UW, C=C)
    for M, C in EXISTING['rbc']:
        assert has('rbc', M=M, C=C)
    for Cout, K, tiles in EXISTING['bnf']:
        assert has('bnf', Cout=Cout, K=K, tiles=tiles)
    for N, H, W, C, dt in EXISTING['pool']:
        assert has('pool', N=N, H=H, W=W, C=C, dt=dt, data='normal')
    assert has('nhwc4', N=2, C=3, H=17, W=23) and has('nchw', N=2, H=19, W=21, C=70)
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for op in ('gn', 'apply', 'b8', 'gnbwd', 'ups', 'rbc', 'bnf', 'axpby', 'pool', 'nhwc4', 'nchw'):
        assert any(c['ops'] for c in of(op)), op + ': no case goes through the ops wrapper'


@pytest.mark.parametrize('c', of('gnbwd'), ids=case_id)
def test_reference_mask_is_unambiguous_enough(c):
    """At most AMBIG_CAP of a case's elements may sit where the fp32 ReLU mask can differ from the fp64 one."""
    R._threads()
    share = gnb_reference(c)['amb_share']
    assert share <= R.AMBIG_CAP, share


# ---- fp32 emulations of the kernels' summation orders ----------------------------------------------------------------
def emu_stats(x, P, drop=None, short_last=0):
    """gn_stats in float32 in the kernel's order: lane (pl, q) adds pixels p0 + pl, p0 + pl + PP, ...; then the PP rows of the
    block in order.  x (HW, C) float32 -> (P, C, 2).  drop = (slot, i): that pixel is skipped; short_last: the last non-empty
    slot ends that many pixels early."""
    HW, C = x.shape
    PP = 256 // (C // 4)
    ext = R.slot_extents(HW, P)
    last = max(i for i, (p0, p1) in enumerate(ext) if p1 > p0)
    out = np.zeros((P, C, 2), np.float32)
    for s, (p0, p1) in enumerate(ext):
        if s == last:
            p1 -= short_last
        v = x[p0:p1].copy()
        if drop is not None and drop[0] == s:
            v[drop[1]] = 0
        n = p1 - p0
        trips = R.cdiv(max(n, 1), PP)
        v = np.concatenate([v, np.zeros((trips * PP - n, C), np.float32)]).reshape(trips, PP, C)
        acc = np.zeros((PP, C), np.float32)
        acq = np.zeros((PP, C), np.float32)
        for t in range(trips):
            acc += v[t]
            acq += v[t] * v[t]
        a = np.zeros(C, np.float32)
        q = np.zeros(C, np.float32)
        for r in range(PP):
            a += acc[r]
            q += acq[r]
        out[s, :, 0], out[s, :, 1] = a, q
    return out


def _worst(got, ref, bar):
    return float(R.ratio(torch.as_tensor(np.asarray(got)).double().reshape(ref.shape), ref, bar).max())


@pytest.mark.parametrize('HW,C,P,ratio', [(16384, 256, 64, 0), (16384, 256, 64, 4), (1600, 256, 6, 4), (16384, 64, 256, 0), (16384, 64, 256, 4)])
def test_slot_bars_pass_the_emulation_and_catch_a_missing_pixel(HW, C, P, ratio):
    gen = torch.Generator().manual_seed(HW + C + P + ratio)
    x = make_x(1, HW, 1, C, 32, ratio, gen, False).view(HW, C)
    ref, bar = R.stats_slots(x.double().view(1, HW, C), P)
    xn = x.numpy()
    ok = _worst(emu_stats(xn, P), ref[0], bar[0])
    assert ok < 0.5, ok
    if HW // P <= 300:          # slots of real size; a slot of thousands of pixels hides one pixel in its worst-case bar
        assert _worst(emu_stats(xn, P, drop=(P // 2, 3)), ref[0], bar[0]) > 1
        assert _worst(emu_stats(xn, P, short_last=1), ref[0], bar[0]) > 1


def test_end_to_end_bar_passes_the_emulation_and_records_conditioning():
    """gn_stats (emulated) + gn_finalize (double) against fp64 GroupNorm: inside the propagated bar at every ratio; the relative
    error of rstd grows with (mean / std)^2 as the module docstring says."""
    errs = {}
    for ratio in (0, 4, 32):
        gen = torch.Generator().manual_seed(7 + ratio)
        HW, C, P, G = 16384, 64, 64, 32
        x = make_x(1, HW, 1, C, G, ratio, gen, False).view(1, HW, C)
        gamma, beta = torch.rand(C, generator=gen).double() + 0.5, torch.randn(C, generator=gen).double()
        _, bar = R.stats_slots(x.double(), P)
        part = torch.as_tensor(emu_stats(x[0].numpy(), P)).double().view(1, P, C, 2)
        fin = R.finalize_from_partials(part, gamma, beta, G, HW, 1e-5)
        e2e = R.groupnorm_end_to_end(x.double(), bar, gamma, beta, G, 1e-5)
        for k in ('mean', 'rstd', 'a', 'b'):
            assert _worst(fin[k][0].float(), e2e[k][0], e2e[k][1]) < 0.5, (ratio, k)
        errs[ratio] = float(((fin['rstd'][0] - e2e['rstd'][0]).abs() / e2e['rstd'][0]).max())
    assert errs[0] < 1e-6 and errs[32] < 1e-3, errs


def _fma32(x, a, b):
    return (x.double() * a.double() + b.double()).float()


def test_apply_bar_catches_the_previous_images_affine_and_bf16_truncation():
    gen = torch.Generator().manual_seed(3)
    N, HW, C = 3, 63, 64
    x = torch.randn((N, HW, C), generator=gen).bfloat16().float()
    a, b = torch.rand((N, 1, C), generator=gen) + 0.5, torch.randn((N, 1, C), generator=gen)
    ref, bar = R.apply_ref(x.double(), a.double(), b.double(), True)
    y = _fma32(x, a, b).relu()
    assert _worst(y, ref, bar) <= 0.5
    bad = y.clone()
    bad[1, :4] = _fma32(x[1, :4], a[0], b[0]).relu()           # the first pixels of image 1 with image 0's affine
    assert _worst(bad, ref, bar) > 1
    ref16, bar16 = R.apply_ref(x.double(), a.double(), b.double(), True, None, True)
    assert _worst(y.bfloat16().float(), ref16, bar16) <= 1.0       # round to nearest even errs by up to the half step itself
    trunc = (y.view(torch.int32) & -65536).view(torch.float32)
    assert _worst(trunc, ref16, bar16) > 1


def test_gn_bwd_bars_pass_fp32_sums_and_catch_a_group_index_off_by_one():
    gen = torch.Generator().manual_seed(4)
    N, HW, C, G, P = 1, 144, 64, 32, 1
    cpg = C // G
    x = make_x(N, 12, 12, C, G, 4, gen, False).view(N, HW, C)
    dz = torch.randn((N, HW, C), generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    xg = x.double().view(N, HW, G, cpg)
    mean = xg.mean((1, 3)).float()
    rstd = ((xg.var((1, 3), unbiased=False) + 1e-5) ** -0.5).float()
    a = rstd.repeat_interleave(cpg, 1) * gamma
    b = -mean.repeat_interleave(cpg, 1) * a
    d = lambda t: t.double()
    ref = R.gn_bwd_ref(d(x), d(dz), d(a), d(b), d(mean), d(rstd), d(gamma), G, P, False)

    def emu(shift):
        grp = np.minimum((np.arange(C) + shift) // cpg, G - 1)
        mu, rs = mean[0, grp], rstd[0, grp]
        s1 = np.zeros(C, np.float32)
        s2 = np.zeros(C, np.float32)
        for p in range(HW):
            s1 += dz[0, p].numpy()
            s2 += (dz[0, p] * (x[0, p] - mu) * rs).numpy()
        return np.stack([s1, s2], -1)

    assert _worst(emu(0), ref['part'][0][0, 0], ref['part'][1][0, 0]) < 0.5
    assert _worst(emu(1), ref['part'][0][0, 0], ref['part'][1][0, 0]) > 1
    # dx: a wrong group for a thread's third and fourth channel (cpg4 mis-derived) shows in the elementwise bar
    k2, k3 = ref['k2'][0].float().double(), ref['k3'][0].float().double()
    n0 = torch.zeros(HW, dtype=torch.long)
    rr, bar, alt, bar_alt = R.gn_bwd_dx(d(x[0]), d(dz[0]), ref['dy'][0], ref['amb'][0], d(a)[n0], k2[n0], k3[n0], G, False)
    k2c, k3c = k2[0].repeat_interleave(cpg).float(), k3[0].repeat_interleave(cpg).float()
    good = dz[0] * a[0] + x[0] * k2c + k3c
    assert float(R.ratio2(good, rr, bar, alt, bar_alt).max()) < 1
    wrong = dz[0] * a[0] + x[0] * torch.roll(k2c, 2) + torch.roll(k3c, 2)
    assert float(R.ratio2(wrong, rr, bar, alt, bar_alt).max()) > 1


def test_upsample_bar_catches_one_dropped_child():
    gen = torch.Generator().manual_seed(5)
    d = torch.randn((1, 25, 8, 8), generator=gen)
    ref, bar = R.upsample_add_bwd_ref(d.double(), 13, 7)
    iy, ix = R.nearest_index(25, 13), R.nearest_index(8, 7)

    def emu(skip=None):
        out = torch.zeros((1, 13, 7, 8))
        for y in range(25):
            for x in range(8):
                if (y, x) != skip:
                    out[0, iy[y], ix[x]] += d[0, y, x]
        return out

    assert _worst(emu(), ref, bar) <= 1.0       # two children: the bar IS the one rounding's bound, so nothing below 1 can be asked
    assert _worst(emu(skip=(24, 7)), ref, bar) > 1 and _worst(emu(skip=(0, 0)), ref, bar) > 1


def test_column_sum_bars_catch_a_dropped_block_tile_and_a_short_dot():
    gen = torch.Generator().manual_seed(6)
    M, C = 70000, 8
    gm = torch.randn((M, C), generator=gen)
    ref, bar = R.relu_colsum_ref(gm.double())
    rpb = R.rows_per_block(M)
    blocks = R.cdiv(M, rpb)
    part = np.zeros((blocks, C), np.float32)
    gn = np.concatenate([gm.numpy(), np.zeros((blocks * rpb - M, C), np.float32)]).reshape(blocks, rpb, C)
    for r in range(rpb):
        part[:, :] += gn[:, r]
    total = part.astype(np.float64).sum(0).astype(np.float32)
    assert _worst(total, ref, bar) < 0.5
    assert _worst((part.astype(np.float64).sum(0) - part[blocks // 2]).astype(np.float32), ref, bar) > 1
    tiles = torch.randn((20000, C, 2), generator=gen)
    ref, bar = R.part_colsum_ref(tiles.double())
    t0 = tiles[..., 0].double()
    assert _worst(t0.sum(0).float(), ref, bar) < 0.5
    assert _worst((t0.sum(0) - t0[12345]).float(), ref, bar) > 1
    # rows_per_split off by one in the two-pass fold: the last row of every split is lost
    nsplit, per = R.colsum_plan(20000)
    lost = t0.sum(0) - sum(t0[min((s + 1) * per, 20000) - 1] for s in range(nsplit))
    assert _worst(lost.float(), ref, bar) > 1
    Cout, K = 8, 576
    Gw, Wt = torch.randn((Cout, K), generator=gen), torch.randn((Cout, K), generator=gen) / 24
    mean, inv = torch.randn(Cout, generator=gen), torch.rand(Cout, generator=gen) + 0.5
    cs = torch.randn(Cout, generator=gen) * 30
    r = R.bn_fold_bwd_ref(Gw.double(), Wt.double(), mean.double(), inv.double(), cs.double())
    full = (inv.double() * ((Gw.double() * Wt.double()).sum(1) - mean.double() * cs.double())).float()
    short = (inv.double() * ((Gw[:, :256].double() * Wt[:, :256].double()).sum(1) - mean.double() * cs.double())).float()
    assert _worst(full, *r['dgamma']) < 0.5 and _worst(short, *r['dgamma']) > 1


# ---- the float32 index rules -----------------------------------------------------------------------------------------
def test_nearest_index_is_torchs_and_the_backward_window_holds_every_child():
    """All 1 <= U < 200, 1 <= H < 400: the forward index equals F.interpolate(mode='nearest'); every fine pixel lies inside
    the candidate window [y0, y1] of its parent (float32 division and truncating casts, as the kernel: IEEE division, which
    the build's flags give -- no fast-math)."""
    for U in range(1, 200):
        src = torch.arange(U, dtype=torch.float32).view(1, 1, U, 1)
        for H in range(1, 400):
            idx = R.nearest_index(H, U)
            want = F.interpolate(src, size=(H, 1), mode='nearest').view(-1).long().numpy()
            assert np.array_equal(idx, want), (U, H)
            s = np.float32(U) / np.float32(H)
            u = np.arange(U, dtype=np.float32)
            y0 = np.maximum(0, (u / s).astype(np.int64) - 1)
            y1 = np.minimum(H - 1, ((u + np.float32(1)) / s).astype(np.int64) + 1)
            y = np.arange(H)
            assert np.all((y0[idx] <= y) & (y <= y1[idx])), (U, H)
    assert R.bwd_window(3, 13, 25) == (4, 8)


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_entry_points_refuse_arguments_that_would_reach_a_bad_launch():
    """Every call returns CPR_ERR_ARG before any launch (no GPU needed; the buffers are host memory no kernel ever sees)."""
    L = _lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    ok = dict(N=1, HW=64, C=64, G=32, P=1)

    def gn_bwd(entry, **kw):
        a = dict(ok, **kw)
        ptrs = [p] * (12 if entry == 'cpr_gn_bwd' else 13)
        return getattr(L, entry)(*ptrs, a['N'], a['HW'], a['C'], a['G'], a['P'], 1, 0, None)

    for entry in ('cpr_gn_bwd', 'cpr_gn_bwd_bf16', 'cpr_gn_bwd_bf16_dz16'):
        for bad in (dict(G=0), dict(G=48), dict(G=128), dict(N=0), dict(P=0), dict(HW=0), dict(C=0, G=1), dict(C=-4, G=1),
                    dict(C=320, G=32), dict(C=2048, G=32), dict(C=6, G=2), dict(G=-1)):
            assert gn_bwd(entry, **bad) == ERR_ARG, (entry, bad)
    for entry in ('cpr_gn_stats', 'cpr_gn_stats_bf16'):
        for N, HW, C, P in ((1, 64, 0, 1), (1, 64, -4, 1), (1, 64, 320, 1), (0, 64, 64, 1), (1, 0, 64, 1), (1, 64, 64, 0)):
            assert getattr(L, entry)(p, p, N, HW, C, P, None) == ERR_ARG, (entry, N, HW, C, P)
    fin = lambda N, P, C, G, HW: L.cpr_gn_finalize(p, p, p, p, p, p, p, N, P, C, G, HW, ctypes.c_float(1e-5), None)
    for args in ((1, 1, 64, 0, 64), (1, 1, 64, 48, 64), (1, 0, 64, 32, 64), (1, 1, 0, 1, 64), (1, 1, 1024, 1, 64), (1, 1, 64, 32, 0)):
        assert fin(*args) == ERR_ARG, args
    for entry in ('cpr_gn_apply', 'cpr_gn_apply_bf16'):
        for N, H, W, C, UH, UW in ((1, 4, 4, 0, 2, 2), (1, 4, 4, 6, 2, 2), (1, 4, 4, 8, 0, 2), (1, 0, 4, 8, 2, 2), (0, 4, 4, 8, 2, 2)):
            assert getattr(L, entry)(p, p, p, p, p, N, H, W, C, UH, UW, 0, None) == ERR_ARG, (entry, N, H, W, C, UH, UW)
    assert L.cpr_gn_apply_b8(p, p, p, p + 64, 1, 4, 4, 0, 0, None) == ERR_ARG and L.cpr_gn_apply_b8(p, p, p, p + 64, 1, 4, 4, 12, 0, None) == ERR_ARG
    for N, H, W, UH, UW, C in ((1, 4, 4, 2, 2, 0), (1, 4, 4, 2, 2, -4), (1, 4, 4, 0, 2, 8), (1, 4, 4, 2, 2, 6), (0, 4, 4, 2, 2, 8)):
        assert L.cpr_upsample_add_bwd(p, p, N, H, W, UH, UW, C, 0, None) == ERR_ARG, (N, H, W, UH, UW, C)
    for N, OH, OW, C, H, W, s in ((1, 2, 2, 0, 4, 4, 2), (1, 2, 2, -4, 4, 4, 2), (1, 2, 2, 8, 4, 4, 0), (1, 2, 2, 8, 0, 4, 2)):
        assert L.cpr_zero_insert(p, p, N, OH, OW, C, H, W, s, None) == ERR_ARG, (N, OH, OW, C, H, W, s)
    for entry in ('cpr_maxpool3x3s2', 'cpr_maxpool3x3s2_bf16'):
        for N, H, W, C in ((1, 4, 4, 0), (1, 4, 4, 6), (1, 0, 4, 8), (0, 4, 4, 8)):
            assert getattr(L, entry)(p, p, N, H, W, C, None) == ERR_ARG, (entry, N, H, W, C)
    assert L.cpr_maxpool3x3s2_rec(p, p, None, 1, 4, 4, 8, None) == ERR_ARG
    for M, C in ((0, 8), (4, 0), (4, 6), (-1, 8)):
        assert L.cpr_relu_bwd_colsum(p, None, None, 0, p, None, p, p, ctypes.c_longlong(M), C, 0, None) == ERR_ARG, (M, C)
        assert L.cpr_relu_bwd_colsum_ws(ctypes.c_longlong(M), C) < 0 or C == 6
    assert L.cpr_part_colsum(p, p, p, 0, 8, None) == ERR_ARG and L.cpr_part_colsum(p, p, p, 4, 0, None) == ERR_ARG
    assert L.cpr_bn_fold_bwd(p, p, p, p, p, p, p, p, 0, 8, None) == ERR_ARG and L.cpr_bn_fold_bwd(p, p, p, p, p, p, p, p, 8, 0, None) == ERR_ARG
    assert L.cpr_bn_fold_bwd_part(p, p, p, p, p, p, 0, p, p, 8, 8, None) == ERR_ARG
    assert L.cpr_axpby(p, p, ctypes.c_float(1), ctypes.c_float(1), ctypes.c_longlong(-1), None) == ERR_ARG
    assert L.cpr_axpby(None, None, ctypes.c_float(1), ctypes.c_float(1), ctypes.c_longlong(0), None) == 0
    assert L.cpr_nchw_to_nhwc4(p, p, 1, 5, 4, 4, None) == ERR_ARG and L.cpr_nhwc_to_nchw(p, p, 1, 0, 4, 4, None) == ERR_ARG
    assert L.cpr_phase_scatter_add(p, p, 1, 2, 2, 6, 4, 4, 0, 0, 0, 0, 2, None) == ERR_ARG
    assert L.cpr_phase_scatter_add(p, p, 1, 2, 2, 8, 4, 4, 2, 0, 0, 0, 2, None) == ERR_ARG
