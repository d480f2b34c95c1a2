"""CPU checks that keep tests/test_gpu_stem_instances.py honest: the geometry restated in tests/stem_fp64_ref.py is the one in the source
text of csrc/stem_f32.hip, stem_bf16.hip, stem_deep.hip and stem_bwd.hip; the tables reach every state; every case meets the admission
rules from the fp64 reference alone (undecided byte-map share, clipped share, pooled zeros, a channel whose relu(bias) towers over the bar);
an fp32 emulation of the kernels stays below half of every bar; and the deliberately wrong emulations below fail at exactly the pixels they
touch."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import stem_fp64_ref as SR
from tests.test_gpu_stem_instances import (BWD_CASES, CONV16_CASES, DEEP_CASES, FUSED_CASES, bwd_image_hw, case_id,
                                           coverage, fused_inputs, seed)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
EMU_SHARE = 0.5


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r'\s+', ' ', f.read())


# ---- the restated geometry against the source text ----------------------------------------------------------------------------------
def test_restated_constants_are_in_the_source_text():
    f32, b16, deep, bwd = _src('stem_f32.hip'), _src('stem_bf16.hip'), _src('stem_deep.hip'), _src('stem_bwd.hip')
    TH, TW = SR.FUSED_TILE
    assert 'constexpr int SF_PH = %d, SF_PW = %d;' % SR.FUSED_PATCH in f32 and 'constexpr int SP_PH = %d, SP_PW = %d;' % SR.FUSED_PATCH in b16
    assert SR.FUSED_PATCH == (2 * (2 * TH) + 7, 2 * (2 * TW) + 7 + 1)      # 17 x 33 conv positions under a 7 x 7 / 2 window, + the zero column
    for s in (f32, b16):
        assert 'const int r0 = %d * ty - 1, c0 = %d * tx - 1;' % (2 * TH, 2 * TW) in s
        assert 'p.tilesY = (p.PH + %d) / %d;' % (TH - 1, TH) in s and 'p.tilesX = (p.PW + %d) / %d;' % (TW - 1, TW) in s
        assert 'const int gy = %d * ty + py, gx = %d * tx + px;' % (TH, TW) in s
        assert 'p.OH = (H - 1) / 2 + 1;' in s and 'p.OW = (W - 1) / 2 + 1;' in s
        assert 'p.PH = (p.OH - 1) / 2 + 1;' in s and 'p.PW = (p.OW - 1) / 2 + 1;' in s
        assert 'const int m16 = l31 < %d ? l31 : %d;' % (2 * TH, 2 * TH) in s                     # the halo column's rows: min(m, 16)
        assert 'const int row = q < %d ? q : m, col = q < %d ? m + 1 : 0;' % (2 * TH + 1, 2 * TH + 1) in s
        assert 'const bool ok = (unsigned)cr < (unsigned)p.OH && (unsigned)cc < (unsigned)p.OW;' in s
    assert 'const int q = qb + 4 * i;' in f32 and 'const bool five = qb < 2;' in f32            # waves own 4 or 5 blocks of 18
    assert 'const int nblk = wave < 2 ? 3 : 2;' in b16                                           # waves own 2 or 3 blocks of 18
    CR, CC = SR.CONV_TILE
    assert 'constexpr int ST_TY = %d, ST_TX = %d;' % (CR, CC) in b16 and 'constexpr int SDA_TR = %d, SDA_TC = %d;' % (CR, CC) in deep
    assert 'p.tilesY = (p.OH + ST_TY - 1) / ST_TY;' in b16 and 'p.tilesX = (p.OW + ST_TX - 1) / ST_TX;' in b16
    assert deep.count('a.tilesY = cdiv(OH, SDA_TR);') == 1 and deep.count('a.tilesY = cdiv(a.OH, SDA_TR);') == 1
    DH, DW = SR.DEEP_C_TILE
    assert 'static constexpr int TR = POOL ? %d : %d;' % (2 * DH + 1, CR) in deep
    assert 'static constexpr int PR = TR + 2, PC = POOL ? %d : %d;' % (2 * DW + 3, CC + 2) in deep
    assert 'static constexpr int NBLK = POOL ? %d : %d;' % (2 * DH + 2, CR) in deep
    assert 'static constexpr int PER_WAVE = POOL ? 3 : 2;' in deep
    assert 'const int r0 = POOL ? %d * ty - 1 : %d * ty, c0 = POOL ? %d * tx - 1 : %d * tx;' % (2 * DH, CR, 2 * DW, CC) in deep
    assert 'q.tilesY = cdiv(OH, %d); q.tilesX = cdiv(OW, %d);' % (CR, CC) in deep
    assert 'q.tilesY = cdiv(q.PH, %d); q.tilesX = cdiv(q.PW, %d);' % (DH, DW) in deep
    assert 'prow = l31 < %d ? l31 : %d; pcol = 0;' % (2 * DH, 2 * DH) in deep                    # the halo column's rows: min(m, 8)
    assert 'const int gy = %d * ty + py, gx = %d * tx + px;' % (DH, DW) in deep
    assert 'const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;' in deep
    assert 'q.PH = (OH - 1) / 2 + 1; q.PW = (OW - 1) / 2 + 1;' in deep
    assert 'constexpr int SPB_PIX = %d;' % SR.SLOT in bwd and 'part[((size_t)blockIdx.x * 64 + c) * 2 + 1] = 0.f;' in bwd
    assert 'const int PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1;' in bwd


def test_geometry_of_the_named_cases():
    g = SR.fused_geom(67, 131)
    assert (g['OH'], g['OW'], g['PH'], g['PW'], g['tilesY'], g['tilesX'], g['lastY'], g['lastX']) == (34, 66, 17, 33, 3, 3, 1, 1)
    g = SR.fused_geom(61, 69)
    assert (g['OH'], g['OW'], g['PW'], g['lastX']) == (31, 35, 18, 2)
    g = SR.fused_geom(33, 257)
    assert (g['PH'], g['PW'], g['tilesX']) == (9, 65, 5)
    g = SR.deep_geom(35, 131)
    assert (g['OH'], g['OW'], g['PH'], g['PW']) == (18, 66, 9, 33) and g['ab'] == dict(tilesY=2, tilesX=3, lastY=2, lastX=2)
    assert g['c'] == dict(tilesY=3, tilesX=3, lastY=1, lastX=1)
    s = SR.slots(2, 34, 66)
    assert len(s) == 5 and s[-1] == (4096, 392) and s[2][0] < 34 * 66 < s[2][0] + s[2][1]
    for c in BWD_CASES:
        H, W = bwd_image_hw(c)
        assert (SR.half(H), SR.half(W)) == (c.OH, c.OW)


def test_tables_reach_every_state():
    missing = [n for n, ok in coverage().items() if not ok]
    assert not missing, missing
    for table in (FUSED_CASES, CONV16_CASES, DEEP_CASES, BWD_CASES):
        assert len({case_id(c) for c in table}) == len(table)
    # a state that leaves the tables is reported
    assert not all(coverage(fused=[c for c in FUSED_CASES if (c.H, c.W) != (67, 131)]).values())
    assert not all(coverage(bwd=[c for c in BWD_CASES if c.OW != 2]).values())


# ---- references, computed once per case and left unchanged ------------------------------------------------------------------------
_CACHE = {}


def fused_ref(c):
    if c not in _CACHE:
        inp = fused_inputs(c)
        t, e = SR.conv_ref(inp['img'], inp['w'], 2, 3, inp['scale'], inp['bias'])
        _CACHE[c] = dict(inp=inp, t=t, e=e, pool=SR.pool_ref(t, e))
    return _CACHE[c]


def deep_ref(c):
    """The deep-stem chain in fp32 emulation, each launch judged like the GPU test judges it: against fp64 on the operands it read."""
    if c not in _CACHE:
        inp = SR.deep_inputs(c.N, c.H, c.W, seed(c))
        x, stages = inp['img'], []
        for w, (s, b), stride in zip(inp['w'], inp['folds'], (2, 1, 1)):
            t, e = SR.conv_ref(x, w, stride, 1, s, b)
            y = SR.conv_emulate(x, w, stride, 1, s, b)
            stages.append(dict(x=x, w=w, s=s, b=b, stride=stride, t=t, e=e, y=y))
            x = y
        _CACHE[c] = dict(inp=inp, stages=stages, pool=SR.pool_ref(stages[2]['t'], stages[2]['e']))
    return _CACHE[c]


def _admit(name, t, e, bias, full_recipe):
    d = SR.decide(t, e)
    clipped = float((t <= 0).double().mean())
    zeros = float((SR.pool_ref(t, e)[0] == 0).double().mean())
    tower = float((bias.double().clamp_min(0) / e.amax((0, 2, 3))).max()) if bias is not None else 0.0
    print('\nADMIT %s undecided %.2e clipped %.3f pooled zeros %.4f relu(bias) / bar %.3g' % (name, d['undecided'], clipped, zeros, tower))
    assert d['undecided'] <= SR.UNDECIDED_MAX, name
    if full_recipe:
        assert 0.3 <= clipped <= 0.7 and zeros >= 0.01 and tower > 100.0, name


@pytest.mark.parametrize('c', FUSED_CASES, ids=case_id)
def test_fused_case_meets_the_admission_rules(c):
    r = fused_ref(c)
    _admit(case_id(c), r['t'], r['e'], r['inp']['bias'], c.combo == '')


@pytest.mark.parametrize('c', DEEP_CASES, ids=case_id)
def test_deep_case_meets_the_admission_rules(c):
    """On launch C of the fp64 chain (the kernel's own mid2 differs from it by rounding only)."""
    inp = SR.deep_inputs(c.N, c.H, c.W, seed(c))
    x = inp['img'].double()
    for w, (s, b), stride in zip(inp['w'][:2], inp['folds'][:2], (2, 1)):
        x = SR.conv_ref(x, w, stride, 1, s, b)[0].clamp_min(0)
    t, e = SR.conv_ref(x, inp['w'][2], 1, 1, *inp['folds'][2])
    _admit(case_id(c), t, e, inp['folds'][2][1], True)


# ---- the fp32 emulation stays below half of every bar -------------------------------------------------------------------------------
@pytest.mark.parametrize('c', FUSED_CASES, ids=case_id)
def test_fused_emulation_share_of_the_bars(c):
    r = fused_ref(c)
    inp = r['inp']
    z = SR.conv_emulate(inp['img'], inp['w'], 2, 3, inp['scale'], inp['bias'])
    out = SR.pool_tiles(z, SR.FUSED_TILE)
    assert torch.equal(out, F.max_pool2d(z, 3, 2, 1))                       # the tile walk is the pool
    q = float(SR.ratio(out.double(), *r['pool']).max())
    mx, am = SR.pool_exact(z.double())
    und = SR.check_argmap(case_id(c), mx, am, r['t'], r['e'])
    print('\nEMULATION fused %s worst |err| / bar %.4f, undecided %.2e' % (case_id(c), q, und))
    assert q <= EMU_SHARE and torch.equal(mx, out.double())


@pytest.mark.parametrize('c', CONV16_CASES, ids=case_id)
def test_bf16_conv_emulation_share_of_the_bars(c):
    from pointtinybenchmark_amd import ops
    inp = fused_inputs(c)
    x16, w16 = SR.bf16_operands(inp['img'], ops.stem_weight_bf16(inp['w']))
    assert torch.equal(w16, inp['w'].to(torch.bfloat16).float())
    t, e = SR.conv_ref(x16, w16, 2, 3, inp['scale'], inp['bias'])
    ref = t.clamp_min(0) if c.relu else t
    y = SR.conv_emulate(x16, w16, 2, 3, inp['scale'], inp['bias'], relu=bool(c.relu))
    q32 = float(SR.ratio(y.double(), ref, e).max())
    q16 = float(SR.ratio(y.to(torch.bfloat16).double(), ref, e + SR.bf16_half_ulp(ref)).max())
    print('\nEMULATION bf16 conv %s fp32 value / fp32 term %.4f, stored / bar %.4f' % (case_id(c), q32, q16))
    assert q32 <= EMU_SHARE and q16 <= 1.0
    trunc = (y.view(torch.int32) & -65536).view(torch.float32)             # a truncating store misses the half-spacing bar
    assert c.H * c.W < 64 or float(SR.ratio(trunc.double(), ref, e + SR.bf16_half_ulp(ref)).max()) > 1.0


@pytest.mark.parametrize('c', DEEP_CASES, ids=case_id)
def test_deep_emulation_share_of_the_bars(c):
    r = deep_ref(c)
    qs = [float(SR.ratio(st['y'].double(), st['t'].clamp_min(0), st['e']).max()) for st in r['stages']]
    out = SR.pool_tiles(r['stages'][2]['y'], SR.DEEP_C_TILE)
    assert torch.equal(out, F.max_pool2d(r['stages'][2]['y'], 3, 2, 1))
    qp = float(SR.ratio(out.double(), *r['pool']).max())
    print('\nEMULATION deep %s worst |err| / bar A %.4f B %.4f C conv %.4f C pooled %.4f' % (case_id(c), qs[0], qs[1], qs[2], qp))
    assert max(qs + [qp]) <= EMU_SHARE


# ---- sensitivity: the wrong emulations fail at exactly the pixels they touch ----------------------------------------------------------
SENS7, SENSD = FUSED_CASES[0], DEEP_CASES[0]


def _pooled_problem(kind):
    """(ReLU output z fp32, pooled tile, relu(bias) per channel, (ref, bar) of the pooled map)."""
    if kind == '7x7':
        r = fused_ref(SENS7)
        inp = r['inp']
        return SR.conv_emulate(inp['img'], inp['w'], 2, 3, inp['scale'], inp['bias']), SR.FUSED_TILE, inp['bias'].clamp_min(0), r['pool']
    r = deep_ref(SENSD)
    return r['stages'][2]['y'], SR.DEEP_C_TILE, r['stages'][2]['b'].clamp_min(0), r['pool']


def _judge(mut, clean, ref, bar, region):
    """The mutant misses the bar at exactly the pixels it changed, all of them inside ``region`` (N or 1, H, W) bool; the clean one passes."""
    assert not bool(SR.over_pixels(clean.double(), ref, bar).any())
    changed = (mut != clean).any(1)
    over = SR.over_pixels(mut.double(), ref, bar)
    assert bool(changed.any()) and torch.equal(over, changed), (int(changed.sum()), int(over.sum()))
    assert not bool((changed & ~region).any())
    return float(changed.double().sum() / region.expand_as(changed).double().sum())


def _grid(PH, PW):
    return torch.arange(PH).view(1, -1, 1), torch.arange(PW).view(1, 1, -1)


@pytest.mark.parametrize('kind', ['7x7', 'deep C'])
def test_bars_catch_relu_bias_at_an_out_of_map_conv_position(kind):
    z, tile, rb, (ref, bar) = _pooled_problem(kind)
    OH, OW = z.shape[2:]
    gy, gx = _grid(*ref.shape[2:])
    region = (gy == 0) | (gx == 0) | ((gy == ref.shape[2] - 1) & (OH % 2 == 1)) | ((gx == ref.shape[3] - 1) & (OW % 2 == 1))
    clean = SR.pool_tiles(z, tile)
    mut = SR.pool_tiles(z, tile, lambda ct, ok, ty, tx: torch.where(ok, ct, rb.view(1, -1, 1, 1).expand_as(ct)))
    share = _judge(mut, clean, ref, bar, region)
    print('\nMUTANT %s relu(bias) outside the map: %.2f of the border pixels change' % (kind, share))
    assert share > 0.25


@pytest.mark.parametrize('kind', ['7x7', 'deep C'])
def test_bars_catch_a_halo_column_one_row_short(kind):
    """min(m, 16) -> min(m, 15) (7x7), min(m, 8) -> min(m, 7) (launch C): the halo column's last row repeats the row above it."""
    z, tile, _, (ref, bar) = _pooled_problem(kind)
    TH, TW = tile
    gy, gx = _grid(*ref.shape[2:])
    region = (gy % TH == TH - 1) & (gx % TW == 0) & (gx > 0) & (2 * gy + 1 < z.shape[2])

    def short(ct, ok, ty, tx):
        ct[:, :, 2 * TH, 0] = ct[:, :, 2 * TH - 1, 0] * ok[2 * TH, 0]
        return ct
    clean = SR.pool_tiles(z, tile)
    share = _judge(SR.pool_tiles(z, tile, short), clean, ref, bar, region)
    print('\nMUTANT %s halo column one row short: %.2f of the corner pixels change' % (kind, share))
    assert share > 0.5


@pytest.mark.parametrize('kind', ['7x7', 'deep C'])
def test_bars_catch_a_zeroed_halo_column(kind):
    z, tile, _, (ref, bar) = _pooled_problem(kind)
    gy, gx = _grid(*ref.shape[2:])
    region = (gx % tile[1] == 0) & (gx > 0) & (gy >= 0)

    def zeroed(ct, ok, ty, tx):
        if tx > 0:
            ct[:, :, :, 0] = 0
        return ct
    share = _judge(SR.pool_tiles(z, tile, zeroed), SR.pool_tiles(z, tile), ref, bar, region)
    print('\nMUTANT %s halo column of tiles tx > 0 zeroed: %.2f of the first-column pixels change' % (kind, share))
    assert share == 1.0


def test_bars_catch_one_dropped_tap_at_the_last_column_of_a_b_tile():
    st = deep_ref(SENSD)['stages'][1]
    w = st['w'].clone()
    w[:, :, 1, 2] = 0                                                  # the 32 channels of tap (kh 1, kw 2): the patch column past the tile
    wrong = SR.conv_emulate(st['x'], w, 1, 1, st['s'], st['b'])
    OW = st['y'].shape[3]
    ox = torch.arange(OW).view(1, 1, -1)
    region = (ox % SR.CONV_TILE[1] == SR.CONV_TILE[1] - 1) & (ox + 1 < OW)
    assert int(region.sum()) == 2
    mut = torch.where(region.unsqueeze(1), wrong, st['y'])
    share = _judge(mut, st['y'], st['t'].clamp_min(0), st['e'], region)
    assert share == 1.0


def _bf16_map():
    inp = fused_ref(SENS7)['inp']
    x16, w16 = inp['img'].to(torch.bfloat16).float(), inp['w'].to(torch.bfloat16).float()
    return SR.conv_emulate(x16, w16, 2, 3, inp['scale'], inp['bias']).to(torch.bfloat16).double()


def test_exact_byte_map_catches_the_second_of_two_tied_positions():
    z = _bf16_map()
    mx, first = SR.pool_exact(z)
    mx2, last = SR.pool_exact_last_of_ties(z)
    w9 = SR.windows(z, -1.0)
    tied = ((w9 == mx.unsqueeze(2)).sum(2) > 1) & (mx > 0)
    assert torch.equal(mx, mx2) and int(tied.sum()) > 100                 # ties are common on the bf16 grid
    assert torch.equal(first != last, tied)                               # the wrong rule differs at exactly the tied windows
    # torch's own pool picks the first of ties too
    _, idx = F.max_pool2d(z, 3, 2, 1, return_indices=True)
    OW = z.shape[3]
    gy, gx = _grid(*mx.shape[2:])
    pos = (idx // OW - (2 * gy - 1)) * 3 + (idx % OW - (2 * gx - 1))
    assert torch.equal(torch.where(mx > 0, pos, torch.full_like(pos, 255)), first)


def test_byte_map_rules_catch_255_over_a_positive_maximum_and_a_wrong_position():
    r = fused_ref(SENS7)
    inp = r['inp']
    z = SR.conv_emulate(inp['img'], inp['w'], 2, 3, inp['scale'], inp['bias']).double()
    mx, am = SR.pool_exact(z)
    bad, d = SR.argmap_violations(mx, am, r['t'], r['e'])
    assert not bool(bad.any())
    hit = torch.zeros_like(bad)
    hit[:, ::7, ::3, ::5] = True
    hit &= mx > 0
    assert int(hit.sum()) > 100
    bad, _ = SR.argmap_violations(mx, torch.where(hit, torch.full_like(am, 255), am), r['t'], r['e'])
    assert torch.equal(bad, hit)
    # a neighbouring position: refused wherever the reference decides the element (all but the undecided share)
    moved = torch.where(hit, (am + 1) % 9, am)
    bad, _ = SR.argmap_violations(mx, moved, r['t'], r['e'])
    assert not bool((bad & ~hit).any()) and torch.equal(bad & d['must_pos'], hit & d['must_pos']) and float(bad[hit].double().mean()) > 0.999
    # a pooled zero over a positive window, byte 255: refused
    zeroed = torch.where(hit, torch.zeros_like(mx), mx)
    bad, _ = SR.argmap_violations(zeroed, torch.where(hit, torch.full_like(am, 255), am), r['t'], r['e'])
    assert torch.equal(bad, hit)


def test_slot_bars_catch_an_uncounted_pixel_and_a_neighbours_index():
    c = BWD_CASES[0]
    g = torch.Generator().manual_seed(seed(c))
    dy = torch.randn((c.N, c.OH, c.OW, 64), generator=g) * (torch.rand((c.N, c.OH, c.OW, 64), generator=g) < 0.3)       # mostly exact zeros
    ref, bar = SR.slot_refs(dy)
    got = SR.slot_sums32(dy)
    q = float(SR.ratio(got.double(), ref, bar).max())
    print('\nEMULATION slots worst |err| / bar %.4f' % q)
    assert q <= EMU_SHARE and ref.shape == (5, 64)
    flat = dy.reshape(-1, 64)
    for s, (first, n) in enumerate(SR.slots(c.N, c.OH, c.OW)):
        px = first + n - 1                                               # the slot's last pixel left out
        miss = got[s] - flat[px]
        over = (miss.double() - ref[s]).abs() > bar[s]                   # the bar is about 0.015 here, a gradient about 1
        assert not bool(over[flat[px] == 0].any()) and bool(over[flat[px].abs() > 2 * bar[s]].all()) and int(over.sum()) >= 10
    shifted = torch.roll(got, 1, 0)
    assert bool(((shifted.double() - ref).abs() > bar).any(1).all())


def test_pool_tiles_hook_sees_the_kernels_tile():
    """A tile holds conv rows 16 ty - 1 .. 16 ty + 15 and columns 32 tx - 1 .. 32 tx + 31, zeros outside the map."""
    z = torch.arange(2 * 1 * 34 * 66, dtype=torch.float32).view(2, 1, 34, 66) + 1
    seen = {}

    def look(ct, ok, ty, tx):
        seen[(ty, tx)] = (ct.clone(), ok.clone())
        return ct
    SR.pool_tiles(z, SR.FUSED_TILE, look)
    assert sorted(seen) == [(ty, tx) for ty in range(3) for tx in range(3)]
    ct, ok = seen[(1, 1)]
    assert ct.shape == (2, 1, 17, 33) and bool(ok.all()) and torch.equal(ct, z[:, :, 15:32, 31:64])
    ct, ok = seen[(0, 0)]
    assert not bool(ok[0].any()) and not bool(ok[:, 0].any()) and not bool(ct[:, :, 0].any()) and torch.equal(ct[:, :, 1:, 1:], z[:, :, :16, :32])
    ct, ok = seen[(2, 2)]
    assert int(ok.sum()) == 3 * 3 and torch.equal(ct[:, :, :3, :3], z[:, :, 31:, 63:]) and not bool(ct[:, :, 3:].any())
