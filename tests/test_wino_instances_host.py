"""CPU checks that keep tests/test_gpu_wino_instances.py honest: the launch rules restated in tests/wino_fp64_ref.py are the ones in the
source text of csrc/conv_wino.hip and csrc/conv_wino32.hip, the walk covers every tile once, the table reaches every state the issue
lists at 256 CUs, every case that takes the direct bar is eligible for it, and the bars catch the faults they exist for (an fp32
emulation of the kernels passes them, the deliberately wrong ones below fail at the pixels they touch)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_fp64_ref as R
from tests import wino_fp64_ref as WR
from tests.test_gpu_wino_instances import CASES, auto_instance, case_id, coverage, flags, make_inputs, seed, takes_bar2

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r'\s+', ' ', f.read())


# ---- the restated rules against the source text ---------------------------------------------------------------------------------
def test_restated_constants_are_in_the_source_text():
    s64, s32 = _src('conv_wino.hip'), _src('conv_wino32.hip')
    rh, rw = WR.REGION['64']
    assert 't.oy0 = ry * %d; t.ox0 = rx * %d; t.n0 = t.tn * %d;' % (rh, rw, WR.COUT_TILE) in s64
    assert 'p.RY = (H + %d) / %d; p.RX = (W + %d) / %d;' % (rh - 1, rh, rw - 1, rw) in s64
    assert 'p.tilesN = Cout / %d; p.nch = Cin / %d;' % (WR.COUT_TILE, WR.CHUNK['64']) in s64
    assert 'constexpr int XFMAX = %d;' % WR.XFMAX['64'] in s64 and 'if (in_a) CPR_CHECK_ARG(in_b && Cin <= %d);' % WR.XFMAX['64'] in s64
    assert 'if (grid > ncu) grid = ncu;' in s64                                        # one workgroup per CU
    assert 'constexpr int WINO_VAR_DEFAULT = 4, WINO_TPX_DEFAULT = 0;' in s64           # tpx = 0: every XCD walks (region, cout tile) runs
    rh, rw = WR.REGION['32']
    assert 'const int oy0 = ry * %d, ox0 = rx * %d, n0 = tn * %d;' % (rh, rw, WR.COUT_TILE) in s32
    assert 'p.RY = (H + %d) / %d; p.RX = (W + %d) / %d;' % (rh - 1, rh, rw - 1, rw) in s32
    assert 'p.tilesN = Cout / %d; p.nch = Cin / %d;' % (WR.COUT_TILE, WR.CHUNK['32']) in s32
    assert 'constexpr int W32_XFMAX = %d;' % WR.XFMAX['32'] in s32 and 'if (in_a) CPR_CHECK_ARG(in_b && Cin <= W32_XFMAX);' in s32
    assert 'constexpr int w32_ablate = 0, w32_wg_per_cu = %d, w32_stagger_pct = 100;' % WR.WG_PER_CU['32'] in s32
    assert 'if (grid > w32_wg_per_cu * ncu) grid = w32_wg_per_cu * ncu;' in s32
    assert 'return H > 0 && W > 0 ? ((H + 7) / 8) * ((W + 15) / 16) : CPR_ERR_ARG;' in s32
    for s in (s64, s32):      # the walk
        assert 'const int per = (T + 7) >> 3;' in s and 'const int tile = (vb & 7) * per + (vb >> 3);' in s
        assert 'vb < per * 8 && tile < T' in s and 'vb += gridDim.x' in s
        assert 'ncu = (ncu + 7) / 8 * 8; int grid = (int)((T + 7) / 8 * 8);' in s
        assert 'const int rg = tile / p.tilesN, tn = tile - rg * p.tilesN;' in s or 't.rg = tl / p.tilesN; t.tn = tl - t.rg * p.tilesN;' in s
    # the pack layouts
    assert 'const int tn = co >> 6, cl = co & 63, chunk = ci >> 3, k = ci & 7, nch = Cin >> 3;' in s64
    assert 'u + ((size_t)(tn * nch + chunk) * 16) * 512 + cl * 8 + 4 * ((k >> 2) ^ ((cl >> 3) & 1)) + (k & 3);' in s64
    assert 'const int tn = co >> 6, cl = co & 63, chunk = ci >> 2, k = ci & 3, nch = Cin >> 2;' in s32
    assert 'u + ((size_t)(tn * nch + chunk) * 16) * 256 + cl * 4 + k;' in s32
    for s, stride in ((s64, 512), (s32, 256)):
        assert 'dst[(i * 4 + 1) * %d] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);' % stride in s


@pytest.mark.parametrize('kind', ['64', '32'])
@pytest.mark.parametrize('ncu', [256, 304])
def test_walk_covers_every_tile_exactly_once(kind, ncu):
    for T in range(1, 3000):
        tile, live, has = WR.run_tiles(T, kind, ncu)
        assert np.array_equal(live, has), (T, 'an id with a tile behind one without: the kernels\' loops would stop before it')
        assert np.array_equal(np.sort(tile[live]), np.arange(T)), T
        assert tile.shape[1] == min((T + 7) // 8 * 8, WR.WG_PER_CU[kind] * ncu) and tile.shape[1] % 8 == 0


def test_walk_names_region_image_and_cout_tile():
    runs = WR.walk(3, 17, 33, 192, '64', 256)
    seen = sorted(t for r in runs for t in r)
    assert [t[0] for t in seen] == list(range(54)) and sum(not r for r in runs) == 56 - 54
    assert all(t == (t[0], t[0] // 3, t[0] // 3 // 6, t[0] % 3) for t in seen)


@pytest.mark.parametrize('kind,Cin,Cout', [('64', 48, 192), ('32', 24, 128)])
def test_pack_layout_is_a_bijection(kind, Cin, Cout):
    idx = WR.u_layout(kind, Cin, Cout)
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(16 * Cin * Cout))


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_state_at_256_cus():
    missing = [n for n, ok in coverage(CASES, 256).items() if not ok]
    assert not missing, missing


def test_case_routes_follow_the_dispatch_rules():
    """entry cases are shapes the dispatcher never gives to the case's kernel; auto cases are shapes it gives to the case's kernel; the rest must be
    shapes ops.PackedConv packs and ops.wino_instance can force onto the case's kernel."""
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for c in CASES:
        f = flags(c)
        if 'entry' in f:
            assert auto_instance(c) != c.kernel, c
        elif 'auto' in f:
            assert auto_instance(c) == c.kernel, c
        else:
            assert c.Cin % 32 == 0 and c.Cout % 64 == 0 and (c.kernel == '64' or 'inab' not in f or c.Cin <= 256), c
        assert 'inab' in f or 'inrelu' not in f
        assert c.N * c.H * c.W * max(c.Cin, c.Cout) * 4 <= 41 << 20, c           # at most 40 MB a map


@pytest.mark.parametrize('c', [c for c in CASES if takes_bar2(c)], ids=case_id)
def test_case_is_eligible_for_the_direct_bar(c):
    f = flags(c)
    inp = make_inputs(c)
    m, _ = WR.sample(c.N, c.H, c.W, c.Cout, c.kernel, 256, n_random=100, seed=seed(c))
    if len(m) > 1500:       # eligibility is a property of the operands' statistics: a thinned sample shows it
        m = m[::len(m) // 1500]
    kw = dict(scale=inp['scale'], bias=inp['bias'], relu='relu' in f)
    r = WR.reference(inp['x'], inp['w'], m, **kw)
    y = WR.emulate(inp['x'], inp['w'], m, kind=c.kernel, **kw)
    q1, q2 = float(R.ratio(y, r['ref'], r['bar_wino']).max()), float(R.ratio(y, r['ref'], r['bar_direct']).max())
    print('\nEMULATION %s bar1 %.4f bar2 %.4f  %s' % (c.kernel, q1, q2, case_id(c)))
    assert q2 <= WR.EMU_SHARE, (q2, case_id(c))
    assert q1 <= 1.0


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_magnitude_equals_the_literal_per_pixel_loop():
    g = torch.Generator().manual_seed(9)
    N, H, W, Cin, Cout = 2, 5, 7, 8, 3
    x = torch.randn((N, H, W, Cin), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g)
    a, b = torch.rand((N, Cin), generator=g) + 0.5, torch.randn((N, Cin), generator=g)
    m = np.arange(N * H * W)
    got = WR.magnitude(x, w, m, in_ab=(a, b))
    aB, aG, aA = WR.BT.abs(), WR.GM.abs(), WR.AM.abs()
    want = torch.zeros((N * H * W, Cout), dtype=torch.float64)
    for n in range(N):
        for oy in range(H):
            for ox in range(W):
                y0, x0 = oy // 2 * 2 - 1, ox // 2 * 2 - 1
                acc = torch.zeros((4, 4, Cout), dtype=torch.float64)
                for c in range(Cin):
                    d = torch.zeros((4, 4), dtype=torch.float64)
                    for r in range(4):
                        for s in range(4):
                            if 0 <= y0 + r < H and 0 <= x0 + s < W:
                                d[r, s] = abs(float(x[n, y0 + r, x0 + s, c]) * float(a[n, c])) + abs(float(b[n, c]))
                    V = aB @ d @ aB.t()
                    for o in range(Cout):
                        acc[:, :, o] += (aG @ w[o, c].double().abs() @ aG.t()) * V
                for o in range(Cout):
                    want[(n * H + oy) * W + ox, o] = (aA.t() @ acc[:, :, o] @ aA)[oy & 1, ox & 1]
    assert torch.allclose(got, want, rtol=1e-12, atol=0)


def test_fp64_winograd_equals_the_direct_reference_and_the_magnitudes_order():
    """The helpers compute the convolution (so the emulation is one), and mag_wino >= the direct magnitude elementwise."""
    g = torch.Generator().manual_seed(10)
    x = torch.randn((2, 9, 13, 16), generator=g)
    w = torch.randn((5, 16, 3, 3), generator=g)
    ab = (torch.rand((2, 16), generator=g) + 0.5, torch.randn((2, 16), generator=g))
    m = np.arange(2 * 9 * 13)
    r = WR.reference(x, w, m, in_ab=ab, in_relu=True)
    y = WR.emulate(x, w, m, in_ab=ab, in_relu=True, dtype=torch.float64)
    xa = (x.double() * ab[0].double()[:, None, None] + ab[1].double()[:, None, None]).clamp_min(0)
    conv = F.conv2d(xa.permute(0, 3, 1, 2), w.double(), None, 1, 1).permute(0, 2, 3, 1).reshape(-1, 5)
    assert torch.allclose(r['ref'], conv, rtol=1e-12, atol=1e-12) and torch.allclose(y, conv, rtol=1e-11, atol=1e-11)
    assert bool((r['mag_wino'] >= r['mag_direct'] * (1 - 1e-12)).all())


def test_sample_takes_whole_regions_of_the_chosen_runs():
    N, H, W, Cout, kind = 5, 70, 90, 192, '64'
    m, rgs = WR.sample(N, H, W, Cout, kind, 256)
    s = set(m.tolist())
    RY, RX = WR.regions(H, W, kind)
    assert {0, RY * RX - 1, (N - 1) * RY * RX, N * RY * RX - 1} <= set(rgs) and set(WR.partial_regions(1, H, W, kind)) <= set(rgs)
    assert len(WR.partial_regions(1, H, W, kind)) == RY + RX - 1
    runs = WR.pick_runs(WR.walk(N, H, W, Cout, kind, 256))
    assert any(a[2] != b[2] for a, b in zip(runs[0], runs[0][1:])) and any(a[2] == b[2] for a, b in zip(runs[1], runs[1][1:]))
    for r in runs:
        assert {t[1] for t in r} <= set(rgs)
    for rg in rgs:
        px = WR.region_pixels(rg, N, H, W, kind)
        assert set(px.tolist()) <= s and 0 < len(px) <= 256
    assert len(WR.region_pixels(RY * RX - 1, N, H, W, kind)) == (H % 16) * (W % 16)
    small, rg_small = WR.sample(2, 19, 21, 64, '32', 256)
    assert len(small) == 2 * 19 * 21 and rg_small == list(range(2 * 3 * 2))


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
SN, SH, SW, SCIN, SCOUT, SKIND = 3, 21, 35, 32, 128, '64'      # 2 x 3 regions an image, partial bottom and right


def _problem():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((SN, SH, SW, SCIN), generator=g)
    w = torch.randn((SCOUT, SCIN, 3, 3), generator=g) / (9 * SCIN) ** 0.5
    ab = (torch.rand((SN, SCIN), generator=g) + 0.5, torch.randn((SN, SCIN), generator=g) * 0.5)
    bias = torch.randn(SCOUT, generator=g)
    return x, w, ab, bias


@pytest.fixture(scope='module')
def sens():
    """The problem, its reference on every pixel (computed once, left unchanged) and the clean emulation."""
    x, w, ab, bias = _problem()
    m = np.arange(SN * SH * SW)
    r = WR.reference(x, w, m, bias=bias, in_ab=ab, in_relu=True)
    y = WR.emulate(x, w, m, in_ab=ab, in_relu=True, kind=SKIND, bias=bias)
    return dict(x=x, w=w, ab=ab, bias=bias, m=m, r=r, y=y)


def _over(s, y):
    """Per pixel: some channel of y misses bar 1."""
    return (R.ratio(y, s['r']['ref'], s['r']['bar_wino']) > 1.0).any(1)


def _mutant(s, **mut):
    return WR.emulate(s['x'], s['w'], s['m'], in_ab=s['ab'], in_relu=True, kind=SKIND, bias=s['bias'], **mut)


def _pix(n, oy, ox):
    return (n * SH + oy) * SW + ox


def test_emulation_passes_both_bars():
    x, w, _, bias = _problem()
    m = np.arange(SN * SH * SW)
    r = WR.reference(x, w, m, bias=bias)
    for kind in ('64', '32'):
        y = WR.emulate(x, w, m, kind=kind, bias=bias)
        q1, q2 = float(R.ratio(y, r['ref'], r['bar_wino']).max()), float(R.ratio(y, r['ref'], r['bar_direct']).max())
        print('\nEMULATION %s worst error / bar 1 %.4f, / bar 2 %.4f' % (kind, q1, q2))
        assert q1 <= 1.0 and q2 <= WR.EMU_SHARE


def test_emulation_with_the_fused_affine_passes_bar_1(sens):
    q = float(R.ratio(sens['y'], sens['r']['ref'], sens['r']['bar_wino']).max())
    print('\nEMULATION fused affine worst error / bar 1 %.4f' % q)
    assert q <= 1.0 and not bool(_over(sens, sens['y']).any())


def test_bar_catches_one_dropped_chunk(sens):
    key, inv, _, _ = WR.tiles_of(sens['m'], SH, SW)
    hit = np.arange(len(key)) % 5 == 2                               # the tiles that lose channels 8 .. 15

    def drop(d, k):
        d = d.clone()
        d[torch.as_tensor(np.isin(k, key[hit])), :, :, 8:16] = 0
        return d
    over = _over(sens, _mutant(sens, d_hook=drop))
    touched = torch.as_tensor(hit[inv])
    assert bool(over[touched].all()) and not bool(over[~touched].any())


def test_bar_catches_the_previous_images_table_on_one_tile(sens):
    y = sens['y'].clone()
    wrong = _mutant(sens, table_shift=1)
    touched = torch.zeros(len(sens['m']), dtype=torch.bool)
    for oy in (16, 17):                                              # one Winograd tile of image 1, and one of image 0 (wraps to the last image)
        for ox in (32, 33):
            touched[_pix(1, oy, ox)] = True
            touched[_pix(0, oy - 10, ox - 20)] = True
    y[touched] = wrong[touched]
    over = _over(sens, y)
    assert bool(over[touched].all()) and not bool(over[~touched].any())


def test_bar_catches_relu_b_at_padding_and_outside_the_map(sens):
    over = _over(sens, _mutant(sens, pad_relu_b=True))
    oy, ox = np.divmod(sens['m'] % (SH * SW), SW)
    border = torch.as_tensor((oy == 0) | (oy == SH - 1) | (ox == 0) | (ox == SW - 1))
    assert SH % 2 == 1 and SW % 2 == 1                               # the last row and column sit in tiles that reach outside the map
    assert bool(over[border].all())
    assert not bool(over[~border].any())                             # an interior pixel's taps never read the fill


def test_bar_catches_the_neighbouring_cout_tiles_weights(sens):
    assert bool(_over(sens, _mutant(sens, u_hook=lambda U: torch.roll(U, 64, 2))).all())


def test_bar_catches_swapped_frequencies(sens):
    swap = (lambda U: U.view(4, 4, *U.shape[1:]).transpose(0, 1).reshape(U.shape))      # 4i + j <-> 4j + i
    assert bool(_over(sens, _mutant(sens, u_hook=swap)).all())


def test_bar_catches_a_missing_half_in_one_row_of_g(sens):
    gm = WR.GM.clone()
    gm[2] *= 2
    assert bool(_over(sens, _mutant(sens, gm=gm)).all())


def test_slot_bars_catch_an_outside_pixel_and_a_neighbours_index():
    x, w, _, bias = _problem()
    m = np.arange(SN * SH * SW)
    r = WR.reference(x, w, m, bias=bias)
    y = WR.emulate(x, w, m, kind=SKIND, bias=bias)
    RY, RX = WR.regions(SH, SW, SKIND)
    rgs = list(range(SN * RY * RX))
    sref, sbar = WR.slot_refs(r, m, rgs, SN, SH, SW, SKIND)
    got = WR.slot_sums(y, m, rgs, SN, SH, SW, SKIND).double()
    assert bool(((got - sref).abs() <= sbar).all())
    # what the kernel computes for the pixel right of the map's first row: its taps see the map's last column and zeros
    xw = F.pad(x, (0, 0, 0, 1))
    out = WR.emulate(xw, w, np.asarray([SW]), kind=SKIND, bias=bias).double()[0]
    for ry in range(RY):
        rg = ry * RX + RX - 1                                        # the partial regions at the right edge of image 0
        bad = got[rg] + torch.stack([out, out * out], -1)
        assert not bool(((bad - sref[rg]).abs() <= sbar[rg]).all())
    shifted = torch.roll(got, 1, 0)                                  # every slot stored at the next region's index
    for rg in rgs:
        assert not bool(((shifted[rg] - sref[rg]).abs() <= sbar[rg]).all())
