"""CPU checks that keep tests/test_gpu_wgrad_instances.py honest: the restated split rules reproduce the library's workspace queries
(for every case and for seeded random shapes), the table covers the loop states and edges it exists for (each a condition asserted
below), and the bars of tests/wgrad_fp64_ref.py catch the faults they exist for (correct fp32 / bf16 / Winograd computations pass,
the deliberately wrong ones fail)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_fp64_ref as R
from tests import test_gpu_wgrad_instances as T
from tests.test_gpu_backward import GRAD_CASES
from tests.test_gpu_bf16 import WGRAD_BF16_CASES, WGRAD_TN_CASES
from tests.test_gpu_wgrad_instances import ALL_CASES, out_hw

DIRECT = [c for c in ALL_CASES if c['kind'] == 'direct']
WINO = [c for c in ALL_CASES if c['kind'] == 'wino']
NT = [c for c in ALL_CASES if c['kind'] == 'nt']
TN = [c for c in ALL_CASES if c['kind'] == 'tn']
STEM = [c for c in ALL_CASES if c['kind'] == 'stem']


def _lib():
    from pointtinybenchmark_amd import _lib
    return _lib.load()


def _xf(c):
    return 'xf' in c['flags'].split()


# ---- the table itself -------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_flags_known():
    ids = [T.case_id(c) for c in ALL_CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for c in ALL_CASES:
        assert set(c['flags'].split()) <= {'xf', 'relu', 'acc', 'ops'}, c
        assert 'relu' not in c['flags'].split() or _xf(c), c
        assert not _xf(c) or c['kind'] in ('direct', 'wino'), c
        assert not (c['kind'] == 'stem' and 'acc' in c['flags'].split()), 'the stem entry point has no accumulate flag'
        if c['kind'] == 'nt':
            assert (c['dy_dt'], c['x_dt']) != ('bf16', 'bf16'), 'two bf16 maps go to the pixel-major kernel'


def test_every_older_shape_is_in_the_table():
    def has(kind, **kw):
        return any(c['kind'] == kind and all(c[k] == v for k, v in kw.items()) for c in ALL_CASES)
    for N, Cin, H, W, Cout, k, s, p in GRAD_CASES:
        assert has('direct', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, p=p), (N, Cin, H, W, Cout, k, s, p)
    for N, H, W, Cin, Cout, k, xdt in WGRAD_BF16_CASES:
        assert has('nt', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, dy_dt='f32', x_dt=xdt)
    for N, H, W, Cin, Cout, k, s in WGRAD_TN_CASES:
        assert has('tn', N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s)
    for N, H, W, Cin, Cout, xf in T.WINO_OLD:
        assert has('wino', N=N, H=H, W=W, Cin=Cin, Cout=Cout, flags='xf relu' if xf else '')
    for N, H, W in T.STEM_OLD:
        assert has('stem', N=N, H=H, W=W, layout=0) and has('stem', N=N, H=H, W=W, layout=1)


def test_each_kernel_accumulates_once_and_goes_through_ops_once():
    for kind in ('direct', 'wino', 'nt', 'tn', 'stem'):
        cs = [c for c in ALL_CASES if c['kind'] == kind]
        assert any('ops' in c['flags'].split() for c in cs), kind
        assert kind == 'stem' or any('acc' in c['flags'].split() for c in cs), kind
    for c in ALL_CASES:                       # the route an 'ops' case expects is the route the restated rule gives
        if 'ops' in c['flags'].split() and c['kind'] in ('direct', 'wino'):
            assert T.wino_route(c) == (c['kind'] == 'wino'), c
    assert any(_xf(c) and 'ops' in c['flags'].split() for c in DIRECT)


def test_cases_stay_below_the_chunking_threshold():
    """Chunked launches (>= 2 GiB per map) belong to test_gpu_fullsize_grads.py; these launches are single."""
    for c in ALL_CASES:
        OH, OW = out_hw(c)
        e_dy = 2 if c.get('dy_dt') == 'bf16' else 4
        e_x = 2 if c.get('x_dt') == 'bf16' else 4
        cin = 4 if c['kind'] == 'stem' else c['Cin']
        assert max(c['N'] * c['H'] * c['W'] * cin * e_x, c['N'] * OH * OW * c['Cout'] * e_dy) < (1 << 30), c
        pl = T.plan(c)
        ws = pl['bytes'] if c['kind'] in ('nt', 'tn') else pl['ws'] * 4
        assert 0 < ws < (1 << 30), (c, ws)
        if c['kind'] == 'wino':
            assert c['N'] * c['H'] * c['W'] <= 100000, c      # wgrad_fp64_ref: where a dropped pixel still shows under the Winograd bar


# ---- restatement pinned to the library --------------------------------------------------------------------------------------
def test_restated_plans_reproduce_the_workspace_queries_of_every_case():
    L = _lib()
    for c in ALL_CASES:
        N, H, W, Cin, Cout, k, s = (c[n] for n in ('N', 'H', 'W', 'Cin', 'Cout', 'k', 's'))
        OH, OW = out_hw(c)
        pl = T.plan(c)
        if c['kind'] == 'direct':
            assert L.cpr_conv2d_wgrad_workspace(N, OH, OW, Cin, Cout, k, k) == pl['ws'] == pl['S'] * Cout * k * k * Cin, c
        elif c['kind'] == 'wino':
            assert L.cpr_conv3x3_wino_wgrad_workspace(N, H, W, Cin, Cout) == pl['ws'] == pl['slices'] * 16 * Cin * Cout, c
        elif c['kind'] == 'stem':
            assert L.cpr_stem_wgrad_f32_workspace(N, H, W) == pl['ws'], c
        else:
            d16, x16 = int(c['dy_dt'] == 'bf16'), int(c['x_dt'] == 'bf16')
            got = L.cpr_conv_wgrad_bf16_workspace_s(N, H, W, Cin, Cout, k, s, d16, x16)
            assert got == T.bf16_units(N, H, W, Cin, Cout, k, s, d16, x16) > 0, c
            assert pl['nt_ok'] if c['kind'] == 'nt' else pl['tn_ok'], c


def test_the_issue_example_of_the_direct_query():
    assert _lib().cpr_conv2d_wgrad_workspace(2, 16, 16, 256, 256, 3, 3) == 16 * 256 * 9 * 256
    assert T.wgrad_split(2 * 16 * 16, 256, 256, 9) == 16


def test_restated_direct_split_on_random_shapes():
    L = _lib()
    rng = np.random.default_rng(11)
    for _ in range(400):
        N, OH, OW = int(rng.integers(1, 48)), int(rng.integers(1, 96)), int(rng.integers(1, 96))
        Cin, Cout = 4 * int(rng.integers(1, 300)), 4 * int(rng.integers(1, 300))
        k = int(rng.choice([1, 1, 3, 3, 7]))
        S = T.wgrad_split(N * OH * OW, Cout, Cin, k * k)
        n = S * Cout * k * k * Cin
        assert S % 8 == 0 and 8 <= S <= 256
        assert L.cpr_conv2d_wgrad_workspace(N, OH, OW, Cin, Cout, k, k) == (n if n < (1 << 31) else T.ERR_UNSUPPORTED), \
            (N, OH, OW, Cin, Cout, k)


def test_restated_wino_split_on_random_shapes():
    L = _lib()
    rng = np.random.default_rng(12)
    for _ in range(300):
        N, H, W = int(rng.integers(1, 40)), int(rng.integers(1, 200)), int(rng.integers(1, 200))
        Cin, Cout = (int(rng.choice([64, 128, 192, 256, 512, 1024, 96, 32])) for _ in range(2))
        assert L.cpr_conv3x3_wino_wgrad_workspace(N, H, W, Cin, Cout) == T.wino_plan(N, H, W, Cin, Cout)['ws'], (N, H, W, Cin, Cout)


def test_restated_bf16_plan_on_random_shapes():
    """Including where the query answers unsupported, for every dtype pair."""
    L = _lib()
    rng = np.random.default_rng(13)
    seen = set()
    for i in range(400):
        N, H, W = int(rng.integers(1, 70)), int(rng.integers(1, 170)), int(rng.integers(1, 170))
        if i % 8 == 0:
            N, H, W = int(rng.integers(16, 64)), int(rng.integers(300, 900)), int(rng.integers(300, 900))     # beyond the index ranges
        Cin, Cout = (int(rng.choice([64, 128, 192, 256, 320, 512, 1024, 2048, 96, 32])) for _ in range(2))
        k, s = int(rng.choice([1, 3, 3, 2])), int(rng.choice([1, 1, 2, 3]))
        for d16, x16 in ((0, 0), (1, 1), (0, 1), (1, 0)):
            want = T.bf16_units(N, H, W, Cin, Cout, k, s, d16, x16)
            assert L.cpr_conv_wgrad_bf16_workspace_s(N, H, W, Cin, Cout, k, s, d16, x16) == want, (N, H, W, Cin, Cout, k, s, d16, x16)
            seen.add((want > 0, d16 and x16))
    assert seen == {(True, 0), (True, 1), (False, 0), (False, 1)}


def test_restated_stem_shape_on_random_shapes():
    L = _lib()
    rng = np.random.default_rng(14)
    for _ in range(300):
        N, H, W = int(rng.integers(1, 20)), int(rng.integers(1, 900)), int(rng.integers(1, 900))
        assert L.cpr_stem_wgrad_f32_workspace(N, H, W) == T.stem_plan(N, H, W)['ws'], (N, H, W)
    assert L.cpr_stem_wgrad_f32_workspace(0, 8, 8) == T.ERR_ARG


# ---- coverage conditions ----------------------------------------------------------------------------------------------------
def _boundary_chunks(c, pl):
    """Chunk index inside its slab, and that slab's chunk count, of every chunk an image boundary falls INSIDE."""
    OH, OW = out_hw(c)
    out = []
    for n in range(1, c['N']):
        m = n * OH * OW
        if m % 32:
            chunk = m // 32
            slab = chunk // pl['cps']
            out.append((chunk % pl['cps'], min(pl['cps'], pl['chunks'] - slab * pl['cps'])))
    return out


@pytest.mark.parametrize('xf', [False, True])
@pytest.mark.parametrize('geo', [2, 1, 0, -1])
def test_direct_instance_runs_its_steady_state_loop(xf, geo):
    """Per <XF, GEO> instance of conv_wgrad_kernel.  Loads issued inside WG_CHUNK are for chunk c + 3 (c + 2 with XF): chunks per
    slab >= 5 consumes them in both halves of the pair-unrolled loop and in its tail."""
    cs = [(c, T.direct_plan(c)) for c in DIRECT if _xf(c) == xf]
    cs = [(c, pl) for c, pl in cs if pl['geo'] == geo]
    assert cs, 'no case for this instance'
    assert any(pl['cps'] >= 5 for c, pl in cs)
    assert any(pl['cps'] >= 5 and pl['last'] < pl['cps'] for c, pl in cs), 'a last slab shorter than the others, behind a long one'
    assert any(pl['cps'] >= 3 and pl['M'] % 32 for c, pl in cs), 'a ragged last chunk'
    assert any(pl['cps'] >= 3 and pl['used'] < pl['S'] for c, pl in cs), 'an empty slab'
    first_loop_chunk = 2 if xf else 3
    found = issue = False
    for c, pl in cs:
        OH, OW = out_hw(c)
        if (OH * OW) % 32 and c['N'] >= 3:
            bc = _boundary_chunks(c, pl)
            issue |= any(n >= 3 for _, n in bc)
            found |= any(i >= first_loop_chunk and n > i for i, n in bc)
    assert issue, 'an image boundary inside a chunk of a slab of >= 3 chunks'
    assert found, 'an image boundary inside a chunk whose loads are issued by the loop'
    if geo == -1:
        assert all(out_hw(c)[0] * out_hw(c)[1] < 32 for c, _ in cs)


def test_direct_plain_instances_cover_the_pair_unrolled_loop():
    cps = {T.direct_plan(c)['cps'] for c in DIRECT if not _xf(c)}
    assert 3 in cps and 4 in cps
    assert any(v >= 5 and v % 2 for v in cps) and any(v >= 5 and v % 2 == 0 for v in cps), sorted(cps)
    assert {1, 2} <= cps         # the older shapes: prologue only


def test_direct_table_covers_the_edges():
    pls = [(c, T.direct_plan(c)) for c in DIRECT]
    couts, cins = {c['Cout'] for c in DIRECT}, {c['Cin'] for c in DIRECT}
    assert 4 in couts and any(v % 128 and v > 128 and (v - 128) % 4 == 0 and v - 128 < 32 for v in couts), sorted(couts)   # 132
    assert any(v % 128 and v > 128 for v in cins), sorted(cins)
    ows = {out_hw(c)[1] for c in DIRECT}
    assert 1 in ows and 32 in ows and any(v < 32 and v > 1 for v in ows) and any(v > 32 for v in ows)
    ohws = {out_hw(c)[0] * out_hw(c)[1] for c in DIRECT}
    assert {31, 32, 33} <= ohws
    for c, pl in pls:
        OH, OW = out_hw(c)
        assert (pl['geo'] == -1) == (OH * OW < 32), c
    assert any(c['s'] == 2 and c['H'] % 2 and c['W'] % 2 and (c['H'] + 2 * c['p'] - c['k']) % 2 == 0 and pl['geo'] == 0 and pl['cps'] >= 5
               for c, pl in pls), 'stride 2 on odd H and odd W'
    assert any(c['s'] == 1 and c['p'] == 0 and c['k'] == 3 and pl['geo'] == 0 for c, pl in pls), 'stride-1 unpadded 3x3'
    assert any(_xf(c) and pl['geo'] == 2 and c['Cout'] in (4, 8) for c, pl in pls)          # the heads' output convs
    assert any(_xf(c) and c['k'] == 3 and c['Cout'] in (4, 8) for c, pl in pls)            # 3x3 with a padded handful of couts
    assert any(_xf(c) and 'relu' not in c['flags'].split() for c in DIRECT) and any('relu' in c['flags'].split() for c in DIRECT)


def test_tn_table_covers_the_loop_and_the_reduce_kernel():
    pls = [(c, T.plan(c)) for c in TN]
    assert all(pl['tn_ok'] for _, pl in pls)
    ch = {pl['tn_chunks'] for _, pl in pls}
    assert any(v >= 3 and v % 2 for v in ch) and any(v >= 3 and v % 2 == 0 for v in ch), sorted(ch)
    sp = {pl['tn_splits'] for _, pl in pls}
    assert 8 in sp and 16 in sp and any(v > 16 and v % 16 == 8 for v in sp) and any(v >= 48 for v in sp), sorted(sp)
    assert any(pl['tn_used'] < pl['tn_splits'] and pl['tn_chunks'] >= 3 for _, pl in pls), 'empty splits'
    assert any(pl['P'] % 64 for _, pl in pls)
    ows = {out_hw(c)[1] for c in TN}
    assert any(v < 64 for v in ows) and any(v > 64 for v in ows)
    assert any(out_hw(c)[0] * out_hw(c)[1] < 64 and c['N'] >= 3 and pl['tn_chunks'] >= 3 for c, pl in pls), 'a chunk spans several images'
    assert any(c['s'] == 2 and c['H'] % 2 and c['W'] % 2 and pl['tn_chunks'] >= 3 for c, pl in pls), 'stride 2 on odd maps'
    assert {128, 192} <= {c['Cin'] for c in TN}
    assert any(c['Cout'] % 256 for c in TN)
    assert {1, 3} <= {c['k'] for c in TN}


def test_nt_table_covers_the_dtype_pairs_and_the_reduce_kernel():
    pls = [(c, T.plan(c)) for c in NT]
    assert all(pl['nt_ok'] for _, pl in pls)
    for k in (1, 3):
        pairs = {(c['dy_dt'], c['x_dt']) for c in NT if c['k'] == k}
        assert pairs == {('f32', 'f32'), ('f32', 'bf16'), ('bf16', 'f32')}, (k, pairs)
    assert any((c['W'] + 2 * c['p']) % 8 for c in NT)
    assert any(pl['splits'] >= 16 for _, pl in pls) and any(pl['splits'] >= 48 for _, pl in pls)
    assert any(pl['used'] < pl['splits'] for _, pl in pls), 'empty splits'


def test_wino_table_covers_the_staging_pipeline():
    """Requests run three chunks ahead (g_x(c + 3)): spp >= 5 runs the pipeline in steady state."""
    pls = [(c, T.plan(c)) for c in WINO]
    for xf in (False, True):
        assert any(_xf(c) == xf and pl['spp'] >= 5 for c, pl in pls), xf
        assert any(_xf(c) == xf and pl['spp'] >= 5 and pl['spi'] % pl['spp'] and c['N'] >= 3 for c, pl in pls), \
            'a slice that crosses an image boundary in its middle'
    assert any(pl['spp'] >= 5 and pl['last'] < pl['spp'] for _, pl in pls), 'a shorter last slice'
    assert any(c['H'] % 2 and pl['spp'] >= 5 for c, pl in pls) and any(c['W'] % 2 and pl['spp'] >= 5 for c, pl in pls)
    assert any(c['W'] % 16 and pl['spp'] >= 5 for c, pl in pls)
    chans = {c['Cin'] for c in WINO} | {c['Cout'] for c in WINO}
    assert {64, 192} <= chans
    assert any(_xf(c) and 'relu' not in c['flags'].split() for c in WINO)


def test_stem_table_covers_both_layouts_and_the_grid_stride_loop():
    for layout in (0, 1):
        pls = [T.plan(c) for c in STEM if c['layout'] == layout]
        assert any(pl['tiles'] > 512 for pl in pls) and any(pl['tiles'] < 512 for pl in pls)
        assert any(pl['tiles'] > 512 and pl['tiles'] % 512 and (pl['OH'] % 16 or pl['OW'] % 32) for pl in pls), 'a wrapped loop on ragged tiles'
        assert any(pl['OH'] % 16 for pl in pls) and any(pl['OW'] % 32 for pl in pls)
        assert any(pl['OW'] < 32 for pl in pls), 'narrower than one tile'
        assert any(c['H'] % 2 and c['W'] % 2 for c in STEM if c['layout'] == layout)


# ---- bar sensitivity: an exact fp64 "kernel", then corrupted ----------------------------------------------------------------
N, H, W, CIN, COUT, K, S, P = 3, 21, 19, 32, 24, 3, 1, 1
M = N * H * W


def _problem(seed=3, affine=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, CIN), generator=g)
    dy = torch.randn((N, H, W, COUT), generator=g)                     # zero-mean: the bars rest on it
    ab = (torch.rand((N, CIN), generator=g) + 0.5, torch.rand((N, CIN), generator=g) + 0.5) if affine else None
    return dy, x, ab


def _gather_wgrad(dy, xv, mode=None, fill=None):
    """fp64 weight gradient by explicit gathers -- xv (N, H, W, C) the input values after any affine -- with a deliberate fault:
    'left': a tap left of the map reads the previous row's last pixel; 'top': a tap above image n reads image n - 1's last row;
    fill (N, C): padded taps read this value instead of 0."""
    d = dy.double().reshape(M, -1)
    xf = xv.double().reshape(M, -1)
    m = torch.arange(M)
    n, rem = m // (H * W), m % (H * W)
    oy, ox = rem // W, rem % W
    out = torch.zeros((d.shape[1], xf.shape[1], K, K), dtype=torch.float64)
    for kh in range(K):
        for kw in range(K):
            iy, ix = oy * S + kh - P, ox * S + kw - P
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            lin = (n * H + iy) * W + ix
            if mode == 'left':
                ok = ok | ((ix == -1) & (iy >= 0) & (iy < H) & (lin >= 0))
            if mode == 'top':
                ok = ok | ((iy == -1) & (ix >= 0) & (ix < W) & (n > 0))
            g = xf[lin.clamp(0, M - 1)]
            pad = torch.zeros_like(g) if fill is None else fill.double()[n]
            out[:, :, kh, kw] = d.t() @ torch.where(ok[:, None], g, pad)
    return out


def _passes(got, r, base=None, mag=None):
    want = r['ref'] if base is None else r['ref'] + base.double()
    try:
        R.check('emulated', got.double(), want, R.bar_fp32(r, None if base is None else base.double(), mag=mag))
        return True
    except AssertionError:
        return False


def _slabbed_fp32(dy, xv, slab=5 * 32):
    """torch fp32: per-slab partial gradients (fp32 GEMMs over `slab` pixels), summed in fp32 in order."""
    d = dy.float().reshape(M, -1)
    taps = list(R._taps(xv.float(), K, S, P, H, W))
    out = torch.zeros((d.shape[1], xv.shape[-1], K, K), dtype=torch.float32)
    for m0 in range(0, M, slab):
        for kh, kw, xt in taps:
            out[:, :, kh, kw] += d[m0:m0 + slab].t() @ xt[m0:m0 + slab]
    return out


def test_gather_kernel_is_the_reference():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    assert torch.allclose(_gather_wgrad(dy, x), r['ref'], rtol=1e-12, atol=1e-12)
    w = torch.zeros((COUT, CIN, K, K), dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double().permute(0, 3, 1, 2), w, None, S, P) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    assert torch.allclose(r['ref'], w.grad, rtol=1e-12, atol=1e-12)


def test_reference_on_a_strided_odd_map_is_autograd():
    g = torch.Generator().manual_seed(8)
    x = torch.randn((2, 11, 9, 8), generator=g)
    dy = torch.randn((2, 6, 5, 12), generator=g)
    r = R.reference(dy, x, 3, 2, 1)
    w = torch.zeros((12, 8, 3, 3), dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double().permute(0, 3, 1, 2), w, None, 2, 1) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    assert torch.allclose(r['ref'], w.grad, rtol=1e-12, atol=1e-12)
    co, ci = np.array([0, 5, 11]), np.array([1, 7])
    rs = R.reference(dy, x, 3, 2, 1, co=co, ci=ci)
    assert torch.equal(rs['ref'], r['ref'][co][:, ci]) and torch.equal(rs['mag'], r['mag'][co][:, ci])


def test_sample_channels_hold_the_tile_and_sub_block_edges():
    for C in (4, 64, 132, 192, 320, 388, 512):
        s = set(R.sample_channels(C).tolist())
        assert max(s) == C - 1 and min(s) == 0
        for b in range(0, C, 32):
            assert b in s and min(b + 31, C - 1) in s
        assert set(range(max(C // 128 * 128, C - 8), C)) <= s


def test_fp32_slabs_pass_the_fp32_bar():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    assert _passes(_slabbed_fp32(dy, x), r)


def test_fp32_slabs_pass_under_the_affine_and_relu():
    dy, x, ab = _problem(affine=True)
    r = R.reference(dy, x, K, S, P, in_ab=ab, in_relu=True)
    xv = (x * ab[0][:, None, None, :] + ab[1][:, None, None, :]).clamp_min(0)          # fp32, as the kernel forms it
    assert _passes(_slabbed_fp32(dy, xv), r)


def test_bf16_operands_in_fp32_slabs_pass_the_bf16_bar():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P, bf16=True)
    assert _passes(_slabbed_fp32(dy.bfloat16().float(), x.bfloat16().float()), r)
    assert not _passes(_slabbed_fp32(dy, x), r)                       # ... and the unrounded operands are another problem


def test_bar_catches_one_dropped_pixel():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    d2 = dy.clone()
    d2[1, 7, 5] = 0
    assert not _passes(_gather_wgrad(d2, x), r)


def test_bar_catches_one_dropped_chunk():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    d2 = dy.clone()
    d2.view(M, -1)[10 * 32:11 * 32] = 0
    assert not _passes(_gather_wgrad(d2, x), r)


def test_bar_catches_one_slab_counted_twice():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    d2 = torch.zeros_like(dy)
    d2.view(M, -1)[160:320] = dy.view(M, -1)[160:320]
    assert not _passes(r['ref'] + _gather_wgrad(d2, x), r)


def test_bar_catches_a_left_border_tap_reading_the_previous_row():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    assert not _passes(_gather_wgrad(dy, x, mode='left'), r)


def test_bar_catches_a_top_border_tap_reading_the_previous_image():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    assert not _passes(_gather_wgrad(dy, x, mode='top'), r)


def test_bar_catches_padding_that_reads_relu_b_under_the_affine():
    dy, x, ab = _problem(affine=True)
    r = R.reference(dy, x, K, S, P, in_ab=ab, in_relu=True)
    xv = (x.double() * ab[0].double()[:, None, None, :] + ab[1].double()[:, None, None, :]).clamp_min(0)
    assert _passes(_gather_wgrad(dy, xv), r)
    assert not _passes(_gather_wgrad(dy, xv, fill=ab[1].clamp_min(0)), r)


def test_bar_catches_the_previous_images_affine_table():
    dy, x, ab = _problem(affine=True)
    r = R.reference(dy, x, K, S, P, in_ab=ab, in_relu=True)
    a, b = (t.double()[:, None, None, :].expand(N, H, W, CIN).clone() for t in ab)
    for n in range(1, N):                                             # the first 5 pixels of image n still use image n - 1's table
        a[n, 0, :5], b[n, 0, :5] = ab[0][n - 1].double(), ab[1][n - 1].double()
    assert not _passes(_gather_wgrad(dy, (x.double() * a + b).clamp_min(0)), r)


def test_bar_catches_bf16_truncation():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P, bf16=True)
    trunc = (x.view(torch.int32) & ~0xFFFF).view(torch.float32)        # bf16 by dropping the low 16 bits
    assert _passes(_gather_wgrad(dy.bfloat16(), x.bfloat16()), r)
    assert not _passes(_gather_wgrad(dy.bfloat16(), trunc), r)
    td = (dy.view(torch.int32) & ~0xFFFF).view(torch.float32)
    assert not _passes(_gather_wgrad(td, x.bfloat16()), r)


def test_bar_catches_accumulate_that_overwrites():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    base = torch.randn((COUT, CIN, K, K), generator=torch.Generator().manual_seed(1)) * M ** 0.5
    fp32 = _slabbed_fp32(dy, x)
    assert _passes(base + fp32, r, base=base)
    assert not _passes(fp32, r, base=base)


def test_bar_catches_the_stem_layouts_swapped_for_one_channel():
    g = torch.Generator().manual_seed(4)
    n, h, w = 2, 37, 29
    x4 = torch.randn((n, h, w, 4), generator=g)
    dy = torch.randn((n, 19, 15, 64), generator=g)
    r = R.stem_reference(dy, x4, 0)
    planes = x4[..., :3].permute(0, 3, 1, 2).contiguous()
    rp = R.stem_reference(dy, planes, 1)
    assert torch.equal(r['ref'], rp['ref']) and tuple(r['ref'].shape) == (64, 3, 7, 7)
    got = R.reference(dy.float(), x4[..., :3].float(), 7, 2, 3)['ref'].float()
    assert _passes(got, r)
    wrong = x4[..., :3].clone()
    wrong[..., 1] = x4.reshape(n, 4, h, w)[:, 1]                       # channel 1 read as a plane of the NHWC4 buffer
    assert not _passes(R.reference(dy, wrong, 7, 2, 3)['ref'], r)


def _wino(dy, x, ab, relu, dtype, swap=None):
    """The Winograd algorithm of conv_wino_wgrad.hip in ``dtype``: transforms, one accumulation over the tiles, output transform."""
    v = x.to(dtype)
    if ab is not None:
        v = v * ab[0].to(dtype)[:, None, None, :] + ab[1].to(dtype)[:, None, None, :]
        if relu:
            v = v.clamp_min(0)
    V, Z = R.wino_tiles(v, dy.to(dtype))
    U = torch.bmm(V.transpose(1, 2), Z)
    if swap:
        U[list(swap)] = U[list(reversed(swap))]
    return R.wino_out(U)


def test_winograd_in_fp64_is_the_reference_and_fp32_passes_its_bar():
    for affine in (False, True):
        dy, x, ab = _problem(affine=affine)
        r = R.reference(dy, x, K, S, P, in_ab=ab, in_relu=True)
        assert torch.allclose(_wino(dy, x, ab, True, torch.float64), r['ref'], rtol=1e-11, atol=1e-11)
        mw = R.wino_magnitude(dy, x, in_ab=ab)
        assert bool((mw >= r['mag'] * (1 - 1e-12)).all())               # the absolute transforms dominate the direct magnitude
        assert 2.0 < float((mw / r['mag']).mean()) < 12.0
        assert _passes(_wino(dy, x, ab, True, torch.float32), r, mag=mw)


def test_winograd_bar_catches_two_frequencies_swapped_and_a_dropped_pixel():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    mw = R.wino_magnitude(dy, x)
    assert not _passes(_wino(dy, x, None, False, torch.float64, swap=(5, 6)), r, mag=mw)
    d2 = dy.clone()
    d2[2, 20, 18] = 0                                                 # the last pixel: alone in its zero-filled partial tile
    assert not _passes(_wino(d2, x, None, False, torch.float64), r, mag=mw)


def test_check_names_the_entry_and_its_tile():
    dy, x, _ = _problem()
    r = R.reference(dy, x, K, S, P)
    got = r['ref'].clone()
    got[17, 9, 2, 1] += 1.0
    with pytest.raises(AssertionError) as e:
        R.check('named', got, r['ref'], R.bar_fp32(r))
    assert '(co=17 ci=9 kh=2 kw=1) tile (0, 0) sub-block (0, 0) lane (17, 9)' in str(e.value)
    got[17, 9, 2, 1] = float('nan')
    with pytest.raises(AssertionError):
        R.check('nan', got, r['ref'], R.bar_fp32(r))
