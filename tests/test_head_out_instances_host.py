"""CPU only: the launch rules tests/head_out_fp64_ref.py restates are the source's and the library's; the tables of
tests/test_gpu_head_out_instances.py reach every state ``coverage()`` names; float32 emulations of every kernel in its own order of
operations stay below half of every bar on the case operands (judged by the GPU file's own judge functions); wrong emulations fail,
only at elements they change, and pass where they cannot change anything; the entry points refuse bad arguments before any launch.

``fma`` here rounds the exact product plus the addend to 53 and then to 24 bits; ``logit_project``'s activation ``x * a + b`` is emulated
in both the fused and the unfused form.

Measured worst emulation error / bar (the last test prints them): logit_project 0.127; taps 0.052, tap_sum 0.339, forward end to end
0.019, tap_sum alone 0.285; dgrad 0.337; wgrad partial 0.420 (the one-pixel map: one fma and the activation's own fma against two
whole ulps), bias partial 0.043, finalize gw 0.49998 / gb 0.483 (R = 2: one addition against one whole ulp, so never above a half),
gw end to end 0.420, gb end to end 0.037.  No bar needed the exception ``bn_fold`` took: every emulation is below a half."""
import os

import pytest
import torch

from tests import head_out_fp64_ref as R
from tests import test_gpu_head_out_instances as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
LOG = {}
F32 = torch.float32


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- launch rules ----------------------------------------------------------------------------------------------------
def test_logit_project_rules_are_the_source():
    s = _src('project.hip')
    assert 'const int q = threadIdx.x & %d;' % (R.PROJ_LANES - 1) in s
    assert 'const long long slot = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;' in s and 1 << 4 == R.PROJ_LANES
    assert 'const long long nslots = ((long long)gridDim.x * blockDim.x) >> 4;' in s and 'for (long long p = slot; p < npix; p += nslots) {' in s
    assert 'wj[j][k] = *reinterpret_cast<const f32x4*>(w + (size_t)j * Cin + k * 64 + q * 4);' in s           # lane q: channels 4q + 64k
    assert 'const float* xp = x + (size_t)p * Cin + q * 4;' in s and 'reinterpret_cast<const f32x4*>(xp + k * 64)' in s
    assert 'const long long want = (npix + 15) / 16;' in s
    assert 'const int blocks = (int)(want < 256 * 7 ? want : 256 * 7);' in s and R.PROJ_BLOCK_CAP == 256 * 7
    assert 'dim3(blocks), dim3(%d)' % R.PROJ_THREADS in s
    assert 'const float floor_ = (in_relu && a) ? 0.f : -INFINITY;' in s                                     # the ReLU belongs to the affine
    assert 'f32x4 t = xv[k] * a4 + b4;' in s                                                                 # a product and a sum: n = 2
    assert ('s = fmaf(xv[k].w, wj[j][k].w, fmaf(xv[k].z, wj[j][k].z, fmaf(xv[k].y, wj[j][k].y, fmaf(xv[k].x, wj[j][k].x, s))));') in s
    assert 'for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);' in s                                 # four additions
    assert 'out[(size_t)p * J + q] = v + bias[q];' in s
    assert 'switch (Cin / 64) {' in s and all('case %d: GO(%d); break;' % (k, k) in s for k in (1, 2, 3)) and 'default: GO(4); break;' in s
    assert all('case %d: launch_project<%d>(' % (j, j) in s for j in range(1, 8)) and 'default: launch_project<8>(' in s
    assert 'CPR_CHECK_ARG(x && w && bias && out && N > 0 && HW > 0 && J > 0);' in s
    assert 'if (J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;' in s
    assert [R.proj_channels(q, 2) for q in (0, 15)] == [[0, 1, 2, 3, 64, 65, 66, 67], [60, 61, 62, 63, 124, 125, 126, 127]]
    assert sorted(c for q in range(16) for c in R.proj_channels(q, 3)) == list(range(192))
    assert [R.proj_n(c) for c in R.CINS] == [9, 13, 17, 21]


def test_p2p_out_rules_are_the_source():
    s = _src('p2p_out_bf16.hip')
    guard = 'if (J < 1 || J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;'
    assert s.count(guard) == 3 and 'J < 1 || J > 8 || Cin < 64 || Cin > 256 || Cin % 64 != 0) return CPR_ERR_UNSUPPORTED;' in s.split('cpr_p2p_out_bf16_wgrad_ws')[1]
    # forward
    assert 'const unsigned grid = (unsigned)cdivll(npix, %d);' % R.FWD_THREADS in s and 'dim3(grid), dim3(%d)' % R.FWD_THREADS in s
    assert 'const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;' in s and 'if (p >= npix) return;' in s
    assert 'v[0] = fmaxf(fmaf(a0.x, v[0], b0.x), 0.f);' in s                                                 # one fma: n = 1
    assert 'const float* wc = w + ((size_t)j * Cin + c0 + i) * 9;' in s
    assert 'for (int t = 0; t < 9; ++t) acc[t * J + j] = fmaf(v[i], wc[t], acc[t * J + j]);' in s            # R[p][t J + j], c ascending
    assert 'return cpr_tap_sum3x3(taps, bias, out, N, H, W, J, stream);' in s
    assert s.count('case %d: GO(%d); break;' % (5, 5)) == 2 and all(s.count('case %d: GO(%d); break;' % (j, j)) == 4 for j in (1, 2, 3))
    assert s.count('case 4: GO(4); break;') == 2 and s.count('default: GO(8); break;') == 2 and s.count('default: GO(4); break;') == 2
    assert all('case %d: launch_wgrad<%d>(' % (j, j) in s for j in range(1, 8)) and 'default: launch_wgrad<8>(' in s
    # the shared tap loader
    assert 'const int oy = y - kh + 1, ox = x - kw + 1;' in s and 'd[kh * 3 + kw][j] = in ? dp[j] : 0.f;' in s
    assert 'const float* dp = dout + ((size_t)nbase + (size_t)cy * W + cx) * ldd;' in s
    # dgrad
    assert 'const int ppw = %d;' % R.DGRAD_PPW in s and 'const int KB = Cin / 64;' in s and 'const int KW = J <= 4 ? KB : 1;' in s
    assert 'const int G = KB / KW;' in s and 'const unsigned grid = (unsigned)(cdivll(npix, ppw) * G);' in s
    assert s.count('const int g = blockIdx.x % G;') == 2 and 'const long long p0 = (long long)(blockIdx.x / G) * ppw;' in s
    assert s.count('if constexpr (J > 4) {') == 2 and s.count('const long long pend = p0 + ppw < npix ? p0 + ppw : npix;') == 2
    assert 'for (int j = 0; j < J; ++j) s = fmaf(d[t][j], wr[k][t][j], s);' in s                             # one chain of 9 J
    assert 'reinterpret_cast<__bf16*>(dx)[o] = (__bf16)acc[k];' in s
    assert 'CPR_CHECK_ARG(dout && w && dx && N > 0 && H > 0 && W > 0 && ldd >= J);' in s
    # wgrad
    assert 'const long long want = %d / G;' % R.WGRAD_WAVES in s and 'const long long by_pix = cdivll(npix, %d);' % R.WGRAD_MIN_PIX in s
    assert 'return (int)(want < by_pix ? want : by_pix);' in s
    assert 'static int wgrad_groups(int Cin, int J) { return J <= 4 ? 1 : Cin / 64; }' in s
    assert 'const long long ppw = cdivll(npix, R);' in s and 'float* wsb = ws + (size_t)R * Cin * 9 * J;' in s
    assert 'return R * (Cin * 9 * J + J);' in s and 'dim3(R * G), dim3(64)' in s
    assert 'const int rg = blockIdx.x / G;' in s and 'const long long p0 = rg * ppw;' in s
    assert 'if (n != cur_n) {' in s and 'an[k] = a[(size_t)n * Cin + c];' in s
    assert 'v[k] = fmaxf(fmaf(an[k], bf16_widen(x[(size_t)p * Cin + (g * KW + k) * 64 + lane]), bn[k]), 0.f);' in s
    assert 'acc[k][t][j] = fmaf(v[k], d[t][j], acc[k][t][j]);' in s and 'for (int j = 0; j < J; ++j) bacc[j] += dp[j];' in s
    assert 'float* o = ws + ((size_t)rg * Cin + c) * (9 * J);' in s and 'for (int j = 0; j < J; ++j) o[t * J + j] = acc[k][t][j];' in s
    assert 'for (int j = 0; j < J; ++j) wsb[(size_t)rg * J + j] = bacc[j];' in s and 'if (g == 0 && lane == 0)' in s
    assert 'for (int r = 0; r < R; ++r) s += ws[(size_t)r * E + e];' in s and 'for (int r = 0; r < R; ++r) s += wsb[(size_t)r * J + j];' in s
    assert 'const int c = e / (9 * J), t = (e / J) % 9, j = e % J;' in s and 'gw[((size_t)j * Cin + c) * 9 + t] = s;' in s
    p = _src('postproc.hip')
    assert 'const int yy = y + kh - 1;' in p and 'if ((unsigned)yy >= (unsigned)H) continue;' in p and 'const int xx = x + kw - 1;' in p
    assert 'if ((unsigned)xx >= (unsigned)W) continue;' in p
    assert 's += R[(((size_t)n * H + yy) * W + xx) * (9 * J) + (kh * 3 + kw) * J + j];' in p and 'out[i] = s + (bias ? bias[j] : 0.f);' in p
    assert 'CPR_CHECK_ARG(R && out && N > 0 && H > 0 && W > 0 && J > 0);' in p


def test_workspace_query_agrees_with_the_restated_plan():
    from pointtinybenchmark_amd import _lib
    L = _lib.load()
    gen = torch.Generator().manual_seed(0)
    shapes = [s for _, _, s in T.wgrad_cases()] + [(1, 1, n) for n in (63, 64, 65, 127, 128, 129, 131071, 131072, 131073, 65535, 65537)]
    shapes += [tuple(int(v) for v in torch.randint(1, 400, (3,), generator=gen)) for _ in range(200)]
    for N, H, W in shapes:
        for Cin in R.CINS:
            for J in R.JS:
                npix = N * H * W
                assert L.cpr_p2p_out_bf16_wgrad_ws(N, H, W, Cin, J) == R.wgrad_ws(npix, Cin, J), (N, H, W, Cin, J)
                G, Rn, ppw = R.wgrad_plan(npix, Cin, J)
                rs = R.wgrad_ranges(npix, Cin, J)
                assert Rn * ppw >= npix and len(rs) == Rn and sum(max(p1 - p0, 0) for p0, p1 in rs) == npix   # every pixel in one range
                assert (R.empty_ranges(npix, Cin, J) > 0) == ((Rn - 1) * ppw >= npix)
    # the issue's claim: at G = 1 no plan up to 131072 pixels has an empty range
    plans = ((n,) + R.wgrad_plan(n, 64, 1) for n in range(1, 131073))
    assert not any((Rn - 1) * ppw >= n for n, _, Rn, ppw in plans)
    assert R.wgrad_plan(131073, 64, 1) == (1, 2048, 65) and R.empty_ranges(131073, 64, 1) == 31             # 2017 ranges of 65 hold them all


# ---- coverage --------------------------------------------------------------------------------------------------------
def test_no_state_is_unreached():
    cov = T.coverage()
    missing = [k for k in T.WANTED if not cov.get(k)]
    assert not missing, missing
    assert len(set(T.WANTED)) == len(T.WANTED) and len(T.PAIRS) == 32


def test_cases_reach_the_states_claimed_for_them():
    """Every plan figure of the case table, re-derived from the integer rules."""
    assert all(R.wgrad_plan(105, Cin, J)[1:] == (2, 53) for J, Cin in T.PAIRS)
    assert all(R.wgrad_ranges(105, Cin, J) == [(0, 53), (53, 105)] and R.straddling_ranges(105, 35, Cin, J) == 2 for J, Cin in T.PAIRS)
    assert {R.groups(Cin, J) for J, Cin in T.PAIRS} == {(k, 1) for k in (1, 2, 3, 4)} | {(1, k) for k in (1, 2, 3, 4)}
    assert R.proj_blocks(105) == 7 and R.proj_passes(105) == 1 and R.proj_blocks(1) == 1
    assert (R.proj_blocks(28800), R.proj_slots(28800), 28800 - R.proj_slots(28800)) == (1792, 28672, 128)
    assert R.fwd_blocks(17 * 19) == 2 and 17 * 19 % 256 == 67 and 17 * 19 % R.DGRAD_PPW == 3
    assert R.dgrad_grid(323, 256, 8) == 21 * 4 and R.dgrad_grid(323, 192, 4) == 21
    for J, Cin in T.SHAPE_PAIRS:
        assert R.wgrad_plan(35, Cin, J)[1:] == (1, 35) and R.wgrad_plan(1, Cin, J)[1:] == (1, 1) and R.wgrad_plan(2 * 33 * 31, Cin, J)[1:] == (32, 64)
        assert R.wgrad_ranges(2046, Cin, J)[-1] == (1984, 2046) and R.straddling_ranges(2046, 1023, Cin, J) == 1
    for J in (1, 3):
        npix = 363 * 362
        assert npix == 131406 and R.wgrad_plan(npix, 64, J) == (1, 2048, 65) and R.empty_ranges(npix, 64, J) == 26
        assert R.wgrad_ranges(npix, 64, J)[2021] == (131365, 131406) and R.wgrad_ranges(npix, 64, J)[2022] == (131430, 131406)
    assert 264 * 250 == 66000 and R.wgrad_plan(66000, 128, 5) == (2, 1024, 65) and R.empty_ranges(66000, 128, 5) == 8
    assert [T.ldds(J) for J in (1, 4, 5, 8)] == [[1, 4], [4, 7], [5, 8], [8, 11]]
    for J, Cin, s in T.wgrad_cases():                                           # in-contract calls whose workspace size fits an int
        assert J in R.JS and Cin in R.CINS and R.wgrad_ws(s[0] * s[1] * s[2], Cin, J) < 2 ** 31


def test_the_matrix_references_are_the_autograd_of_conv2d():
    for J, Cin, shape in ((3, 64, (2, 4, 5)), (8, 128, (1, 1, 1)), (5, 64, (2, 1, 6)), (2, 64, (1, 7, 1))):
        o = T.f64(T.operands(J, Cin, shape))
        act, ba = R.act_ref(o['x'], o['a'], o['b'])
        d = o['dout'][..., :J]
        dact, gw, gb = R.conv_grads_ref(act, o['w'], d)
        assert float((R.dgrad_ref(d, o['w'])[0] - dact).abs().max()) <= 1e-13
        wref, _, bref, _, _ = R.wgrad_partial_ref(act, ba, d, Cin, J)
        fw, _, fb, _ = R.finalize_ref(wref.view(-1, Cin, 9, J), bref)
        assert float((fw - gw).abs().max()) <= 1e-12 and float((fb - gb).abs().max()) <= 1e-12
        tref, tbar = R.taps_ref(act, ba, o['w'])
        assert float((R.tap_sum_ref(tref, o['bias'], J)[0] - R.conv_ref(act, o['w'], o['bias'])).abs().max()) <= 1e-13
    assert R.in_map_taps(3, 4).flatten().tolist() == [4, 6, 6, 4, 6, 9, 9, 6, 4, 6, 6, 4] and R.in_map_taps(1, 1).item() == 1


# ---- emulations of the kernels' own order, float32 -----------------------------------------------------------------------
def fma(a, b, c):
    """fmaf: the product of two floats is exact in double, the sum is rounded to 53 bits and then to 24."""
    return (a.double() * b.double() + c.double()).float()


def emu_act(x, a, b, fused=True, relu=True, img=None):
    """x (N, H, W, C) fp32 (a widened bf16 map or the fp32 map); img: the image whose (a, b) every pixel uses (None: its own)."""
    N, H, W, C = x.shape
    av, bv = (a[:, None, None, :], b[:, None, None, :]) if img is None else (a[img].view(N, H, W, C), b[img].view(N, H, W, C))
    t = fma(av, x, bv) if fused else x * av + bv
    return t.clamp_min(0) if relu else t


def emu_project(o, J, Cin, shape, affine=True, in_relu=1, fused=True, wrong=None):
    npix, KC = shape[0] * shape[1] * shape[2], Cin // 64
    t = o['x32']
    if affine:
        t = emu_act(t, o['a'], o['b'], fused, relu=bool(in_relu))
    elif wrong == 'relu_no_affine' and in_relu:
        t = t.clamp_min(0)
    v, w = t.reshape(npix, 1, KC, 16, 4), o['wp'].view(1, J, KC, 16, 4)
    s = torch.zeros((npix, J, 16), dtype=F32)
    for k in range(KC):
        for i in range(4):
            s = fma(v[:, :, k, :, i], w[:, :, k, :, i], s)
    lane = torch.arange(16)
    for step in (8, 4, 2, 1):
        s = s + s[..., lane ^ step]
    out = torch.stack([s[:, j, j] for j in range(J)], 1) + o['bias']
    return out + o['bias'] if wrong == 'bias_twice' else out


def emu_taps(act, w):
    npix, C = act.numel() // act.shape[-1], act.shape[-1]
    v, m = act.reshape(npix, C), R.w9(w)
    acc = torch.zeros((npix, m.shape[0]), dtype=F32)
    for c in range(C):
        acc = fma(v[:, c:c + 1], m[:, c][None], acc)
    return acc


def emu_tap_sum(Rm, bias, J, wrong=None):
    N, H, W, _ = Rm.shape
    Rp = torch.nn.functional.pad(Rm, (0, 0, 1, 1, 1, 1))                      # s + 0.f is s: a skipped tap and a zero tap are the same bits
    s = torch.zeros((N, H, W, J), dtype=F32)
    for kh in range(3):
        for kw in range(3):
            t = kh * 3 + kw
            s = s + Rp[:, kh:kh + H, kw:kw + W, t * J:(t + 1) * J]
    bz = torch.zeros(J) if bias is None else bias
    out = s + bz
    return out + bz if wrong == 'bias_twice' else out


def emu_load_taps(dout, J, wrong=None):
    """dout (N, H, W, ldd) -> (npix, 9 J) as ``load_taps`` reads it."""
    N, H, W, ldd = dout.shape
    if wrong == 'ldd_as_J':
        dout = dout.reshape(-1)[:N * H * W * J].view(N, H, W, J)
    ys, xs = torch.arange(H), torch.arange(W)
    cols = []
    for kh in range(3):
        for kw in range(3):
            oy, ox = (ys + kh - 1, xs + kw - 1) if wrong == 'flip' else (ys - kh + 1, xs - kw + 1)
            inside = ((oy >= 0) & (oy < H)).view(1, H, 1, 1) & ((ox >= 0) & (ox < W)).view(1, 1, W, 1)
            v = dout[:, oy.clamp(0, H - 1)][:, :, ox.clamp(0, W - 1)][..., :J]
            cols.append(v if wrong == 'clamp_no_zero' else torch.where(inside, v, torch.zeros_like(v)))
    return torch.cat(cols, 3).reshape(N * H * W, 9 * J)


def emu_dgrad(o, J, Cin, shape, wrong=None):
    """-> (dx fp32, dx bf16), (npix, Cin)."""
    d, m = emu_load_taps(o['dout'], J, wrong), R.w9(o['w'])
    s = torch.zeros((d.shape[0], Cin), dtype=F32)
    for i in range(9 * J):
        s = fma(d[:, i:i + 1], m[i][None], s)
    if wrong == 'truncate':
        return s, (s.view(torch.int32) & -65536).view(F32).bfloat16()
    return s, s.bfloat16()


def emu_wgrad(o, J, Cin, shape, wrong=None):
    N, H, W = shape
    npix, HW = N * H * W, H * W
    _, Rn, ppw = R.wgrad_plan(npix, Cin, J)
    rs = R.wgrad_ranges(npix, Cin, J)
    img = None
    if wrong == 'no_reload':                                                   # every pixel of a range uses the affine of the range's first image
        img = torch.cat([torch.full((max(p1 - p0, 0),), min(p0, npix - 1) // HW, dtype=torch.int64) for p0, p1 in rs])
    act = emu_act(o['x'].float(), o['a'], o['b'], img=img).reshape(npix, Cin)
    v, d = R._by_range(act, Rn, ppw), R._by_range(emu_load_taps(o['dout'], J, wrong), Rn, ppw)
    db = R._by_range(o['dout'].reshape(npix, -1)[:, :J].contiguous(), Rn, ppw)
    last = torch.tensor([p1 - p0 - (1 if wrong == 'skip_last' else 0) for p0, p1 in rs])
    acc, bacc = torch.zeros((Rn, Cin, 9 * J), dtype=F32), torch.zeros((Rn, J), dtype=F32)
    for i in range(ppw):
        live = i < last
        acc = torch.where(live.view(Rn, 1, 1), fma(v[:, i, :, None], d[:, i, None, :], acc), acc)
        bacc = torch.where(live.view(Rn, 1), bacc + db[:, i], bacc)
    if wrong == 'empty_unwritten':
        empty = torch.tensor([p1 <= p0 for p0, p1 in rs])
        acc[empty], bacc[empty] = float('nan'), float('nan')
    sw, sb = torch.zeros((Cin, 9 * J), dtype=F32), torch.zeros(J, dtype=F32)
    for r in range(Rn):
        sw, sb = sw + acc[r], sb + bacc[r]
    gw = sw.view(Cin, 9, J).permute(2, 0, 1).reshape(J, Cin, 3, 3).contiguous()
    return dict(gw=gw, gb=sb, ws=torch.cat([acc.reshape(-1), bacc.reshape(-1)]))


def emu_fwd(o, J, Cin, shape):
    taps = emu_taps(emu_act(o['x'].float(), o['a'], o['b']), o['w']).view(shape + (9 * J,))
    return dict(taps=taps, out=emu_tap_sum(taps, o['bias'], J))


@pytest.fixture(autouse=True)
def _keep_the_gpu_files_log():
    saved = dict(T.WORST)
    yield
    T.WORST.clear()
    T.WORST.update(saved)


def note(qs):
    for k, v in qs.items():
        LOG[k] = max(LOG.get(k, 0.0), v)
        assert v <= 0.5, (k, v, qs)


def test_the_activation_emulation_meets_its_bar_and_clips_to_zero():
    o = T.operands(4, 192, T.BASE)
    d = T.f64(o)
    for x, n, forms in ((o['x'].float(), 1, (True,)), (o['x32'], 2, (True, False))):
        ref, bar = R.act_ref(x.double(), d['a'], d['b'], n=n)
        y = d['a'][:, None, None, :] * x.double() + d['b'][:, None, None, :]
        for fused in forms:
            got = emu_act(x, o['a'], o['b'], fused)
            assert float(R.ratio(got, ref, bar).max()) <= 0.5
            clipped = y < -R.gs(n) * ((d['a'][:, None, None, :] * x.double()).abs() + d['b'].abs()[:, None, None, :])
            assert int(clipped.sum()) > 1000 and R.positive_zero(got[clipped]) and bool((bar[clipped] == 0).all())


@pytest.mark.parametrize('J,Cin', T.PAIRS, ids=lambda v: str(v))
def test_emulations_of_every_instance_stay_below_half_of_every_bar(J, Cin):
    o = T.operands(J, Cin, T.BASE)
    for fused in (True, False):
        note(T.judge_project('emulation', o, emu_project(o, J, Cin, T.BASE, fused=fused), J, T.BASE))
    note(T.judge_fwd('emulation', o, emu_fwd(o, J, Cin, T.BASE), J, T.BASE))
    note(T.judge_dgrad('emulation', o, *emu_dgrad(o, J, Cin, T.BASE), J, Cin, T.BASE))
    note(T.judge_wgrad('emulation', o, emu_wgrad(o, J, Cin, T.BASE), J, Cin, T.BASE))


@pytest.mark.parametrize('J,Cin', T.SHAPE_PAIRS, ids=lambda v: str(v))
def test_emulations_of_the_shape_and_plan_cases_stay_below_half_of_every_bar(J, Cin):
    for shape in T.SHAPES:
        for ldd in (T.ldds(J) if shape == T.LDD_SHAPE else [J + 3]):
            o = T.operands(J, Cin, shape, ldd)
            note(T.judge_dgrad('emulation', o, *emu_dgrad(o, J, Cin, shape), J, Cin, shape))
        note(T.judge_fwd('emulation', o, emu_fwd(o, J, Cin, shape), J, shape))
    for shape in T.WGRAD_SHAPES:
        o = T.operands(J, Cin, shape, max(4, J))
        note(T.judge_wgrad('emulation', o, emu_wgrad(o, J, Cin, shape), J, Cin, shape))


@pytest.mark.parametrize('J,Cin', T.PROJ_PAIRS, ids=lambda v: str(v))
def test_emulations_of_the_logit_project_variants(J, Cin):
    for shape, affine, relu in ((T.BASE, True, 0), (T.BASE, False, 1), ((1, 1, 1), True, 1)):
        o = T.operands(J, Cin, shape)
        for fused in (True, False):
            note(T.judge_project('emulation', o, emu_project(o, J, Cin, shape, affine, relu, fused), J, shape, affine, relu))


def test_emulation_of_the_longest_logit_project_walk_and_of_an_empty_range_plan():
    J, Cin, shape = T.PROJ_STRIDE[1]
    o = T.operands(J, Cin, shape)
    note(T.judge_project('emulation', o, emu_project(o, J, Cin, shape), J, shape))
    J, Cin, shape = T.WGRAD_BIG[0]
    o = T.operands(J, Cin, shape, max(4, J))
    note(T.judge_wgrad('emulation', o, emu_wgrad(o, J, Cin, shape), J, Cin, shape))


@pytest.mark.parametrize('J,shape,bias', T.TAPSUM_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_emulation_of_the_tap_sum_alone(J, shape, bias):
    Rm, bv = T.tapsum_operands(J, shape, bias)
    note(T.judge_tapsum('emulation', Rm, bv, emu_tap_sum(Rm, bv, J), J))


# ---- wrong emulations: each fails, only at elements it changes, and passes where it cannot change anything -----------------------
def verdict(got, right, ref, bar):
    """(failing, changed) boolean maps of a wrong emulation: it must fail somewhere, only where its bits differ from the right
    emulation's, and wherever it moved an element by more than 1.5 bars."""
    bar = bar.expand_as(ref)
    got, right = got.reshape(ref.shape), right.reshape(ref.shape)
    fail = ~(R.ratio(got, ref, bar) <= 1.0)
    changed = got.view(torch.int32) != right.view(torch.int32)
    assert bool(fail.any()), 'the wrong emulation passes'
    assert not bool((fail & ~changed).any()), 'an unchanged element fails'
    assert not bool(((got.double() - right.double()).abs() > 1.5 * bar).logical_and(~fail).any())
    assert bool((R.ratio(right, ref, bar) <= 0.5).all())
    return fail, changed


def _wgrad_refs(o, J, Cin):
    d = T.f64(o)
    act, ba = R.act_ref(d['x'], d['a'], d['b'])
    return R.wgrad_partial_ref(act, ba, d['dout'][..., :J], Cin, J)


def test_a_dropped_affine_reload_fails_in_the_ranges_that_straddle_an_image():
    J, Cin, shape = 5, 128, (2, 33, 31)
    o = T.operands(J, Cin, shape, J)
    right, bad = emu_wgrad(o, J, Cin, shape), emu_wgrad(o, J, Cin, shape, 'no_reload')
    wref, wbar, _, _, _ = _wgrad_refs(o, J, Cin)
    E = 32 * Cin * 9 * J
    fail, changed = verdict(bad['ws'][:E], right['ws'][:E], wref, wbar)
    straddle = [r for r, (p0, p1) in enumerate(R.wgrad_ranges(2046, Cin, J)) if p0 // 1023 != (p1 - 1) // 1023]
    assert straddle == [15] and not bool(changed[:15].any()) and not bool(changed[16:].any()) and bool(fail[15].any())      # one pixel of range 15 lies in image 1
    one = T.operands(J, Cin, (1, 5, 7), J)                                    # one image: nothing to reload
    assert torch.equal(emu_wgrad(one, J, Cin, (1, 5, 7))['ws'], emu_wgrad(one, J, Cin, (1, 5, 7), 'no_reload')['ws'])


@pytest.mark.parametrize('wrong', ['clamp_no_zero', 'flip'])
def test_wrong_tap_loads_fail_at_the_pixels_they_change(wrong):
    J, Cin, shape = 4, 192, (1, 17, 19)
    o = T.operands(J, Cin, shape, J)
    d = T.f64(o)
    ref, bar = R.dgrad_ref(d['dout'][..., :J], d['w'])
    fail, changed = verdict(emu_dgrad(o, J, Cin, shape, wrong)[0], emu_dgrad(o, J, Cin, shape)[0], ref, bar)
    fail = fail.view(17, 19, Cin)
    if wrong == 'clamp_no_zero':                                              # interior pixels have every tap in the map
        assert not bool(changed.view(17, 19, Cin)[1:-1, 1:-1].any())
        border = torch.ones(17, 19, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        assert float(fail[border].double().mean()) > 0.9
    else:
        assert float(fail.double().mean()) > 0.9
    wref, wbar, _, _, _ = _wgrad_refs(o, J, Cin)
    E = R.wgrad_plan(323, Cin, J)[1] * Cin * 9 * J
    verdict(emu_wgrad(o, J, Cin, shape, wrong)['ws'][:E], emu_wgrad(o, J, Cin, shape)['ws'][:E], wref, wbar)
    if wrong == 'flip':                                                       # a one-pixel map has only the centre tap: the flip cannot show
        one = T.operands(J, Cin, (1, 1, 1), J)
        assert torch.equal(emu_dgrad(one, J, Cin, (1, 1, 1), wrong)[0], emu_dgrad(one, J, Cin, (1, 1, 1))[0])


def test_a_skipped_last_pixel_and_unwritten_empty_ranges_fail_in_the_partials():
    J, Cin, shape = T.WGRAD_BIG[0]
    o = T.operands(J, Cin, shape, max(4, J))
    wref, wbar, bref, bbar, cnt = _wgrad_refs(o, J, Cin)
    right = emu_wgrad(o, J, Cin, shape)
    E = 2048 * Cin * 9 * J
    bad = emu_wgrad(o, J, Cin, shape, 'skip_last')
    fail, changed = verdict(bad['ws'][:E], right['ws'][:E], wref, wbar)
    assert not bool(changed[cnt == 0].any()) and float(fail[cnt > 0].double().mean()) > 0.3            # relu: half of a pixel's channels are 0
    fail, changed = verdict(bad['ws'][E:], right['ws'][E:], bref, bbar)
    assert not bool(changed[cnt == 0].any()) and bool(fail[cnt > 0].all())
    bad = emu_wgrad(o, J, Cin, shape, 'empty_unwritten')
    fail, changed = verdict(bad['ws'][:E], right['ws'][:E], wref, wbar)
    assert bool(fail[cnt == 0].all()) and not bool(fail[cnt > 0].any()) and int((cnt == 0).sum()) == 26
    assert not bool(torch.isfinite(bad['gw']).any())                                                   # and the finalize sum carries it everywhere
    o = T.operands(J, Cin, T.BASE)                                                                    # no empty range: nothing to leave unwritten
    assert torch.equal(emu_wgrad(o, J, Cin, T.BASE, 'empty_unwritten')['ws'], emu_wgrad(o, J, Cin, T.BASE)['ws'])


def test_a_bias_added_twice_fails_unless_it_is_absent():
    J, Cin = 2, 256
    o = T.operands(J, Cin, T.BASE)
    d = T.f64(o)
    ref, bar = R.project_ref(d['x32'], d['wp'], d['bias'], d['a'], d['b'])
    fail, _ = verdict(emu_project(o, J, Cin, T.BASE, wrong='bias_twice'), emu_project(o, J, Cin, T.BASE), ref, bar)
    assert bool(fail.all())
    Rm, bv = T.tapsum_operands(J, (2, 5, 7), True)
    fail, _ = verdict(emu_tap_sum(Rm, bv, J, 'bias_twice'), emu_tap_sum(Rm, bv, J), *R.tap_sum_ref(Rm.double(), bv.double(), J))
    assert bool(fail.all())
    assert torch.equal(emu_tap_sum(Rm, None, J, 'bias_twice'), emu_tap_sum(Rm, None, J))


def test_ldd_taken_as_j_fails_unless_ldd_is_j():
    J, Cin, shape = 5, 128, (1, 17, 19)
    for ldd in T.ldds(J):
        o = T.operands(J, Cin, shape, ldd)
        right, bad = emu_dgrad(o, J, Cin, shape)[0], emu_dgrad(o, J, Cin, shape, 'ldd_as_J')[0]
        if ldd == J:
            assert torch.equal(right, bad)
        else:
            d = T.f64(o)
            verdict(bad, right, *R.dgrad_ref(d['dout'][..., :J], d['w']))
            assert not bool(torch.isfinite(bad).all())                        # the pad channels are NaN


def test_truncation_fails_the_bit_comparison_of_the_bf16_store():
    J, Cin, shape = 1, 64, (1, 17, 19)
    o = T.operands(J, Cin, shape)
    dx, dx16 = emu_dgrad(o, J, Cin, shape)
    T.same('rne', dx16, R.bf16_rne(dx))
    _, bad = emu_dgrad(o, J, Cin, shape, 'truncate')
    with pytest.raises(AssertionError):
        T.same('truncated', bad, R.bf16_rne(dx))
    up = (R.bf16_rne(dx).float().abs() > dx.abs())                            # truncation differs exactly where RNE rounds away from zero
    assert torch.equal(T.bits(bad) != T.bits(dx16), up) and 0.3 < float(up.double().mean()) < 0.7


def test_a_relu_without_an_affine_fails_at_the_pixels_with_a_negative_input():
    J, Cin = 8, 192
    o = T.operands(J, Cin, T.BASE)
    d = T.f64(o)
    ref, bar = R.project_ref(d['x32'], d['wp'], d['bias'], None, None, 1)
    fail, _ = verdict(emu_project(o, J, Cin, T.BASE, False, 1, wrong='relu_no_affine'), emu_project(o, J, Cin, T.BASE, False, 1), ref, bar)
    assert float(fail.double().mean()) > 0.99
    assert torch.equal(emu_project(o, J, Cin, T.BASE, True, 1, wrong='relu_no_affine'), emu_project(o, J, Cin, T.BASE, True, 1))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    T.test_entry_points_refuse_bad_arguments_before_any_launch()


def test_print_worst_emulation_ratio_per_stage():
    for k in sorted(LOG):
        print('HEADOUT emulation worst |err| / bar  %-22s %.4f' % (k, LOG[k]))
