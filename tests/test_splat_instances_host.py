"""CPU only: the launch rules tests/splat_fp64_ref.py restates are the source's and the library's; the tables of
tests/test_gpu_splat_instances.py reach every state ``coverage()`` names; numpy-float32 emulations of every kernel of csrc/splat.hip in
its own order of operations, in both the fused and the unfused form of each ``a * b + c``, stay below half of every bar on the small
cases (judged by the GPU file's own judge functions); wrong emulations fail, and only at elements they change; the entry points refuse
bad arguments before any launch.

The softmax is the one exception to the half: its subtraction term ``U32 |a0 - a1| r0 r1`` is a sharp bound (one rounding of
``a_r - max`` against a bar of exactly that rounding), so on the saturated variants the emulation only has to stay below 1; on the
cases with ``|a0 - a1| <= 8`` it stays below a half.  ``gap final`` counts its K + 1 roundings exactly, so for 4 < K + 1 < 16 it may
be met to the whole (0.716 at K = 4) and only has to stay below 1 there.

Measured worst emulation error / bar over the small cases (the last test prints them): gap partial 0.381, final 0.716, end to end
0.235; apply 0.323, pooled 0.356; attn_grad partial 0.357, pooled 0.220, final 0.4999; apply_bwd du 0.495 (the unfused form),
pooled 0.430, chunk sums 0.308, per image and colsum 0.4996; attn z 0.191, att 0.187 (0.136 where |a0 - a1| > 8), end to end 0.187;
attn_bwd da 0.340, xhat 0.176, dh' 0.139, dh 0.081, dg 0.221, the six parameter sums 0.234 .. 0.4998.

The softmax without the maximum subtracted fails at logits of +-200 and of +-97, NOT at +-60: exp(60) = 1.1e26 is finite in fp32 and
e0 / (e0 + e1) lands inside the bar."""
import os

import numpy as np
import pytest
import torch

from tests import splat_fp64_ref as R
from tests import test_gpu_splat_instances as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
F = np.float32
SMALL_MAPS = [c for c in T.MAP_CASES if c[1] <= 8]
LOG = {}


def _src():
    with open(os.path.join(CSRC, 'splat.hip')) as f:
        return f.read()


# ---- launch rules ----------------------------------------------------------------------------------------------------
def test_restated_constants_are_the_source():
    s = _src()
    assert '#define SPLAT_MAX_W %d ' % R.MAX_W in s and '#define SPLAT_MAX_INTER %d\n' % R.MAX_INTER in s
    assert '#define SPLAT_WALK %d ' % R.WALK in s and '#define SPLAT_ATTN_THREADS %d ' % R.ATTN_THREADS in s
    assert 'static inline int splat_pp(int w) { return %d / (w / 4); }' % R.THREADS in s
    assert 'static inline int splat_chunk(int w) { return SPLAT_WALK * splat_pp(w); }' in s
    assert s.count('const int cv = threadIdx.x % WV, prow = threadIdx.x / WV, PP = 256 / WV;') == 4          # gap, apply, attn_grad, apply_bwd
    assert s.count('const int end = min(HW, (k + 1) * CH);') == 3 and s.count('for (int p = k * CH + prow; p < end; p += PP)') == 3
    assert 'for (int r = 1; r < PP; ++r) s += lds[(v * PP + r) * WV + cv];' in s                              # prow ascending
    assert 'for (int r = 1; r < rows; ++r) s += p[(size_t)r * cols];' in s and 'out[i] = s * scale;' in s       # chunks / images ascending
    assert 'splat_rows_sum(ws, g, N, K, w, 1.f / (float)hw, stream);' in s and 'splat_rows_sum(ws, datt, N, K, 2 * w, 1.f, stream);' in s
    assert 'float* per_image = ws + (size_t)N * K * 2 * w;' in s and 'splat_rows_sum(ws, per_image, N, K, 2 * w, 1.f, stream);' in s
    assert 'splat_rows_sum(per_image, colsum, 1, N, 2 * w, 1.f, stream);' in s
    assert 'float* wn = ws + (size_t)n * (2 * w + 3 * inter);' in s and 'float *wda = wn, *wdhp = wn + 2 * w, *wdh = wdhp + inter, *wxh = wdh + inter;' in s
    assert s.count('const int OH = pool ? (H - 1) / 2 + 1 : H, OW = pool ? (W - 1) / 2 + 1 : W;') == 3
    assert 'for (int oh = ih >> 1; oh <= ((ih + 1) >> 1); ++oh) {' in s and 'if (oh >= OH) break;' in s
    assert 'for (int ow = iw >> 1; ow <= ((iw + 1) >> 1); ++ow) {' in s and 'if (ow >= OW) break;' in s
    assert s.count('(1.f / 9.f)') == 2
    assert 'const int grid = (int)(blocks < %d ? blocks : %d);' % (R.APPLY_GRID_CAP, R.APPLY_GRID_CAP) in s
    assert 'pix += (long long)gridDim.x * PP' in s and 'if (n != ncur) {' in s
    assert s.count('N <= %d' % R.N_CAP) == 3
    assert 'for (int c = lane; c < len; c += 64) s = fmaf(row[c], v[c], s);' in s and 'return wave_sum(s);' in s
    with open(os.path.join(CSRC, 'common.h')) as f:
        assert 'for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);' in f.read()
    assert s.count('dim3(SPLAT_ATTN_THREADS)') == 2 and 'for (int j = wave; j < inter; j += NW)' in s
    assert 'const float e0 = expf(a0 - m), e1 = expf(a1 - m), inv = 1.f / (e0 + e1);' in s


def test_chunk_query_agrees_with_the_restated_rule():
    from pointtinybenchmark_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(0)
    shapes = [(c[2], c[3], c[0]) for c in T.MAP_CASES + [T.STRIDE_PLAIN, T.STRIDE_POOL]]
    shapes += [(int(h), int(wd), int(4 * v)) for h, wd, v in zip(rng.integers(1, 300, 300), rng.integers(1, 300, 300), rng.integers(1, 257, 300))]
    for w in (4, 24, 64, 96, 128, 256, 512, 1000, 1024):
        shapes += [(1, R.chunk(w) * m + d, w) for m in (1, 2, 7) for d in (-1, 0, 1)]
    for H, W, w in shapes:
        assert L.cpr_splat_chunks(H, W, w) == R.chunks(H * W, w), (H, W, w)
        assert sum(R.chunk_counts(H * W, w)) == H * W
    for w in (4, 24, 96, 512):
        for HW in (1, R.chunk(w) - 1, R.chunk(w) + 1):
            seen = sorted(p for k in range(R.chunks(HW, w)) for lane in R.lane_pixels(HW, w, k) for p in lane)
            assert seen == list(range(HW))                                          # every pixel walked exactly once
    assert [R.idle_lanes(w) for w in (24, 96, 1000, 64, 1024)] == [4, 16, 6, 0, 0]


# ---- coverage --------------------------------------------------------------------------------------------------------
def test_no_state_is_unreached():
    cov = T.coverage()
    missing = [k for k in T.WANTED if not cov.get(k)]
    assert not missing, missing
    assert len({T.map_id(c) for c in T.MAP_CASES}) == len(T.MAP_CASES) and len({T.mlp_id(r) for r in T.MLP_RUNS}) == len(T.MLP_RUNS)


def test_cases_reach_the_states_claimed_for_them():
    """Re-derived from the integer rules, case by case of the table in the module docstring of the GPU file."""
    cnt = lambda c: R.chunk_counts(c[2] * c[3], c[0])         # noqa: E731
    assert (R.pp(4), cnt((4, 2, 1, 1))) == (256, [1])
    assert cnt((4, 1, 64, 65)) == [4096, 64]                                                  # second chunk: 64 pixels on 256 row lanes
    assert (R.wv(24), R.pp(24), R.idle_lanes(24)) == (6, 42, 4) and [len(x) for x in R.lane_pixels(169, 24, 0)] == [5] + [4] * 41
    assert cnt((64, 3, 16, 16)) == [256] and cnt((64, 2, 1, 257)) == [256, 1] and cnt((64, 1, 255, 1)) == [255]
    assert (R.pp(96), len(cnt((96, 2, 40, 40)))) == (10, 10)
    assert (R.pp(128), R.pp(256), R.pp(512), R.pp(1000), R.pp(1024)) == (8, 4, 2, 1, 1)
    assert {(c[2] % 2, c[3] % 2) for c in T.MAP_CASES if c[0] == 128} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for H, OH in ((17, 9), (18, 9), (23, 12), (24, 12)):
        assert R.pooled(H, H, True)[0] == OH
        wins = [R.adjoint_window(i, OH) for i in range(H)]
        assert {len(x) for x in wins} == {1, 2}
        assert (len(wins[H - 1]) == 1) and ((H % 2 == 0) == ((H >> 1) == OH))               # even: the second window of the last row is clipped
        for o in range(OH):                                                                 # the adjoint windows are the forward taps
            assert [i for i in range(H) if o in wins[i]] == [i for i in (2 * o - 1, 2 * o, 2 * o + 1) if 0 <= i < H]
    assert cnt((256, 3, 5, 13)) == [64, 1] and cnt((512, 2, 9, 7)) == [32, 31] and R.idle_lanes(1000) == 6 and len(cnt((1024, 2, 40, 40))) == 100
    assert T.MAP_CASES[-1][1] == R.N_CAP
    w, N, H, W = T.STRIDE_PLAIN
    assert (N * H * W, R.apply_grid(N * H * W, w), R.apply_reloads(N, H * W, w)) == (66248, 65536, 712)
    w, N, H, W = T.STRIDE_POOL
    OH, OW = R.pooled(H, W, True)
    assert (OH, OW, N * OH * OW - R.apply_grid(N * OH * OW, w), R.apply_reloads(N, OH * OW, w)) == (129, 129, 1028, 1028)
    for c in T.MAP_CASES:
        assert c[1] * c[2] * c[3] < 2 ** 31 and 0 < c[0] <= R.MAX_W and c[0] % 4 == 0 and c[1] <= R.N_CAP          # in-contract calls
    for (w, inter, N), _ in T.MLP_RUNS:
        assert 0 < w <= R.MAX_W and w % 4 == 0 and 0 < inter <= R.MAX_INTER


def test_pool_adjoint_is_the_autograd_adjoint():
    gen = torch.Generator().manual_seed(1)
    for H, W in ((17, 23), (18, 24), (17, 24), (18, 23), (1, 5), (2, 1), (3, 3), (1, 1)):
        x = torch.randn((2, H, W, 3), generator=gen, dtype=torch.float64, requires_grad=True)
        y = R.pool9(x)
        assert tuple(y.shape[1:3]) == R.pooled(H, W, True)
        d = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        want, = torch.autograd.grad((y * d).sum(), x)
        got, mag = R.pool9_adjoint(d, H, W)
        assert float((got - want).abs().max()) <= 1e-14 and bool((mag >= got.abs() - 1e-14).all())


# ---- emulations of the kernels' own order, numpy float32 -----------------------------------------------------------------
def fma(a, b, c):
    """fmaf: the product of two floats is exact in double, the sum is rounded to 53 bits and then to 24."""
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def mad(a, b, c, fused):
    return fma(a, b, c) if fused else (a * b + c).astype(F)


def walk(HW, w, wrong=None):
    """idx (K, S, L): the pixel lane l of chunk k reads at step s (-1: none); ok (L, WV): the lane exists in the 256-thread workgroup."""
    WV = w // 4
    P = -(-256 // WV) if wrong == 'pp_ceil' else 256 // WV
    CH = R.WALK * P
    K = R.cdiv(HW, CH)
    L = P + (1 if wrong == 'idle_merged' and 256 - P * WV else 0)
    idx = -np.ones((K, R.WALK + 1, L), np.int64)
    for k in range(K):
        end = min(HW, (k + 1) * CH)
        if wrong == 'drop_last':
            end -= 1
        if wrong == 'seam_twice' and k + 1 < K:
            end += 1
        for r in range(L):
            px = np.arange(k * CH + r, end, P)
            idx[k, :len(px), r] = px
    ok = (np.arange(L)[:, None] * WV + np.arange(WV)[None]) < 256
    return idx, ok


def chunk_reduce(step, HW, w, N, C, wrong=None):
    """step(acc, p): the accumulators (N, K, L, C) after pixel p (K, L) -> the chunk sums (N, K, C), lanes added prow ascending."""
    idx, ok = walk(HW, w, wrong)
    K, S, L = idx.shape
    okc = ok[:, (np.arange(C) % w) // 4]
    acc = np.zeros((N, K, L, C), F)
    for s in range(S):
        p = idx[:, s]
        if (p < 0).all():
            continue
        new = step(acc, np.maximum(p, 0))
        acc = np.where((p >= 0)[None, :, :, None] & okc[None, None], new, acc)
    out = acc[:, :, 0]
    for r in range(1, L):
        out = (out + np.where(okc[r], acc[:, :, r], F(0))).astype(F)
    return out


def rows_sum(p, scale=F(1)):
    s = p[:, 0]
    for r in range(1, p.shape[1]):
        s = (s + p[:, r]).astype(F)
    return (s * scale).astype(F)


def emu_dv(dout, H, W, pool, wrong=None):
    if not pool:
        return dout.reshape(dout.shape[0], H * W, -1)
    N, OH, OW, C = dout.shape
    ih, iw = np.arange(H), np.arange(W)
    if wrong == 'adj_minus':
        rows, cols = ((ih - 1) >> 1, ih >> 1), ((iw - 1) >> 1, iw >> 1)
    else:
        rows, cols = (ih >> 1, (ih + 1) >> 1), (iw >> 1, (iw + 1) >> 1)
    ext = np.concatenate([dout, np.roll(dout, -1, axis=0)[:, :1]], 1)                 # row OH: what lies behind the image in memory
    s = np.zeros((N, H, W, C), F)
    for a, oh in enumerate(rows):
        okh = (oh >= 0) & ((oh < OH) | ((wrong == 'no_oh_clip') & (oh == OH))) & ((a == 0) | (rows[1] != rows[0]))
        for b, ow in enumerate(cols):
            okw = (ow >= 0) & (ow < OW) & ((b == 0) | (cols[1] != cols[0]))
            t = ext[:, np.clip(oh, 0, OH)][:, :, np.clip(ow, 0, OW - 1)]
            s = (s + np.where((okh[:, None] & okw[None])[None, :, :, None], t, F(0))).astype(F)
    return (s * (F(1) / F(9))).astype(F).reshape(N, H * W, C)


def emu_apply(u, att, pool, fused, wrong=None):
    N, H, W, w2 = u.shape
    w = w2 // 2
    a0, a1 = att[:, 0].reshape(N, 1, 1, w), att[:, 1].reshape(N, 1, 1, w)
    if wrong == 'no_reload':                                   # image n keeps image 0's vectors
        a0, a1 = np.broadcast_to(a0[:1], a0.shape), np.broadcast_to(a1[:1], a1.shape)
    v = lambda x: mad(a0, x[..., :w], (a1 * x[..., w:]).astype(F), fused)         # noqa: E731
    if not pool:
        return v(u)
    OH, OW = R.pooled(H, W, True)
    s = np.zeros((N, OH, OW, w), F)
    taps = np.zeros((1, OH, OW, 1), F)
    for kh in range(3):
        ih = 2 * np.arange(OH) - 1 + kh
        for kw in range(3):
            iw = 2 * np.arange(OW) - 1 + kw
            ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None]
            t = v(u[:, np.clip(ih, 0, H - 1)][:, :, np.clip(iw, 0, W - 1)])
            s = (s + np.where(ok[None, :, :, None], t, F(0))).astype(F)
            taps = taps + ok[None, :, :, None]
    return (s * (F(1) / (taps if wrong == 'div_by_count' else F(9)).astype(F))).astype(F)


def emu_map(o, c, pool, fused, wrong=None):
    """Every output and workspace of the four map entries, as flat float32 torch tensors keyed like run_map's buffers."""
    w, N, H, W = c
    HW = H * W
    u, dout, att, dg = (o[k].numpy() for k in ('u', 'dout', 'att', 'dg'))
    uf = u.reshape(N, HW, 2 * w)
    G = {}
    G['ws_gap'] = chunk_reduce(lambda acc, p: (acc + (uf[:, p, :w] + uf[:, p, w:])).astype(F), HW, w, N, w, wrong)
    G['g'] = rows_sum(G['ws_gap'], F(1) / F(HW))
    G['out'] = emu_apply(u, att, pool, fused, wrong)
    dv = emu_dv(dout, H, W, pool, wrong)
    dv2 = np.concatenate([dv, dv], 2)
    G['ws_ag'] = chunk_reduce(lambda acc, p: mad(dv2[:, p], uf[:, p], acc, fused), HW, w, N, 2 * w, wrong)
    G['datt'] = rows_sum(G['ws_ag'])
    a = att.reshape(N, 1, 2 * w)
    gm = (np.concatenate([dg, dg], 1).reshape(N, 1, 2 * w) * (F(1) / F(HW))).astype(F)
    d = (a * (dv2 + gm)).astype(F) if wrong == 'dg_before_att' else mad(a, dv2, gm, fused)
    du = np.where(uf > 0, d, F(0)).astype(F)
    G['du'] = du
    part = chunk_reduce(lambda acc, p: (acc + du[:, p]).astype(F), HW, w, N, 2 * w, wrong)
    per = rows_sum(part)
    G['cs'] = rows_sum(per[None])
    G['ws_ab'] = np.concatenate([part.reshape(-1), per.reshape(-1)])
    return {k: torch.from_numpy(np.ascontiguousarray(v, F).reshape(-1)) for k, v in G.items()}


def row_dot(M, v):
    """M (rows, len), v (N, len) -> (N, rows): lanes stride over the columns by 64 with fmaf, then the xor butterfly 32 .. 1."""
    rows, n = M.shape
    T_ = R.cdiv(n, 64)
    Mp = np.zeros((rows, T_ * 64), F)
    Mp[:, :n] = M
    vp = np.zeros((v.shape[0], T_ * 64), F)
    vp[:, :n] = v
    s = np.zeros((v.shape[0], rows, 64), F)
    for t in range(T_):
        s = fma(Mp[None, :, t * 64:(t + 1) * 64], vp[:, None, t * 64:(t + 1) * 64], s)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, :, lane ^ o]).astype(F)
    assert bool((s == s[:, :, :1]).all())                      # every lane holds the same sum
    return s[:, :, 0]


def emu_attn(o, shape, wrong=None):
    w, inter, N = shape
    p = {k: v.numpy() for k, v in o.items()}
    h = (row_dot(p['fc1_w'], p['g']) + p['fc1_b']).astype(F)
    z = np.maximum(fma(p['s1'], h, p['t1']), F(0))
    a = (row_dot(p['fc2_w'], z) + p['fc2_b']).astype(F)
    a0, a1 = a[:, :w], a[:, w:]
    m = F(0) if wrong == 'no_max' else np.maximum(a0, a1)
    with np.errstate(over='ignore', invalid='ignore'):
        e0, e1 = np.exp((a0 - m).astype(F)).astype(F), np.exp((a1 - m).astype(F)).astype(F)
        inv = (F(1) / (e0 + e1)).astype(F)
        att = np.stack([e0 * inv, e1 * inv], 1).astype(F)
    return dict(att=torch.from_numpy(att.reshape(-1)), z=torch.from_numpy(z.reshape(-1).copy())), h


def emu_attn_bwd(o, att, z, shape, fused, wrong=None):
    w, inter, N = shape
    p = {k: v.numpy() for k, v in o.items()}
    att, z = att.numpy().reshape(N, 2, w), z.numpy().reshape(N, inter)
    a0, a1, d0, d1 = att[:, 0], att[:, 1], p['datt'][:, 0], p['datt'][:, 1]
    s = F(0) if wrong == 'no_s' else mad(a0, d0, (a1 * d1).astype(F), fused)
    da = np.concatenate([a0 * (d0 - s), a1 * (d1 - s)], 1).astype(F)
    h = (row_dot(p['fc1_w'], p['g']) + p['fc1_b']).astype(F)
    if wrong == 'xhat_post_bn':
        h = fma(p['s1'], h, p['t1'])
    xh = ((h - p['mean']) * p['inv']).astype(F)
    sdz = np.zeros((N, inter), F)
    for k in range(2 * w):
        sdz = fma(p['fc2_w'][k][None], da[:, k:k + 1], sdz)
    dhp = np.where(z > 0, sdz, F(0)).astype(F)
    dh = (p['s1'] * dhp).astype(F)
    dg = np.zeros((N, w), F)
    for j in range(inter):
        dg = fma(p['fc1_w'][j][None], dh[:, j:j + 1], dg)
    order = range(N - 1, -1, -1) if wrong == 'desc_order' else range(N)

    def total(a, b=None):
        t = np.zeros(a.shape[1:] if b is None else (a.shape[1], b.shape[1]), F)
        for n in order:
            t = (t + a[n]).astype(F) if b is None else fma(a[n][:, None], b[n][None], t)
        return t
    G = dict(dg=dg, ws=np.concatenate([da, dhp, dh, xh], 1), fc2_w=total(da, z), fc2_b=total(da), fc1_w=total(dh, p['g']), fc1_b=total(dh),
             bn_w=total_fma(dhp, xh, order), bn_b=total(dhp))
    return {k: torch.from_numpy(np.ascontiguousarray(v, F).reshape(-1)) for k, v in G.items()}


def total_fma(a, b, order):
    t = np.zeros(a.shape[1:], F)
    for n in order:
        t = fma(a[n], b[n], t)
    return t


@pytest.fixture(autouse=True)
def _keep_the_gpu_files_log():
    saved = dict(T.WORST)
    yield
    T.WORST.clear()
    T.WORST.update(saved)


def note(qs, worst=LOG):
    for k, v in qs.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize('c', SMALL_MAPS, ids=T.map_id)
def test_map_emulations_stay_below_half_of_every_bar(c):
    for pool in T.POOLS:
        o = T.map_operands(c, pool)
        for fused in (False, True):
            qs = T.judge_map('emulation %s pool=%d fused=%d' % (T.map_id(c), pool, fused), o, emu_map(o, c, pool, fused), c, pool)
            note(qs)
            n_final = R.chunks(c[2] * c[3], c[0]) + 1
            for k, v in qs.items():
                # gap final counts its n = K + 1 roundings exactly: for 4 < n < 16 such a bar can be met to the whole (0.70 at K = 4)
                assert v <= (1.0 if k == 'gap final' and 4 < n_final < 16 else 0.5), (k, v, qs)


def test_the_colsum_chain_of_the_largest_batch_stays_below_half_of_its_bar():
    c = T.MAP_CASES[-1]
    w, N, H, W = c
    o = T.map_operands(c, False)
    att, dv, gm = o['att'].numpy().reshape(N, 2 * w), o['dout'].numpy().reshape(N, w), o['dg'].numpy()            # HW 1: dg / HW is dg
    d = fma(att, np.concatenate([dv, dv], 1), np.concatenate([gm, gm], 1))
    per = np.where(o['u'].numpy().reshape(N, 2 * w) > 0, d, F(0)).astype(F)             # one pixel: the per-image sum is du itself
    cs = rows_sum(per[None])
    ref, bar = R.rows_sum_ref(torch.from_numpy(per).double().view(1, N, 2 * w))
    q = float(R.ratio(torch.from_numpy(cs), ref, bar).max())
    note({'apply_bwd colsum, N 65535': q})
    assert q <= 0.5, q


@pytest.mark.parametrize('run', T.MLP_RUNS, ids=T.mlp_id)
def test_mlp_emulations_stay_below_half_of_every_bar(run):
    shape, variant = run
    o = T.mlp_operands(shape, variant)
    A, _ = emu_attn(o, shape)
    name = 'emulation ' + T.mlp_id(run)
    qs = T.judge_attn(name, o, A, shape, variant)
    a64, _ = R.logits_ref(A['z'].double().view(shape[2], -1), o['fc2_w'].double(), o['fc2_b'].double())
    spread = float((a64[:, :shape[0]] - a64[:, shape[0]:]).abs().max())
    soft = ('attn att', 'attn end to end', 'attn att, a == b2')
    assert (spread > 8) == (variant in ('pm60', 'pm200', 'spread60')), (name, spread)
    for k, v in qs.items():
        assert v <= (1.0 if k in soft and spread > 8 else 0.5), (name, k, v)
    note({k + (' (|a0 - a1| > 8)' if k in soft and spread > 8 else ''): v for k, v in qs.items()})
    for fused in (False, True):
        qb = T.judge_attn_bwd(name, o, A['att'], A['z'].view(shape[2], -1), emu_attn_bwd(o, A['att'], A['z'], shape, fused), shape)
        note(qb)
        assert all(v <= 0.5 for v in qb.values()), (name, qb)


# ---- wrong emulations: each fails, and only at elements it changes --------------------------------------------------------------
def verdict(got, right, ref, bar):
    """(failing, changed) boolean maps of a wrong emulation: it must fail somewhere, only where its bits differ from the right
    emulation's, and wherever it moved an element by more than 1.5 bars."""
    got, right = got.reshape(ref.shape), right.reshape(ref.shape)
    fail = ~(R.ratio(got, ref, bar) <= 1.0)
    changed = got.view(torch.int32) != right.view(torch.int32)
    assert bool(fail.any()), 'the wrong emulation passes'
    assert not bool((fail & ~changed).any()), 'an unchanged element fails'
    assert not bool(((got.double() - right.double()).abs() > 1.5 * bar).logical_and(~fail).any())
    assert bool((R.ratio(right, ref, bar) <= 0.5).all())
    return fail, changed


def _maps(c, pool, wrong):
    o = T.map_operands(c, pool)
    return o, {k: v.double() for k, v in o.items()}, emu_map(o, c, pool, True), emu_map(o, c, pool, True, wrong)


@pytest.mark.parametrize('wrong,c', [('drop_last', (64, 2, 1, 257)), ('seam_twice', (96, 2, 40, 40)), ('idle_merged', (24, 3, 13, 13)),
                                     ('pp_ceil', (24, 3, 13, 13))])
def test_wrong_walks_fail_at_the_partials_they_change(wrong, c):
    w, N, H, W = c
    o, d, right, bad = _maps(c, False, wrong)
    K = R.chunks(H * W, w)
    ref, bar = R.gap_partial_ref(d['u'].view(N, H * W, 2 * w), w)
    fail, changed = verdict(bad['ws_gap'], right['ws_gap'], ref, bar)
    if wrong == 'idle_merged':                 # only the channel quads the four idle lanes own
        assert not bool(changed[..., 4 * R.idle_lanes(w):].any()) and bool(fail[..., :4 * R.idle_lanes(w)].any())
    if wrong == 'pp_ceil':                     # lane 42 exists only for those quads: every other channel loses pixels
        assert bool(fail[..., 4 * R.idle_lanes(w):].any())
    if wrong == 'seam_twice':
        assert not bool(changed[:, K - 1].any())
    if wrong == 'drop_last':                   # a dropped pixel is missed wherever it was not zero
        lastpix = d['u'].view(N, H * W, 2 * w)[:, [min(H * W, (k + 1) * R.chunk(w)) - 1 for k in range(K)]]
        there = (lastpix[..., :w] + lastpix[..., w:]) != 0
        assert not bool((fail & ~there).any()) and int(fail.sum()) >= 0.95 * int(there.sum())
    # the same walks under the other two reductions
    ref, bar = R.attn_grad_partial_ref(d['dout'], d['u'], False)
    verdict(bad['ws_ag'], right['ws_ag'], ref, bar)
    nk = N * K * 2 * w
    ref, bar = R.du_partial_ref(right['du'].double().view(N, H * W, 2 * w), w)
    verdict(bad['ws_ab'][:nk], right['ws_ab'][:nk], ref, bar)


def test_wrong_pool_divisor_fails_at_the_border_outputs():
    c = (128, 3, 17, 23)
    o, d, right, bad = _maps(c, True, 'div_by_count')
    ref, bar = R.apply_ref(d['u'], d['att'], True)
    fail, changed = verdict(bad['out'], right['out'], ref, bar)
    assert not bool(changed[:, 1:-1, 1:-1].any())                     # odd sizes: the first and the last window of a row or column are cut
    assert all(bool(f.any()) for f in (fail[:, 0], fail[:, -1], fail[:, :, 0], fail[:, :, -1]))


@pytest.mark.parametrize('wrong,c', [('adj_minus', (128, 3, 18, 24)), ('no_oh_clip', (128, 3, 18, 24)), ('no_oh_clip', (128, 2, 18, 23)),
                                     ('dg_before_att', (256, 3, 5, 13))])
def test_wrong_adjoints_fail_at_the_pixels_they_change(wrong, c):
    w, N, H, W = c
    pool = wrong != 'dg_before_att'
    o, d, right, bad = _maps(c, pool, wrong)
    ref, bar, keep = R.du_ref(d['dout'], d['u'], d['att'], d['dg'], pool)
    fail, changed = verdict(bad['du'], right['du'], ref, bar)
    fail, changed = fail.view(N, H, W, 2 * w), changed.view(N, H, W, 2 * w)
    if wrong == 'no_oh_clip':
        assert not bool(changed[:, :H - 1].any()) and bool(fail[:, H - 1].any())                            # the last row of an even H alone
    assert not bool((changed & ~keep.view(N, H, W, 2 * w)).any())
    if pool:
        ref, bar = R.attn_grad_partial_ref(d['dout'], d['u'], True)
        verdict(bad['ws_ag'], right['ws_ag'], ref, bar)


def test_clip_at_an_odd_height_changes_nothing():
    c = (128, 3, 17, 23)
    o = T.map_operands(c, True)
    a, b = emu_map(o, c, True, True), emu_map(o, c, True, True, 'no_oh_clip')
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_attention_vectors_not_reloaded_fail_at_every_pixel_of_the_later_image():
    """The second-trip pixels of the grid-stride case lie in image 1; a lane that keeps image 0's vectors fails there."""
    gen = torch.Generator().manual_seed(5)
    w, rows = 1024, 712
    u = torch.relu(torch.randn((2, 1, rows, 2 * w), generator=gen))
    att = torch.softmax(torch.randn((2, 2, w), generator=gen), 1)
    right, bad = emu_apply(u.numpy(), att.numpy(), False, True), emu_apply(u.numpy(), att.numpy(), False, True, 'no_reload')
    ref, bar = R.apply_ref(u.double(), att.double(), False)
    fail, changed = verdict(torch.from_numpy(bad), torch.from_numpy(right), ref, bar)
    assert not bool(changed[0].any()) and float(fail[1].double().mean()) > 0.7        # all but the quarter where both splits are zero


def test_wrong_mlp_emulations():
    shape = T.VARIANT_SHAPE
    w, inter, N = shape
    failed = {}
    for run in T.MLP_RUNS:
        if run[0][0] * run[0][1] > 70000:
            continue
        o = T.mlp_operands(*run)
        A, _ = emu_attn(o, run[0], 'no_max')
        try:
            T.judge_attn('no_max ' + T.mlp_id(run), o, A, run[0], None)
            failed.setdefault(run[1], False)
        except AssertionError:
            failed[run[1]] = True
    # without the maximum subtracted: exp(60) = 1.1e26 is finite in fp32 and e0 / (e0 + e1) lands inside the bar; exp(200) is not
    assert failed == {None: False, 'tie': False, 'zeroz': False, 'pm60': False, 'pm200': True, 'spread60': False}, failed
    o = T.mlp_operands(shape, 'spread60')
    o['fc2_b'] = o['fc2_b'] * 2.5                                         # logits up to +-97: exp overflows
    A, _ = emu_attn(o, shape, 'no_max')
    with pytest.raises(AssertionError):
        T.judge_attn('no_max, logits to +-97', o, A, shape, None)
    T.judge_attn('logits to +-97', o, emu_attn(o, shape)[0], shape, None)
    o = T.mlp_operands(shape)
    d = {k: v.double() for k, v in o.items()}
    A, _ = emu_attn(o, shape)
    right = emu_attn_bwd(o, A['att'], A['z'], shape, True)
    rec = lambda G: G['ws'].view(N, 2 * w + 3 * inter)         # noqa: E731
    bad = emu_attn_bwd(o, A['att'], A['z'], shape, True, 'no_s')
    ref, bar = R.da_ref(A['att'].double().view(N, 2, w), d['datt'])
    verdict(rec(bad)[:, :2 * w].contiguous(), rec(right)[:, :2 * w].contiguous(), ref, bar)
    bad = emu_attn_bwd(o, A['att'], A['z'], shape, True, 'xhat_post_bn')
    ref, bar = R.xhat_ref(d['g'], d['fc1_w'], d['fc1_b'], d['mean'], d['inv'])
    fail, _ = verdict(rec(bad)[:, 2 * w + 2 * inter:].contiguous(), rec(right)[:, 2 * w + 2 * inter:].contiguous(), ref, bar)
    assert bool(fail.all())
    # the bars of the parameter sums are order-free: images in descending order pass
    desc = emu_attn_bwd(o, A['att'], A['z'], shape, True, 'desc_order')
    assert any(not torch.equal(desc[k], right[k]) for k in T.GRADS)
    T.judge_attn_bwd('descending images', o, A['att'], A['z'].view(N, inter), desc, shape)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    T.test_entry_points_refuse_bad_arguments_before_any_launch()


def test_print_worst_emulation_ratio_per_stage():
    for k in sorted(LOG):
        print('SPLAT emulation worst |err| / bar  %-36s %.4f' % (k, LOG[k]))
