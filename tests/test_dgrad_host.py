"""CPU checks that keep tests/test_gpu_dgrad.py honest: the three forms of the fp64 data-gradient reference agree, every case's
expected route follows from the restated rules, the case table meets its conditions, and the bars catch the faults they exist for
(a correct fp32 computation passes them; a flipped tap, a dropped scale and a dropped row block fail)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dgrad_fp64_ref as D
from tests.conv_fp64_ref import sample_pixels
from tests.test_gpu_dgrad import CASES, ROUTES, case_id, flags, make_inputs, make_mask, predict_route

KSP = sorted({c[5:8] for c in CASES})
MAPS = [(2, 7, 6), (2, 6, 7), (1, 1, 5), (2, 3, 2)]       # odd x even, even x odd, one row, smaller than the taps


@pytest.mark.parametrize('ksp', KSP, ids=lambda t: 'k%d_s%d_p%d' % t)
def test_reference_forms_agree(ksp):
    k, s, p = ksp
    for N, H, W in MAPS:
        g = torch.Generator().manual_seed(H * 31 + W)
        OH, OW = D.out_hw(H, W, k, s, p)
        dy = torch.randn((N, OH, OW, 5), generator=g)
        ws = D.scaled_weights(torch.randn((5, 3, k, k), generator=g), torch.rand(5, generator=g) + 0.5)
        t, mag = D.full_map(dy, ws, s, p, (H, W))
        m = np.arange(N * H * W)
        for name, (t2, mag2) in (('gather', D.gather(dy, ws, s, p, (H, W), m)), ('tap_scatter', D.tap_scatter(dy, ws, s, p, (H, W)))):
            assert bool(((t2 - t).abs() <= 1e-12 * mag).all()), (name, ksp, H, W)
            assert bool(((mag2 - mag).abs() <= 1e-12 * mag).all()), (name, ksp, H, W)
        assert float(mag.max()) > 0
        sub = m[::3]
        t3, _ = D.gather(dy, ws, s, p, (H, W), sub)
        assert torch.equal(t3, D.gather(dy, ws, s, p, (H, W), m)[0][::3])


def test_reference_is_the_forward_definition():
    """The literal sum of the module docstring, in Python loops, on one strided and one padded shape."""
    for k, s, p, H, W in ((3, 2, 1, 5, 4), (1, 2, 0, 4, 4), (3, 1, 1, 3, 4)):
        g = torch.Generator().manual_seed(k + s)
        OH, OW = D.out_hw(H, W, k, s, p)
        dy = torch.randn((1, OH, OW, 2), generator=g)
        w = torch.randn((2, 3, k, k), generator=g)
        scale = torch.rand(2, generator=g) + 0.5
        ref = torch.zeros((H, W, 3), dtype=torch.float64)
        for oy in range(OH):
            for ox in range(OW):
                for kh in range(k):
                    for kw in range(k):
                        iy, ix = oy * s - p + kh, ox * s - p + kw
                        if 0 <= iy < H and 0 <= ix < W:
                            for co in range(2):
                                ref[iy, ix] += dy[0, oy, ox, co].double() * w[co, :, kh, kw].double() * scale[co].double()
        t, _ = D.full_map(dy, D.scaled_weights(w, scale), s, p, (H, W))
        assert torch.allclose(t, ref.reshape(-1, 3), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize('i', range(len(CASES)), ids=lambda i: case_id(CASES[i]))
def test_case_expects_the_route_the_rules_give(i):
    c = CASES[i]
    assert predict_route(c)[0] == c[9], (c, predict_route(c))


def test_every_route_has_a_case():
    seen = {c[9] for c in CASES}
    assert seen == set(ROUTES), (sorted(set(ROUTES) - seen), sorted(seen - set(ROUTES)))
    assert any(c[9] == 'zero-insert' and c[5] == 3 for c in CASES) and any('fused' in flags(c) for c in CASES)


def test_strided_geometries_run_on_two_images():
    """The phase scatter and the zero insertion step over images: every strided (conv, map) is run with N >= 2 (the one-row map is
    also kept at the single image the parity-class case was stated for)."""
    for c in CASES:
        if c[6] > 1:
            assert any(d[0] >= 2 and d[1:8] == c[1:8] and ('nophase' in flags(d)) == ('nophase' in flags(c)) for d in CASES), c


def test_masks_keep_about_half_and_hold_both_zeros():
    seen = 0
    for c in CASES:
        f = flags(c)
        if 'mask' not in f and 'fused' not in f:
            continue
        seen += 1
        m = make_mask(c).float()
        keep = float((m > 0).float().mean())
        assert 0.25 <= keep <= 0.75, (c, keep)
        sign = torch.signbit(m)
        assert bool(((m == 0) & ~sign).any()) and bool(((m == 0) & sign).any()) and bool((m > 0).any()), c
        assert not bool((m < 0).any())
    assert seen >= 10


# ---- bar sensitivity: an fp32 data gradient computed by torch on the CPU stands in for the kernel -------------------------------
def _emulated(c, inp, w=None, scale='same'):
    """fp32 dx (N * H * W, Cin) by CPU autograd of the fp32 forward, with the scale folded in fp32 as the pack folds it."""
    N, Cin, H, W, Cout, k, s, p = c[:8]
    w = inp['w'] if w is None else w
    sc = inp['scale'] if scale == 'same' else scale
    ws = w if sc is None else w * sc.view(-1, 1, 1, 1)
    x = torch.zeros((N, Cin, H, W), requires_grad=True)
    dx, = torch.autograd.grad(F.conv2d(x, ws, None, s, p), x, inp['dy'].permute(0, 3, 1, 2))
    dx = dx.permute(0, 2, 3, 1)
    if inp['add'] is not None:
        dx = dx + inp['add']
    if inp['mask'] is not None:
        dx = torch.where(inp['mask'] > 0, dx, torch.zeros_like(dx))
    return dx.reshape(-1, Cin)


def _ref(c, inp):
    N, Cin, H, W, Cout, k, s, p = c[:8]
    t, mag = D.full_map(inp['dy'], D.scaled_weights(inp['w'], inp['scale']), s, p, (H, W))
    return D.finish(t, mag, None if inp['add'] is None else D.rows(inp['add']), None if inp['mask'] is None else D.rows(inp['mask']),
                    scaled=inp['scale'] is not None)


def _passes(got, r):
    try:
        D.check('emulated', got.double(), r['ref'], r['bar32'])
        return True
    except AssertionError:
        return False


SENS = [c for c in CASES if c[8] in ('scale mask colsum', 'scale add') and c[:8] in ((2, 128, 17, 14, 128, 3, 2, 1), (2, 64, 17, 15, 96, 3, 1, 1),
                                                                                 (3, 256, 13, 11, 64, 1, 1, 0))]


def test_bars_pass_fp32_and_catch_pack_and_block_faults():
    assert len(SENS) >= 4
    for c in SENS:
        inp = make_inputs(c)
        r = _ref(c, inp)
        good = _emulated(c, inp)
        assert good.dtype == torch.float32 and _passes(good, r), c
        assert not _passes(_emulated(c, inp, scale=None), r), c                       # the scale multiply dropped
        s2 = inp['scale'].clone()
        s2[5] = s2[5] * (1 + 2.0 ** -12)
        assert not _passes(_emulated(c, inp, scale=s2), r), c                         # one channel's scale off by 2^-12
        if c[5] == 3:
            w2 = inp['w'].clone()
            w2[:, :, 0, 0], w2[:, :, 0, 2] = inp['w'][:, :, 0, 2], inp['w'][:, :, 0, 0]
            assert not _passes(_emulated(c, inp, w=w2), r), c                         # one tap index flipped
        cref, cbar = D.colsum_ref(r)
        cs = good.sum(0)
        assert bool(((cs.double() - cref).abs() <= cbar).all()), c
        M = good.shape[0]
        short = good[:M - 1].sum(0)                                                   # the last pixel not counted
        assert not bool(((short.double() - cref).abs() <= cbar).all()), c
        m, slots = sample_pixels(c[0], c[2], c[3], 64, slot=64)
        rs = dict(ref=r['ref'][torch.as_tensor(m)], bar32=r['bar32'][torch.as_tensor(m)])
        sref, sbar = D.slot_colsum_refs(rs, m, slots, 64, M)
        aref, abar = D.all_slot_colsum_refs(r, 64)                                    # the every-slot form: the same sums and bars
        assert aref.shape[0] == (M + 63) // 64 and M % 64 != 0
        assert torch.allclose(aref[slots], sref, rtol=1e-12, atol=1e-15) and torch.allclose(abar[slots], sbar, rtol=1e-12, atol=1e-30)
        for i, sl in enumerate(slots):
            v = good[sl * 64:min(sl * 64 + 64, M)]
            assert bool(((v.sum(0).double() - sref[i]).abs() <= sbar[i]).all()), (c, sl)
            assert not bool(((v[:-1].sum(0).double() - sref[i]).abs() <= sbar[i]).all()), (c, sl)      # a mis-sized last slot


def test_never_read_pixels_have_a_zero_bar():
    """1x1 / stride 2 on an even map: no tap reaches an odd row or column, so mag and the bar are 0 there (one ulp of the add)."""
    c = next(c for c in CASES if c[:8] == (2, 256, 14, 16, 512, 1, 2, 0) and c[8] == 'add')
    inp = make_inputs(c)
    r = _ref(c, inp)
    N, Cin, H, W = c[:4]
    bar = r['bar32'].reshape(N, H, W, Cin)
    ref = r['ref'].reshape(N, H, W, Cin)
    assert torch.equal(ref[:, 1::2], inp['add'].double()[:, 1::2]) and torch.equal(ref[:, :, 1::2], inp['add'].double()[:, :, 1::2])
    assert torch.equal(bar[:, 1::2], D.ULP32 * ref[:, 1::2].abs())
