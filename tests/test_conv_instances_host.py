"""CPU checks that keep tests/test_gpu_conv_instances.py honest: every instance the forward launchers can choose has a case, each
case's expected variant word follows from the dispatch rules, and the fp64 bars of tests/conv_fp64_ref.py catch the faults they
exist for (a correct fp32 / bf16 computation passes them, the deliberately wrong ones below fail)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_fp64_ref as R
from tests.test_gpu_conv_instances import ALL_CASES, CASES, INSTANCES, predict_variant, slot_pixels


def test_every_instance_has_a_case():
    seen = {c['want'] for c in ALL_CASES}
    missing = [i for i in INSTANCES if i not in seen]
    assert not missing, 'instances without a case: %r' % missing
    unknown = sorted(seen - set(INSTANCES))
    assert not unknown, 'cases expect instances missing from INSTANCES: %r' % unknown


@pytest.mark.parametrize('i', range(len(ALL_CASES)))
def test_case_expects_what_the_dispatch_rule_chooses(i):
    c = ALL_CASES[i]
    assert predict_variant(c) == c['want'], (c, predict_variant(c))


def test_cases_stay_below_the_chunking_threshold():
    """Chunked launches (>= 2 GiB per tensor) belong to test_gpu_fullsize.py; these launches are single."""
    for c in CASES:
        OH = (c['H'] + 2 * c['p'] - c['k']) // c['s'] + 1
        OW = (c['W'] + 2 * c['p'] - c['k']) // c['s'] + 1
        e = 2 if c['kind'] == 'bf16' else 4
        biggest = max(c['N'] * c['H'] * c['W'] * c['Cin'] * e, c['N'] * OH * OW * c['Cout'] * 4)
        assert biggest < (1 << 30), c


def test_every_edge_kind_is_covered_per_fp32_tile():
    """Per fp32 tiled instance: a ragged last M tile and a Cout that is not a multiple of the tile edge, where the kernel admits it."""
    for want in INSTANCES:
        cs = [c for c in CASES if c['want'] == want]
        if want[0] != 'fp32' or want[1] % 10 == 3 or not cs:      # the streamed kernel takes whole tiles only
            continue
        bm, bn = want[1] // 1000000, want[1] // 1000 % 1000
        ragged_m = any((c['N'] * ((c['H'] + 2 * c['p'] - c['k']) // c['s'] + 1) * ((c['W'] + 2 * c['p'] - c['k']) // c['s'] + 1))
                       % bm for c in cs)
        ragged_n = any(c['Cout'] % bn for c in cs)
        whole = all({'gn', 'inab'} & set(c['flags'].split()) for c in cs)   # these need OH * OW % 128 == 0: never ragged
        assert ragged_n, want
        assert ragged_m or whole, want


# ---- bar sensitivity --------------------------------------------------------------------------------------------------------
N, H, W, CIN, COUT, K, S, P, BM = 2, 13, 11, 64, 96, 3, 1, 1, 64


def _problem(seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, CIN), generator=g)
    w = torch.randn((COUT, CIN, K, K), generator=g) / (CIN * K * K) ** 0.5
    sc = torch.rand(COUT, generator=g) + 0.5
    bi = torch.randn(COUT, generator=g)
    res = torch.randn((N, H, W, COUT), generator=g)
    return x, w, sc, bi, res


def _conv64(x, w, sc, bi, res, relu=True):
    """Whole fp64 output (N*OH*OW, Cout) of the problem, an exact 'kernel' to corrupt."""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, S, P)
    y = y * sc.double()[None, :, None, None] + bi.double()[None, :, None, None]
    y = y.permute(0, 2, 3, 1) + res.double()
    if relu:
        y = y.clamp_min(0)
    return y.reshape(-1, COUT)


def _ref(x, w, sc, bi, res):
    m, _ = R.sample_pixels(N, H, W, BM, n_random=100)
    return m, R.reference(x, w, S, P, m, scale=sc, bias=bi, residual=res, relu=True)


def _passes(got_all, m, r, bf16=False):
    try:
        R.check('emulated', got_all[torch.as_tensor(m)], r['ref'], R.out_bar(r, bf16), m=m, bm=BM, OHW=(H, W))
        return True
    except AssertionError:
        return False


def test_sample_set_holds_the_tile_edges():
    m, slots = R.sample_pixels(N, H, W, BM, slot=128)
    M = N * H * W
    s = set(m.tolist())
    assert set(range((M - 1) // BM * BM, M)) <= s                 # the last, ragged M tile
    t0 = (H * W) // BM * BM
    assert set(range(t0, t0 + BM)) <= s                            # the tile across the image boundary
    for n in (0, N - 1):
        for oy in range(H):
            for ox in range(W):
                if oy in (0, H - 1) or ox in (0, W - 1):
                    assert n * H * W + oy * W + ox in s
    assert 0 in slots and (M - 1) // 128 in slots
    for sl in slots:
        assert set(range(sl * 128, min(sl * 128 + 128, M))) <= s


def test_fp32_computation_passes_the_fp32_bar():
    x, w, sc, bi, res = _problem()
    m, r = _ref(x, w, sc, bi, res)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, S, P) * sc[None, :, None, None] + bi[None, :, None, None]
    y = (y.permute(0, 2, 3, 1) + res).clamp_min(0).reshape(-1, COUT)
    assert y.dtype == torch.float32
    assert _passes(y.double(), m, r)
    assert _passes(y.bfloat16().double(), m, r, bf16=True)        # round-to-nearest-even bf16 store of it


def test_bar_catches_one_dropped_k_element():
    x, w, sc, bi, res = _problem()
    m, r = _ref(x, w, sc, bi, res)
    w2 = w.clone()
    w2[:, 37, 2, 1] = 0                                            # one (tap, channel) product missing from every output
    assert not _passes(_conv64(x, w2, sc, bi, res), m, r)


def test_bar_catches_one_dropped_32_channel_chunk():
    x, w, sc, bi, res = _problem()
    m, r = _ref(x, w, sc, bi, res)
    w2 = w.clone()
    w2[:, 32:64, 1, 1] = 0                                         # the second K chunk of the centre tap
    assert not _passes(_conv64(x, w2, sc, bi, res), m, r)


def test_bar_catches_the_ragged_tile_shifted_by_one_pixel():
    x, w, sc, bi, res = _problem()
    m, r = _ref(x, w, sc, bi, res)
    y = _conv64(x, w, sc, bi, res)
    M = N * H * W
    last = (M - 1) // BM * BM
    assert M % BM != 0
    y2 = y.clone()
    y2[last:M - 1] = y[last + 1:M]                                 # rows of the last tile read one pixel late
    assert not _passes(y2, m, r)
    y3 = y.clone()
    y3[last + 1:M] = y[last:M - 1]                                 # ... or one pixel early
    assert not _passes(y3, m, r)


def test_bar_catches_bias_on_the_wrong_channel():
    x, w, sc, bi, res = _problem()
    m, r = _ref(x, w, sc, bi, res)
    b2 = bi.clone()
    b2[64], b2[65] = bi[65], bi[64]                                # channels 64 / 65 (the second cout tile) swapped
    assert not _passes(_conv64(x, w, sc, b2, res), m, r)


def test_bar_catches_bf16_truncation():
    x, w, sc, bi, res = _problem()
    m, r = _ref(x, w, sc, bi, res)
    y = _conv64(x, w, sc, bi, res).float()
    trunc = (y.view(torch.int32) & ~0xFFFF).view(torch.float32)    # bf16 by dropping the low 16 bits
    assert _passes(y.bfloat16().double(), m, r, bf16=True)
    assert not _passes(trunc.double(), m, r, bf16=True)


def test_slot_bars_pass_fp32_sums_and_catch_a_missing_pixel():
    x, w, sc, bi, res = _problem()
    M = N * H * W
    m, slots = R.sample_pixels(N, H, W, BM, slot=BM, n_random=50)
    r = R.reference(x, w, S, P, m, scale=sc, bias=bi, residual=res, relu=True)
    y = _conv64(x, w, sc, bi, res).float()
    sref, sbar = R.slot_refs(r, m, slots, BM, M)
    for s_i, sl in enumerate(slots):
        v = y[sl * BM:min(sl * BM + BM, M)]
        got = torch.stack([v.sum(0), (v * v).sum(0)], -1).double()
        assert bool(((got - sref[s_i]).abs() <= sbar[s_i]).all())
        v2 = v[:-1]                                                # the slot's last pixel not counted
        bad = torch.stack([v2.sum(0), (v2 * v2).sum(0)], -1).double()
        assert not bool(((bad - sref[s_i]).abs() <= sbar[s_i]).all())


def test_slot_pixels_follow_the_instance():
    for c in ALL_CASES:
        sp = slot_pixels(c, c['want'])
        if 'gn' in c['flags'].split():
            assert sp == 128
        elif sp is not None:
            assert sp in (64, 128)


def test_in_ab_reference_zero_pads_after_the_affine():
    """The fused input affine applies to real pixels only; a padded tap reads 0, not relu(b)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 4, 5, 32), generator=g)
    w = torch.randn((8, 32, 3, 3), generator=g)
    a, b = torch.rand((1, 32), generator=g) + 0.5, torch.rand((1, 32), generator=g) + 1.0
    m = np.arange(20)
    r = R.reference(x, w, 1, 1, m, in_ab=(a, b), in_relu=True)
    xa = (x.double() * a.double().view(1, 1, 1, -1) + b.double().view(1, 1, 1, -1)).clamp_min(0)
    ref = F.conv2d(xa.permute(0, 3, 1, 2), w.double(), None, 1, 1).permute(0, 2, 3, 1).reshape(-1, 8)
    assert torch.allclose(r['ref'], ref, rtol=1e-12, atol=1e-12)


def test_dual_reference_matches_two_convolutions():
    g = torch.Generator().manual_seed(6)
    x = torch.randn((2, 5, 7, 32), generator=g)
    x2 = torch.randn((2, 9, 13, 64), generator=g)
    w = torch.randn((16, 32, 1, 1), generator=g)
    w2 = torch.randn((16, 64, 1, 1), generator=g)
    m = np.arange(70)
    r = R.reference(x, w, 1, 0, m, src2=(x2, w2, 2, None, None))
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double()) + F.conv2d(x2.double().permute(0, 3, 1, 2), w2.double(), None, 2)
    assert torch.allclose(r['ref'], ref.permute(0, 2, 3, 1).reshape(-1, 16), rtol=1e-12, atol=1e-12)
