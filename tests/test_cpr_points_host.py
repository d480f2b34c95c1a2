"""CPU only: the table of tests/test_gpu_cpr_points.py reaches every state it is there for (asserted from the table, the
references' own coverage figures and the constants read from csrc/cpr_points.hip), the fp64 references of
tests/cpr_points_fp64_ref.py agree with the fp32 functions of oracle/cpr_oracle.py inside their bars, the references alone keep
every case's ambiguous share inside the cap (none in the exact cases), the bars pass fp32 emulations of the kernels' formulas
and fail each wrong variant they are there for, and the entry points refuse the arguments that would reach a bad launch."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import cpr_oracle as O
from tests import cpr_points_fp64_ref as R
from tests.test_gpu_cpr_points import BY_NAME, CASES, make_inputs, of, reference

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
ERR_ARG = -1001
_CACHE = {}


def setup_module(module):
    torch.set_num_threads(min(16, torch.get_num_threads()))


def case(name):
    """(case, inputs, reference) of one table row, computed once and shared (never modified)."""
    if name not in _CACHE:
        c = BY_NAME[name]
        i = make_inputs(c)
        _CACHE[name] = (c, i, reference(c, i))
    return _CACHE[name]


def _src():
    with open(os.path.join(CSRC, 'cpr_points.hip')) as f:
        return f.read()


def _const(text, name):
    m = re.search(r'(?:#define|constexpr int)\s+%s\s*=?\s*(\d+)' % name, text) or re.search(r'%s = (\d+)' % name, text)
    return int(m.group(1))


def constants():
    t = _src()
    return dict(MAX_GT_LDS=_const(t, 'MAX_GT_LDS'), MIL_NW=_const(t, 'MIL_NW'), MIL_MAXT=_const(t, 'MIL_MAXT'))


# ---- constants and launch rules --------------------------------------------------------------------------------------------
def test_constants_and_launch_rules_are_the_source():
    t = _src()
    k = constants()
    assert k == dict(MAX_GT_LDS=1024, MIL_NW=8, MIL_MAXT=512)
    assert 'if (!allpos && terms >= MIL_NW && terms <= MIL_MAXT)' in t and 'const int terms = C * (binary_ins ? 2 : 1);' in t
    assert 'const int blocks = cdiv(H * W * C, 256);' in t and 'dim3(blocks, N), dim3(256)' in t
    # one wave per gt / bag, 4 waves per 256-thread block: grid_select, mil_bag, refine
    assert len(re.findall(r'dim3\(cdiv\(G, 4\)\), dim3\(256\)', t)) == 3
    assert t.count('const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);') == 3
    assert 'dim3(G), dim3(64 * MIL_NW)' in t and 'for (int xb = x0; xb <= x1; xb += 64)' in t
    assert 'for (int base = g0; base < g1; base += MAX_GT_LDS)' in t and '(dmin >= d2_thr)' in t and '<= thr);' in t
    assert 'loss_finalize_kernel, dim3(1), dim3(256)' in t


def mil_kernel(c, k):
    terms = c['C'] * (2 if c['binary'] else 1)
    return 'cls' if (not c['allpos'] and k['MIL_NW'] <= terms <= k['MIL_MAXT']) else 'wave'


# ---- coverage ------------------------------------------------------------------------------------------------------------
def test_table_sizes_stay_small():
    for c in CASES:
        if c['op'] in ('neg', 'bag', 'grid'):
            assert 1 <= c['N'] <= 3 and c['H'] <= 96 and c['W'] <= 96, c['name']
    js = sorted(c['J'] for c in of('neg') + of('bag') + of('grid'))
    assert js.count(256) == 1 and all(1 <= j <= 12 for j in js if j != 256)
    big = {c['name']: make_inputs(c)['logits'].shape[-1] for c in of('mil') if c['C'] > 12}
    assert big == {'mil_t512_J768': 768, 'mil_t513_J1026': 1026}
    assert all(BY_NAME[n]['K'] <= 9 and BY_NAME[n]['nb'] <= 5 for n in big)


def test_coverage_neg_mask_loss():
    k = constants()
    cs = of('neg')
    assert any(max(c['counts']) > k['MAX_GT_LDS'] and c['exact'] for c in cs), 'no image with a second trip of the gt loop'
    assert any(0 in c['counts'] and c['N'] > 1 for c in cs), 'no image without gts'
    assert any((c['H'] * c['W'] * c['C']) % 256 and c['H'] * c['W'] * c['C'] > 256 for c in cs), 'no ragged last block'
    assert any(not c['class_wise'] for c in cs) and any(c['Cm'] == 1 and c['C'] == 2 for c in cs)
    assert any(c['prob'] == 'softmax' for c in cs)
    assert {c['norm_p'] for c in cs if c['prob'] == 'normed_sigmoid'} == {1.0, 2.0, 3.0}
    assert any(c['J'] > c['C'] for c in cs)
    # pad_hw smaller than the map: a cell centre inside the map and outside the padded image
    assert any(any(p[0] < c['H'] * c['stride'] - c['stride'] / 2 or p[1] < c['W'] * c['stride'] - c['stride'] / 2 for p in c['pads'])
               for c in cs if c['pads'])
    # the exact threshold case: a pixel at d2 == d2_thr which the mask keeps (and the image without gts is all valid inside its pad)
    c, i, ref = case('neg_345_exact')
    assert i['d2_thr'] == 400.0 and float(i['stride'] * c['radius']) ** 2 == 400.0
    px, py = R._pixels(c['H'], c['W'], c['stride'])
    for gi, (cx, cy) in enumerate(((5, 7), (15, 4))):
        pix = cy * c['W'] + cx
        d2 = float((px[pix] - i['ctr'][gi, 0]) ** 2 + (py[pix] - i['ctr'][gi, 1]) ** 2)
        assert d2 == 400.0 and bool(ref['mask'][0, pix, gi])
    assert int(ref['mask'][1].sum()) == int(R.inside(torch.stack([px, py], -1), i['pad_hw'][1]).sum()) * c['C'] > 0
    # the second chunk decides pixels: the mask changes when only the first MAX_GT_LDS gts are seen
    c, i, ref = case('neg_1100gts_exact')
    assert int((R.emu_neg(i, 'first1024')['mask'] != ref['mask']).sum()) > 50


def _axis_states(q, n):
    return dict(on=bool(((q == 0) | (q == n)).any()), beyond=bool(((q < 0) | (q > n)).any()), far=bool((q.abs() > 2 * n).any()))


def test_coverage_sampling():
    cs = of('bag')
    assert any(c['J'] < 4 for c in cs) and any(c['J'] > 4 and c['J'] % 4 for c in cs) and any(c['J'] % 4 == 0 and c['J'] <= 12 for c in cs)
    assert any(c['H'] == 1 and not c['align'] for c in cs) and any(c['W'] == 1 and not c['align'] for c in cs)
    assert sum(c['J'] == 256 for c in cs) == 1
    for c in cs:
        if c['extra'] == 0:
            continue
        _, i, ref = case(c['name'])
        q = ref['pts'].double() / c['stride']
        for ax, n in ((0, c['W']), (1, c['H'])):
            assert all(_axis_states(q[..., ax], n).values()), (c['name'], ax)
        assert float(q.abs().max()) < 8 * max(c['W'], c['H']), 'a point too far out for the kernels\' int casts'
        assert bool(ref['valid'].any()) and not bool(ref['valid'].all())
    for name, pad in (('bag_align_pad_J5', True), ('bag_align_nopad_J12', False)):
        c, i, ref = case(name)
        assert c['align'] and (i['pad'] is not None) == pad
        seen = set(ref['dropped'].flatten().tolist())
        assert {0, 2, 3, 4} <= seen and 1 not in seen, (name, seen)      # taps drop by whole rows / columns: never exactly one


def test_coverage_grid_bag():
    c, i, ref = case('grid_wide')
    G = ref['count'].numel()
    assert max(ref['cols']) > 64 and bool((ref['count'] > c['Kmax']).any()) and G % 4 != 0
    assert bool(ref['valid'][ref['count'] > c['Kmax']][:, :c['Kmax']].all())
    c, i, ref = case('grid_345_exact')
    assert ref['on_radius'] >= 3 and c['exact'] and c['radius_px'] == 20.0
    assert int((R.emu_grid(i, 'lt')['count'] != ref['count']).sum()) == 3
    c, i, ref = case('grid_R3_align_pad')
    assert c['R'] > 1 and bool((ref['count'] == 0).any()) and bool(((c['Kmax'] - ref['count']) > 64).all()) and i['pad'] is not None
    pts = i['points'].view(-1, c['R'], 2)
    assert float((pts[:, 0] - pts[:, -1]).abs().max()) > c['stride']                       # spread refine points
    assert bool((ref['cell'][:, -1] == -2).all()) and bool((ref['cell'][:, c['Kmax']] == -2 - (c['R'] - 1)).all())
    assert any(c['R'] > 1 and not c['align'] for c in of('grid')) and any(c['J'] % 4 for c in of('grid'))


def test_coverage_mil_loss():
    k = constants()
    cs = of('mil')
    terms = {c['C'] * (2 if c['binary'] else 1): mil_kernel(c, k) for c in cs if not c['allpos']}
    assert terms[k['MIL_NW'] - 1] == 'wave' and terms[k['MIL_NW']] == 'cls' and terms[k['MIL_MAXT']] == 'cls' and terms[k['MIL_MAXT'] + 1] == 'wave'
    assert any(c['binary'] and mil_kernel(c, k) == 'cls' for c in cs) and any(c['allpos'] and c['K'] > 64 for c in cs)
    lens = {make_inputs(c)['bags'][3] for c in cs}
    assert {1, 63, 64, 65} <= lens and max(lens) > 128
    assert {c['geom'] for c in cs} == {'independent', 'merge', 'only_refine'}
    assert any(make_inputs(c)['centres'][3] > 1 for c in cs) and any(make_inputs(c)['centres'][2] > 1 for c in cs)
    assert any(c['prob'] == 'identity' for c in cs) and any(c['prob'] == 'softmax' for c in cs) and any(c['prob'] == 'normed_sigmoid' for c in cs)
    assert any(c['nb'] > 256 and c['npart'] > 256 for c in cs) and any(c['neg_from_gt'] for c in cs)
    assert any(make_inputs(c)['ins_off'] > c['C'] for c in cs)
    c, i, ref = case('mil_bin_t8_K65')
    assert bool((i['gt_weight'] == 0).any()) and bool((i['valid'].view(-1, 65).sum(1) == 0).any())
    c, i, ref = case('mil_all_invalid')
    assert float(ref['bag'][:, 2].sum()) == 0 and float(ref['bag'][:, 3].sum()) == 0            # both clamps at 1
    c, i, ref = case('mil_neg_from_gt')
    assert float(ref['bag'][:, 2].sum()) != float(ref['bag'][:, 3].sum()) and float(ref['bag'][:, 3].sum()) >= 1


def test_coverage_refine():
    cs = of('refine')
    assert any(c['Rv'] * c['Kv'] > 64 for c in cs)
    c, i, ref = case('refine_R2_same')
    assert c['Rv'] > 1 and ref['cov']['multi_class'] >= 2 and i['not_refine_in'] is not None and bool(i['not_refine_in'].any())
    assert bool(ref['not_refine'][1]) and c['score_max']
    # the sub-bag test bites: an entry of sub-bag 1 whose nearest candidate is refine point 0 of its own gt is dropped
    keep = ref['chosen']
    assert 0 < int(keep.sum()) < keep.numel()
    c, i, ref = case('refine_ties_exact')
    assert c['exact'] and ref['cov']['dist_ties'] >= 6 and ref['cov']['prob_ties'] >= 3 and ref['cov']['single_class'] == 1
    assert ref['chosen'][0, :3].all() and not ref['chosen'][1, :3].any()          # equidistant entries: the first candidate (gt 0) owns them
    assert bool(ref['chosen'][0, 3]) and bool(ref['chosen'][1, 4]) and not bool(ref['chosen'][2, 5])      # equal logits: the lowest class wins
    c, i, ref = case('refine_none_kept')
    assert ref['cov']['none_kept'] == 2 and c['score_max'] and bool(ref['not_refine'].all())
    assert torch.equal(ref['scores'], torch.full((2,), R.f32(i['refine_th']) * 0.5, dtype=torch.float64))
    assert torch.equal(ref['refine_pts'].float(), i['ctr'])
    assert case('refine_K130')[2]['cov']['single_class'] == 1
    assert {c['prob'] for c in cs} == {'sigmoid', 'softmax', 'normed_sigmoid'}


# ---- the references against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in of('neg') if c['Cm'] == c['C']])
def test_neg_reference_against_oracle(name):
    """oracle.cpr_oracle.neg_valid_mask (torch.cdist in fp32) gives the reference's mask outside the ambiguous pixels, and
    oracle.cpr_oracle.gfocal the reference's per-pixel terms inside their bars (sigmoid cases)."""
    c, i, ref = case(name)
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    for n in range(N):
        g0, g1 = int(i['gt_start'][n]), int(i['gt_start'][n + 1])
        if g1 == g0 and not c['class_wise']:
            continue
        _, v = O.neg_valid_mask(H, W, c['stride'], c['radius'], i['ctr'][g0:g1], i['labels'][g0:g1].long(), C, int(i['pad_hw'][n][0]),
                                int(i['pad_hw'][n][1]), c['class_wise'])
        assert int(((v != ref['mask'][n]) & ~ref['amb'][n]).sum()) == 0, (name, n)
    if c['prob'] == 'sigmoid':
        l = i['logit'][..., :C].reshape(-1, 1)
        got = O.gfocal(l.sigmoid(), torch.zeros_like(l), torch.ones_like(l), i['eps'])
        t, dt = R.gfocal_ref(*R.prob(l.double(), 0), torch.zeros_like(l, dtype=torch.bool), R.f32(i['eps']))
        assert R.worst(got, t[:, 0], dt[:, 0]) <= 1


@pytest.mark.parametrize('name', [c['name'] for c in of('bag')])
def test_bag_reference_against_oracle(name):
    """Bag points and validity equal oracle.cpr_oracle.bag_points / inside bit for bit (the ring offsets are the oracle's), and
    the sampled values agree with its grid_sample wrapper inside the bars (the oracle samples features: no pad share)."""
    c, i, ref = case(name)
    assert torch.equal(i['off'], O.circle_offsets(c['radius'], c['stride']).float())
    assert torch.equal(ref['pts'], O.bag_points(i['ctr'], c['radius'], c['stride']))
    for gi in range(ref['pts'].shape[0]):
        n = int(i['gt_img'][gi])
        assert torch.equal(ref['valid'][gi], O.inside(ref['pts'][gi], int(i['pad_hw'][n][0]), int(i['pad_hw'][n][1])))
        got = O.sample_bilinear(i['map'][n:n + 1].permute(0, 3, 1, 2), ref['pts'][gi:gi + 1] / c['stride'], c['align'])[0]
        want, bar, _ = R.sample_ref(i['map'][n].double(), ref['pts'][gi, :, 0].double(), ref['pts'][gi, :, 1].double(), c['stride'], c['align'], None)
        assert R.worst(got, want, bar) <= 1, (name, gi)


@pytest.mark.parametrize('name', ['mil_t7_K63', 'mil_t8_K64', 'mil_K1', 'mil_300bags', 'mil_all_invalid'])
def test_mil_reference_against_oracle(name):
    """oracle.cpr_oracle.mil_loss (fp32; sigmoid, one bag per gt) gives the finalised reference: the loss inside the summed bag
    bars plus its own fp32 sum over the bags, the accuracy and the sample count exactly."""
    c, i, ref = case(name)
    nb, _, _, K = i['bags']
    C = c['C']
    lg = i['logits'].view(nb, K, -1)
    loss, acc, ns = O.mil_loss(lg[..., :C].sigmoid(), lg[..., i['ins_off']:i['ins_off'] + C], i['labels'].long(), i['valid'].view(nb, K, 1).float(),
                               i['w_mil'], i['eps'])
    assert float(ref['amb4'].sum()) == 0
    want_ns = max(float(ref['bag'][:, 2].sum()), 1.0)
    want = float(ref['bag'][:, 0].sum()) / want_ns * R.f32(i['w_mil'])
    bar = (float(ref['bar'][:, 0].sum()) + float(R.g(nb + 2)) * float(ref['bag'][:, 0].abs().sum())) / want_ns * R.f32(i['w_mil'])
    assert ns == want_ns and abs(float(loss) - want) <= bar, (float(loss), want, bar)
    assert abs(float(acc) - float(ref['bag'][:, 4].sum()) * 100.0 / nb) <= 1e-4


# ---- ambiguity -------------------------------------------------------------------------------------------------------
EMU = dict(centers=lambda i, w=None: dict(centers=R.emu_centers(i['boxes'])), neg=R.emu_neg, bag=R.emu_bag, grid=R.emu_grid, mil=R.emu_mil,
           refine=R.emu_refine)


def emulate(name, wrong=None, finalize_wrong=None):
    c, i, ref = case(name)
    got = EMU[c['op']](i, wrong)
    if c['op'] == 'mil':
        den = float(got['bag'].shape[0] * (i['bags'][3] if i['allpos'] else 1))
        got['out5'] = R.emu_finalize(got['bag'], i['neg_partial'], i['w_mil'], i['w_gt'], i['w_neg'], den, i['neg_from_gt'], finalize_wrong)
    return c, R.compare(c['op'], i, got, ref)


@pytest.mark.parametrize('name', list(BY_NAME))
def test_right_formula_passes_and_ambiguity_stays_inside_the_cap(name):
    """The fp32 emulation of the kernel's own formula meets every bar of the case (with room: the bars are worst-case counts), no
    discrete output differs outside the ambiguous set, and the reference alone keeps the ambiguous share inside AMBIG_CAP -- zero
    for the exact cases."""
    c, res = emulate(name)
    print(name, res)
    assert all(r <= 1 for r in res['ratios'].values()), res['ratios']
    assert all(w == 0 for w in res['wrong'].values()), res['wrong']
    assert R.amb_ok(res, c['exact']), res['amb']
    if c['exact']:
        assert all(a == 0 for a, _ in res['amb'].values())


def test_ambiguous_mask_pixels_per_gt_measured():
    """Random fp32 centres at stride 4, radius 5 on a 33 x 29 map, two gts per image over 1000 images.  The squared distances
    inside the d2 bar (g(8) M <= 4.8e-7 * 6.3e4 = 0.03 either side of 400) form a ring of area pi * 0.06 px^2, which holds
    pi * 0.06 / 16 = 0.012 cell centres per gt on average (less where the map's border cuts the ring); 2000 gts put that mean at
    24 pixels with a deviation of 5, and the bar used is below its worst case.  Measured here and held below the derived 0.012."""
    from pointtinybenchmark_amd.dense_heads.cpr_head import sqrt_threshold
    gen = torch.Generator().manual_seed(5)
    N, H, W = 1000, 33, 29
    ctr = torch.rand((2 * N, 2), generator=gen) * torch.tensor([W * 4.0, H * 4.0])
    i = dict(logit=torch.zeros((N, H, W, 1)), ctr=ctr, labels=torch.zeros(2 * N, dtype=torch.int32), gt_start=torch.arange(N + 1, dtype=torch.int32) * 2,
             pad_hw=torch.tensor([(H * 4, W * 4)] * N, dtype=torch.int32), C=1, Cm=1, stride=4, d2_thr=sqrt_threshold(20), eps=1e-6, class_wise=True,
             ptype=0, norm_p=1.0, exact=False)
    per_gt = float(R.neg_ref(i)['amb'].sum()) / (2 * N)
    print('ambiguous mask pixels per gt: %.4f' % per_gt)
    assert per_gt <= 0.012


# ---- sharpness -------------------------------------------------------------------------------------------------------
# variant -> (cases it must be caught on, emulation flag, finalize flag, the output that must fail)
WRONG = {
    'softmax_entry_dropped': (['mil_t7_K63', 'mil_t8_K64', 'mil_K130_merge_softmax'], 'drop_entry', None, 'bag_mil'),
    'eps_omitted_bag_loss': (['mil_saturated'], 'noeps', None, 'bag_mil'),
    'eps_omitted_gt_loss': (['mil_saturated', 'mil_t7_K63'], 'noeps', None, 'bag_gt'),
    # eps is 8 fp32 ulps of a probability near 1: left out of log(1 - p + eps) it clears the bar by 2.6 only on neg_sigmoid_c3, a
    # margin that a larger TRANS_ULP cap would eat; the two log(p + eps) entries above carry the variant at more than 1e2
    'eps_omitted_negative_loss': (['neg_sigmoid_c3'], 'noeps', None, 'img_sum'),
    'centre_first_in_bag': (['bag_J1', 'bag_J6'], 'centre_first', None, 'pts'),
    'refine_points_not_reversed': (['grid_R3_align_pad', 'grid_R2_nopad'], 'no_reverse', None, 'pts'),
    'dropped_tap_without_pad': (['bag_align_pad_J5'], 'nopad', None, 'out'),
    'gt_instead_of_ge_at_mask_threshold': (['neg_345_exact'], 'gt', None, 'mask'),
    'only_first_1024_gts': (['neg_1100gts_exact'], 'first1024', None, 'mask'),
    'last_instead_of_first_argmin': (['refine_ties_exact'], 'last_argmin', None, 'chosen'),
    'num_sample_not_clamped': (['mil_all_invalid'], None, 'noclamp', 'out5'),
    'lt_instead_of_le_at_radius': (['grid_345_exact'], 'lt', None, 'count'),
}


@pytest.mark.parametrize('variant', list(WRONG))
def test_bars_catch_the_wrong_variant(variant):
    names, flag, fin, key = WRONG[variant]
    for name in names:
        c, res = emulate(name, flag, fin)
        bad = res['ratios'].get(key, 0) > 1 or res['wrong'].get(key, 0) > 0
        print('%s on %s: %s %s' % (variant, name, res['ratios'], res['wrong']))
        assert bad, '%s passes the bars of %s (%s)' % (variant, name, key)
        assert not R.passes(res, c['exact'])


def test_a_wrong_tap_or_slot_is_orders_of_magnitude_over_the_bar():
    """TRANS_ULP is a cap, not a measurement: the faults the bars are there for overshoot them by far more than any choice of cap.
    (eps itself is only 8 fp32 ulps of a probability near 1, so leaving it out of log(1 - p + eps) overshoots by 2.5 .. 4 and no
    more; in log(p + eps) with p of the order of eps it overshoots like the others.)"""
    assert emulate('bag_align_pad_J5', 'nopad')[1]['ratios']['out'] > 1e4
    assert emulate('mil_t8_K64', 'drop_entry')[1]['ratios']['bag_mil'] > 1e2
    assert emulate('mil_saturated', 'noeps')[1]['ratios']['bag_mil'] > 1e2


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_arguments_that_would_reach_a_bad_launch():
    """Every call returns CPR_ERR_ARG before any launch (no GPU needed; the buffers are host memory no kernel ever sees).  Each bad
    call differs from an acceptable argument set in the named fields only."""
    from pointtinybenchmark_amd import _lib
    L = _lib.load()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data

    def neg(**kw):
        a = dict(logit=p, J=2, N=1, H=8, W=8, C=2, stride=4.0, cw=1, pt=0, norm_p=1.0, mc=2, gt_start=p)
        a.update(kw)
        return L.cpr_neg_mask_loss(a['logit'], a['J'], p, p, a['gt_start'], p, p, p, a['N'], a['H'], a['W'], a['C'], a['stride'], 400.0, 1e-6, a['cw'],
                                   a['pt'], a['norm_p'], a['mc'], None, None)

    for bad in (dict(stride=0.0), dict(stride=-4.0), dict(H=65536, W=65536, C=1, mc=1), dict(H=46341, W=46341, C=1, mc=1),
                dict(H=1, W=2147483448, C=1, mc=1), dict(H=32768, W=32768, C=2), dict(N=65536),
                dict(J=1), dict(N=0), dict(H=0), dict(C=0, mc=0), dict(mc=1, C=3), dict(pt=3), dict(pt=-1), dict(norm_p=0.0), dict(logit=None),
                dict(gt_start=None)):
        assert neg(**bad) == ERR_ARG, bad

    def mil(**kw):
        a = dict(logits=p, J=4, ins_off=2, G=2, bs=8, bo=0, K=8, co=7, cs=8, cc=1, cm=1, C=2, pt=0, norm_p=1.0, binary=0, allpos=0, npart=0, part=None)
        a.update(kw)
        return L.cpr_mil_loss(a['logits'], a['J'], a['ins_off'], p, p, None, p, a['part'], a['npart'], a['G'], a['bs'], a['bo'], a['K'], a['co'], a['cs'],
                              a['cc'], a['cm'], a['C'], 1e-6, a['pt'], a['norm_p'], a['binary'], a['allpos'], 0.25, 0.25, 0.75, 0, p, None)

    for bad in (dict(ins_off=-1), dict(ins_off=-2, J=0), dict(ins_off=-2147483647), dict(cs=-1, cc=2), dict(cs=-8, cc=2, co=7), dict(cs=2147483647, cc=3),
                dict(J=1, ins_off=0, C=2), dict(G=0), dict(K=0), dict(C=0), dict(bo=-1), dict(bs=7), dict(cc=-1), dict(cm=0), dict(J=3), dict(binary=1),
                dict(co=-1), dict(co=8), dict(cs=4, cc=2, co=7), dict(pt=4), dict(pt=-1), dict(norm_p=0.0), dict(npart=3), dict(logits=None)):
        assert mil(**bad) == ERR_ARG, bad

    bag = lambda G=2, K=5, J=3, H=8, W=8, stride=4.0, align=0, m=p: L.cpr_bag_sample(m, J, p, p, p, p, p, p, p, G, K, H, W, stride, align, None, None)
    for bad in (dict(G=-1), dict(K=0), dict(J=0), dict(H=0), dict(stride=0.0), dict(align=1, H=1), dict(align=1, W=1), dict(m=None)):
        assert bag(**bad) == ERR_ARG, bad
    assert bag(G=0) == 0
    grid = lambda G=2, R=1, Kmax=9, J=3, H=8, W=8, stride=4.0, rad=8.0, align=0, m=p: L.cpr_grid_bag(m, J, p, p, R, Kmax, rad, None, p, p, p, p, p, G, H, W,
                                                                                                     stride, align, None)
    for bad in (dict(G=-1), dict(R=0), dict(Kmax=0), dict(J=0), dict(W=0), dict(stride=0.0), dict(rad=-1.0), dict(align=1, H=1), dict(m=None)):
        assert grid(**bad) == ERR_ARG, bad
    assert grid(G=0) == 0

    def refine(**kw):
        a = dict(logits=p, J=3, Rv=2, cs=2, G=2, Kt=10, Kv=5, C=2, pt=0, norm_p=1.0)
        a.update(kw)
        return L.cpr_refine(a['logits'], a['J'], p, p, p, a['Rv'], a['cs'], p, p, p, p, None, p, p, p, p, a['G'], a['Kt'], a['Kv'], a['C'], a['pt'],
                            a['norm_p'], 0.5, 0.1, 0.3, 1, 1, 0, None)

    for bad in (dict(G=0), dict(Kt=11), dict(Kv=0, Kt=0), dict(Rv=0), dict(cs=1), dict(C=0), dict(J=1), dict(pt=3), dict(norm_p=-1.0), dict(logits=None)):
        assert refine(**bad) == ERR_ARG, bad
    assert L.cpr_box_centers(p, p, -1, None) == ERR_ARG and L.cpr_box_centers(None, None, 0, None) == 0
