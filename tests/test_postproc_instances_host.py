"""CPU only: the exact references of tests/postproc_exact_ref.py equal ``oracle.cpr_oracle.batched_nms`` / ``multiclass_nms`` and
``torch.topk`` / the stable ``argsort`` on every table case without a +-0; the tables meet their coverage conditions -- asserted from
the data: every planted chain sits at its stated sorted ranks with a and c kept and b removed, every threshold pair's IoU equals the
threshold bit for bit, the top-k tie copies touch every pass and the stated lanes and ``take_eq`` has the stated value; and every
deliberately wrong variant of the references (``R.VARIANTS``) disagrees with the true reference on a named case.

Refuting cases, the first of each table walk (the last test prints them): iou_ge grid_n2_L0; filter_ge n1_c1_none_absent_bs4 (its one score equals
thr); filter_scaled n1_c1_all_zero_bs4; removed_suppress grid_n63_L0; clear_8192 grid_n8256_L0; count_restart grid_n8193_L0; ignore_intra_tile
grid_n2_L0_below; no_offset grid_n63_L0; class_max
class_max_trap; tie_higher grid_n63_L0 (NMS) and all_equal_n5000_k1500 (top-k); thr_tie_highest all_equal_n5000_k1500; neg_zero_below
mixed_sign_n1500_k1500 (top-k) and grid_n129_pm0 (NMS)."""
import os

import numpy as np
import torch

from oracle import cpr_oracle as O
from tests import postproc_exact_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
F32 = np.float32
LOG = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the restated seams are the source's -------------------------------------------------------------------------------
def test_seams_are_the_source():
    with open(os.path.join(CSRC, 'postproc.hip')) as f:
        s = f.read()
    assert s.count('dim3(%d), 0, stream, scores, n, k, out_vals, out_idx);' % R.BLOCK) == 2                    # top-k: one block of 1024
    assert '__shared__ unsigned long long sel[%d];' % R.TOPK_MAX in s and 'k <= n && k <= %d' % R.TOPK_MAX in s
    assert 'if (u == 0x80000000u) u = 0u;' in s and 'out_vals[i] = scores[src];' in s and 'key2f' not in s           # +-0 equal; values keep their bits
    assert 'for (int pass = 3; pass >= 0; --pass) {' in s and 'for (int base = 0; base < n; base += blockDim.x) {' in s
    assert 'if (eq && rank < take_eq) sel[(k - take_eq) + rank]' in s
    assert s.count('hipLaunchKernelGGL(nms_candidates_kernel, dim3(1), dim3(%d)' % R.BLOCK) == 1
    assert s.count('hipLaunchKernelGGL(nms_candidates_kernel, dim3(B), dim3(%d)' % R.BLOCK) == 1
    assert 'const bool a = j < total && sc > thr;' in s and 'cscores[o] = factors ? __fmul_rn(sc, factors[row]) : sc;' in s
    assert 'constexpr int NMS_BAND_ROWS = %d;' % R.BAND in s and 'constexpr int NMS_SCAN_WORDS = %d;' % (R.NMS_MAX // 64) in s
    assert 'CPR_CHECK_ARG(B >= 0 && cap >= 0 && cap <= %d);' % R.NMS_BATCHED_CAP_MAX in s
    assert 'const float off1 = __fadd_rn(s_max, 1.f);' in s and 'const float o = __fmul_rn((float)labels[src], off1);' in s
    assert 'const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, aj), inter));' in s and 'if (ovr > thr) bits |= 1ull << t;' in s
    assert 'const int cnt = min(%d, n - cb * %d);' % (R.TILE, R.TILE) in s


# ---- the references are the oracle's and torch's -------------------------------------------------------------------
def test_topk_ref_equals_torch_where_no_zero():
    seen = 0
    for c in R.topk_cases():
        v, i = R.topk_ref(c['scores'], c['k'])
        assert np.array_equal(_bits(v), _bits(c['scores'][i])), c['id']
        if c['pm0']:
            continue
        s = _t(c['scores'])
        assert torch.equal(_t(i), torch.argsort(s, descending=True, stable=True)[:c['k']]), c['id']
        assert np.array_equal(_bits(v), _bits(torch.topk(s, c['k']).values.numpy())), c['id']
        seen += 1
    for c in R.topk_batched_cases():
        for b, row in enumerate(c['rows']):
            s = c['scores'][b]
            if R.has_pm0(s):
                continue
            v, i = R.topk_ref(s, c['k'])
            assert torch.equal(_t(i), torch.argsort(_t(s), descending=True, stable=True)[:c['k']]), (c['id'], row)
            seen += 1
    assert seen >= 11 + 3 * 4
    assert np.array_equal(R.topk_ref(R.topk_all_equal(5000), 1500)[1], np.arange(1500))


def _cand_torch(c, boxes, scores, factors):
    """multiclass_nms's candidate list restated with torch (bbox_nms.py:28-60): nonzero of the raw filter, row-major."""
    n, C = c['n'], c['C']
    s = _t(scores)[:, :C]
    b = _t(boxes).view(n, -1, 4).expand(n, C, 4)
    valid = (s > float(c['thr'])).reshape(-1)
    inds = valid.nonzero(as_tuple=False).squeeze(1)
    stored = s if factors is None else s * _t(factors)[:, None]
    labels = torch.arange(C).view(1, -1).expand(n, C).reshape(-1)
    return b.reshape(-1, 4)[inds], stored.reshape(-1)[inds], labels[inds], inds


def test_candidates_ref_equals_torch():
    for c in R.cand_cases():
        got = R.candidates_ref(c['boxes'], c['box_stride'], c['scores'], c['factors'], c['thr'])
        tb, ts, tl, ti = _cand_torch(c, c['boxes'], c['scores'], c['factors'])
        assert np.array_equal(_bits(got[0]), _bits(tb.numpy())) and np.array_equal(_bits(got[1]), _bits(ts.numpy())), c['id']
        assert np.array_equal(got[2], tl.numpy()) and np.array_equal(got[3], ti.numpy()) and got[2].dtype == np.int32, c['id']
    for c in R.cand_batched_cases():
        for b in range(3):
            f = None if c['factors'] is None else c['factors'][b]
            got = R.candidates_ref(c['boxes'][b], c['box_stride'], c['scores'][b], f, c['thr'])
            ti = _cand_torch(c, c['boxes'][b], c['scores'][b], f)[3]
            assert np.array_equal(got[3], ti.numpy()), (c['id'], b)
        assert len(R.candidates_ref(c['boxes'][1], c['box_stride'], c['scores'][1], None, c['thr'])[3]) == 0, c['id']     # the empty image


def test_nms_ref_equals_the_oracle_where_no_zero():
    seen = 0
    for c in R.nms_cases():
        p = R.nms_problem(c)
        if p['pm0']:
            continue
        want = O.batched_nms(_t(p['boxes']), _t(p['scores']), _t(p['labels']).long(), float(c['thr']))
        assert np.array_equal(R.nms_expected(c), want.numpy()), c['id']
        seen += 1
    assert seen == len(R.nms_cases()) - 2
    for b in R.NMS_BATCHED:
        for n in b['counts']:
            if n:
                p = R.batched_slab(n)
                want = O.batched_nms(_t(p['boxes']), _t(p['scores']), _t(p['labels']).long(), float(R.THIRD))
                assert np.array_equal(R.batched_expected(n), want.numpy()), (b['id'], n)


def test_multiclass_ref_equals_the_oracle():
    for n, C, seed in ((300, 3, 0), (65, 5, 1)):
        boxes, scores = R.multiclass_problem(n, C, seed)
        for max_num in (-1, 50):
            dets, labels, inds = R.multiclass_ref(boxes, 4, scores, None, R.MULTI_SCORE_THR, R.THIRD, max_num)
            od, ol, oi = O.multiclass_nms(_t(boxes), _t(scores), float(R.MULTI_SCORE_THR), float(R.THIRD), max_num)
            assert np.array_equal(_bits(dets), _bits(od.numpy())) and np.array_equal(labels, ol.numpy()) and np.array_equal(inds, oi.numpy())
            assert 0 < len(dets) < (n * C if max_num < 0 else max_num + 1)


# ---- coverage, from the data -------------------------------------------------------------------------------------------
def test_topk_tables_reach_their_seams():
    ids = {c['id']: c for c in R.topk_cases()}
    assert [(len(c['scores']), c['k']) for c in R.topk_cases()][:7] == [(1, 1), (63, 63), (1024, 1024), (1025, 512), (4096, 4096), (4097, 4096), (4099, 1)]
    assert all(not np.isnan(c['scores']).any() and c['why'] for c in R.topk_cases() + R.topk_batched_cases())
    T, gt, take = R.topk_take_eq(ids['all_equal_n5000_k1500']['scores'], 1500)
    assert (gt, take) == (0, 1500) and -(-5000 // R.BLOCK) == 5
    for s, k in ((ids['planted_tie_n5000_k1400']['scores'], 1400), (R.topk_batched_cases()[0]['scores'][2], 1400)):
        T, gt, take = R.topk_take_eq(s, k)
        assert T == R.TIE_T and (gt, take) == (300, 1100), (T, gt, take)
        eq = np.nonzero(s == T)[0]
        assert len(eq) == (3000 if len(s) == 5000 else len(eq)) and len(eq) > 2 * take
        assert int((s > T).sum()) == 300 and len(np.unique(s[s > T])) == 300
        assert set(eq // R.BLOCK) == set(range(-(-len(s) // R.BLOCK)))                   # copies in every 1024-pass
        assert (eq % R.WAVE == 0).any() and (eq % R.WAVE == R.WAVE - 1).any() and (eq % R.BLOCK == R.BLOCK - 1).any()
        assert all(len(set(eq[(eq // R.WAVE) == w] % R.WAVE)) > 1 for w in (0, 17))       # several copies inside one wave
        last, nxt = eq[take - 1], eq[take]
        assert R.BLOCK <= last < 2 * R.BLOCK and last % R.WAVE not in (0, R.WAVE - 1) and nxt // R.WAVE == last // R.WAVE   # ends mid-wave, pass 2
    m = ids['mixed_sign_n1500_k1500']['scores']
    u = _bits(m)
    assert (m < 0).any() and np.isposinf(m).any() and np.isneginf(m).any() and (u == 0).any() and (u == 0x80000000).any()
    den = (u & 0x7F800000 == 0) & (u & 0x007FFFFF != 0)
    assert (den & (m > 0)).any() and (den & (m < 0)).any()
    z = np.nonzero(m == 0)[0]
    assert (u[z[:-1]] != u[z[1:]]).all()                                                  # the two zeros alternate in index order
    T, gt, take = R.topk_take_eq(m, 700)
    assert T == 0 and take > 1                                                            # the k-th place falls among the zeros
    lb, tb = _bits(ids['last_byte_n3000_k1000']['scores']), _bits(ids['top_byte_n2048_k777']['scores'])
    assert len(np.unique(lb >> 8)) == 1 and len(np.unique(lb & 255)) == 256
    assert len(np.unique(tb & 0x00FFFFFF)) == 1 and len(np.unique(tb >> 24)) == 256 and np.isfinite(ids['top_byte_n2048_k777']['scores']).all()
    b = R.topk_batched_cases()
    assert b[0]['scores'].shape == (5, 4099) and 'all_equal' in b[0]['rows'] and [c['k'] for c in b] == [1400, 4096, 1]


def test_candidate_tables_reach_their_seams():
    cases = R.cand_cases()
    assert sorted({(c['n'], c['C']) for c in cases}) == sorted(R.CAND_SHAPES) and len(cases) == 6 * 6 * 3 + 2 * 6 * 3
    for c in cases:
        n, C, s = c['n'], c['C'], c['scores']
        fg = s[:, :C].reshape(-1)
        take = fg > c['thr']
        j = np.nonzero(take)[0]
        assert (s[:, C] > c['thr']).all() and c['why']                                    # the background column passes the filter and is never taken
        if c['pattern'] == 'none':
            assert len(j) == 0 and ((fg == c['thr']).any() or n * C == 1)
        if c['pattern'] == 'all':
            assert len(j) == n * C
        if c['pattern'] in ('lane0', 'lane63'):
            assert (j % R.WAVE == (0 if c['pattern'] == 'lane0' else R.WAVE - 1)).all() and len(j) == (n * C + (R.WAVE if c['pattern'] == 'lane0' else 0) - (0 if c['pattern'] == 'lane63' else 1)) // R.WAVE
        if c['pattern'] == 'eq_thr':
            assert (fg[0::3] == c['thr']).all() and not take[0::3].any() and take[1::3].all() and not take[2::3].any()
        if c['factors_kind'] == 'zero':
            assert (c['factors'][::3] == 0).all() and (take.reshape(n, C)[::3].any() or c['pattern'] in ('none', 'lane0', 'lane63', 'eq_thr'))
    assert any(c['factors_kind'] == 'zero' and (c['scores'][::3, :c['C']] > c['thr']).any() for c in cases)
    assert {c['box_stride'] for c in cases if c['C'] == 80} == {4, 320}
    assert any(c['n'] * c['C'] > 2 * R.BLOCK and c['n'] * c['C'] % R.BLOCK for c in cases)          # three passes, the last ragged


def _iou(p, ra, rb):
    """fp32 IoU of the boxes at sorted ranks ra, rb after the class offset, in the kernel's order."""
    b = R.offset_boxes(p['boxes'], p['labels'])[p['perm']]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    return R.iou_row(b, area, ra, rb)[0]


def test_nms_tables_reach_their_seams():
    cases = R.nms_cases()
    assert sorted({R.nms_problem(c)['n'] for c in cases if c['builder'][0] == 'grid'}) == sorted(R.NMS_SIZES)
    chains, pairs_kept, pairs_supp, tie_seams, seen = set(), set(), set(), set(), dict(identical=0, zero_area=0, two_class=0, pm0=0)
    for c in cases:
        p, keep = R.nms_problem(c), R.nms_expected(c)
        n, perm, pl, thr = p['n'], p['perm'], p['planted'], c['thr']
        assert c['why'] and not np.isnan(p['scores']).any() and not np.isnan(p['boxes']).any()
        assert np.array_equal(R.order_desc(p['scores']), perm), c['id']                   # every planted rank IS its sorted rank
        if c['builder'][0] == 'grid':
            assert (p['boxes'] == np.round(p['boxes'])).all() and n < 3 or not np.array_equal(perm, np.arange(n))   # integer grid; order hidden
        kept = np.zeros(n, dtype=bool)
        kept[keep] = True
        rk = lambda r: bool(kept[perm[r]])             # noqa: E731
        for a, b, cc in pl['chains']:
            assert rk(a) and not rk(b) and rk(cc), (c['id'], a, b, cc)
            assert _iou(p, a, b) > thr and _iou(p, b, cc) > thr and _iou(p, a, cc) == 0, (c['id'], a, b, cc)
            chains.add((a, b, cc))
        for a, b in pl['thr_pairs']:
            assert _iou(p, a, b).view(np.uint32) == R.THIRD.view(np.uint32) and rk(a), (c['id'], a, b)
            assert rk(b) == (thr.view(np.uint32) == R.THIRD.view(np.uint32)), (c['id'], a, b)
            (pairs_kept if rk(b) else pairs_supp).add((n, a, b))
        for a, b in pl['identical']:
            assert _iou(p, a, b) == 1 and rk(a) and not rk(b)
            seen['identical'] += 1
        for z in pl['zero_area']:
            assert all(np.isnan(_iou(p, z[i], z[j])) for i in range(3) for j in range(i + 1, 3)) and all(rk(r) for r in z)
            seen['zero_area'] += 1
        for a, b in pl['two_class']:
            i, j = perm[a], perm[b]
            assert np.array_equal(p['boxes'][i], p['boxes'][j]) and p['labels'][i] != p['labels'][j] and rk(a) and rk(b)
            seen['two_class'] += 1
        for r0, r1 in pl['ties']:
            assert r1 > r0 and len(np.unique(p['scores'][perm[r0:r1 + 1]])) == 1 and (np.diff(perm[r0:r1 + 1]) > 0).all()
            assert (r0 == 0 or p['scores'][perm[r0 - 1]] > p['scores'][perm[r0]]) and (r1 == n - 1 or p['scores'][perm[r1]] > p['scores'][perm[r1 + 1]])
            tie_seams |= {s for s in (R.TILE, R.BAND) if r0 < s <= r1}
        for a, b in pl['pm0']:
            u = _bits(p['scores'])
            assert u[perm[a]] == 0x80000000 and u[perm[b]] == 0 and perm[a] < perm[b] and rk(a) and rk(b)
            seen['pm0'] += 1
    assert chains == {ch for L in R.CHAINS.values() for ch in L}, chains
    a, b, _ = R.CHAINS[0][3]
    assert a // R.BAND == 0 and b // R.BAND == 2                                          # a in band 0, b in band 2
    assert {(0, 1, 2), (62, 63, 64), (63, 64, 65), (8190, 8191, 8192), (8191, 8192, 8193), (100, 8191, 16384)} <= chains
    assert {(2, 0, 1), (65, 4, 6), (129, 20, 70), (8193, 20, 70)} <= pairs_supp and {(2, 0, 1), (8256, 8189, 8200)} <= pairs_kept
    assert tie_seams == {R.TILE, R.BAND} and all(v >= 2 for v in seen.values()), (tie_seams, seen)


def test_float_negative_and_class_cases_depend_on_the_offset():
    ids = {c['id']: c for c in R.nms_cases()}
    p = R.nms_problem(ids['float_x37_c80'])
    keep = set(R.nms_expected(ids['float_x37_c80']).tolist())
    assert p['labels'].max() == 79 and 1200 < p['boxes'].max() < 1300 and np.allclose(p['boxes'] % 1, 0.37, atol=1e-3)
    raw = p['boxes'][p['perm']]
    area = ((raw[:, 2] - raw[:, 0]) * (raw[:, 3] - raw[:, 1])).astype(F32)
    flips = {(True, False): 0, (False, True): 0, (True, True): 0, (False, False): 0}
    for a, b in p['planted']['float_pairs']:
        with_offset = p['perm'][b] not in keep                                             # suppressed by the reference (two roundings per edge)
        without = bool(R.iou_row(raw, area, a, b)[0] > R.THIRD)                            # the same pair without the class offset
        assert p['perm'][a] in keep and abs(float(_iou(p, a, b)) - 1 / 3) < 2e-3
        flips[(with_offset, without)] += 1
    # the offset (ulp 1/128 near 1e5) rounds both edges of a pair onto one grid, which restores the exact shift of 8 and IoU == thr: kept;
    # the un-offset .37 coordinates round per binade and leave some IoUs one ulp above thr.  Measured: 12 pairs kept only because of the
    # offset's rounding, 4 suppressed either way (their offset edges straddle a binade), 240 kept either way.
    assert flips[(False, True)] >= 8 and flips[(True, True)] >= 2 and flips[(False, False)] >= 8, flips
    LOG['float pairs (suppressed with offset, suppressed without)'] = flips
    p = R.nms_problem(ids['negative_max'])
    keep = set(R.nms_expected(ids['negative_max']).tolist())
    assert p['boxes'].max() == -100 and [p['perm'][r] in keep for r in (0, 1, 2)] == [True, False, True]
    p = R.nms_problem(ids['class_max_trap'])
    assert R.nms_expected(ids['class_max_trap']).tolist() == [0, 1, 2]


def test_capacity_and_batched_tables():
    p = R.capacity_problem(4096)
    assert np.array_equal(R.nms_ref(p['boxes'], p['scores'], p['labels'], R.THIRD), p['expected'])      # disjoint: the keep list is the stable argsort
    assert len(np.unique(p['scores'])) == 1024
    assert R.NMS_MAX == 262144 and (R.NMS_MAX // 512) * 32 < 2 ** 23
    assert [b['counts'] for b in R.NMS_BATCHED] == [(0, 1, 64, 65, 200), (8191, 8192, 0)] and [b['cap'] for b in R.NMS_BATCHED] == [200, 8192]
    assert sorted({-(-n // R.TILE) for n in R.NMS_BATCHED[0]['counts']}) == [0, 1, 2, 4]


# ---- sharpness -----------------------------------------------------------------------------------------------------------
def _refute_nms(variant, min_n=0):
    for c in sorted(R.nms_cases(), key=lambda c: R.nms_problem(c)['n']):
        p = R.nms_problem(c)
        if p['n'] < min_n:
            continue
        if not np.array_equal(R.nms_ref(p['boxes'], p['scores'], p['labels'], c['thr'], variant), R.nms_expected(c)):
            return c['id']
    return None


def _refute_topk(variant):
    for c in R.topk_cases():
        v, i = R.topk_ref(c['scores'], c['k'])
        wv, wi = R.topk_ref(c['scores'], c['k'], variant)
        if not (np.array_equal(i, wi) and np.array_equal(_bits(v), _bits(wv))):
            return c['id']
    return None


def _refute_cand(variant):
    for c in R.cand_cases():
        a = R.candidates_ref(c['boxes'], c['box_stride'], c['scores'], c['factors'], c['thr'])
        b = R.candidates_ref(c['boxes'], c['box_stride'], c['scores'], c['factors'], c['thr'], variant)
        if not (np.array_equal(a[3], b[3]) and np.array_equal(_bits(a[1]), _bits(b[1]))):
            return c['id']
    return None


def test_every_wrong_variant_is_refuted_by_a_named_case():
    band = R.BAND + 1                      # the band variants cannot differ at or below 8192 rows
    found = {
        'iou_ge': _refute_nms('iou_ge'), 'filter_ge': _refute_cand('filter_ge'), 'filter_scaled': _refute_cand('filter_scaled'),
        'removed_suppress': _refute_nms('removed_suppress'), 'clear_8192': _refute_nms('clear_8192', band),
        'count_restart': _refute_nms('count_restart', band), 'ignore_intra_tile': _refute_nms('ignore_intra_tile'),
        'no_offset': _refute_nms('no_offset'), 'class_max': _refute_nms('class_max'),
        'tie_higher': (_refute_nms('tie_higher'), _refute_topk('tie_higher')), 'thr_tie_highest': _refute_topk('thr_tie_highest'),
        'neg_zero_below': (_refute_topk('neg_zero_below'), _refute_nms('neg_zero_below')),
    }
    assert set(found) == set(R.VARIANTS)
    for k, v in found.items():
        print('%-18s %-55s refuted by %s' % (k, R.VARIANTS[k], v))
        assert v is not None and (not isinstance(v, tuple) or all(x is not None for x in v)), 'no case refutes the wrong variant %r: a case is missing' % k
    # the planted top-k tie refutes the threshold-tie variant too (not only the all-equal case found first)
    tie = [c for c in R.topk_cases() if c['id'] == 'planted_tie_n5000_k1400'][0]
    assert not np.array_equal(R.topk_ref(tie['scores'], 1400)[1], R.topk_ref(tie['scores'], 1400, 'thr_tie_highest')[1])
    for k, v in LOG.items():
        print(k, v)
