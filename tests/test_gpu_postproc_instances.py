"""-m gpu: the detection tail through its C entry points -- ``cpr_topk_desc[_batched]``, ``cpr_nms_candidates[_batched]``,
``cpr_nms_workspace``, ``cpr_nms`` and ``cpr_nms_batched`` (csrc/postproc.hip) -- against the exact references and the case tables of
tests/postproc_exact_ref.py.  The answers are integers and fp32 values with one rounding per operation, so every comparison is
``torch.equal`` on the bits: indices, counts, values, stored candidate boxes, scores and labels.

Every workspace has exactly the size the query (or the documented formula of the batched form) reports and is filled with 0xA5 bytes, with
a guard tail that must stay 0xA5; every output is guard-filled -- floats with NaN, indices with -1 -- and every element past ``num_keep``,
past ``count``, past ``k`` and in other images' slabs must still hold its guard bit for bit.  Each case runs twice and must give the same
bits; the ``ops`` wrapper gives the same result; each image of a batched launch equals its single-problem run; ``multiclass_nms`` and
``multiclass_nms_batched`` equal candidates-then-NMS of the references (one slab above 16384 routes image by image).  The refusals pass
null buffers, so nothing can launch.

The capacity case (n = 262144, pairwise disjoint boxes: the reference is the stable argsort) prints its wall time; CHANGELOG.md records it.
tests/test_postproc_instances_host.py asserts without a GPU that the tables reach the seams and that wrong references fail on them."""
import time

import numpy as np
import pytest
import torch

from tests import postproc_exact_ref as R

pytestmark = pytest.mark.gpu

TAIL = 64                    # guard elements after every output and workspace
WS_BYTE = 0xA5


# ---- plumbing ----------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args, **kw):
    from pointtinybenchmark_amd import _lib
    return _lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream(), **kw)


def raw(name, *args):
    """The entry point's own return code (the refusals)."""
    from pointtinybenchmark_amd import _lib
    return getattr(_lib.load(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def guard(n, dtype):
    """n + TAIL guard-filled elements: NaN (floats), -1 (indices, counts)."""
    return torch.full((n + TAIL,), float('nan') if dtype == torch.float32 else -1, dtype=dtype, device='cuda')


def ws(nbytes):
    return torch.full((nbytes + 8 * TAIL,), WS_BYTE, dtype=torch.uint8, device='cuda')


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(name, got, want):
    """got (device) == want (numpy or tensor) in shape, type and bits."""
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, '%s: %s %s != %s %s' % (name, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    ne = int((bits(got) != bits(want)).sum())
    assert ne == 0 and torch.equal(bits(got), bits(want)), '%s: %d of %d elements differ' % (name, ne, got.numel())


def untouched(name, t):
    """Every element of t still holds its guard (NaN bits / -1 / 0xA5)."""
    ref = torch.full_like(t, WS_BYTE if t.dtype == torch.uint8 else float('nan') if t.dtype == torch.float32 else -1)
    assert torch.equal(bits(t), bits(ref)), '%s: guard elements were written' % name


# ---- top-k -----------------------------------------------------------------------------------------------------------
def run_topk(scores, k, batched):
    s = dev(scores)
    B = s.shape[0] if batched else 1
    vals, idx = guard(B * k, torch.float32), guard(B * k, torch.int64)
    if batched:
        call('cpr_topk_desc_batched', s, B, s.shape[1], k, vals, idx)
    else:
        call('cpr_topk_desc', s, s.numel(), k, vals, idx)
    torch.cuda.synchronize()
    return vals, idx


def check_topk(name, scores, k, batched):
    from pointtinybenchmark_amd import ops
    rows = scores if batched else scores[None]
    want = [R.topk_ref(r, k) for r in rows]
    wv, wi = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    vals, idx = run_topk(scores, k, batched)
    n_out = len(rows) * k
    diff = int((idx[:n_out].cpu() != torch.from_numpy(wi)).sum())
    print('%s: %d of %d indices differ from the reference' % (name, diff, n_out))
    same(name + ' indices', idx[:n_out], wi)
    same(name + ' values', vals[:n_out], wv)
    untouched(name + ' past k (values)', vals[n_out:])
    untouched(name + ' past k (indices)', idx[n_out:])
    v2, i2 = run_topk(scores, k, batched)
    same(name + ' second run values', v2, vals.cpu())
    same(name + ' second run indices', i2, idx.cpu())
    ov, oi = (ops.topk_desc_batched if batched else ops.topk_desc)(dev(scores), k)
    same(name + ' ops values', ov.reshape(-1), wv)
    same(name + ' ops indices', oi.reshape(-1), wi)
    return vals[:n_out].cpu(), idx[:n_out].cpu()


@pytest.mark.parametrize('case', R.topk_cases(), ids=lambda c: c['id'])
def test_topk_single(case):
    check_topk(case['id'], case['scores'], case['k'], False)
    check_topk(case['id'] + ' as a batch of one', case['scores'][None], case['k'], True)


@pytest.mark.parametrize('case', R.topk_batched_cases(), ids=lambda c: c['id'])
def test_topk_batched_equals_each_segment_alone(case):
    vals, idx = check_topk(case['id'], case['scores'], case['k'], True)
    k = case['k']
    for b, row in enumerate(case['rows']):
        v1, i1 = run_topk(case['scores'][b], k, False)
        same('%s row %s alone, values' % (case['id'], row), v1[:k], vals[b * k:(b + 1) * k])
        same('%s row %s alone, indices' % (case['id'], row), i1[:k], idx[b * k:(b + 1) * k])


# ---- candidates ------------------------------------------------------------------------------------------------------
def run_cands(boxes, box_stride, scores, factors, thr, batched):
    b, s = dev(boxes), dev(scores)
    f = None if factors is None else dev(factors)
    B = s.shape[0] if batched else 1
    n, C = s.shape[-2], s.shape[-1] - 1
    cap = n * C
    out = dict(boxes=guard(B * cap * 4, torch.float32), scores=guard(B * cap, torch.float32), labels=guard(B * cap, torch.int32),
               inds=guard(B * cap, torch.int64), count=guard(B, torch.int32))
    args = (out['boxes'], out['scores'], out['labels'], out['inds'], out['count'])
    if batched:
        call('cpr_nms_candidates_batched', b, box_stride, s, f, B, n, C, float(thr), *args)
    else:
        call('cpr_nms_candidates', b, box_stride, s, f, n, C, float(thr), *args)
    torch.cuda.synchronize()
    return out


def check_cands(name, boxes, box_stride, scores, factors, thr, batched):
    B = scores.shape[0] if batched else 1
    n, C = scores.shape[-2], scores.shape[-1] - 1
    cap = n * C
    out = run_cands(boxes, box_stride, scores, factors, thr, batched)
    for b in range(B):
        sl = (lambda a: a[b]) if batched else (lambda a: a)
        wb, wsc, wl, wi = R.candidates_ref(sl(boxes), box_stride, sl(scores), None if factors is None else sl(factors), thr)
        m, nm = len(wi), '%s image %d' % (name, b)
        assert int(out['count'][b]) == m, '%s: count %d != %d' % (nm, int(out['count'][b]), m)
        same(nm + ' boxes', out['boxes'][b * cap * 4:(b * cap + m) * 4], wb.reshape(-1))
        same(nm + ' scores', out['scores'][b * cap:b * cap + m], wsc)
        same(nm + ' labels', out['labels'][b * cap:b * cap + m], wl)
        same(nm + ' inds', out['inds'][b * cap:b * cap + m], wi)
        untouched(nm + ' boxes past count', out['boxes'][(b * cap + m) * 4:(b + 1) * cap * 4])
        for k in ('scores', 'labels', 'inds'):
            untouched('%s %s past count' % (nm, k), out[k][b * cap + m:(b + 1) * cap])
    for k, t in out.items():
        untouched('%s %s tail' % (name, k), t[(B * cap * (4 if k == 'boxes' else 1) if k != 'count' else B):])
    again = run_cands(boxes, box_stride, scores, factors, thr, batched)
    for k in out:
        same('%s second run %s' % (name, k), again[k], out[k].cpu())
    return out


def check_cands_ops(name, c):
    from pointtinybenchmark_amd import ops
    f = None if c['factors'] is None else dev(c['factors'])
    want = R.candidates_ref(c['boxes'], c['box_stride'], c['scores'], c['factors'], c['thr'])
    got = ops.nms_candidates(dev(c['boxes']), dev(c['scores']), float(c['thr']), f)
    for g, w, k in zip(got, want, ('boxes', 'scores', 'labels', 'inds')):
        same('%s ops %s' % (name, k), g, w)


@pytest.mark.parametrize('shape', R.CAND_SHAPES, ids=lambda s: 'n%d_c%d' % s)
def test_candidates_single(shape):
    cases = [c for c in R.cand_cases() if (c['n'], c['C']) == shape]
    assert len(cases) == len(R.CAND_PATTERNS) * len(R.CAND_FACTORS) * (1 if shape[1] == 1 else 2)
    for c in cases:
        check_cands(c['id'], c['boxes'], c['box_stride'], c['scores'], c['factors'], c['thr'], False)
        check_cands_ops(c['id'], c)


@pytest.mark.parametrize('shape', R.CAND_SHAPES, ids=lambda s: 'n%d_c%d' % s)
def test_candidates_batched_equal_each_image_alone(shape):
    from pointtinybenchmark_amd import ops
    for c in [c for c in R.cand_batched_cases() if (c['n'], c['C']) == shape]:
        out = check_cands(c['id'], c['boxes'], c['box_stride'], c['scores'], c['factors'], c['thr'], True)
        assert int(out['count'][1]) == 0, c['id']
        cap = c['n'] * c['C']
        for b in range(3):
            one = run_cands(c['boxes'][b], c['box_stride'], c['scores'][b], None if c['factors'] is None else c['factors'][b], c['thr'], False)
            assert int(one['count'][0]) == int(out['count'][b])
            for k in ('boxes', 'scores', 'labels', 'inds'):
                w = 4 if k == 'boxes' else 1
                same('%s image %d alone, %s' % (c['id'], b, k), one[k][:cap * w], out[k][b * cap * w:(b + 1) * cap * w].cpu())
        got = ops.nms_candidates_batched(dev(c['boxes']), dev(c['scores']), float(c['thr']), None if c['factors'] is None else dev(c['factors']))
        same(c['id'] + ' ops count', got[4], out['count'][:3].cpu())
        for b in range(3):
            m = int(out['count'][b])
            same('%s ops inds image %d' % (c['id'], b), got[3][b, :m], out['inds'][b * cap:b * cap + m].cpu())
            same('%s ops scores image %d' % (c['id'], b), got[1][b, :m], out['scores'][b * cap:b * cap + m].cpu())


# ---- NMS -------------------------------------------------------------------------------------------------------------
def run_nms(boxes, scores, labels, thr):
    n = len(scores)
    words = raw('cpr_nms_workspace', n)
    nblk = -(-n // R.TILE)
    assert words == max(min(n, R.BAND) * nblk + nblk + 1, 1 << max(n - 1, 0).bit_length()), words      # one band + the carried bits and count | the sort pad
    out = dict(keep=guard(n, torch.int64), num=guard(1, torch.int32))
    w = dict(order=ws(4 * n), boxes=ws(16 * n), mask=ws(8 * words))
    call('cpr_nms', boxes, scores, labels, n, float(thr), out['keep'], out['num'], w['order'], w['boxes'], w['mask'])
    torch.cuda.synchronize()
    for k, nbytes in (('order', 4 * n), ('boxes', 16 * n), ('mask', 8 * words)):
        untouched('workspace %s tail' % k, w[k][nbytes:])
    return out


def check_nms(name, p, thr, want):
    from pointtinybenchmark_amd import ops
    b, s, lab = dev(p['boxes']), dev(p['scores']), dev(p['labels'])
    out = run_nms(b, s, lab, thr)
    m = int(out['num'][0])
    kc = out['keep'].cpu()
    if m == len(want):
        print('%s: %d of %d keep indices differ from the reference' % (name, int((kc[:m] != torch.from_numpy(want)).sum()), m))
    assert m == len(want), '%s: num_keep %d != %d' % (name, m, len(want))
    same(name + ' keep', out['keep'][:m], want)
    untouched(name + ' keep past num_keep', out['keep'][m:])
    untouched(name + ' num tail', out['num'][1:])
    again = run_nms(b, s, lab, thr)
    same(name + ' second run keep', again['keep'], kc)
    same(name + ' second run num', again['num'], out['num'].cpu())
    same(name + ' ops', ops.nms(b, s, lab, float(thr)), want)
    return kc[:m]


@pytest.mark.parametrize('case', R.nms_cases(), ids=lambda c: c['id'])
def test_nms_single(case):
    check_nms(case['id'], R.nms_problem(case), case['thr'], R.nms_expected(case))


def _slabs(spec):
    cap, counts = spec['cap'], spec['counts']
    B = len(counts)
    boxes, scores = np.full((B, cap, 4), np.nan, dtype=np.float32), np.full((B, cap), np.nan, dtype=np.float32)
    labels = np.full((B, cap), -1, dtype=np.int32)
    for b, n in enumerate(counts):
        if n:
            p = R.batched_slab(n)
            boxes[b, :n], scores[b, :n], labels[b, :n] = p['boxes'], p['scores'], p['labels']
    return boxes, scores, labels


def run_nms_batched(boxes, scores, labels, counts, cap, thr):
    B = len(counts)
    nblk = -(-cap // 64)
    P = 1
    while P < cap:
        P <<= 1
    stride = max(cap * nblk, P)
    out = dict(keep=guard(B * cap, torch.int64), num=guard(B, torch.int32))
    w = dict(order=ws(4 * B * cap), boxes=ws(16 * B * cap), mask=ws(8 * B * stride))
    call('cpr_nms_batched', boxes, scores, labels, counts, B, cap, float(thr), out['keep'], out['num'], w['order'], w['boxes'], w['mask'], stride)
    torch.cuda.synchronize()
    for k, nbytes in (('order', 4 * B * cap), ('boxes', 16 * B * cap), ('mask', 8 * B * stride)):
        untouched('workspace %s tail' % k, w[k][nbytes:])
    return out


@pytest.mark.parametrize('spec', R.NMS_BATCHED, ids=lambda s: s['id'])
def test_nms_batched_equals_each_slab_alone(spec):
    from pointtinybenchmark_amd import ops
    cap, counts = spec['cap'], spec['counts']
    B = len(counts)
    boxes, scores, labels = (dev(a) for a in _slabs(spec))
    cnt = dev(np.array(counts, dtype=np.int32))
    out = run_nms_batched(boxes, scores, labels, cnt, cap, R.THIRD)
    for b, n in enumerate(counts):
        want = R.batched_expected(n)
        nm = '%s slab %d (n = %d)' % (spec['id'], b, n)
        assert int(out['num'][b]) == len(want), '%s: num_keep %d != %d' % (nm, int(out['num'][b]), len(want))
        same(nm + ' keep', out['keep'][b * cap:b * cap + len(want)], want)
        untouched(nm + ' keep past num_keep', out['keep'][b * cap + len(want):(b + 1) * cap])
        if n:
            one = run_nms(boxes[b, :n].contiguous(), scores[b, :n].contiguous(), labels[b, :n].contiguous(), R.THIRD)
            same(nm + ' alone', one['keep'][:n], out['keep'][b * cap:b * cap + n].cpu())
    untouched(spec['id'] + ' keep tail', out['keep'][B * cap:])
    untouched(spec['id'] + ' num tail', out['num'][B:])
    again = run_nms_batched(boxes, scores, labels, cnt, cap, R.THIRD)
    same(spec['id'] + ' second run keep', again['keep'], out['keep'].cpu())
    same(spec['id'] + ' second run num', again['num'], out['num'].cpu())
    keep, num = ops.nms_batched(boxes, scores, labels, cnt, float(R.THIRD))
    same(spec['id'] + ' ops num', num, out['num'][:B].cpu())
    for b in range(B):
        m = int(num[b])
        same('%s ops keep slab %d' % (spec['id'], b), keep[b, :m], out['keep'][b * cap:b * cap + m].cpu())


def test_nms_capacity_262144():
    """The largest problem ``cpr_nms`` takes: 32 bands, 4096 words of removed bits.  Disjoint boxes: the keep list is the stable argsort."""
    p = R.capacity_problem()
    b, s, lab = dev(p['boxes']), dev(p['scores']), dev(p['labels'])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run_nms(b, s, lab, R.THIRD)
    dt = time.perf_counter() - t0
    print('capacity n = %d: %.3f s wall (launches, synchronise and guard checks)' % (p['n'], dt))
    assert int(out['num'][0]) == p['n']
    same('capacity keep', out['keep'][:p['n']], p['expected'])
    untouched('capacity keep tail', out['keep'][p['n']:])


# ---- composed: multiclass_nms ----------------------------------------------------------------------------------------
CFG = dict(type='nms', iou_threshold=float(R.THIRD))


def _same_dets(name, got, want):
    same(name + ' dets', got[0], want[0])
    same(name + ' labels', got[1], want[1])


@pytest.mark.parametrize('n,C,seed,max_num,factors', [(300, 3, 0, -1, False), (300, 3, 0, 50, True), (65, 5, 1, -1, True)])
def test_multiclass_nms_equals_candidates_then_nms(n, C, seed, max_num, factors):
    from pointtinybenchmark_amd.core.post_processing import multiclass_nms
    boxes, scores = R.multiclass_problem(n, C, seed)
    f = R.cand_factors(n, 'zero') if factors else None
    want = R.multiclass_ref(boxes, 4, scores, f, R.MULTI_SCORE_THR, R.THIRD, max_num)
    got = multiclass_nms(dev(boxes), dev(scores), float(R.MULTI_SCORE_THR), CFG, max_num, None if f is None else dev(f), return_inds=True)
    _same_dets('multiclass_nms n%d c%d' % (n, C), got, want)
    same('multiclass_nms inds', got[2], want[2])
    assert 0 < len(want[0])


def test_multiclass_nms_batched_equals_candidates_then_nms():
    from pointtinybenchmark_amd.core.post_processing import multiclass_nms_batched
    n, C = 300, 3
    probs = [R.multiclass_problem(n, C, seed) for seed in (0, 2, 3)]
    scores = np.stack([p[1] for p in probs])
    scores[1, :, :C] = 0.125                                                      # an image without a candidate
    boxes = np.stack([p[0] for p in probs])
    for max_num in (-1, 50):
        out = multiclass_nms_batched(dev(boxes), dev(scores), float(R.MULTI_SCORE_THR), CFG, max_num)
        for b in range(3):
            _same_dets('multiclass_nms_batched image %d' % b, out[b], R.multiclass_ref(boxes[b], 4, scores[b], None, R.MULTI_SCORE_THR, R.THIRD, max_num)[:2])
        assert len(out[1][0]) == 0 and len(out[0][0]) > 0


def test_multiclass_nms_batched_above_16384_goes_image_by_image():
    from pointtinybenchmark_amd.core import post_processing as PP
    n, C = 5500, 3                                                                # capacity 16500 > 16384
    b0, s0 = R.multiclass_problem(n, C, 4, all_pass=True)                         # every pair a candidate: 16500 in the banded form
    b1, s1 = R.multiclass_problem(n, C, 5)
    s1[:, :C] *= np.float32(0.41)                                                 # a few hundred candidates
    boxes, scores = np.stack([b0, b1]), np.stack([s0, s1])
    assert n * C > PP.NMS_SLAB_MAX and int((s0[:, :C] > R.MULTI_SCORE_THR).sum()) == n * C
    out = PP.multiclass_nms_batched(dev(boxes), dev(scores), float(R.MULTI_SCORE_THR), CFG, -1)
    for b in range(2):
        _same_dets('image %d' % b, out[b], R.multiclass_ref(boxes[b], 4, scores[b], None, R.MULTI_SCORE_THR, R.THIRD)[:2])


# ---- refusals: null buffers, nothing can launch ------------------------------------------------------------------------
def test_refusals_and_empty_problems():
    S = _stream()
    for n, k in ((10000, 4097), (5, 6), (-1, 0), (5, -1)):
        assert raw('cpr_topk_desc', None, n, k, None, None, S) == R.ERR_ARG, (n, k)
        assert raw('cpr_topk_desc_batched', None, 2, n, k, None, None, S) == R.ERR_ARG, (n, k)
    assert raw('cpr_topk_desc_batched', None, -1, 5, 5, None, None, S) == R.ERR_ARG
    assert raw('cpr_topk_desc', None, 5, 5, None, None, S) == R.ERR_ARG                       # a launch would need its buffers
    assert raw('cpr_nms_workspace', R.NMS_MAX + 1) == R.ERR_ARG and raw('cpr_nms_workspace', R.NMS_MAX) > 0
    assert raw('cpr_nms_workspace', 0) == 1 and raw('cpr_nms_workspace', 3) == 5 and raw('cpr_nms_workspace', 8193) == 8192 * 129 + 129 + 1
    num = guard(3, torch.int32)
    assert raw('cpr_nms', None, None, None, R.NMS_MAX + 1, 0.5, None, num, None, None, None, S) == R.ERR_ARG
    assert raw('cpr_nms', None, None, None, -1, 0.5, None, num, None, None, None, S) == R.ERR_ARG
    assert raw('cpr_nms', None, None, None, 5, 0.5, None, num, None, None, None, S) == R.ERR_ARG
    assert raw('cpr_nms_batched', None, None, None, num, 3, R.NMS_BATCHED_CAP_MAX + 1, 0.5, None, num, None, None, None, 1 << 40, S) == R.ERR_ARG
    # ws_stride too small: the pointer check comes first, so these buffers are real -- full-sized for cap = 200 and zeroed (counts 0)
    cap, nblk, P = 200, 4, 256
    one = torch.zeros(3 * cap * 4, device='cuda')
    onei, onel = torch.zeros(3 * cap, dtype=torch.int32, device='cuda'), torch.zeros(3 * cap * nblk, dtype=torch.int64, device='cuda')
    for stride in (cap * nblk - 1, P - 1, 0, -1):
        assert raw('cpr_nms_batched', one, one, onei, onei, 3, cap, 0.5, onel, num, onei, one, onel, stride, S) == R.ERR_ARG, stride
    assert raw('cpr_nms_batched', one, one, onei, onei, 3, 40, 0.5, onel, num, onei, one, onel, 50, S) == R.ERR_ARG      # cap nblk = 40 <= 50 < the sort pad 64
    for bs in (0, 3, 5, 8, -4):
        assert raw('cpr_nms_candidates', None, bs, None, None, 4, 3, 0.5, None, None, None, None, num, S) == R.ERR_ARG, bs
        assert raw('cpr_nms_candidates_batched', None, bs, None, None, 2, 4, 3, 0.5, None, None, None, None, num, S) == R.ERR_ARG, bs
    assert raw('cpr_nms_candidates', None, 4, None, None, 4, 0, 0.5, None, None, None, None, num, S) == R.ERR_ARG          # C == 0
    assert raw('cpr_nms_candidates', None, 4, None, None, 4, 3, 0.5, None, None, None, None, None, S) == R.ERR_ARG
    torch.cuda.synchronize()
    untouched('refused calls: num', num)
    # empty problems: OK, nothing launched, only the counts are zeroed
    assert raw('cpr_topk_desc', None, 7, 0, None, None, S) == 0 and raw('cpr_topk_desc', None, 0, 0, None, None, S) == 0
    assert raw('cpr_topk_desc_batched', None, 3, 7, 0, None, None, S) == 0 and raw('cpr_topk_desc_batched', None, 0, 7, 7, None, None, S) == 0
    for name, args, B in (('cpr_nms_candidates', (None, 4, None, None, 0, 3, 0.5, None, None, None, None), 1),
                          ('cpr_nms_candidates_batched', (None, 12, None, None, 2, 0, 3, 0.5, None, None, None, None), 2),
                          ('cpr_nms', (None, None, None, 0, 0.5, None), 1)):
        cnt = guard(3, torch.int32)
        tail = (cnt, None, None, None, S) if name == 'cpr_nms' else (cnt, S)
        assert raw(name, *(args + tail)) == 0, name
        torch.cuda.synchronize()
        assert cnt[:B].tolist() == [0] * B, name
        untouched(name + ' past the counts', cnt[B:])
    cnt = guard(3, torch.int32)
    assert raw('cpr_nms_batched', None, None, None, num, 2, 0, 0.5, None, cnt, None, None, None, 0, S) == 0
    torch.cuda.synchronize()
    assert cnt[:2].tolist() == [0, 0]
    untouched('cpr_nms_batched cap 0 past the counts', cnt[2:])
    assert raw('cpr_nms_batched', None, None, None, None, 0, 200, 0.5, None, None, None, None, None, 0, S) == 0           # B == 0
