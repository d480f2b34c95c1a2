"""Exact references of the detection tail -- ``topk_desc_kernel``, ``nms_candidates_kernel``, ``nms_prepare_kernel``, ``nms_mask_kernel``
and ``nms_scan_kernel`` (csrc/postproc.hip) -- and the case tables that pin them at their seams.  CPU only, numpy float32.

These kernels have exact answers: integer indices, and fp32 values with ONE rounding per operation (``__f*_rn`` throughout, no
contraction).  numpy's float32 ufuncs round once per operation too, so every reference below performs the kernels' operations in the
kernels' order and the bar is EQUALITY, bit for bit.  ``oracle.cpr_oracle`` is not used here; tests/test_postproc_instances_host.py
holds the two together.

Contracts restated:
  topk_ref        stable descending order, +0.0 and -0.0 equal (ties by lower index); values are ``scores[idx]`` with their original bits.
  candidates_ref  every (proposal, class) pair whose RAW score is ``> thr``, row-major (proposal, class); the background column (the
                  last) is never a candidate; the stored score is ``fp32(score * factor[proposal])`` -- a zero factor stores 0 and keeps
                  the pair; boxes are shared (box_stride 4) or per class (box_stride 4 C).
  nms_ref         offset ``fp32(label) * fp32(max + 1)`` (max over every coordinate of the problem), added to the four coordinates;
                  area ``(x2 - x1) * (y2 - y1)``; ``inter / ((ai + aj) - inter)``; suppression where that is strictly ``> thr``; 0 / 0 =
                  NaN never suppresses; greedy scan in stable descending score order (a removed row suppresses nothing); the keep list
                  holds input indices in that order.
NaN scores (and NaN coordinates) are out of contract: the sort key of a NaN is not ordered against the references' comparisons.  No
table below holds one.

Every table row has an ``id`` and a ``why``.  The NMS tables also record where each planted structure landed (sorted ranks and input
indices); the host test asserts the coverage conditions from that data.  ``variant=`` selects a DELIBERATELY WRONG reference (``VARIANTS``);
only the sharpness test of the host file passes it.

Kernel seams (restated, the host test ties each to the source text):
  top-k       one block of 1024 threads; 4 radix passes over key bytes 3..0; the gather walks the input 1024 at a time, equal keys ranked by
              wave ballots with the running rank carried in LDS; k <= 4096.
  candidates  one block of 1024 threads per image walks n C flat pairs 1024 at a time, ordered compaction by wave ballots.
  NMS         sort padded to a power of two; 64 x 64 mask tiles; whole mask for n <= 8192, bands of 8192 rows above with the removed
              bits and the keep count carried from band to band; n <= 262144.
"""
import functools

import numpy as np

F32 = np.float32
BLOCK = 1024              # threads of the top-k and candidate blocks = elements per gather pass
WAVE = 64
TOPK_MAX = 4096
TILE = 64
BAND = 8192
NMS_MAX = 64 * 4096
NMS_BATCHED_CAP_MAX = 16384
ERR_ARG = -1001
THIRD = F32(1.0) / F32(3.0)                       # fp32(1/3) = fdiv_rn(128, 384): the IoU of two 16 x 16 boxes shifted by 8
THIRD_BELOW = np.nextafter(THIRD, F32(0))

VARIANTS = {
    'iou_ge': 'IoU >= thr suppresses',
    'filter_ge': 'candidate filter score >= thr',
    'filter_scaled': 'candidate filter applied to score * factor',
    'removed_suppress': 'removed rows still suppress',
    'clear_8192': 'removed bits cleared at every multiple of 8192',
    'count_restart': 'keep count restarted per band',
    'ignore_intra_tile': 'pairs inside one 64-tile ignored',
    'no_offset': 'class offset dropped',
    'class_max': "class offset from this class's max only",
    'tie_higher': 'ties taken by the higher index',
    'thr_tie_highest': 'top-k threshold ties taken from the highest indices',
    'neg_zero_below': '-0.0 ordered below +0.0',
}


# ---- references ------------------------------------------------------------------------------------------------------
def f2key(s):
    """The monotone sort key WITHOUT the canonical zero (uint32; -0.0 strictly below +0.0, as the kernels keyed it before they mapped
    -0.0 to +0.0): used by the 'neg_zero_below' variant only."""
    u = np.ascontiguousarray(s, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order_desc(s, variant=None):
    """Stable descending argsort of fp32 scores, +-0 equal, ties by lower index."""
    s = np.ascontiguousarray(s, dtype=F32).ravel()
    if variant == 'tie_higher':
        return (len(s) - 1 - np.argsort(-s[::-1], kind='stable')).astype(np.int64)
    if variant == 'neg_zero_below':
        return np.argsort(-f2key(s).astype(np.int64), kind='stable').astype(np.int64)
    return np.argsort(-s, kind='stable').astype(np.int64)


def topk_ref(scores, k, variant=None):
    """-> (values fp32 (k), indices int64 (k)) of one segment."""
    s = np.ascontiguousarray(scores, dtype=F32).ravel()
    order = order_desc(s, variant)
    idx = order[:k]
    if variant == 'thr_tie_highest' and k > 0:
        T = s[order[k - 1]]
        gt = order[s[order] > T]
        eq = np.nonzero(s == T)[0]
        idx = np.concatenate([gt, eq[len(eq) - (k - len(gt)):]]).astype(np.int64)
    return s[idx].copy(), idx.astype(np.int64)


def topk_take_eq(scores, k):
    """(T, number of keys > T, take_eq): the k-th largest value and how many of its copies the gather must take."""
    s = np.ascontiguousarray(scores, dtype=F32).ravel()
    T = s[order_desc(s)[k - 1]]
    gt = int((s > T).sum())
    return T, gt, k - gt


def candidates_ref(boxes, box_stride, scores, factors, thr, variant=None):
    """boxes (n, box_stride), scores (n, C + 1), factors (n) or None -> (cand_boxes (m, 4), cand_scores (m), cand_labels int32 (m),
    cand_inds int64 (m)); m is the count."""
    scores = np.ascontiguousarray(scores, dtype=F32)
    n, C = scores.shape[0], scores.shape[1] - 1
    boxes = np.ascontiguousarray(boxes, dtype=F32).reshape(n, box_stride)
    assert box_stride in (4, 4 * C)
    thr = F32(thr)
    raw = scores[:, :C].reshape(-1)
    row, cls = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    stored = raw if factors is None else (raw * np.ascontiguousarray(factors, dtype=F32)[row]).astype(F32)
    judged = stored if variant == 'filter_scaled' else raw
    take = np.nonzero(judged >= thr if variant == 'filter_ge' else judged > thr)[0]
    r, c = row[take], cls[take]
    b4 = boxes.reshape(n, -1, 4)
    cb = b4[r, c if box_stride > 4 else 0]
    return cb.reshape(-1, 4).copy(), stored[take].astype(F32), c.astype(np.int32), take.astype(np.int64)


def offset_boxes(boxes, labels, variant=None):
    """boxes + fp32(label) * fp32(max + 1): two roundings per coordinate."""
    boxes = np.ascontiguousarray(boxes, dtype=F32).reshape(-1, 4)
    lab = np.asarray(labels).astype(F32)
    if variant == 'no_offset':
        return boxes.copy()
    if variant == 'class_max':
        off1 = np.zeros(len(boxes), dtype=F32)
        for c in np.unique(labels):
            off1[np.asarray(labels) == c] = boxes[np.asarray(labels) == c].max() + F32(1)
    else:
        off1 = F32(boxes.max()) + F32(1)
    o = (lab * off1).astype(F32)
    return (boxes + o[:, None]).astype(F32)


def iou_row(b, area, i, j0=None):
    """fp32 IoU of sorted row i against rows j0.. (default i + 1..), in the mask kernel's order of operations."""
    j0 = i + 1 if j0 is None else j0
    w = np.maximum(F32(0), np.minimum(b[i, 2], b[j0:, 2]) - np.maximum(b[i, 0], b[j0:, 0]))
    h = np.maximum(F32(0), np.minimum(b[i, 3], b[j0:, 3]) - np.maximum(b[i, 1], b[j0:, 1]))
    inter = w * h
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / ((area[i] + area[j0:]) - inter)


def nms_ref(boxes, scores, labels, thr, variant=None):
    """-> keep: input indices (int64) of the kept boxes in descending score order."""
    boxes = np.ascontiguousarray(boxes, dtype=F32).reshape(-1, 4)
    n = len(boxes)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    thr = F32(thr)
    order = order_desc(scores, variant)
    b = offset_boxes(boxes, labels, variant)[order]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    removed = np.zeros(n, dtype=bool)
    keep = np.zeros(n, dtype=np.int64)
    cnt = 0
    for i in range(n):
        if variant == 'clear_8192' and i and i % BAND == 0:
            removed[:] = False
        if variant == 'count_restart' and i and i % BAND == 0:
            cnt = 0
        kept = not removed[i]
        if kept:
            keep[cnt] = order[i]
            cnt += 1
        if (kept or variant == 'removed_suppress') and i + 1 < n:
            ovr = iou_row(b, area, i)
            hit = ovr >= thr if variant == 'iou_ge' else ovr > thr
            if variant == 'ignore_intra_tile':
                hit[:(i // TILE + 1) * TILE - (i + 1)] = False
            removed[i + 1:] |= hit
    return keep[:cnt].copy()


def multiclass_ref(boxes, box_stride, scores, factors, score_thr, iou_thr, max_num=-1):
    """candidates, then NMS of the candidate list -> (dets (m, 5), labels int64 (m), inds int64 (m))."""
    cb, cs, cl, ci = candidates_ref(boxes, box_stride, scores, factors, score_thr)
    keep = nms_ref(cb, cs, cl, iou_thr)
    if max_num > 0:
        keep = keep[:max_num]
    return np.concatenate([cb[keep], cs[keep, None]], axis=1).astype(F32), cl[keep].astype(np.int64), ci[keep]


def has_pm0(x):
    return bool((np.asarray(x) == 0).any())


# ---- top-k table -----------------------------------------------------------------------------------------------------
TIE_T = F32(0.5)


def _rng(*seed):
    return np.random.RandomState(list(seed))


def topk_random(n, seed=0):
    return _rng(1, n, seed).standard_normal(n).astype(F32)


def topk_all_equal(n):
    return np.full(n, F32(0.625))


def topk_planted_tie(n):
    """Copies of T at every index i with i % 5 < 3 (3000 of n = 5000), 300 distinct values above T and the rest distinct below T at the
    other indices, in a fixed shuffle."""
    s = np.empty(n, dtype=F32)
    eq = np.arange(n) % 5 < 3
    s[eq] = TIE_T
    other = np.nonzero(~eq)[0]
    other = other[_rng(2, n).permutation(len(other))]
    above, below = other[:300], other[300:]
    s[above] = TIE_T + (np.arange(300) + 1).astype(F32) * F32(2.0 ** -10)
    s[below] = TIE_T - (np.arange(len(below)) + 1).astype(F32) * F32(2.0 ** -13)
    return s


def topk_mixed_sign(n):
    """Negatives, +-inf, denormals and both zeros interleaved: every residue of i % 8 is one kind."""
    r = _rng(3, n)
    mag = np.exp(r.uniform(-20, 20, n)).astype(F32)
    den = (r.randint(1, 1 << 22, n).astype(np.uint32)).view(F32)                 # positive denormals
    i = np.arange(n)
    s = np.select([i % 8 == 0, i % 8 == 1, i % 8 == 2, i % 8 == 3, i % 8 == 4, i % 8 == 5, i % 8 == 6],
                  [mag, -mag, np.zeros(n, F32), -np.zeros(n, F32), den, -den, np.where(i % 16 == 6, np.inf, -np.inf).astype(F32)],
                  (mag * F32(0.5))).astype(F32)
    return s


def topk_last_byte(n):
    """[1, 1 + 255 ulp]: bytes 3..1 of every key agree, only the last radix pass discriminates (and ties are frequent)."""
    return (np.uint32(0x3F800000) + _rng(4, n).randint(0, 256, n).astype(np.uint32)).view(F32)


def topk_top_byte(n):
    """Bit patterns (b << 24) | 0x00400000, b = i * 37 % 256: the set differs in the top byte only, both signs, no inf / NaN."""
    b = (np.arange(n) * 37 % 256).astype(np.uint32)
    return ((b << np.uint32(24)) | np.uint32(0x00400000)).view(F32)


def _tk(id_, scores, k, why):
    return dict(id=id_, scores=scores, k=k, why=why, pm0=has_pm0(scores))


@functools.lru_cache(None)
def topk_cases():
    c = []
    whys = {(1, 1): 'one element', (63, 63): 'one wave less a lane, full sort', (1024, 1024): 'exactly one gather pass, k = n',
            (1025, 512): 'one element in a second gather pass', (4096, 4096): 'k at its ceiling, the bitonic sort without pad',
            (4097, 4096): 'k at its ceiling, one element rejected', (4099, 1): 'k = 1 of an odd length'}
    for (n, k), why in whys.items():
        c.append(_tk('random_n%d_k%d' % (n, k), topk_random(n), k, why))
    c.append(_tk('all_equal_n5000_k1500', topk_all_equal(5000), 1500, 'no key > T; the equal keys span five passes; answer 0..1499'))
    c.append(_tk('planted_tie_n5000_k1400', topk_planted_tie(5000), 1400,
                 '300 above T, 3000 copies of T in every pass: take_eq = 1100 ends mid-wave in the second pass'))
    c.append(_tk('mixed_sign_n1500_k1500', topk_mixed_sign(1500), 1500, 'negative half of the key map, +-inf, denormals, +-0: full sort'))
    c.append(_tk('mixed_sign_n1500_k700', topk_mixed_sign(1500), 700, 'the k-th place falls among the zeros / denormals'))
    c.append(_tk('last_byte_n3000_k1000', topk_last_byte(3000), 1000, 'only radix byte 0 discriminates'))
    c.append(_tk('top_byte_n2048_k777', topk_top_byte(2048), 777, 'only radix byte 3 discriminates; 8 copies of each value'))
    return c


@functools.lru_cache(None)
def topk_batched_cases():
    n = 4099
    rows = [('random', topk_random(n, 1)), ('all_equal', topk_all_equal(n)), ('planted_tie', topk_planted_tie(n)),
            ('mixed_sign', topk_mixed_sign(n)), ('last_byte', topk_last_byte(n))]
    S = np.stack([r for _, r in rows])
    return [dict(id='b5_n4099_k%d' % k, scores=S, k=k, rows=[r for r, _ in rows], pm0=True,
                 why='segments start at multiples of 4099: off any alignment; ' + why)
            for k, why in ((1400, 'take_eq = 1100 in the planted row'), (4096, 'k at its ceiling'), (1, 'k = 1'))]


# ---- candidate table -------------------------------------------------------------------------------------------------
CAND_THR = F32(0.3)
CAND_SHAPES = [(1, 1), (1000, 1), (1024, 1), (1025, 1), (700, 3), (37, 80)]
CAND_PATTERNS = {
    'none': 'no pair passes: count 0, nothing written',
    'all': 'every pair passes: the compaction is the identity',
    'lane0': 'only lane 0 of each wave passes',
    'lane63': 'only lane 63 of each wave passes',
    'eq_thr': 'scores exactly thr (not taken) between scores one ulp above (taken) and one ulp below',
    'dense': 'dense random',
}
CAND_FACTORS = {'absent': 'no factors: the raw score is stored', 'present': 'fp32(score * factor)',
                'zero': 'a zero factor stores 0 and keeps the pair'}


def cand_scores(n, C, pattern):
    """(n, C + 1); the background column always holds 0.99 > thr and is never a candidate."""
    j = np.arange(n * C)
    lo, hi = F32(0.125), F32(0.875)
    if pattern == 'none':
        fg = np.where(j % 3 == 0, CAND_THR, lo)
    elif pattern == 'all':
        fg = np.full(n * C, hi)
    elif pattern == 'lane0':
        fg = np.where(j % WAVE == 0, hi, lo)
    elif pattern == 'lane63':
        fg = np.where(j % WAVE == WAVE - 1, hi, lo)
    elif pattern == 'eq_thr':
        fg = np.select([j % 3 == 0, j % 3 == 1], [CAND_THR, np.nextafter(CAND_THR, F32(1))], np.nextafter(CAND_THR, F32(0)))
    else:
        fg = _rng(5, n, C).uniform(0, 1, n * C)
    s = np.empty((n, C + 1), dtype=F32)
    s[:, :C] = fg.astype(F32).reshape(n, C)
    s[:, C] = F32(0.99)
    return s


def cand_boxes(n, C, box_stride, seed=0):
    return _rng(6, n, C, box_stride, seed).uniform(-50, 500, (n, box_stride)).astype(F32)


def cand_factors(n, kind, seed=0):
    if kind == 'absent':
        return None
    f = _rng(7, n, seed).uniform(0.5, 1.5, n).astype(F32)
    if kind == 'zero':
        f[::3] = 0
    return f


@functools.lru_cache(None)
def cand_cases():
    c = []
    for n, C in CAND_SHAPES:
        for pat in CAND_PATTERNS:
            for fk in CAND_FACTORS:
                for bs in sorted({4, 4 * C}):
                    c.append(dict(id='n%d_c%d_%s_%s_bs%d' % (n, C, pat, fk, bs), n=n, C=C, pattern=pat, factors_kind=fk, box_stride=bs,
                                  boxes=cand_boxes(n, C, bs), scores=cand_scores(n, C, pat), factors=cand_factors(n, fk), thr=CAND_THR,
                                  why='%s; %s; box_stride %s' % (CAND_PATTERNS[pat], CAND_FACTORS[fk], '4' if bs == 4 else '4 C')))
    return c


@functools.lru_cache(None)
def cand_batched_cases():
    """B = 3: (dense, none, lane63) -- the middle image has no candidate."""
    c = []
    for n, C in CAND_SHAPES:
        for fk in ('absent', 'zero'):
            for bs in sorted({4, 4 * C}):
                pats = ('dense', 'none', 'lane63')
                c.append(dict(id='b3_n%d_c%d_%s_bs%d' % (n, C, fk, bs), n=n, C=C, patterns=pats, box_stride=bs, thr=CAND_THR, factors_kind=fk,
                              boxes=np.stack([cand_boxes(n, C, bs, b) for b in range(3)]), scores=np.stack([cand_scores(n, C, p) for p in pats]),
                              factors=None if fk == 'absent' else np.stack([cand_factors(n, fk, b) for b in range(3)]),
                              why='three slabs of capacity n C, the middle one empty'))
    return c


# ---- NMS table -------------------------------------------------------------------------------------------------------
NMS_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097, 8191, 8192, 8193, 8256, 16384, 16385, 16449)
# layout -> the greedy chains (a, b, c) by sorted rank; chains that share a rank cannot share an input
CHAINS = {
    0: [(0, 1, 2), (62, 63, 64), (8190, 8191, 8192), (200, 16390, 16400)],
    1: [(63, 64, 65), (8191, 8192, 8193)],
    2: [(100, 8191, 16384)],
}
THR_PAIRS = [(4, 6), (20, 70), (8189, 8200)]        # inside a tile, across the 63|64 tile seam, across the 8191|8192 band seam
IDENTICAL = (8, 9)
ZERO_AREA = (10, 11, 12)
TWO_CLASS = (14, 15)
TIE_RUNS = [(61, 66), (8188, 8195)]
GRID_W, PITCH, GRID_Y0 = 128, 48, 256


def _grid_box(r):
    x, y = (r % GRID_W) * PITCH, (r // GRID_W) * PITCH + GRID_Y0
    return np.stack([x, y, x + 16, y + 16], axis=-1).astype(F32)


def grid_problem(n, layout=0, pm0=False):
    """One NMS input on the integer grid.  Built in sorted-rank order, then hidden by a fixed permutation.

    Background: rank r owns a 16 x 16 box in its own cell (label r % 3); ranks r % 7 == 3 are the cell of rank r - 1 shifted by 4
    (IoU 0.6, same label: suppressed where r - 1 is kept), r % 7 == 5 the cell of r - 1 shifted by 12 (IoU 1/7: kept), r % 11 == 6
    above 700 the cell of rank r - 640 shifted by 4 (suppressed from ten tiles back).  Planted structures live in a strip y < 200, 64
    apart, so they meet nothing else."""
    r = np.arange(n)
    box = _grid_box(r)
    lab = (r % 3).astype(np.int32)
    for cond, src, dx in ((r % 7 == 3, r - 1, 4), (r % 7 == 5, r - 1, 12), ((r % 11 == 6) & (r >= 700), r - 640, 4)):
        cond = cond & (src >= 0)
        box[cond] = _grid_box(src[cond]) + F32(dx) * np.array([1, 0, 1, 0], dtype=F32)
        lab[cond] = (src[cond] % 3).astype(np.int32)
    planted = dict(chains=[], thr_pairs=[], identical=[], zero_area=[], two_class=[], ties=[], pm0=[])
    slot = [0]

    def put(rank, x1, y1, x2, y2, label):
        x0 = 64 * slot[0]
        box[rank] = np.array([x0 + x1, y1, x0 + x2, y2], dtype=F32)
        lab[rank] = label

    def fits(*ranks):
        return max(ranks) < n

    for a, b, c in CHAINS[layout]:
        if fits(a, b, c):
            put(a, 0, 0, 16, 16, 1), put(b, 4, 0, 28, 16, 1), put(c, 16, 0, 32, 16, 1)
            planted['chains'].append((a, b, c))
            slot[0] += 1
    pairs = [(0, 1)] if n == 2 else [p for p in THR_PAIRS if fits(*p)] if layout == 0 else []
    for p, q in pairs:
        put(p, 0, 32, 16, 48, 2), put(q, 8, 32, 24, 48, 2)
        planted['thr_pairs'].append((p, q))
        slot[0] += 1
    if layout == 0:
        if fits(*IDENTICAL):
            for k in IDENTICAL:
                put(k, 0, 64, 16, 80, 0)
            planted['identical'].append(IDENTICAL)
            slot[0] += 1
        if fits(*ZERO_AREA):
            for k in ZERO_AREA:
                put(k, 7, 96, 7, 96, 1)
            planted['zero_area'].append(ZERO_AREA)
            slot[0] += 1
        if fits(*TWO_CLASS):
            put(TWO_CLASS[0], 0, 128, 16, 144, 0), put(TWO_CLASS[1], 0, 128, 16, 144, 1)
            planted['two_class'].append(TWO_CLASS)
            slot[0] += 1
    score = ((n - r).astype(F32) * F32(2.0 ** -18)).astype(F32)          # strictly decreasing, exact, in (0, 1]
    runs = [(r0, min(r1, n - 1)) for r0, r1 in TIE_RUNS if r0 + 1 < n]
    for r0, r1 in runs:
        score[r0:r1 + 1] = score[r0]
    if pm0:
        assert n >= 4 and all(r1 < n - 2 for _, r1 in runs)
        score[n - 2], score[n - 1] = F32(-0.0), F32(0.0)                   # equal: the lower input index (the -0.0) goes first
        runs = runs + [(n - 2, n - 1)]
        planted['pm0'].append((n - 2, n - 1))
    planted['ties'] = runs
    perm = _rng(8, n, layout).permutation(n)                             # perm[rank] = input index
    for r0, r1 in runs:
        perm[r0:r1 + 1] = np.sort(perm[r0:r1 + 1])                        # inside a run the planted order is the index order
    boxes, scores, labels = np.empty_like(box), np.empty_like(score), np.empty_like(lab)
    boxes[perm], scores[perm], labels[perm] = box, score, lab
    return dict(n=n, boxes=boxes, scores=scores, labels=labels, perm=perm, planted=planted, pm0=pm0)


def float_problem():
    """256 pairs of 16 x 16 boxes shifted by 8 at coordinates x.37, 80 classes, max coordinate ~1225: the un-offset IoU is 1/3 up to
    the rounding of the .37 coordinates, and the class offset (up to 79 * 1225 ~ 1e5, where an ulp is 1/128) rounds every edge again --
    whether a pair's IoU is above fp32(1/3) depends on those roundings (the host test counts the pairs whose outcome they decide).
    Pair i sits at sorted ranks (2 i, 2 i + 1), label 7 i % 80."""
    P = 256
    i = np.arange(P)
    x0, y0 = (80 * (i % 16)).astype(np.float64) + 0.37, (80 * (i // 16)).astype(np.float64) + 0.37
    A = np.stack([x0, y0, x0 + 16, y0 + 16], axis=-1).astype(F32)
    B = np.stack([x0 + 8, y0, x0 + 24, y0 + 16], axis=-1).astype(F32)
    n = 2 * P
    box = np.empty((n, 4), dtype=F32)
    box[0::2], box[1::2] = A, B
    lab = np.repeat((7 * i % 80).astype(np.int32), 2)
    r = np.arange(n)
    score = ((n - r).astype(F32) * F32(2.0 ** -18)).astype(F32)
    perm = _rng(9).permutation(n)
    boxes, scores, labels = np.empty_like(box), np.empty_like(score), np.empty_like(lab)
    boxes[perm], scores[perm], labels[perm] = box, score, lab
    planted = dict(chains=[], thr_pairs=[], identical=[], zero_area=[], two_class=[], ties=[], pm0=[], float_pairs=[(2 * k, 2 * k + 1) for k in range(P)])
    return dict(n=n, boxes=boxes, scores=scores, labels=labels, perm=perm, planted=planted, pm0=False)


def negative_problem():
    """Every coordinate negative, maximum -100: max + 1 = -99, so class c is shifted by -99 c and the classes OVERLAP (the published
    algorithm does the same).  Rank 0 (class 0) at [-500, -484] and rank 1 (class 1) at [-401, -385] coincide after the offset: rank 1
    is suppressed ACROSS classes; rank 2 (class 1) at [-500, -484] coincides with rank 0 before the offset and is kept."""
    n = 70
    r = np.arange(n)
    x, y = -5000 + 40 * (r % 8), -3000 + 40 * (r // 8)
    box = np.stack([x, y, x + 16, y + 16], axis=-1).astype(F32)
    lab = (r % 2).astype(np.int32)
    box[0], lab[0] = (-500, -500, -484, -484), 0
    box[1], lab[1] = (-401, -401, -385, -385), 1
    box[2], lab[2] = (-500, -500, -484, -484), 1
    box[3], lab[3] = (-116, -116, -100, -100), 0                           # holds the maximum, -100
    score = ((n - r).astype(F32) * F32(2.0 ** -18)).astype(F32)
    perm = _rng(10).permutation(n)
    boxes, scores, labels = np.empty_like(box), np.empty_like(score), np.empty_like(lab)
    boxes[perm], scores[perm], labels[perm] = box, score, lab
    planted = dict(chains=[], thr_pairs=[], identical=[], zero_area=[], two_class=[], ties=[], pm0=[], negative=[(0, 1, 2)])
    return dict(n=n, boxes=boxes, scores=scores, labels=labels, perm=perm, planted=planted, pm0=False)


def class_max_problem():
    """The offset uses the maximum over EVERY class: class 1's only box [83, 99] goes to [283, 299]; with class 1's own maximum it would go
    to [183, 199], on top of the higher-scored class-0 box there."""
    box = np.array([[0, 0, 16, 16], [183, 183, 199, 199], [83, 83, 99, 99]], dtype=F32)
    lab = np.array([0, 0, 1], dtype=np.int32)
    score = np.array([0.75, 0.5, 0.25], dtype=F32)
    planted = dict(chains=[], thr_pairs=[], identical=[], zero_area=[], two_class=[], ties=[], pm0=[])
    return dict(n=3, boxes=box, scores=score, labels=lab, perm=np.arange(3), planted=planted, pm0=False)


def _nc(id_, builder, thr, why):
    return dict(id=id_, builder=builder, thr=F32(thr), why=why)


@functools.lru_cache(None)
def nms_cases():
    """Rows are light: ``nms_problem(row)`` builds (and caches) the arrays, ``nms_expected(row)`` the reference keep list."""
    seam = {1: 'one box', 2: 'one pair: the threshold pair alone', 63: 'a wave less a lane', 64: 'exactly one tile, sort without pad', 65: 'one row in a second tile',
            127: 'two tiles less a row', 128: 'two tiles exactly', 129: 'three tiles, sort pad 256', 4096: 'sort without pad, 64 tiles', 4097: 'sort pad 8192',
            8191: 'whole mask, one row short of the band', 8192: 'the largest whole-mask problem', 8193: 'first banded size: one row in band 1',
            8256: 'band 1 holds one whole tile', 16384: 'two full bands, sort without pad', 16385: 'one row in band 2', 16449: 'band 2 holds a tile and a row'}
    c = []
    for n in NMS_SIZES:
        c.append(_nc('grid_n%d_L0' % n, ('grid', n, 0, False), THIRD, seam[n] + '; IoU 128/384 == thr: kept'))
        if n <= 129 or n == 8193:
            c.append(_nc('grid_n%d_L0_below' % n, ('grid', n, 0, False), THIRD_BELOW, seam[n] + '; thr one ulp below 128/384: suppressed'))
    for n in (127, 8256, 16449):
        c.append(_nc('grid_n%d_L1' % n, ('grid', n, 1, False), THIRD, 'chains (63, 64, 65) / (8191, 8192, 8193): a is the last row of a tile / band'))
    c.append(_nc('grid_n16385_L2', ('grid', 16385, 2, False), THIRD, 'chain (100, 8191, 16384): a, b, c in three bands, c alone in band 2'))
    for n in (129, 8256):
        c.append(_nc('grid_n%d_pm0' % n, ('grid', n, 0, True), THIRD, 'the last two scores are -0.0 (lower index) and +0.0: equal, index order'))
    c.append(_nc('float_x37_c80', ('float',), THIRD, 'the class offset rounds the edges: near-threshold outcomes depend on it'))
    c.append(_nc('negative_max', ('negative',), THIRD, 'negative maximum: max + 1 = -99, classes overlap after the offset'))
    c.append(_nc('class_max_trap', ('class_max',), THIRD, 'the offset uses the maximum over every class'))
    return c


@functools.lru_cache(None)
def _problem(builder):
    kind = builder[0]
    if kind == 'grid':
        return grid_problem(*builder[1:])
    return {'float': float_problem, 'negative': negative_problem, 'class_max': class_max_problem}[kind]()


def nms_problem(row):
    return _problem(row['builder'])


@functools.lru_cache(None)
def _expected(builder, thr_bits):
    p = _problem(builder)
    return nms_ref(p['boxes'], p['scores'], p['labels'], np.uint32(thr_bits).view(F32))


def nms_expected(row):
    return _expected(row['builder'], int(row['thr'].view(np.uint32)))


# capacity: the largest problem cpr_nms takes.  Pairwise disjoint boxes (two classes), scores in runs of four equal values: the keep
# list is the stable argsort -- no O(n^2) host loop.
def capacity_problem(n=NMS_MAX):
    r = np.arange(n)
    x, y = (r % 512) * 32, (r // 512) * 32
    boxes = np.stack([x, y, x + 16, y + 16], axis=-1).astype(F32)
    labels = (r % 2).astype(np.int32)
    scores = ((_rng(11, n).permutation(n) // 4 + 1).astype(F32) * F32(2.0 ** -16)).astype(F32)
    return dict(n=n, boxes=boxes, scores=scores, labels=labels, expected=order_desc(scores))


# batched NMS: slabs of the grid table, padded to cap
NMS_BATCHED = [dict(id='cap200', cap=200, counts=(0, 1, 64, 65, 200), why='per-image nblk 0, 1, 1, 2, 4 below nblk_cap 4: the mask row stride is per image'),
               dict(id='cap8192', cap=8192, counts=(8191, 8192, 0), why='the largest whole-mask slabs next to an empty one; nblk 128 of 128')]


def batched_slab(count):
    return _problem(('grid', count, 0, False)) if count else None


@functools.lru_cache(None)
def batched_expected(count):
    p = batched_slab(count)
    return nms_ref(p['boxes'], p['scores'], p['labels'], THIRD) if count else np.zeros(0, np.int64)


# composed: multiclass_nms = candidates, then NMS
def multiclass_problem(n, C, seed, all_pass=False):
    """Proposals on the grid table's boxes (shared by the classes), scores (n, C + 1) uniform (or all above the threshold)."""
    p = _problem(('grid', n, 0, False))
    s = _rng(12, n, C, seed).uniform(0, 1, (n, C + 1)).astype(F32)
    if all_pass:
        s = (s * F32(0.5) + F32(0.5)).astype(F32)
    return p['boxes'].copy(), s


MULTI_SCORE_THR = F32(0.4)
