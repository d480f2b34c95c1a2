"""-m gpu: the forward CPR point kernels of csrc/cpr_points.hip (cpr_box_centers, cpr_neg_mask_loss, cpr_bag_sample, cpr_grid_bag,
cpr_mil_loss, cpr_refine) through the ops.* wrappers on synthetic inputs, each against the fp64 reference and the derived bars of
tests/cpr_points_fp64_ref.py, at the states the model-level tests never reach: the second trip of the gt loop (> 1024 gts in an
image), images without gts, dead threads in the last block, every probability type, points on / beyond / far beyond every
border, 2 / 3 / 4 dropped taps with and without the pad share (exactly one dropped tap cannot occur: the taps drop by whole rows
and columns), cell ranges wider than a wave, clipped and empty grid bags, the 7 | 8 and 512 | 513 dispatch boundaries of the bag
loss, every bag geometry, clamped sample counts, distance and probability ties.

One table (CASES).  ``make_inputs`` builds a case's CPU operands from its name alone (fixed seeds).  Outputs and workspaces are
filled with NaN / 0xFF before every launch (the wrappers' allocations are intercepted), every case runs twice and the two runs
must be bit-equal, and every case prints its worst error / bar ratio per output and its ambiguous counts.
tests/test_cpr_points_host.py asserts, without a GPU, that the table meets its coverage conditions, that the references agree
with oracle/cpr_oracle.py, that the ambiguous shares stay inside the cap and that the bars are sharp."""
import zlib

import numpy as np
import pytest
import torch

from tests import cpr_points_fp64_ref as R

pytestmark = pytest.mark.gpu

EPS = 1e-6
INT_FILL = 0x7f7f7f7f


def _case(op, name, exact=False, why='', **kw):
    return dict(op=op, name=name, exact=exact, why=why, **kw)


def NEG(name, N, H, W, C, J, counts, stride=4, radius=5, pads=None, class_wise=True, prob='sigmoid', norm_p=1.0, Cm=None, exact=False,
        layout='random', why=''):
    return _case('neg', name, exact, why, N=N, H=H, W=W, C=C, J=J, counts=counts, stride=stride, radius=radius, pads=pads,
                 class_wise=class_wise, prob=prob, norm_p=norm_p, Cm=C if Cm is None else Cm, layout=layout)


def BAG(name, N, H, W, J, radius, stride=4, align=False, pad=False, extra=4, why=''):
    return _case('bag', name, False, why, N=N, H=H, W=W, J=J, radius=radius, stride=stride, align=align, pad=pad, extra=extra)


def GRID(name, N, H, W, J, R, Kmax, radius_px, layout, stride=4, align=False, pad=False, exact=False, why=''):
    return _case('grid', name, exact, why, N=N, H=H, W=W, J=J, R=R, Kmax=Kmax, radius_px=radius_px, layout=layout, stride=stride,
                 align=align, pad=pad)


def MIL(name, nb, K, C, geom='independent', R=1, binary=False, allpos=False, prob='sigmoid', norm_p=1.0, weights=False, npart=3,
        neg_from_gt=False, valid='random', ins_gap=0, with_gt=True, sat=False, why=''):
    return _case('mil', name, False, why, sat=sat, nb=nb, K=K, C=C, geom=geom, R=R, binary=binary, allpos=allpos, prob=prob, norm_p=norm_p,
                 weights=weights, npart=npart, neg_from_gt=neg_from_gt, valid=valid, ins_gap=ins_gap, with_gt=with_gt)


def REF(name, counts, labels, Rv, Kv, C, prob='sigmoid', norm_p=1.0, nearest=True, classify=True, score_max=False, nr_in=False,
        layout='random', exact=False, why=''):
    return _case('refine', name, exact, why, counts=counts, labels=labels, Rv=Rv, Kv=Kv, C=C, prob=prob, norm_p=norm_p, nearest=nearest,
                 classify=classify, score_max=score_max, nr_in=nr_in, layout=layout)


CASES = [
    _case('centers', 'centers_300', n=300, why='two blocks, the second ragged'),
    # ---- cpr_neg_mask_loss
    NEG('neg_1100gts_exact', 1, 40, 40, 1, 1, [1100], exact=True, layout='split',
        why='> MAX_GT_LDS gts in one image: the second trip of the chunk loop decides the right half; 1600 threads: dead lanes'),
    NEG('neg_345_exact', 2, 24, 24, 2, 2, [2, 0], exact=True, layout='345', pads=[(96, 96), (61, 50)],
        why='d2 == d2_thr on 3-4-5 triangles (>=); an image without gts; pad_hw smaller than the map'),
    NEG('neg_sigmoid_c3', 3, 33, 29, 3, 5, [3, 1, 2], pads=[(132, 116), (100, 116), (132, 77)], why='class-wise, J > C, H*W*C % 256 != 0'),
    NEG('neg_no_classwise_c2', 2, 20, 21, 2, 2, [2, 3], class_wise=False, why='class_wise off'),
    NEG('neg_bg_cls', 2, 18, 19, 2, 3, [2, 2], Cm=1, why='mask_classes == 1 with C == 2: one validity for both outputs'),
    NEG('neg_softmax_c3', 2, 12, 10, 3, 4, [2, 1], prob='softmax', why='prob type 1'),
    NEG('neg_normed_p1_c3', 2, 12, 10, 3, 3, [1, 2], prob='normed_sigmoid', norm_p=1.0, why='prob type 2, p = 1'),
    NEG('neg_normed_p2_c3', 2, 12, 10, 3, 3, [1, 2], prob='normed_sigmoid', norm_p=2.0, why='prob type 2, p = 2 (sqrt)'),
    NEG('neg_normed_p3_c2', 1, 11, 13, 2, 2, [2], prob='normed_sigmoid', norm_p=3.0, why='prob type 2, p = 3 (powf)'),
    # ---- cpr_bag_sample
    BAG('bag_J1', 2, 9, 9, 1, 2, why='J < 4; points on, beyond and far beyond every border'),
    BAG('bag_J6', 2, 11, 7, 6, 3, why='J % 4 != 0: the second channel group holds 2'),
    BAG('bag_J12_s8', 1, 10, 12, 12, 2, stride=8, why='three full channel groups, stride 8'),
    BAG('bag_H1', 1, 1, 7, 3, 2, why='H == 1 without align_corners: the row clip collapses'),
    BAG('bag_W1', 1, 5, 1, 2, 2, why='W == 1 without align_corners'),
    BAG('bag_align_pad_J5', 2, 8, 9, 5, 2, align=True, pad=True, why='align_corners: 2, 3 and 4 dropped taps, with the pad share'),
    BAG('bag_align_nopad_J12', 2, 8, 9, 12, 2, align=True, why='align_corners without pad'),
    BAG('bag_J256', 1, 6, 6, 256, 1, extra=0, why='the raw-feature path'),
    # ---- cpr_grid_bag
    GRID('grid_wide', 1, 12, 96, 3, 1, 200, 140.0, 'wide', why='cell range of 71+ columns: the xb += 64 loop; count > Kmax; G % 4 != 0'),
    GRID('grid_345_exact', 1, 24, 24, 1, 1, 100, 20.0, '345', exact=True, why='distance == radius on 3-4-5 triangles (<=)'),
    GRID('grid_R3_align_pad', 2, 20, 22, 6, 3, 150, 12.0, 'spread', align=True, pad=True,
         why='R > 1 spread refine points, reversed; a gt wholly outside the map; padding count > 64; pad_value'),
    GRID('grid_R2_nopad', 2, 16, 16, 5, 2, 40, 10.0, 'spread', why='R = 2, border sampling, zero padding slots, J % 4 != 0'),
    # ---- cpr_mil_loss
    MIL('mil_t7_K63', 5, 63, 7, why='terms 7: the one-wave kernel; K 63'),
    MIL('mil_t8_K64', 5, 64, 8, why='terms 8: the workgroup-per-bag kernel; K 64'),
    MIL('mil_bin_t8_K65', 6, 65, 4, binary=True, weights=True, valid='one_empty', why='binary_ins terms 8; K 65; a gt_weight of 0; an empty bag'),
    MIL('mil_t512_J768', 5, 9, 256, binary=True, why='terms 512: the last workgroup-per-bag size'),
    MIL('mil_t513_J1026', 3, 5, 513, why='terms 513: back to the one-wave kernel'),
    MIL('mil_K1', 6, 1, 2, why='K 1'),
    MIL('mil_K130_merge_softmax', 3, 65, 3, geom='merge', R=2, prob='softmax', why='merge_to_gt_bag: K 130 > 128; softmax'),
    MIL('mil_only_refine_normed', 4, 9, 3, geom='only_refine', R=3, prob='normed_sigmoid', norm_p=2.0, why='only_refine_bag geometry'),
    MIL('mil_indep_ctr_mod', 3, 11, 2, geom='independent', R=2, ins_gap=1, why='independent bags of 2 refine points: ctr_mod 2; a gap before the ins channels'),
    MIL('mil_allpos_K70', 4, 70, 3, allpos=True, weights=True, why='AllPosLoss, K > 64'),
    MIL('mil_identity', 5, 20, 2, prob='identity', with_gt=False, why='prob type 3; no annotated-point loss'),
    MIL('mil_saturated', 4, 10, 2, sat=True, why='class logits near -12 in two bags: p of the order of eps in log(p + eps)'),
    MIL('mil_300bags', 300, 3, 1, npart=300, why='loss_finalize: > 256 bags and > 256 negative partials'),
    MIL('mil_all_invalid', 2, 8, 2, valid='none', why='num_sample and num_pos_gt clamped at 1'),
    MIL('mil_neg_from_gt', 4, 8, 2, neg_from_gt=True, valid='centre_only', why='neg_from_gt: the negative loss over the gt count'),
    # ---- cpr_refine
    REF('refine_K130', [3, 2], [0, 0, 1, 1, 1], 1, 130, 2, why='Kt > 64; a class with a single gt'),
    REF('refine_R2_same', [3, 1], [0, 0, 0, 0], 2, 17, 1, score_max=True, nr_in=True, classify=False,
        why='same > 1 with Rv > 1; not_refine_in; score_max'),
    REF('refine_ties_exact', [3], [0, 0, 1], 1, 9, 3, exact=True, layout='ties', why='exact distance ties and equal-logit ties'),
    REF('refine_none_kept', [2], [0, 0], 1, 12, 1, score_max=True, layout='low', why='nothing kept: fall-back point, refine_th / 2'),
    REF('refine_softmax_c3', [2, 2], [0, 1, 2, 2], 1, 40, 3, prob='softmax', why='softmax probabilities'),
    REF('refine_normed_p3', [2], [1, 1], 1, 30, 2, prob='normed_sigmoid', norm_p=3.0, why='normed_sigmoid, p = 3'),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def of(op):
    return [c for c in CASES if c['op'] == op]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7fffffff)


def _csr(counts):
    start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    img = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts))
    return start, img


def _clear(l, ths, ptype):
    """Keep sigmoid probabilities at least 1e-3 away from the fixed thresholds."""
    if ptype != 0:
        return l
    for th in ths:
        l = torch.where((torch.sigmoid(l.double()) - th).abs() < 2e-3, l + 0.1, l)
    return l


def make_inputs(c):
    """CPU operands of one case (fp32 / int32 / uint8 tensors and Python numbers), from the case alone."""
    from pointtinybenchmark_amd.dense_heads.cpr_head import circle_offsets, sqrt_threshold
    gen = _gen(c['name'])
    rnd = lambda *s: torch.randn(s, generator=gen)
    uni = lambda *s: torch.rand(s, generator=gen)
    op = c['op']
    if op == 'centers':
        b = uni(c['n'], 4) * 600 - 20
        b[:, 2:] += b[:, :2]
        return dict(boxes=b)
    ptype = R.PROB[c.get('prob', 'sigmoid')]
    if op == 'neg':
        N, H, W, C, J, s = c['N'], c['H'], c['W'], c['C'], c['J'], c['stride']
        counts = c['counts']
        G = sum(counts)
        pads = c['pads'] or [(H * s, W * s)] * N
        if c['layout'] == 'split':      # the first 1024 gts on the left, the rest on the right: only the second chunk covers it
            n1 = 1024
            x = torch.cat([torch.randint(0, 60 * 8, (n1,), generator=gen), torch.randint(100 * 8, W * s * 8, (G - n1,), generator=gen)]) / 8.0
            ctr = torch.stack([x, torch.randint(0, H * s * 8, (G,), generator=gen) / 8.0], -1)
        elif c['layout'] == '345':      # cell centre + (12, 16) and + (-16, 12): cells (5, 7) and (15, 4) lie at distance 20 exactly
            ctr = torch.tensor([[(5 + 0.5) * s + 12, (7 + 0.5) * s + 16], [(15 + 0.5) * s - 16, (4 + 0.5) * s + 12]])
        else:
            ctr = torch.cat([uni(n, 2) * torch.tensor([pads[k][1], pads[k][0]]) for k, n in enumerate(counts)])
        labels = torch.arange(G, dtype=torch.int32) % c['Cm'] if c['layout'] != 'random' else torch.randint(0, c['Cm'], (G,), generator=gen).int()
        start, _ = _csr(counts)
        # the exact cases put the threshold ON the dyadic grid, (stride * radius)^2, so that d2 == d2_thr occurs; the host-derived
        # threshold of the product may be the float below it (its sqrt already rounds up to stride * radius)
        d2_thr = float((s * c['radius']) ** 2) if c['exact'] else sqrt_threshold(s * c['radius'])
        return dict(logit=2 * rnd(N, H, W, J), ctr=ctr.float(), labels=labels, gt_start=start, pad_hw=torch.tensor(pads, dtype=torch.int32),
                    C=C, Cm=c['Cm'], stride=s, d2_thr=d2_thr, eps=EPS, class_wise=c['class_wise'], ptype=ptype,
                    prob=c['prob'], norm_p=c['norm_p'], exact=c['exact'])
    if op == 'bag':
        N, H, W, J, s = c['N'], c['H'], c['W'], c['J'], c['stride']
        w, h = W * s, H * s
        special = [(0.0, 0.0), (w, h), (w - 0.25, 0.5 * h), (-0.5, -0.5), (-3.0 * w, 2.5 * h), (4.0 * w, -3.0 * h), (0.5 * s, h - 0.5 * s),
                   ((W // 2 + 0.5) * s, (H // 2) * s), (w - s, -0.75 * s), (w + 1.5 * s, h + 0.25 * s)]
        pts = special + [(float(uni(1)) * w, float(uni(1)) * h) for _ in range(c['extra'])]
        if c['extra'] == 0:
            pts = pts[:3]
        ctr = torch.tensor(pts, dtype=torch.float32)
        gt_img = (torch.arange(ctr.shape[0]) % N).sort()[0].int()
        pad_hw = torch.tensor([(h - (3 if n else 0), w - (5 if n else 0)) for n in range(N)], dtype=torch.int32)
        return dict(map=rnd(N, H, W, J), ctr=ctr, gt_img=gt_img, pad_hw=pad_hw, off=circle_offsets(c['radius'], s), stride=s,
                    align=c['align'], pad=rnd(J) if c['pad'] else None)
    if op == 'grid':
        N, H, W, J, s, Rr = c['N'], c['H'], c['W'], c['J'], c['stride'], c['R']
        w, h = W * s, H * s
        if c['layout'] == 'wide':
            pts = torch.tensor([[0.5 * w + 1.3, 0.5 * h - 0.7], [0.3 * w + 0.123, 7.77], [w - 3.21, h + 9.4]])
        elif c['layout'] == '345':      # cell (8, 9) at (+12, +16), cell (17, 6) at (-16, +12), cell (3, 18) at (20, 0): distance 20 exactly
            pts = torch.tensor([[(8 + 0.5) * s - 12, (9 + 0.5) * s - 16], [(17 + 0.5) * s + 16, (6 + 0.5) * s - 12], [(3 + 0.5) * s - 20, (18 + 0.5) * s]])
        else:
            G = 5 if Rr == 3 else 3
            base = uni(G, 1, 2) * torch.tensor([w, h])
            pts = base + rnd(G, Rr, 2) * 2.5 * s
            pts[0] = torch.tensor([-100.0, -100.0]) + rnd(Rr, 2) * 8       # wholly outside the map
            pts[1, 0] = torch.tensor([0.3, h - 0.2])                         # refine points at the border
            pts = pts.reshape(-1, 2)
        G = pts.shape[0] // Rr
        gt_img = (torch.arange(G) % N).sort()[0].int()
        return dict(map=rnd(N, H, W, J), points=pts.float().contiguous(), gt_img=gt_img, R=Rr, Kmax=c['Kmax'], radius_px=c['radius_px'],
                    stride=s, align=c['align'], pad=rnd(J) if c['pad'] else None, exact=c['exact'])
    if op == 'mil':
        nb, Kv, C, Rr = c['nb'], c['K'], c['C'], c['R']
        nj = 2 if c['binary'] else 1
        ins_off = C + c['ins_gap']
        J = ins_off + C * nj
        if c['geom'] == 'independent':
            G = nb
            nb, bags, centres = G * Rr, (G * Rr, Kv, 0, Kv), (Kv - 1, Kv, 1, Rr)
        elif c['geom'] == 'merge':
            G, bags, centres = nb, (nb, Rr * Kv, 0, Rr * Kv), (Kv - 1, Kv, Rr, 1)
        else:
            G, bags, centres = nb, (nb, Rr * Kv, Kv, (Rr - 1) * Kv), (Kv - 1, Kv, 1, 1)
        if not c['with_gt']:
            centres = (0, 1, 0, 1)
        E = G * Rr * Kv
        logits = 2 * rnd(E, J)
        if ptype == 3:
            logits[:, :C] = 0.02 + 0.96 * uni(E, C)
        if c['sat']:
            logits[:2 * Kv, :C] = -12 + 0.5 * rnd(2 * Kv, C)
        valid = (uni(E) < 0.8)
        if c['valid'] == 'none':
            valid[:] = False
        elif c['valid'] == 'one_empty':
            valid[bags[1]:2 * bags[1]] = False
        elif c['valid'] == 'centre_only':
            valid[:] = False
            valid[Kv - 1::Kv] = True
            valid[Kv - 1] = False
            valid[0] = True                            # bag 0: a sample without a valid annotated point
        gw = None
        if c['weights']:
            gw = 0.5 + uni(nb)
            gw[nb - 1] = 0.0
        part = (uni(c['npart']).double() * 3.0) if c['npart'] else None
        return dict(logits=logits.view(G, Rr * Kv, J), valid=valid.view(G, Rr * Kv).to(torch.uint8), labels=torch.randint(0, C, (nb,), generator=gen).int(),
                    gt_weight=gw, bags=bags, centres=centres, C=C, ins_off=ins_off, eps=EPS, ptype=ptype, prob=c['prob'], norm_p=c['norm_p'],
                    binary=c['binary'], allpos=c['allpos'], neg_partial=part, w_mil=0.25, w_gt=0.3, w_neg=0.75, neg_from_gt=c['neg_from_gt'])
    assert op == 'refine'
    counts, Rv, Kv, C = c['counts'], c['Rv'], c['Kv'], c['C']
    G, Kt, J = sum(counts), Rv * Kv, C + 1
    start, gt_img = _csr(counts)
    img_hw = torch.tensor([(120, 128)] * len(counts), dtype=torch.int32)
    merge_th, refine_th, alpha = 0.1, 0.3, 0.5
    if c['layout'] == 'ties':
        # gts 0 and 1 (class 0) at (16, 16) and (48, 16); entries on x = 32 are equidistant: the first candidate (gt 0) wins
        ctr = torch.tensor([[16.0, 16.0], [48.0, 16.0], [80.0, 40.0]])
        ring = torch.tensor([[16.0, -8.0], [16.0, 8.0], [16.0, 0.0], [-4.0, 2.5], [3.125, -6.0], [0.0, 5.0], [7.0, 7.0], [-2.0, -2.0], [0.0, 0.0]])
        pts = torch.stack([ctr[0] + ring, ctr[1] + ring * torch.tensor([-1.0, 1.0]), ctr[2] + ring])
        logits = torch.zeros((G, Kt, J))
        logits[..., 0], logits[..., 1], logits[..., 2], logits[..., 3] = 1.0, -2.0, -1.5, 9.0
        logits[2, :, 0], logits[2, :, 1] = -2.0, 1.0
        logits[0, 3, 1] = logits[1, 4, 1] = 1.0      # label 0 ties with class 1: the lowest class (the label) wins, kept
        logits[2, 5, 0] = 1.0                        # label 1 ties with class 0: class 0 wins, dropped
        valid = torch.ones((G, Kt), dtype=torch.uint8)
    else:
        ctr = torch.cat([torch.stack([10 + uni(n * Rv) * 100, 10 + uni(n * Rv) * 95], -1) for n in counts])
        if Rv > 1:      # the refine points of a gt stay near its annotated point
            a = ctr.view(G, Rv, 2)
            a[:, 1:] = a[:, :1] + rnd(G, Rv - 1, 2) * 6
            a[1] = a[0] + torch.tensor([9.0, 3.0])     # two gts of the class close together: the nearest filter bites
            ctr = a.reshape(-1, 2)
        pts = ctr.view(G, Rv, 1, 2) + rnd(G, Rv, Kv, 2) * 14
        pts[:, :, Kv - 1] = ctr.view(G, Rv, 2)
        pts = pts.reshape(G, Kt, 2)
        pts[0, 0] = torch.tensor([-3.0, 20.0])
        pts[G - 1, 1] = torch.tensor([128.0, 119.5])
        logits = (0.5 * rnd(G, Kt, J) - 6.0) if c['layout'] == 'low' else (1.5 * rnd(G, Kt, J) + 0.3)
        logits = _clear(logits, (merge_th,), ptype)
        valid = (uni(G, Kt) < 0.9).to(torch.uint8)
        valid[:, Kv - 1] = 1
    nr_in = None
    if c['nr_in']:
        nr_in = torch.zeros(G, dtype=torch.uint8)
        nr_in[1] = 1
    return dict(logits=logits.contiguous(), pts=pts.contiguous(), valid=valid, ctr=ctr.contiguous(), labels=torch.tensor(c['labels'], dtype=torch.int32),
                gt_img=gt_img, gt_start=start, img_hw=img_hw, not_refine_in=nr_in, C=C, Kv=Kv, Rv=Rv, ctr_stride=Rv, ptype=ptype, prob=c['prob'],
                norm_p=c['norm_p'], gt_alpha=alpha, merge_th=merge_th, refine_th=refine_th, use_nearest=c['nearest'], use_classify=c['classify'],
                score_max=c['score_max'], exact=c['exact'])


def reference(c, i):
    op = c['op']
    return dict(centers=lambda: R.centers_ref(i['boxes']), neg=lambda: R.neg_ref(i), bag=lambda: R.bag_ref(i), grid=lambda: R.grid_ref(i),
                mil=lambda: R.mil_ref(i), refine=lambda: R.refine_ref(i))[op]()


# ---- the device side ---------------------------------------------------------------------------------------------------
class _Filled:
    """Stands in for ``torch`` inside ops: ``empty`` hands out NaN / 0xFF-filled memory, so a slot no kernel wrote shows.  Wider
    integers get INT_FILL, a value no kernel emits (-1 is grid_select's padding code for ``cell``)."""

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        return t.fill_(float('nan')) if t.is_floating_point() else t.fill_(255 if t.dtype == torch.uint8 else INT_FILL)


def _cu(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().flatten().view(torch.uint8)


def _flag(t):
    """A uint8 output holds only 0 / 1."""
    assert int(t.max()) <= 1 if t.numel() else True, 'a flag byte was never written'
    return t.cpu()


def run_device(ops, c, i):
    """One launch through the ops wrapper -> the outputs as CPU tensors, named as R.compare expects."""
    op = c['op']
    if op == 'centers':
        return dict(centers=ops.box_centers(i['boxes'].cuda()).cpu())
    if op == 'neg':
        N, H, W, _ = i['logit'].shape
        mask, part = ops.neg_mask_loss(i['logit'].cuda(), i['ctr'].cuda(), i['labels'].cuda(), i['gt_start'].cuda(), i['pad_hw'].cuda(), i['C'],
                                       i['stride'], i['d2_thr'], i['eps'], i['class_wise'], i['prob'], i['norm_p'], mask_classes=i['Cm'])
        return dict(mask=_flag(mask).view(N, H * W, i['C']), img_sum=part.cpu().view(N, -1).sum(1), partial=part.cpu())
    if op == 'bag':
        pts, valid, out = ops.bag_sample(i['map'].cuda(), i['ctr'].cuda(), i['gt_img'].cuda(), i['pad_hw'].cuda(), i['off'].cuda(), i['stride'],
                                         align_corners=i['align'], pad_value=_cu(i['pad']))
        return dict(pts=pts.cpu(), valid=_flag(valid), out=out.cpu())
    if op == 'grid':
        pts, valid, out, count, cell = ops.grid_bag(i['map'].cuda(), i['points'].cuda(), i['gt_img'].cuda(), i['R'], i['Kmax'], i['radius_px'],
                                                    i['stride'], pad_value=_cu(i['pad']), align_corners=i['align'], want_cell=True)
        assert not bool((count == INT_FILL).any() | (cell == INT_FILL).any()), 'a count or cell slot was never written'
        return dict(pts=pts.cpu(), valid=_flag(valid), out=out.cpu(), count=count.cpu(), cell=cell.cpu())
    if op == 'mil':
        out5, bag = ops.mil_loss(i['logits'].cuda(), i['ins_off'], i['valid'].cuda(), i['labels'].cuda(), i['C'], _cu(i['neg_partial']), i['w_mil'],
                                 i['w_gt'], i['w_neg'], _cu(i['gt_weight']), i['eps'], bags=i['bags'], centres=i['centres'], prob_type=i['prob'],
                                 norm_p=i['norm_p'], binary_ins=i['binary'], allpos=i['allpos'], neg_from_gt=i['neg_from_gt'])
        return dict(out5=out5.cpu(), bag=bag.cpu())
    rp, sc, nr, chosen = ops.refine(i['logits'].cuda(), i['pts'].cuda(), i['valid'].cuda(), i['ctr'].cuda(), i['labels'].cuda(), i['gt_img'].cuda(),
                                    i['gt_start'].cuda(), i['img_hw'].cuda(), i['C'], i['gt_alpha'], i['merge_th'], i['refine_th'],
                                    use_nearest=i['use_nearest'], use_classify=i['use_classify'], not_refine_in=_cu(i['not_refine_in']),
                                    sub_bags=i['Rv'], ctr_stride=i['ctr_stride'], prob_type=i['prob'], norm_p=i['norm_p'], score_max=i['score_max'])
    return dict(refine_pts=rp.cpu(), scores=sc.cpu(), not_refine=_flag(nr), chosen=_flag(chosen))


def report(c, res):
    print('CPR %-26s %s | wrong %s | ambiguous %s' % (
        c['name'], ' '.join('%s %.3f' % kv for kv in res['ratios'].items()), sum(res['wrong'].values()),
        ' '.join('%s %d/%d' % (k, a, n) for k, (a, n) in res['amb'].items()) or '-'), flush=True)


@pytest.mark.parametrize('name', list(BY_NAME))
def test_cpr_point_kernel_vs_fp64(name, monkeypatch):
    from pointtinybenchmark_amd import ops
    monkeypatch.setattr(ops, 'torch', _Filled())
    R_threads = min(16, torch.get_num_threads())
    torch.set_num_threads(R_threads)
    c = BY_NAME[name]
    i = make_inputs(c)
    a = run_device(ops, c, i)
    b = run_device(ops, c, i)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), '%s: two launches differ in %s' % (name, k)
    res = R.compare(c['op'], i, a, reference(c, i))
    report(c, res)
    assert all(w == 0 for w in res['wrong'].values()), (name, res['wrong'])
    assert all(r <= 1 for r in res['ratios'].values()), (name, res['ratios'])
    assert R.amb_ok(res, c['exact']), (name, res['amb'])


def test_cls_kernel_bits_equal_the_one_wave_kernel(monkeypatch):
    """mil_bag_cls_kernel is documented as bit-identical to mil_bag_kernel.  The eight class columns of a terms = 8 problem (the
    workgroup-per-bag kernel) run again through the one-wave kernel as a terms = 7 problem on the SAME tensor (classes 0 .. 6; with
    sigmoid probabilities a class's terms do not depend on the other classes) plus a one-class problem holding column 7 (label 1:
    no positive class, as for column 7 in the full problem whose labels are all below 7).  Both kernels add the class terms in
    ascending order from 0, gt_weight is None (every weight 0 or 1: the products are exact), so
    loss_8 = fl(loss_7 + term_7) and gt_loss_8 = fl(gt_loss_7 + gt_term_7) bit for bit, and has_valid / #gt-valid are equal.  The
    correct-class flag is not shared (the arg-max runs over different class sets) and is left out."""
    from pointtinybenchmark_amd import ops
    monkeypatch.setattr(ops, 'torch', _Filled())
    G, K, C = 9, 70, 8
    gen = _gen('cls_vs_wave')
    logits = 2 * torch.randn((G, K, 2 * C), generator=gen)
    valid = (torch.rand((G, K), generator=gen) < 0.8).to(torch.uint8)
    valid[3] = 0
    labels = torch.randint(0, 7, (G,), generator=gen).int()
    run = lambda lg, ins_off, lab, c: ops.mil_loss(lg.cuda().contiguous(), ins_off, valid.cuda(), lab.cuda(), c, None, 0.25, 0.3, 0.75, None, EPS)[1].cpu()
    b8 = run(logits, C, labels, 8)
    b7 = run(logits, C, labels, 7)
    b1 = run(torch.stack([logits[..., 7], logits[..., 15]], -1), 1, torch.ones(G, dtype=torch.int32), 1)
    assert not bool(torch.isnan(b8).any() | torch.isnan(b7).any() | torch.isnan(b1).any())
    for k in (0, 1):
        assert torch.equal(_bits(b8[:, k]), _bits(b7[:, k] + b1[:, k])), 'slot %d: the two kernels differ' % k
    assert torch.equal(b8[:, 2:4], b7[:, 2:4]) and float(b8[:, 0].abs().sum()) > 0

