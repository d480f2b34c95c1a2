"""-m gpu: the P2P loss kernels driven directly through the ops wrappers on synthetic inputs, against fp64 torch autograd of the
oracle on the CPU -- no network and no assigner in between, so the test chooses which cells are positive, negative (gt_inds 0) and
invalid (gt_inds < 0), and the gradient maps themselves are compared, not a head weight gradient that sums them over every pixel.

  loss           ops.p2p_loss (p2p_loss_kernel + p2p_loss_finalize_kernel) against oracle.p2p_options_oracle.p2p_loss_from_assignment
  loss backward  ops.p2p_loss_bwd (p2p_loss_bwd_kernel) against torch.autograd.grad of sum_b up[b,0] loss_cls[b] + up[b,1] loss_pts[b]
                 wrt the logits and wrt reg, through pred = anchor + reg * pts_gamma * stride
  decode         ops.p2p_decode against oracle.p2p_options_oracle.get_pred_points, bit for bit
  sigmoid        ops.sigmoid_exact / ops.rowmax_sigmoid against oracle.cpr_oracle._sigmoid_vector_path, bit for bit
  plumbing       P2PHead.loss + P2PTrainer._backward_head with a non-default head against fp64 autograd through the oracle head

Bar of the loss kernels: per-image losses within 1e-5 relative; gradients per element |got - ref| <= 1e-5 * max|ref| and relative
L2 <= 1e-5.  Error model: every point (gts, predictions) sits on a 1/256 grid and every stride * reg_norm is a power of two, so the
regression error e = pred / s / reg_norm - gt / s / reg_norm is exact in fp32 and the regression gradient carries only the few
roundings of its product chain.  The classification terms add fp32 expf / log1pf / powf and a sequential softmax sum (at most 81
terms), a few ulps each of the largest gradient.  Logits saturated past fp32 (17..30: fp32 p is exactly 1, fp64 p is not) are
compared against fp64 like the rest; past 38 fp64 saturates too (torch's pow backward is NaN there), so those cells are only checked
to be finite and equal to the analytic limit.  Worst errors are printed (run with -s)."""
import numpy as np
import pytest
import torch

from oracle import cpr_oracle as O
from oracle import p2p_options_oracle as PO

pytestmark = pytest.mark.gpu

BAR = 1e-5
BETA_SHIPPED = float(np.float32(1.0 / 9.0))     # the shipped SmoothL1 beta as the kernel sees it (fp32)
GRID = 1.0 / 256                                 # every point coordinate is a multiple of this


def _cp(C):
    """The trainer's padded class-gradient width (training.P2PTrainer._backward_head)."""
    return 4 if C <= 4 else (C + 31) // 32 * 32


def _report(name, got, ref, bar=BAR):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name + ': non-finite gradient'
    m = float(ref.abs().max())
    e = float((got - ref).abs().max()) / max(m, 1e-300)
    l2 = float((got - ref).norm()) / max(float(ref.norm()), 1e-300)
    print('ERR %-40s elem %.2e  l2 %.2e  (bar %.0e, max|ref| %.2e)' % (name, e, l2, bar, m), flush=True)
    if m == 0:
        assert float(got.abs().max()) == 0.0, name + ': non-zero where the reference is zero'
        return
    assert e <= bar and l2 <= bar, '%s: elem %.3e l2 %.3e > %.0e' % (name, e, l2, bar)


# ------------------------------------------------------------------------------------------------ cases
#        cls_mode reg_mode gamma alpha (pts_gamma, reg_norm) (pos_w, neg_w)  C   Rp  B  M      stride beta
CASES = {
    'focal_sl1':        (0, 0, 2.0, 0.25, (12.5, 0.125), (1.0, 1.0), 1, 4, 3, 1600, 4, 0.125),
    'focal_mse_g15':    (0, 1, 1.5, 0.25, (3.0, 2.0), (2.0, 0.5), 3, 4, 3, 257, 8, None),
    'focal_l1_g3':      (0, 2, 3.0, 0.375, (1.0, 1.0), (1.0, -1.0), 15, 4, 1, 1600, 4, None),
    'focal_sl1_g05':    (0, 0, 0.5, 0.25, (12.5, 0.125), (2.0, 0.5), 1, 4, 3, 1600, 4, BETA_SHIPPED),
    'focal_mse_g0':     (0, 1, 0.0, 0.5, (3.0, 2.0), (1.0, 1.0), 3, 8, 1, 257, 8, None),
    'focal_sl1_shipped': (0, 0, 2.0, 0.25, (1.0, 1.0), (1.0, 1.0), 1, 4, 3, 25600, 4, BETA_SHIPPED),
    'bce_sl1':          (1, 0, 2.0, 0.25, (3.0, 2.0), (2.0, 0.5), 15, 4, 3, 1600, 8, 0.125),
    'bce_mse':          (1, 1, 2.0, 0.25, (1.0, 1.0), (1.0, 1.0), 1, 4, 3, 25600, 4, None),
    'bce_l1':           (1, 2, 2.0, 0.25, (12.5, 0.125), (1.0, -1.0), 3, 4, 1, 257, 4, None),
    'softmax_sl1_coco': (2, 0, 2.0, 0.25, (12.5, 0.125), (2.0, 0.5), 81, 4, 3, 1600, 4, 0.125),
    'softmax_mse':      (2, 1, 2.0, 0.25, (1.0, 1.0), (1.0, -1.0), 2, 4, 1, 257, 8, None),
    'softmax_l1':       (2, 2, 2.0, 0.25, (3.0, 2.0), (1.0, 1.0), 16, 4, 3, 1600, 4, None),
}
W_CLS, W_REG = 1.5, 0.5


def _inputs(case, seed):
    """Host inputs of one case: logits (B, M, C) over +-8 with a saturated band, pred (B, M, 3) with the stride in column 2,
    gt_inds (B, M) int64 with invalid / negative / positive cells, ragged gts (image 1 of three has a single gt).  Positives sit
    at gt + e * stride * reg_norm with e on a 1/64 grid (exact in fp32), some with e == 0 and, when beta is on that grid, |e| == beta.
    Returns the numpy arrays and the (b, m, c) index of the cells past fp64 saturation (x >= 38)."""
    cls_mode, reg_mode, gamma, alpha, (pg, rn), (pw, nw), C, Rp, B, M, s, beta = case
    rng = np.random.default_rng(seed)
    nfg = C - 1 if cls_mode == 2 else C
    counts = [int(rng.integers(4, 12)) if (B == 1 or b != 1) else 1 for b in range(B)]
    G = sum(counts)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    gt_labels = rng.integers(0, nfg, size=G).astype(np.int32)
    gt_pts = (rng.integers(0, 640 * 256, size=(G, 2)) * GRID).astype(np.float32)
    logits = rng.uniform(-8, 8, size=(B, M, C)).astype(np.float32)
    gt_inds = np.zeros((B, M), np.int64)
    for b in range(B):
        perm = rng.permutation(M)
        npos = max(counts[b], M // 20)
        pos = perm[:npos]
        gt_inds[b, pos] = np.concatenate([np.arange(1, counts[b] + 1), rng.integers(1, counts[b] + 1, size=npos - counts[b])])
        gt_inds[b, perm[npos:npos + M // 10]] = -1
        # saturated band: whole rows at +-(17..30), and the label column of some positives at +(17..30) (t = 1, fp32 1 - p == 0)
        sat = perm[npos + M // 10:npos + M // 10 + M // 25]
        logits[b, sat] = (rng.uniform(17, 30, size=(len(sat), C)) * rng.choice([-1, 1], size=(len(sat), C))).astype(np.float32)
        lab = gt_labels[start[b] + gt_inds[b, pos[:npos // 3]] - 1]
        logits[b, pos[:npos // 3], lab] = rng.uniform(17, 30, size=npos // 3).astype(np.float32)
    pred = np.empty((B, M, 3), np.float32)
    pred[..., 2] = s
    pred[..., :2] = rng.integers(0, 640 * 256, size=(B, M, 2)) * GRID
    for b in range(B):
        pos = np.nonzero(gt_inds[b] > 0)[0]
        e = rng.integers(-3 * 64, 3 * 64 + 1, size=(len(pos), 2)) / 64.0
        e[::5] = 0.0                                                  # e == 0: L1 / SmoothL1 take sign(0) = 0
        if beta is not None and beta * 64 == int(beta * 64):
            e[1::5, 0], e[1::5, 1] = beta, -beta                      # |e| == beta: the SmoothL1 branch boundary
        g = start[b] + gt_inds[b, pos] - 1
        pred[b, pos, :2] = gt_pts[g] + (e * s * rn).astype(np.float32)
    extreme = []
    if cls_mode != 2:                                                 # past fp64 saturation: limits only
        for b in range(B):
            pos = np.nonzero(gt_inds[b] > 0)[0][-3:]
            neg = np.nonzero(gt_inds[b] == 0)[0][-3:]
            for m in pos:
                c = int(gt_labels[start[b] + gt_inds[b, m] - 1])
                extreme.append((b, m, c, 1.0))
            for m in neg:
                extreme.append((b, m, int(rng.integers(0, C)), 0.0))
        for b, m, c, _ in extreme:
            logits[b, m, c] = np.float32(rng.uniform(38, 60))
    return dict(logits=logits, pred=pred, gt_inds=gt_inds, gt_pts=gt_pts, gt_labels=gt_labels, gt_start=start), extreme


def _exact_e(inp, rn):
    """The kernel's fp32 regression error of every positive coordinate (pred / s / reg_norm - gt / s / reg_norm)."""
    f = np.float32
    pos = inp['gt_inds'] > 0
    b, m = np.nonzero(pos)
    g = inp['gt_start'][b] + inp['gt_inds'][b, m] - 1
    s = inp['pred'][b, m, 2:3]
    return (inp['pred'][b, m, :2] / s / f(rn) - inp['gt_pts'][g] / s / f(rn)).astype(f)


def _reference(case, inp, up):
    """fp64 oracle losses (B,), (B,) and the gradients of sum_b up[b,0] loss_cls[b] + up[b,1] loss_pts[b] wrt the logits and reg."""
    cls_mode, reg_mode, gamma, alpha, (pg, rn), (pw, nw), C, Rp, B, M, s, beta = case
    cls = torch.from_numpy(inp['logits']).double().requires_grad_(True)
    reg = torch.zeros((B, M, 2), dtype=torch.float64, requires_grad=True)     # pred = anchor + reg * pts_gamma * stride, at reg's value
    p = torch.from_numpy(inp['pred']).double()
    pred = torch.cat([p[..., :2] + reg * pg * p[..., 2:], p[..., 2:]], -1)
    lc, lp = PO.p2p_loss_from_assignment(cls, pred, torch.from_numpy(inp['gt_inds']), torch.from_numpy(inp['gt_pts']).double(),
                                         torch.from_numpy(inp['gt_labels']), torch.from_numpy(inp['gt_start']), alpha, gamma,
                                         beta if beta is not None else 1.0, pw, nw, rn, W_CLS, W_REG, cls_mode, reg_mode)
    total = (up[:, 0] * lc + up[:, 1] * lp).sum()
    dcls, dreg = torch.autograd.grad(total, (cls, reg))
    return lc.detach(), lp.detach(), dcls, dreg


def _launch(case, d, up=None):
    from pointtinybenchmark_amd import ops
    cls_mode, reg_mode, gamma, alpha, (pg, rn), (pw, nw), C, Rp, B, M, s, beta = case
    return ops.p2p_loss_bwd(d['logits'], d['pred'], d['gt_inds'], d['gt_pts'], d['gt_labels'], d['gt_start'], alpha, gamma,
                            beta if beta is not None else 1.0, pw, nw, rn, W_CLS, W_REG, pg, _cp(C), Rp, upstream=up,
                            cls_mode=cls_mode, reg_mode=reg_mode)


def _to_cuda(inp):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}


@pytest.mark.parametrize('name', list(CASES))
def test_p2p_loss_and_backward_vs_fp64_autograd(name):
    from pointtinybenchmark_amd import ops
    case = CASES[name]
    cls_mode, reg_mode, gamma, alpha, (pg, rn), (pw, nw), C, Rp, B, M, s, beta = case
    seed = 900 + list(CASES).index(name)
    inp, extreme = _inputs(case, seed)
    if reg_mode != 1:
        e = _exact_e(inp, rn)
        assert (e == 0).any(), 'no positive with e == 0'
        if reg_mode == 0 and beta == 0.125:
            assert (np.abs(e) == np.float32(beta)).any(), 'no positive with |e| == beta'
    up = torch.from_numpy(np.random.default_rng(seed).integers(1, 9, size=(B, 2)) / 4.0)    # dyadic, exact in fp32
    lc, lp, rcls, rreg = _reference(case, inp, up)
    d = _to_cuda(inp)
    upd = up.float().cuda().contiguous()

    # forward: per-image losses within 1e-5 relative
    out = ops.p2p_loss(d['logits'], d['pred'], d['gt_inds'], d['gt_pts'], d['gt_labels'], d['gt_start'], alpha, gamma,
                       beta if beta is not None else 1.0, pw, nw, rn, W_CLS, W_REG, cls_mode, reg_mode).cpu().double()
    ref = torch.stack([lc, lp], 1)
    rel = ((out - ref).abs() / ref.abs()).max()
    print('ERR %-40s loss rel %.2e' % (name, float(rel)), flush=True)
    assert bool(torch.isfinite(out).all()) and float(rel) <= BAR, (out, ref)

    dcls, dreg = _launch(case, d, upd)
    dcls2, dreg2 = _launch(case, d, upd)
    torch.cuda.synchronize()
    assert torch.equal(dcls, dcls2) and torch.equal(dreg, dreg2), 'two launches differ'
    dcls, dreg = dcls.cpu(), dreg.cpu()
    assert dcls.shape == (B, M, _cp(C)) and dreg.shape == (B, M, Rp)
    # layout: padded columns, invalid rows and every non-positive regression row exactly zero
    gi = torch.from_numpy(inp['gt_inds'])
    assert bool((dcls[..., C:] == 0).all()) and bool((dreg[..., 2:] == 0).all()), 'padded columns not zero'
    assert bool((dcls[gi < 0] == 0).all()), 'gt_inds < 0 rows of dcls not zero'
    assert bool((dreg[gi <= 0] == 0).all()), 'non-positive rows of dreg not zero'

    # cells past fp64 saturation: finite and the analytic limit (t = 1: 0; t = 0: dL/dx -> (1 - alpha) resp. 1 times the weights)
    keep = torch.ones_like(rcls, dtype=torch.bool)
    npos = float((gi > 0).sum())
    for b, m, c, t in extreme:
        keep[b, m, c] = False
        got = float(dcls[b, m, c])
        w = pw if t else (1.0 if nw <= 0 else nw)
        lim = 0.0 if t else ((1 - alpha) if cls_mode == 0 else 1.0) * w * W_CLS * float(up[b, 0]) / (npos if cls_mode == 0 else B * M)
        assert np.isfinite(got) and abs(got - lim) <= 1e-6 * abs(lim), (b, m, c, t, got, lim)
    assert bool(torch.isfinite(rcls[keep]).all()) and bool(torch.isfinite(rreg).all())
    _report(name + ' dcls', dcls[..., :C][keep], rcls[keep])
    _report(name + ' dreg', dreg[..., :2], rreg)


@pytest.mark.parametrize('name', ['focal_sl1', 'bce_l1', 'softmax_sl1_coco', 'focal_mse_g0'])
def test_p2p_loss_bwd_upstream_weights(name):
    """upstream None == ones bit for bit; zeroing up[b, t] zeroes exactly image b's term t and leaves every other bit; doubling it
    doubles exactly that term (a power of two: every rounding scales with it).  Exactness needs every intermediate of the product
    chain to be normal: saturated focal negatives (p ~ 1e-13, pt^gamma * (p - t) ~ 1e-40) pass through subnormals, so gradients
    below 2^-100 are held to 2^-120 instead."""
    case = CASES[name]
    B = case[8]
    inp, _ = _inputs(case, 950 + list(CASES).index(name))
    d = _to_cuda(inp)
    ones = torch.ones((B, 2), device='cuda')
    c0, r0 = _launch(case, d, None)
    c1, r1 = _launch(case, d, ones)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1) and torch.equal(r0, r1), 'upstream=None differs from ones'
    small = 2.0 ** -100
    for b in range(B):
        for t in range(2):
            for scale in (0.0, 2.0):
                up = ones.clone()
                up[b, t] = scale
                c, r = _launch(case, d, up.contiguous())
                torch.cuda.synchronize()
                term, other = (c, r) if t == 0 else (r, c)
                base_term, base_other = (c0, r0) if t == 0 else (r0, c0)
                assert torch.equal(other, base_other), (b, t, scale, 'the other term changed')
                rest = torch.ones(B, dtype=torch.bool, device='cuda')
                rest[b] = False
                assert torch.equal(term[rest], base_term[rest]), (b, t, scale, 'another image changed')
                want = base_term[b] * scale
                diff = (term[b] - want).abs()
                big = want.abs() >= small
                assert bool((diff[big] == 0).all()), (b, t, scale, float(diff[big].max()))
                assert bool((diff[~big] <= 2.0 ** -120).all()), (b, t, scale, float(diff[~big].max()))


def test_p2p_loss_bwd_checks_its_inputs():
    """A wrong dtype, a non-contiguous tensor or a wrong shape raises instead of being read as garbage."""
    case = CASES['bce_sl1']                 # B = 3: a transposed view is not contiguous (with B = 1 it would be)
    inp, _ = _inputs(case, 990)
    d = _to_cuda(inp)
    _launch(case, d)
    for key, bad in (('gt_inds', d['gt_inds'].int()), ('gt_labels', d['gt_labels'].long()), ('gt_start', d['gt_start'].long()),
                     ('gt_pts', d['gt_pts'].double()), ('pred', d['pred'].double()),
                     ('pred', d['pred'].transpose(0, 1).contiguous().transpose(0, 1)), ('gt_inds', d['gt_inds'][:, :-1]),
                     ('gt_inds', d['gt_inds'][:, :-1].contiguous()), ('pred', d['pred'][:, :-1].contiguous())):
        with pytest.raises(AssertionError):
            _launch(case, dict(d, **{key: bad}))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize('k', [1, 4])
@pytest.mark.parametrize('stride,pts_gamma', [(4, 1.0), (8, 12.5), (4, 12.5), (8, 1.0)])
def test_p2p_decode_bit_exact(k, stride, pts_gamma):
    """ops.p2p_decode == oracle get_pred_points in fp32, bit for bit (both form anchor = x*s + pa*s, then anchor + (reg*gamma)*s),
    on odd maps; the anchor output == the oracle's grid points + point_anchor * stride."""
    from pointtinybenchmark_amd import ops
    pa = [(0., 0.)] if k == 1 else [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]
    N, H, W = 2, 13, 7
    g = torch.Generator().manual_seed(77 + k + stride)
    reg = torch.randn((N, 2 * k, H, W), generator=g) * 3
    reg[0, :, 0, 0] = 0.0
    ref, _ = PO.get_pred_points([torch.zeros((N, k, H, W))], [reg], [stride], pa, pts_gamma, 1)
    pred, anchor = ops.p2p_decode(reg.permute(0, 2, 3, 1).contiguous().cuda(), torch.tensor(pa).cuda(), stride, pts_gamma,
                                  want_anchor=True)
    torch.cuda.synchronize()
    pred, anchor = pred.cpu(), anchor.cpu()
    assert pred.shape == ref.shape == (N, H * W * k, 3)
    mism = int((pred != ref).sum())
    assert mism == 0, '%d of %d decoded coordinates differ' % (mism, pred.numel())
    ra = (O.p2p_grid_points(H, W, stride)[:, None, :2] + torch.tensor(pa, dtype=torch.float32)[None] * stride).reshape(-1, 2)
    assert torch.equal(anchor[..., :2], ra[None].expand(N, -1, -1)) and bool((anchor[..., 2] == stride).all())
    assert torch.equal(ops.p2p_decode(reg.permute(0, 2, 3, 1).contiguous().cuda(), torch.tensor(pa).cuda(), stride,
                                      pts_gamma).cpu(), pred)


# ------------------------------------------------------------------------------------------------ sigmoid
def _vector_path_ref(x):
    """_sigmoid_vector_path on one thread: ATen splits a parallel loop into chunks whose ends run the scalar tail, so the
    reference is taken single-threaded (one vector body + the padded tail)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return O._sigmoid_vector_path(x)
    finally:
        torch.set_num_threads(n)


def _sweep_inputs():
    """Every 5th fp32 bit pattern of [-17, 17], every fp32 value of [-104, -87] (torch returns subnormals there), specials."""
    top = int(np.array(17.0, np.float32).view(np.int32))
    mag = np.arange(0, top + 1, 5, dtype=np.int32).view(np.float32)
    lo, hi = (int(np.array(v, np.float32).view(np.int32)) for v in (87.0, 104.0))
    deep = -np.arange(lo, hi + 1, dtype=np.int32).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 104.5, -104.5, 104.0, -104.0, 17.0, -17.0], np.float32)
    return [mag, -mag, deep, special]


def test_sigmoid_exact_bit_exact_sweep():
    from pointtinybenchmark_amd import ops
    chunk = 1 << 25
    for part in _sweep_inputs():
        for i in range(0, part.size, chunk):
            x = torch.from_numpy(np.ascontiguousarray(part[i:i + chunk]))
            got = ops.sigmoid_exact(x.cuda()).cpu()
            ref = _vector_path_ref(x)
            bad = (got.view(torch.int32) != ref.view(torch.int32))
            if bool(bad.any()):
                j = int(bad.nonzero()[0])
                raise AssertionError('%d mismatches, first x=%r got %r ref %r' % (int(bad.sum()), float(x[j]), float(got[j]), float(ref[j])))
    torch.cuda.synchronize()


@pytest.mark.parametrize('C', [1, 2, 15, 80])
def test_rowmax_sigmoid_bit_exact(C):
    from pointtinybenchmark_amd import ops
    M = 1000
    g = torch.Generator().manual_seed(500 + C)
    x = torch.randn((M, C), generator=g) * 6
    x[::11] *= 4
    x[5, 0], x[6, -1], x[7, 0], x[8, 0] = float('inf'), float('-inf'), 0.0, -0.0
    x[9, :] = -104.5
    x[10, :] = -95.0
    got = ops.rowmax_sigmoid(x.cuda()).cpu()
    ref = _vector_path_ref(x).max(1)[0]
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), int((got != ref).sum())


# ------------------------------------------------------------------------------------------------ head plumbing
def test_p2p_head_nondefault_config_vs_fp64_autograd():
    """P2PHead.loss + P2PTrainer._backward_head (head-only, as test_gpu_p2p_options.py) with pts_gamma 12.5, reg_norm 0.125, pos/neg
    weights 2 / 0.5, focal gamma 1.5 / alpha 0.375, SmoothL1 beta 0.125, loss weights 0.75 / 0.5: losses and head gradients against
    fp64 autograd through oracle.cpr_oracle.p2p_head_forward + get_pred_points + p2p_loss_from_assignment, evaluated on the device's
    own assignment (no assignment flips).  The expected values come from this config dict, not from the head."""
    import pointtinybenchmark_amd as P
    from oracle.gen_golden import GN
    from oracle.gen_golden_r6 import SHIPPED_ASSIGNER, TEST_CFG, head_inputs, head_state_dict
    from pointtinybenchmark_amd.training import P2PTrainer
    cfg = dict(C=1, hw=40, G=7, strides=[4], anchors=[(0., 0.)], std=0.05, seed=17,
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.375, loss_weight=0.75),
               loss_reg=dict(type='SmoothL1Loss', beta=0.125, loss_weight=0.5), assigner=SHIPPED_ASSIGNER,
               pts_gamma=12.5, reg_norm=0.125, pos_weight=2.0, neg_weight=0.5)
    head = P.build_head(dict(type='P2PHead', norm_cfg=GN, num_classes=cfg['C'], in_channels=256, feat_channels=256, stacked_convs=4,
                             strides=cfg['strides'], point_anchor=cfg['anchors'], loss_cls=cfg['loss_cls'], loss_reg=cfg['loss_reg'],
                             pts_gamma=cfg['pts_gamma'], reg_norm=cfg['reg_norm'],
                             train_cfg=dict(pos_weight=cfg['pos_weight'], neg_weight=cfg['neg_weight'], assigner=cfg['assigner'],
                                            sampler=dict(type='PseudoSampler')),
                             test_cfg=dict(TEST_CFG))).cuda()
    sd = head_state_dict(cfg)
    head.load_state_dict({k[len('bbox_head.'):]: v for k, v in sd.items()}, strict=True)

    class HeadOnly(P2PTrainer):
        def __init__(self, head):
            self.side = None
            for p in head.parameters():
                p.grad = torch.zeros_like(p)

        def _done(self, p):
            pass
    tr = HeadOnly(head)
    feats, batch = head_inputs(cfg)
    raw = feats[0].permute(0, 2, 3, 1).contiguous().cuda()
    ones, zeros = torch.ones((2, 256), device='cuda'), torch.zeros((2, 256), device='cuda')
    losses, saved = tr._forward_head(head, [(raw, (ones, zeros))], batch['img_metas'], [b.cuda() for b in batch['gt_bboxes']],
                                     [l.cuda() for l in batch['gt_labels']], None, None)
    tr._backward_head(head, saved)
    torch.cuda.synchronize()
    gt_inds = saved['gt_inds'].cpu()
    assert int((gt_inds > 0).sum()) > 0

    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    co, po = O.p2p_head_forward(sd64, [feats[0].double()])
    pred, cls = PO.get_pred_points(co, po, cfg['strides'], cfg['anchors'], cfg['pts_gamma'], cfg['C'])
    ctr = [(b[:, :2] + b[:, 2:]) / 2 for b in batch['gt_bboxes']]
    counts = [len(c) for c in ctr]
    lc, lr = cfg['loss_cls'], cfg['loss_reg']
    rc, rp = PO.p2p_loss_from_assignment(cls, pred.double(), gt_inds, torch.cat(ctr).double(), torch.cat(list(batch['gt_labels'])),
                                         torch.tensor([0] + counts[:-1]).cumsum(0), lc['alpha'], lc['gamma'], lr['beta'],
                                         cfg['pos_weight'], cfg['neg_weight'], cfg['reg_norm'], lc['loss_weight'], lr['loss_weight'],
                                         0, 0)
    got_l = torch.tensor([[float(losses['loss_cls'][b]), float(losses['loss_pts'][b])] for b in range(2)], dtype=torch.float64)
    ref_l = torch.stack([rc, rp], 1).detach()
    print('ERR head losses', got_l.tolist(), ref_l.tolist(), flush=True)
    assert float((got_l - ref_l).abs().max()) <= 3e-4 * max(1.0, float(ref_l.abs().max())), (got_l, ref_l)
    (rc.sum() + rp.sum()).backward()
    gmax = max(float(v.grad.norm()) for v in sd64.values())
    for n, p in head.named_parameters():
        k = 'bbox_head.' + n
        gr, ref = p.grad.detach().double().cpu().flatten(), sd64[k].grad.flatten()
        rel = float((gr - ref).norm()) / max(float(ref.norm()), 1e-5 * gmax)
        # the bars of test_gpu_p2p_options.py::test_p2p_head_option_backward_vs_reference_autograd
        bar = 2e-3 if ('cls_' in k or 'reg_out' in k or 'reg_convs.3' in k) else 3e-2
        print('ERR head %-40s rel %.2e (bar %.0e)' % (k, rel, bar), flush=True)
        assert rel <= bar, (k, rel)
