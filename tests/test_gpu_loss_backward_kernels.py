"""-m gpu: the CPR loss-backward kernels and the bag gathers (csrc/backward.hip) driven directly through the ops wrappers on
synthetic logit maps, against fp64 torch autograd of the oracle on the CPU -- no network in between, so the gradient map
``dmap`` itself (not a weight gradient that sums it over every pixel) and the bag-entry gradient ``dbag`` are compared.

  gathers        ops.bag_gather_bwd (bag_window_kernel + bag_window_add_kernel, ring bags) and ops.bag_points_gather_bwd
                 (bag_points_gather_kernel: grid bags, align_corners=True, padding slots and the bias share) against
                 d/dmap sum(dsample * sample(map64, pts)) with oracle.cpr_oracle.sample_bilinear
  loss terms     ops.cpr_loss_bwd (sigmoid, the shipped configs) against oracle.cpr_oracle.cpr_loss, ops.cpr_loss_bwd_general
                 (+ the gather) against oracle.cpr_options_oracle.cpr_loss -- both differentiated in fp64 wrt the map through
                 an exact channel-selecting classifier (identity rows, zero bias: the oracle's logits are the map's channels)

The window gather has four paths (bag_gather_launch): the full walk (K < 32), per-cell hit lists, lists with some cells
over the 16-point cap (mixed), and no lists at all (cap 0: the lists do not fit beside the taps in LDS).  ``_window_path``
recomputes on the host, with the kernel's own fp32 tap arithmetic, which one a launch takes; every case names and asserts it.

Bar, unless a test says otherwise: per element |got - ref| <= 1e-5 * max|ref| and relative L2 <= 1e-5.  The expected error is
a few fp32 ulps of the tap weights (the kernels compute the grid_sample coordinate round trip in fp32, the reference in fp64)
plus fp32 sums of at most K terms; the loss terms add fp32 expf / logf / divisions, a few ulps each.  Worst errors are printed
(run with -s)."""
import math
import os
import types

import numpy as np
import pytest
import torch

from oracle import cpr_oracle as O
from oracle import cpr_options_oracle as OO
from pointtinybenchmark_amd.dense_heads.cpr_head import CPRHead, _Extractor, circle_offsets, sqrt_threshold

EPS = 1e-6
BAR = 1e-5          # per element (of max|ref|) and relative L2
MASS = 1e-6         # mass conservation, of sum|dsample|
LDS_BUDGET = 60000  # bag_gather_launch: taps + hit lists must fit in this many bytes for the list path
W_MIL, W_NEG, W_GT = 0.25, 0.75, 0.25


# ------------------------------------------------------------------------------------------------ host helpers
def _generator(radius, base=8, start=0.0, same=False, stride=4):
    """Ring offsets (K-1, 2) fp32 and the gather window radius in cells, as CPRHead's extractor makes them."""
    pg = dict(type='CirclePtFeatGenerator', radius=radius, base_num_point=base, start_angle=start, same_num_all_radius=same)
    ex = _Extractor(pg, dict(type='OutCirclePtFeatGenerator', radius=radius), [stride], 1)
    return ex.offsets(stride, 'cpu'), ex.window_radius_cells(stride, 'cpu')


def _taps_fp32(ctr, off, stride, H, W):
    """Tap cells (x0, y0) (G, K) of every bag point exactly as bag_window_kernel computes them: px = off + c in fp32, the
    grid_sample coordinate round trip in fp32 round-to-nearest, border clamp, floor.  The centre is entry K-1."""
    f = np.float32
    ctr, off = np.asarray(ctr, f), np.asarray(off, f).reshape(-1, 2)
    p = np.concatenate([off[None] + ctr[:, None], ctr[:, None]], axis=1).astype(f)
    s = f(stride)
    out = []
    for a, n in ((0, f(W)), (1, f(H))):
        g = ((f(2) * (p[..., a] / s) + f(1)) / n - f(1)).astype(f)
        i = (((g + f(1)) * n - f(1)) * f(0.5)).astype(f)
        i = np.minimum(n - f(1), np.maximum(i, f(0)))
        out.append(np.floor(i).astype(np.int64))
    return out


def _window_path(ctr, off, stride, H, W, rc):
    """Which path bag_gather_launch + bag_window_kernel take: 'full' (K < 32), 'cap0' (the lists do not fit), else 'lists'
    or 'mixed' (some in-map window cell is covered by more than 16 points: that cell walks all K)."""
    K = off.shape[0] + 1
    win = 2 * int(math.ceil(rc)) + 3
    cap = 16 if (32 <= K <= 65535 and K * 16 + win * win * 36 <= LDS_BUDGET) else 0
    if cap == 0:
        return 'full' if K < 32 else 'cap0'
    x0, y0 = _taps_fp32(ctr, off, stride, H, W)
    worst = 0
    for g in range(x0.shape[0]):
        ox, oy = x0[g].min(), y0[g].min()
        hits = np.zeros((win + 2, win + 2), np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                np.add.at(hits, (y0[g] - oy + dy, x0[g] - ox + dx), 1)
        ys, xs = np.meshgrid(np.arange(win) + oy, np.arange(win) + ox, indexing='ij')
        worst = max(worst, int(np.where((xs < W) & (ys < H), hits[:win, :win], 0).max()))
    return 'mixed' if worst > cap else 'lists'


def _csr(counts, N, R=1):
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    gt_img = np.repeat(np.arange(N, dtype=np.int32), counts)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t(start), t(gt_img), t(start * R), t(np.repeat(gt_img, R))


def _centres(counts, H, W, stride, pad, seed, interior=0):
    """Per-image gt centres (fp32 pixels): the first ones of an image on the map / padding border and on exact cell
    boundaries (integer grid coordinate: tap weight 0 or 1), the rest uniform inside the padded image.  interior = r > 0:
    every centre at least r + 2 cells from the map border, on exact cell boundaries or uniform (no tap is clamped)."""
    rng = np.random.default_rng(seed)
    ph, pw = pad
    if interior:
        lo, hx, hy = (interior + 2) * stride, (W - interior - 2) * stride, (H - interior - 2) * stride
        out = []
        for c in counts:
            pts = [((rng.integers(lo // stride, hx // stride) + 0.5) * stride, rng.integers(lo // stride, hy // stride) * stride)
                   for _ in range(min(c, 2))]
            pts += [(rng.uniform(lo, hx), rng.uniform(lo, hy)) for _ in range(c - len(pts))]
            out.append(torch.tensor(pts, dtype=torch.float32).reshape(-1, 2))
        return out
    special = [(0.0, 0.0), (pw - 0.5, ph * 0.5), ((3 + 0.5) * stride, 5 * stride), (W * stride - 0.25, 2.0),
               (0.25 * pw, ph - 0.5), ((W // 2 + 0.5) * stride, (H // 2 + 0.5) * stride)]
    out = []
    for n, c in enumerate(counts):
        pts = [special[(n + i) % len(special)] for i in range(min(c, 3))]
        pts += [(rng.uniform(0, pw), rng.uniform(0, ph)) for _ in range(c - len(pts))]
        out.append(torch.tensor(pts, dtype=torch.float32).reshape(-1, 2))
    return out


def _report(name, got, ref, bar=BAR):
    """Per-element error of max|ref| and relative L2; asserts both <= bar and returns them."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    m = float(ref.abs().max())
    e = float((got - ref).abs().max()) / max(m, 1e-300)
    l2 = float((got - ref).norm()) / max(float(ref.norm()), 1e-300)
    print('ERR %-48s elem %.2e  l2 %.2e  (bar %.0e, max|ref| %.2e)' % (name, e, l2, bar, m), flush=True)
    if m == 0:                       # a term that does not reach this tensor: exactly zero
        assert float(got.abs().max()) == 0.0, name + ': non-zero where the reference is zero'
        return 0.0, 0.0
    assert e <= bar and l2 <= bar, '%s: elem %.3e l2 %.3e > %.0e' % (name, e, l2, bar)
    return e, l2


def _jd(J):
    return 4 if J <= 4 else (J + 31) // 32 * 32


class _Recorder:
    """Wraps oracle.cpr_oracle.sample_bilinear: keeps every sampled tensor, so the fp64 backward also yields the gradient
    wrt the bag logits (dbag) next to the one wrt the map."""

    def __init__(self, fn):
        self.fn, self.out = fn, []

    def __call__(self, *a, **k):
        s = self.fn(*a, **k)
        self.out.append(s)
        return s



def _per_image(fn, K):
    """oracle.cpr_oracle.cpr_points_and_logits one image at a time: it cannot take an image without gts (its FC reshape of an
    empty bag tensor is ambiguous), which the kernels' ABI allows.  Such an image has no bags and all of its grid points
    are negatives (cpr_oracle.py:203-209 with no centres)."""
    def run(sd, cls_feat, gt_bboxes, gt_labels, img_metas, stride, radius, num_classes, prefix='bbox_head.'):
        out = []
        for b in range(len(gt_bboxes)):
            if len(gt_labels[b]):
                out += fn(sd, cls_feat[b:b + 1], gt_bboxes[b:b + 1], gt_labels[b:b + 1], img_metas[b:b + 1], stride, radius,
                          num_classes, prefix)
                continue
            h, w = cls_feat.shape[2:]
            ph, pw = img_metas[b]['pad_shape'][:2]
            npts, nvalid = O.neg_valid_mask(h, w, stride, radius, gt_bboxes[b].new_zeros((0, 2)), gt_labels[b], num_classes, ph, pw)
            f = cls_feat[b].permute(1, 2, 0).flatten(0, 1)
            Wc, bc = sd[prefix + 'cls_out.weight'], sd[prefix + 'cls_out.bias']
            z = lambda c: cls_feat.new_zeros((0, K, c))
            out.append(dict(centers=gt_bboxes[b].new_zeros((0, 2)), pts=gt_bboxes[b].new_zeros((0, K, 2)),
                            valid=torch.zeros((0, K), dtype=torch.bool), cls_logit=z(Wc.shape[0]),
                            ins_logit=z(sd[prefix + 'ins_out.weight'].shape[0]), neg_pts=npts, neg_valid=nvalid,
                            neg_logit=torch.nn.functional.linear(f, Wc, bc)))
        return out
    return run


def _identity_sd(J, C, n_ins):
    eye = torch.eye(J, dtype=torch.float64)
    z = lambda n: torch.zeros(n, dtype=torch.float64)
    return {'bbox_head.cls_out.weight': eye[:C], 'bbox_head.cls_out.bias': z(C),
            'bbox_head.ins_out.weight': eye[C:C + n_ins], 'bbox_head.ins_out.bias': z(n_ins)}


# ------------------------------------------------------------------------------------------------ host-only test
GEN_OPTIONS = [  # radius, base_num_point, start_angle, same_num_all_radius
    (2, 8, 0.0, False), (5, 8, 0.0, False), (8, 8, 0.0, False), (5, 32, 0.0, False), (16, 8, 0.0, False),
    (5, 8, 22.5, False), (5, 8, 0.0, True), (5, 8, 22.5, True), (3, 12, 7.0, True)]


@pytest.mark.parametrize('stride', [4, 8])
@pytest.mark.parametrize('gen', GEN_OPTIONS, ids=lambda g: 'r%d_b%d_a%g_%s' % (g[0], g[1], g[2], 'same' if g[3] else 'grow'))
def test_window_holds_every_tap_host(gen, stride):
    """No GPU.  bag_window_kernel accumulates only the (2*ceil(r)+3)^2 cells from the smallest tap cell of a bag and drops
    what falls outside without an error; window_radius_cells sizes r from the offsets.  For every generator option set and
    4096 random fractional centres (plus exact cell boundaries and the map border), each axis' tap span
    max(x0) + 1 - min(x0) + 1 cells, computed in fp32 as the kernel computes it, must fit in the window."""
    off, rc = _generator(*gen, stride=stride)
    assert rc == math.ceil(float(off.abs().max()) / stride)
    win = 2 * rc + 3
    H = W = 4 * rc + 40
    rng = np.random.default_rng(gen[0] * 100 + gen[1] + stride)
    c = rng.uniform(0, W * stride, size=(4096, 2)).astype(np.float32)
    k = rng.integers(0, W, size=(512, 2)).astype(np.float32)
    c = np.concatenate([c, (k + 0.5) * stride, k * stride, [[0, 0], [W * stride - 1e-3, H * stride - 1e-3]]]).astype(np.float32)
    x0, y0 = _taps_fp32(c, off.numpy(), stride, H, W)
    for name, t in (('x', x0), ('y', y0)):
        span = t.max(1) + 1 - t.min(1) + 1
        assert int(span.max()) <= win, '%s span %d cells > window %d (gen %s, stride %d)' % (name, span.max(), win, gen, stride)


def test_loss_reference_is_the_oracle_host():
    """No GPU.  The loss reference below is oracle.cpr_oracle.cpr_loss itself, run in fp64 through an identity classifier with
    its ring offsets swapped for the generator's: at the default generator options the two offset sets are bit-equal, and
    the channel-selecting classifier reproduces the map's channels bit for bit."""
    off, _ = _generator(5, stride=4)
    assert torch.equal(off, O.circle_offsets(5, 4).float())
    assert torch.equal(circle_offsets(3, 8, 12, 7.0, False), O.circle_offsets(3, 8, 12, 7.0).float())
    m = torch.randn((1, 6, 5, 7), dtype=torch.float64)
    sd = _identity_sd(6, 2, 4)
    f = m.permute(0, 2, 3, 1)
    assert torch.equal(torch.nn.functional.linear(f, sd['bbox_head.cls_out.weight'], sd['bbox_head.cls_out.bias']), f[..., :2])
    assert torch.equal(torch.nn.functional.linear(f, sd['bbox_head.ins_out.weight'], sd['bbox_head.ins_out.bias']), f[..., 2:])


# ------------------------------------------------------------------------------------------------ GPU: ring-bag window gather
def _ops():
    from pointtinybenchmark_amd import ops
    return ops


# Expected paths: a bag at the map border is clamped onto the edge cells, which then collect more than 16 points -- such
# launches are 'mixed' even at 8 base points; the '_interior' cases keep every bag off the border.
RING_CASES = {  # radius, base, start, same, stride, N, H, W, J, counts, interior, expected path
    'r2_b8_s8_J14_full': (2, 8, 0.0, False, 8, 2, 24, 20, 14, [3, 2], False, 'full'),
    'r5_b8_s4_J2_lists_interior': (5, 8, 0.0, False, 4, 2, 40, 40, 2, [1, 4], True, 'lists'),
    'r5_b8_s4_J3_border': (5, 8, 0.0, False, 4, 2, 40, 40, 3, [3, 4], False, 'mixed'),
    'r8_b8_s4_J33_G64_interior': (8, 8, 0.0, False, 4, 2, 64, 64, 33, [40, 24], True, 'lists'),
    'r8_b8_s4_J33_G64_border': (8, 8, 0.0, False, 4, 2, 64, 64, 33, [40, 24], False, 'mixed'),
    'r5_b32_s4_J16_mixed_interior': (5, 32, 0.0, False, 4, 2, 48, 48, 16, [3, 3], True, 'mixed'),
    'r16_b8_s4_J6_cap0': (16, 8, 0.0, False, 4, 2, 96, 96, 6, [2, 3], False, 'cap0'),
    'r5_a22.5_s8_J160': (5, 8, 22.5, False, 8, 1, 32, 32, 160, [5], False, 'mixed'),
    'r5_same_s4_J7_interior': (5, 8, 0.0, True, 4, 2, 40, 36, 7, [2, 3], True, 'lists'),
    'r5_a22.5_same_s8_empty_middle_J5': (5, 8, 22.5, True, 8, 3, 32, 32, 5, [2, 0, 3], False, 'mixed'),
    'r5_b8_s4_G1_J1': (5, 8, 0.0, False, 4, 1, 32, 32, 1, [1], False, 'mixed'),
}


def _ring_setup(case, seed):
    radius, base, start, same, stride, N, H, W, J, counts, interior, _ = case
    off, rc = _generator(radius, base, start, same, stride)
    pad = (H * stride - 3, W * stride) if N > 1 else (H * stride, W * stride)
    ctr_l = _centres(counts, H, W, stride, pad, seed, interior=rc if interior else 0)
    ctr = torch.cat(ctr_l)
    return off, rc, pad, ctr_l, ctr


def _ring_ref(ctr_l, off, stride, N, H, W, J, ds, align=False):
    """fp64 d/dmap sum(ds * sample_bilinear(map64, pts / stride)) over every image's bags; also the dropped weight of
    each image (align_corners=True zeros padding: 1 - the in-map weight of every entry) as (N, J)."""
    m64 = torch.zeros((N, J, H, W), dtype=torch.float64, requires_grad=True)
    ones = torch.ones((1, 1, H, W), dtype=torch.float64)
    tot, s0, drop = 0.0, 0, torch.zeros((N, J), dtype=torch.float64)
    for n, c in enumerate(ctr_l):
        g = c.shape[0]
        if g == 0:
            continue
        pts = torch.cat([off[None] + c[:, None], c[:, None]], dim=1)
        d = ds[s0:s0 + g].double()
        tot = tot + (O.sample_bilinear(m64[n:n + 1], pts / stride, align) * d).sum()
        drop[n] = ((1 - O.sample_bilinear(ones, pts / stride, align)) * d).sum(dim=(0, 1))
        s0 += g
    tot.backward()
    return m64.grad.permute(0, 2, 3, 1), drop


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(RING_CASES))
def test_ring_gather_vs_fp64(name):
    """ops.bag_gather_bwd for random dsample against fp64 autograd of the oracle's bilinear sampling (border padding); the
    bag points / validity the forward sampled are the host's bit for bit.  Mass conservation per (image, channel): every
    entry's four tap weights sum to one, so sum(dmap) = the image's sum(dsample) to 1e-6 of sum|dsample| (fp32 products
    and sums of at most 4K terms) -- the check that catches a dropped tap.  The gather ADDS: a pre-filled dmap keeps its
    values and channels J..Jd-1 stay exactly zero.  Two launches are bit-equal (no float atomics)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ops = _ops()
    case = RING_CASES[name]
    radius, base, start, same, stride, N, H, W, J, counts, _, path = case
    off, rc, pad, ctr_l, ctr = _ring_setup(case, seed=len(name))
    K = off.shape[0] + 1
    G = ctr.shape[0]
    got_path = _window_path(ctr.numpy(), off.numpy(), stride, H, W, rc)
    print('PATH %s K=%d win=%d -> %s' % (name, K, 2 * rc + 3, got_path))
    assert got_path == path, (name, got_path)
    start_t, gt_img, _, _ = _csr(counts, N)
    pad_hw = torch.tensor(list(pad) * N, dtype=torch.int32).cuda()
    gen = torch.Generator().manual_seed(K + J)
    lmap = torch.randn((N, H, W, J), generator=gen).cuda()
    pts, valid, _ = ops.bag_sample(lmap, ctr.cuda(), gt_img, pad_hw, off.cuda(), stride)
    ref_pts = torch.cat([off[None] + ctr[:, None], ctr[:, None]], dim=1)
    assert torch.equal(pts.cpu(), ref_pts)
    assert torch.equal(valid.cpu().bool(), O.inside(ref_pts, *pad))
    ds = torch.randn((G, K, J), generator=gen)
    ds[:, ::7] = 0.0                                  # exact zeros are skipped by the kernel
    Jd = _jd(J)
    ref, _ = _ring_ref(ctr_l, off, stride, N, H, W, J, ds)
    a = ops.bag_gather_bwd(ds.cuda(), ctr.cuda(), gt_img, off.cuda(), torch.zeros((N, H, W, Jd)).cuda(), stride, rc)
    b = ops.bag_gather_bwd(ds.cuda(), ctr.cuda(), gt_img, off.cuda(), torch.zeros((N, H, W, Jd)).cuda(), stride, rc)
    torch.cuda.synchronize()
    assert torch.equal(a, b), 'two launches of the same gather differ'
    a = a.cpu()
    assert bool((a[..., J:] == 0).all())
    _report('ring %s dmap' % name, a[..., :J], ref)
    counts_t = torch.tensor(counts)
    for n in range(N):
        lo = int(counts_t[:n].sum())
        want = ds[lo:lo + counts[n]].double().sum(dim=(0, 1))
        scale = max(float(ds[lo:lo + counts[n]].double().abs().sum()), 1.0)
        err = float((a[n, ..., :J].double().sum(dim=(0, 1)) - want).abs().max()) / scale
        assert err <= MASS, 'image %d: sum(dmap) - sum(dsample) = %.3e of sum|dsample|' % (n, err)
    pre = torch.zeros((N, H, W, Jd))
    pre[..., :J] = torch.randn((N, H, W, J), generator=gen)
    c = ops.bag_gather_bwd(ds.cuda(), ctr.cuda(), gt_img, off.cuda(), pre.cuda(), stride, rc).cpu()
    assert bool((c[..., J:] == 0).all())
    _report('ring %s prefilled dmap' % name, c[..., :J], ref + pre[..., :J].double())


@pytest.mark.gpu
@pytest.mark.parametrize('gen', [(5, 8), (5, 32)], ids=['r5_b8_lists', 'r5_b32_mixed'])
def test_window_paths_bit_equal(gen):
    """The window kernel gives the same bits whichever path a cell takes.  The same bags and dsample run once as they are
    (hit lists; with 32 base points some cells overflow the 16-point cap and walk all K) and once with K pushed over the LDS
    budget (cap 0: every cell walks all K) by zero offsets inserted before the centre entry, whose dsample is exactly 0:
    the kernel skips zero entries and the non-zero contributors keep their order, so the two dmaps are bit-equal."""
    ops = _ops()
    stride, N, H, W, J, counts = 4, 2, 48, 48, 12, [4, 3]
    off, rc = _generator(gen[0], gen[1], stride=stride)
    K = off.shape[0] + 1
    win = 2 * rc + 3
    Kp = 3500
    assert Kp * 16 <= LDS_BUDGET < Kp * 16 + win * win * 36         # accepted by the ABI, no room for the lists
    ctr = torch.cat(_centres(counts, H, W, stride, (H * stride, W * stride), seed=gen[1], interior=rc))
    G = ctr.shape[0]
    off2 = torch.cat([off, torch.zeros((Kp - K, 2))])
    p1, p2 = _window_path(ctr.numpy(), off.numpy(), stride, H, W, rc), _window_path(ctr.numpy(), off2.numpy(), stride, H, W, rc)
    print('PATH r%d_b%d: %s vs %s' % (gen[0], gen[1], p1, p2))
    assert p1 == ('mixed' if gen[1] == 32 else 'lists') and p2 == 'cap0'
    ds = torch.randn((G, K, J), generator=torch.Generator().manual_seed(K))
    ds2 = torch.cat([ds[:, :K - 1], torch.zeros((G, Kp - K, J)), ds[:, K - 1:]], dim=1)
    _, gt_img, _, _ = _csr(counts, N)
    a = ops.bag_gather_bwd(ds.cuda(), ctr.cuda(), gt_img, off.cuda(), torch.zeros((N, H, W, 32)).cuda(), stride, rc)
    b = ops.bag_gather_bwd(ds2.cuda().contiguous(), ctr.cuda(), gt_img, off2.cuda().contiguous(),
                           torch.zeros((N, H, W, 32)).cuda(), stride, rc)
    torch.cuda.synchronize()
    assert torch.equal(a, b), 'hit-list and full-walk windows differ: max %.3e' % float((a - b).abs().max())
    assert float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ GPU: point-list gather
@pytest.mark.gpu
@pytest.mark.parametrize('align', [False, True], ids=['border', 'align_corners'])
def test_point_list_gather_ring_vs_fp64(align):
    """ops.bag_points_gather_bwd with every entry a bilinear sample (code None: ring bags under align_corners=True, and the
    border-clip form) against fp64 autograd of sample_bilinear.  Zeros padding (align_corners=True) drops the taps outside
    the map: per (image, channel) sum(dmap) = sum(dsample) - the dropped weight, and want_bias returns that weight summed
    over the batch (1e-6 of sum|dsample|).  Border padding drops nothing.  Channel slices: J = 33 (two 32-channel slices)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ops = _ops()
    stride, N, H, W, J, counts = 4, 3, 30, 34, 33, [3, 0, 4]
    off, _ = _generator(5, stride=stride)
    K = off.shape[0] + 1
    pad = (H * stride, W * stride - 5)
    ctr_l = _centres(counts, H, W, stride, pad, seed=3 + align)
    ctr = torch.cat(ctr_l)
    G = ctr.shape[0]
    _, _, _, gt_img = _csr(counts, N)
    pad_hw = torch.tensor(list(pad) * N, dtype=torch.int32).cuda()
    gen = torch.Generator().manual_seed(11)
    lmap = torch.randn((N, H, W, J), generator=gen).cuda()
    pts, valid, _ = ops.bag_sample(lmap, ctr.cuda(), gt_img, pad_hw, off.cuda(), stride, align_corners=align)
    assert torch.equal(pts.cpu(), torch.cat([off[None] + ctr[:, None], ctr[:, None]], dim=1))
    ds = torch.randn((G, K, J), generator=gen)
    ref, drop = _ring_ref(ctr_l, off, stride, N, H, W, J, ds, align)
    Jd = _jd(J)
    dmap = torch.zeros((N, H, W, Jd)).cuda()
    dbias = ops.bag_points_gather_bwd(ds.cuda(), pts, None, gt_img, dmap, stride, align, want_bias=True)
    torch.cuda.synchronize()
    got = dmap.cpu()
    assert bool((got[..., J:] == 0).all())
    _report('points ring align=%d dmap' % align, got[..., :J], ref)
    scale = float(ds.double().abs().sum())
    if align:
        assert float(drop.abs().max()) > 0, 'no tap fell outside the map'
        err = float((dbias.cpu().double() - drop.sum(0)).abs().max()) / scale
        print('ERR points ring align dbias %.2e of sum|ds| (bar %.0e)' % (err, MASS))
        assert err <= MASS, err
    else:
        assert float(drop.abs().max()) <= 1e-12 * scale and float(dbias.abs().max()) == 0.0
    s0 = 0
    for n in range(N):
        want = ds[s0:s0 + counts[n]].double().sum(dim=(0, 1)) - drop[n]
        err = float((got[n, ..., :J].double().sum(dim=(0, 1)) - want).abs().max()) / scale
        assert err <= MASS, (n, err)
        s0 += counts[n]


@pytest.mark.gpu
@pytest.mark.parametrize('R,radius,stride,align', [(1, 3, 4, False), (2, 2, 8, True)], ids=['R1_r3_s4', 'R2_r2_s8_align'])
def test_grid_bag_gather_vs_fp64(R, radius, stride, align):
    """GridCirclesPtFeatGenerator bags: ops.grid_bag(want_cell=True) gives the entry codes; its cells and counts agree with
    the oracle's grid_circle_bag (host).  The gather takes the device's own code list as geometry: a cell entry has weight 1
    on that cell, a padding slot (-1) sends its dsample to the bias, a refine point (<= -2) is a bilinear sample (border
    clip, or zeros padding with align_corners=True, whose dropped weight also goes to the bias).  dmap and dbias against
    fp64 autograd of that description; the same bar, dbias to 1e-6 of sum|dsample|."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ops = _ops()
    N, H, W, J, counts = 2, 28, 26, 9, [3, 2]
    G = sum(counts)
    mp = 2 * (2 * radius) ** 2
    pad = (H * stride, W * stride)
    gen = torch.Generator().manual_seed(R * 10 + radius)
    ctr_l = [c.reshape(-1, R, 2) for c in _centres([c * R for c in counts], H, W, stride, pad, seed=R)]
    pts_all = torch.cat([c.reshape(-1, 2) for c in ctr_l])
    _, gt_img, _, _ = _csr(counts, N)
    lmap = torch.randn((N, H, W, J), generator=gen)
    pts, valid, _, count, code = ops.grid_bag(lmap.cuda(), pts_all.cuda(), gt_img, R, mp + R, radius * stride, stride,
                                              align_corners=align, want_cell=True)
    pts, valid, count, code = pts.cpu(), valid.cpu().bool(), count.cpu(), code.cpu()
    Kt = code.shape[1]
    # host recomputation of the integer geometry
    s0 = 0
    for n, c in enumerate(ctr_l):
        rp, rv, _ = OO.grid_circle_bag(lmap[n:n + 1].permute(0, 3, 1, 2), c, radius, stride, mp, align)
        g = c.shape[0]
        assert torch.equal(valid[s0:s0 + g], rv)
        for i in range(g):
            k = int(count[s0 + i])
            assert k == int(rv[i, :mp + R].sum())
            cells = code[s0 + i, :k]
            xy = torch.stack([cells % W, cells // W], -1).float() * stride + stride / 2
            assert torch.equal(xy, rp[i, :k]) and bool((code[s0 + i, k:Kt - R] == -1).all())
            assert bool((code[s0 + i, Kt - R:] <= -2).all()) and torch.equal(pts[s0 + i, Kt - R:], rp[i, Kt - R:])
        s0 += g
    ds = torch.randn((G, Kt, J), generator=gen)
    # fp64 reference on the device's code list
    m64 = torch.zeros((N, J, H, W), dtype=torch.float64, requires_grad=True)
    ones = torch.ones((1, 1, H, W), dtype=torch.float64)
    tot, dbias_ref = 0.0, torch.zeros(J, dtype=torch.float64)
    gi = gt_img.cpu()
    for e in range(G):
        n, d = int(gi[e]), ds[e].double()
        cell = code[e] >= 0
        flat = m64[n].reshape(J, H * W)
        tot = tot + (flat[:, code[e][cell].long()].t() * d[cell]).sum()
        dbias_ref += d[code[e] == -1].sum(0)
        bl = code[e] <= -2
        p = pts[e][bl][None] / stride
        tot = tot + (O.sample_bilinear(m64[n:n + 1], p, align)[0] * d[bl]).sum()
        dbias_ref += ((1 - O.sample_bilinear(ones, p, align)[0]) * d[bl]).sum(0)
    tot.backward()
    ref = m64.grad.permute(0, 2, 3, 1)
    Jd = _jd(J)
    dmap = torch.zeros((N, H, W, Jd)).cuda()
    dbias = ops.bag_points_gather_bwd(ds.cuda(), pts.cuda(), code.cuda(), gt_img, dmap, stride, align, want_bias=True)
    torch.cuda.synchronize()
    got = dmap.cpu()
    assert bool((got[..., J:] == 0).all())
    _report('grid R%d r%d align=%d dmap' % (R, radius, align), got[..., :J], ref)
    scale = float(ds.double().abs().sum())
    err = float((dbias.cpu().double() - dbias_ref).abs().max()) / scale
    print('ERR grid dbias %.2e of sum|ds| (bar %.0e)' % (err, MASS))
    assert err <= MASS, err
    tot_err = float((got[..., :J].double().sum(dim=(0, 1, 2)) + dbias.cpu().double() - ds.double().sum(dim=(0, 1))).abs().max())
    assert tot_err <= MASS * scale, tot_err


# ------------------------------------------------------------------------------------------------ GPU: loss backward
def _saturate(m, J, C, H, W):
    """A block of saturated logits in image 0 (the top-left 10 x 10 cells): class logits -15 (p ~ 3e-7 < eps: the clamps of
    log(p + eps)), instance logits +-15 in a checkerboard (softmax weights of ~e^-30 over a bag)."""
    y, x = torch.meshgrid(torch.arange(10), torch.arange(10), indexing='ij')
    m[0, :10, :10, :C] = -15.0
    m[0, :10, :10, C:] = torch.where(((x + y) % 2 == 0)[..., None], 15.0, -15.0).expand(10, 10, J - C)
    # instance logits +15 beyond the padded width, -15 inside: a bag straddling it has all its softmax mass on invalid
    # points (sum over the valid ones < 1e-12: the F.normalize clamp)
    m[0, :, W - 4:, C:] = 15.0
    m[0, :, W - 8:W - 4, C:] = -15.0


LOSS_CASES = {  # C, radius, base, start, same, stride, N, H, W, counts, with_gt, saturate
    'c1_r5_s4_G5': (1, 5, 8, 0.0, False, 4, 2, 40, 40, [3, 2], True, False),
    'c7_r2_s8_G5_full': (7, 2, 8, 0.0, False, 8, 2, 24, 20, [1, 4], True, False),
    'c8_r8_s4_G64_cls8': (8, 8, 8, 0.0, False, 4, 2, 64, 64, [40, 24], True, False),
    'c80_r5_s4_nogt': (80, 5, 8, 0.0, False, 4, 1, 48, 48, [5], False, False),
    'c3_r16_s4_cap0': (3, 16, 8, 0.0, False, 4, 2, 96, 96, [2, 2], True, False),
    'c1_r5_b32_mixed': (1, 5, 32, 0.0, False, 4, 2, 48, 48, [3, 3], True, False),
    'c2_r5_a22.5_same_s8': (2, 5, 8, 22.5, True, 8, 2, 32, 32, [2, 3], True, False),
    'c3_empty_middle': (3, 5, 8, 0.0, False, 4, 3, 36, 36, [2, 0, 3], True, False),
    'c5_G1': (5, 5, 8, 0.0, False, 4, 1, 32, 32, [1], True, False),
    'c1_saturated': (1, 5, 8, 0.0, False, 4, 1, 40, 40, [4], True, True),
}


def _loss_inputs(C, J, stride, N, H, W, counts, saturate, seed, radius):
    gen = torch.Generator().manual_seed(seed)
    m = 2.0 * torch.randn((N, H, W, J), generator=gen)
    pad = (H * stride, (W - 4) * stride) if saturate else ((H * stride - 6, W * stride) if N > 1 else (H * stride, W * stride))
    ctr_l = _centres(counts, H, W, stride, pad, seed)
    if saturate:
        _saturate(m, J, C, H, W)
        ctr_l[0] = torch.cat([torch.tensor([[2.5 * stride, 3.0 * stride], [pad[1] + 1.5 * stride, H * stride / 2]]),
                              ctr_l[0][2:]])
    labels_l = [torch.randint(0, C, (c,), generator=gen) for c in counts]
    return m, pad, ctr_l, labels_l


def _upstream(seed):
    return torch.rand(5, generator=torch.Generator().manual_seed(seed)) + 0.5


# (upstream slots zeroed): every term at its own random weight, the bag terms (gt_loss, pos_loss) alone, the negative term alone
SPLITS = (('all', (1, 1, 1, 1, 1)), ('bag_terms', (1, 1, 1, 0, 1)), ('neg_term', (0, 0, 1, 1, 1)))
SLOTS = {0: 'gt_loss', 1: 'pos_loss', 3: 'neg_loss'}


def _check_terms(name, bwd, up, losses, m64, rec, J, neg_bar=BAR):
    """For each split of SPLITS: the device backward with that upstream vector against torch.autograd.grad of the same
    weighted sum of the oracle's losses, wrt the map (dmap) and wrt the recorded bag samples (dbag).  neg_bar: the bar of
    the dmaps that carry the negative term (see GENERAL_CASES)."""
    for split, keep in SPLITS:
        u = (up * torch.tensor(keep, dtype=up.dtype, device=up.device)).contiguous()
        dmap, dbag = bwd(u)
        torch.cuda.synchronize()
        ud = u.cpu().double()
        total = sum(ud[i] * losses[k] for i, k in SLOTS.items() if k in losses and keep[i])
        g = torch.autograd.grad(total, [m64] + rec.out, retain_graph=True, allow_unused=True)
        ref_bag = torch.cat([t if t is not None else torch.zeros_like(s) for t, s in zip(g[1:], rec.out)])
        dmap = dmap.cpu()
        assert bool((dmap[..., J:] == 0).all()), 'channels J..Jd-1 of dmap are not zero'
        _report('loss %s %s dmap' % (name, split), dmap[..., :J], g[0].permute(0, 2, 3, 1), neg_bar if keep[3] else BAR)
        _report('loss %s %s dbag' % (name, split), dbag, ref_bag.reshape(dbag.shape))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(LOSS_CASES))
def test_cpr_loss_bwd_vs_fp64_oracle(name, monkeypatch):
    """ops.cpr_loss_bwd (sigmoid probabilities, independent bags: the shipped configs' kernels) after the forward calls the
    head makes (neg_mask_loss, bag_sample, mil_loss) against oracle.cpr_oracle.cpr_loss differentiated in fp64 wrt the map,
    upstream weights random per term: dmap and dbag to the file's bar.  The negative mask and the bag validity are the
    oracle's fp32 ones bit for bit.  upstream[2] (bag_acc) and upstream[4] (num_sample) change no bit; two launches are
    bit-equal.  Cases: C = 1 / 5 / 7 (4 bags per workgroup, G = 1 and 5 ragged), 8 / 80 (8-wave form, G = 64), J = 2C not a
    multiple of 4 with Jd > J, the full-walk / mixed / cap-0 window paths, an image without bags, a block of saturated logits."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ops = _ops()
    C, radius, base, start, same, stride, N, H, W, counts, with_gt, saturate = LOSS_CASES[name]
    J, Jd = 2 * C, _jd(2 * C)
    off, rc = _generator(radius, base, start, same, stride)
    K = off.shape[0] + 1
    m, pad, ctr_l, labels_l = _loss_inputs(C, J, stride, N, H, W, counts, saturate, len(name) + C, radius)
    ctr, labels = torch.cat(ctr_l), torch.cat(labels_l)
    G = ctr.shape[0]
    print('PATH %s K=%d -> %s' % (name, K, _window_path(ctr.numpy(), off.numpy(), stride, H, W, rc)))
    # ---- device: the head's forward calls (cpr_head.py loss), then the backward
    gt_start, gt_img, _, _ = _csr(counts, N)
    pad_hw = torch.tensor(list(pad) * N, dtype=torch.int32).cuda()
    lmap, c_d, l_d, off_d = m.cuda(), ctr.cuda(), labels.to(torch.int32).cuda(), off.cuda()
    w_gt = W_GT if with_gt else 0.0
    mask, partial = ops.neg_mask_loss(lmap, c_d, l_d, gt_start, pad_hw, C, stride, sqrt_threshold(stride * radius), EPS, True,
                                      'sigmoid', 1.0, mask_classes=C)
    pts, valid, bag = ops.bag_sample(lmap, c_d, gt_img, pad_hw, off_d, stride)
    out5, bag_ws = ops.mil_loss(bag, C, valid, l_d, C, partial, W_MIL, w_gt, W_NEG, None, EPS, bags=(G, K, 0, K),
                                centres=(K - 1, K, 1, 1) if with_gt else (0, 1, 0, 1), prob_type='sigmoid')
    up = _upstream(G).cuda()

    def bwd(u):
        return ops.cpr_loss_bwd(lmap, mask, out5, bag, valid, l_d, bag_ws, c_d, gt_img, off_d, C, C, stride, W_MIL, w_gt,
                                W_NEG, Jd, gt_weight=None, eps=EPS, upstream=u, radius_cells=rc)
    dmap, dbag = bwd(up)
    dmap2, dbag2 = bwd(up)
    up2 = up.clone()
    up2[2] += 3.0
    up2[4] -= 0.25
    dmap3, dbag3 = bwd(up2)
    torch.cuda.synchronize()
    assert torch.equal(dmap, dmap2) and torch.equal(dbag, dbag2), 'two launches differ'
    assert torch.equal(dmap, dmap3) and torch.equal(dbag, dbag3), 'upstream[2] / upstream[4] changed the gradient'
    # ---- fp64 oracle: identity classifier, the generator's ring offsets
    rec = _Recorder(O.sample_bilinear)
    monkeypatch.setattr(O, 'sample_bilinear', rec)
    monkeypatch.setattr(O, 'circle_offsets', lambda r, s: off)
    monkeypatch.setattr(O, 'cpr_points_and_logits', _per_image(O.cpr_points_and_logits, K))
    m64 = m.permute(0, 3, 1, 2).double().contiguous().requires_grad_(True)
    boxes = [torch.cat([c, c], dim=1) for c in ctr_l]
    metas = [dict(pad_shape=(pad[0], pad[1], 3))] * N
    losses, per = O.cpr_loss(_identity_sd(J, C, C), m64, boxes, labels_l, metas, stride, radius, C, W_MIL, W_NEG, W_GT,
                             with_gt_loss=with_gt)
    assert torch.equal(valid.cpu().bool(), torch.cat([p['valid'] for p in per]))
    assert torch.equal(mask.cpu().bool(), torch.cat([p['neg_valid'] for p in per]))
    assert float(out5[4]) == max(1.0, float((valid.cpu().sum(1) > 0).sum()))           # num_sample
    assert torch.equal(torch.cat([p['pts'] for p in per]), pts.cpu())
    _check_terms(name, bwd, up, losses, m64, rec, J)


# neg_bar: the negative term's gradient through softmax / normed_sigmoid is p_c (g_c - sum_j g_j p_j) (resp. g_c / n -
# (sum_j g_j s_j) s_c n^-3), which cancels where one class dominates a pixel and g_c ~ p^2 / (1 - p + eps) is large.  That
# formula evaluated in fp32 by torch on the CPU is off from fp64 by 5.1e-5 (softmax) and 1.22e-4 (normed_sigmoid) of max|ref|
# on these maps (the kernels: 4.2e-5 and 1.2e-4): the bar there is twice the fp32 evaluation's error, every other bar stays 1e-5.
GENERAL_CASES = {  # cfg for oracle.cpr_options_oracle (+ C, R, neg_bar)
    'softmax_c3': dict(num_classes=3, prob='softmax', neg_bar=1e-4),
    'normed_sigmoid_p2_c3': dict(num_classes=3, prob='normed_sigmoid', norm_p=2, neg_bar=2.5e-4),
    'binary_ins_c2': dict(num_classes=2, binary_ins=True),
    'allpos_c3': dict(num_classes=3, loss='AllPosLoss'),
    'merge_to_gt_bag_R2_c2': dict(num_classes=2, policy='merge_to_gt_bag', R=2),
    'no_mil_c3': dict(num_classes=3, with_mil_loss=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GENERAL_CASES))
def test_cpr_loss_bwd_general_vs_fp64_oracle(name, monkeypatch):
    """ops.cpr_loss_bwd_general + ops.bag_gather_bwd (the loss options off the shipped configs) against
    oracle.cpr_options_oracle.cpr_loss differentiated in fp64 wrt the map: softmax, normed_sigmoid (p = 2), binary_ins,
    AllPosLoss, merged bags (num_refine = 2, merge_to_gt_bag) and with_mil_loss=False, random per-term upstream.  dmap and
    dbag to the file's bar (the negative term under softmax / normed_sigmoid: see neg_bar above); mask and validity
    bit-equal; upstream[2] / upstream[4] change no bit; two launches bit-equal."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ops = _ops()
    cfg = dict(GENERAL_CASES[name])
    C, R, neg_bar = cfg['num_classes'], cfg.pop('R', 1), cfg.pop('neg_bar', BAR)
    bi, allpos, with_mil = cfg.pop('binary_ins', False), cfg.get('loss') == 'AllPosLoss', cfg.get('with_mil_loss', True)
    prob, p = cfg.get('prob', 'sigmoid'), float(cfg.get('norm_p', 1))
    stride, radius, N, H, W, counts = 4, 5, 2, 32, 36, [3, 2]
    cfg.update(stride=stride, radius=radius)
    nins = 2 * C if bi else C
    J, Jd = C + nins, _jd(C + nins)
    off, rc = _generator(radius, stride=stride)
    K = off.shape[0] + 1
    m, pad, ctr_l, labels_l = _loss_inputs(C, J, stride, N, H, W, [c * R for c in counts], False, len(name), radius)
    labels_l = [l[::R].contiguous() for l in labels_l]
    G = sum(counts)
    ctr, labels = torch.cat(ctr_l), torch.cat(labels_l)
    # ---- device, in the head's layout (points gt-major; cpr_head.py _gt_tensors / _loss_geometry)
    gt_start, gt_img, pt_start, pt_img = _csr(counts, N, R)
    pad_hw = torch.tensor(list(pad) * N, dtype=torch.int32).cuda()
    lmap, c_d, off_d = m.cuda(), ctr.cuda(), off.cuda()
    l_d = labels.to(torch.int32).cuda()
    pt_l = l_d.repeat_interleave(R).contiguous()
    loss_cfg = dict(refine_bag_policy=cfg.get('policy', 'independent_with_gt_bag'), with_gt_loss=True, with_mil_loss=with_mil)
    gts = types.SimpleNamespace(G=G, R=R, labels=l_d, pt_labels=pt_l)
    bags, centres, lab_b, _ = CPRHead._loss_geometry(types.SimpleNamespace(loss_cfg=loss_cfg), gts, (R, K), None, lmap.device)
    w_mil = W_MIL if with_mil else 0.0
    mask, partial = ops.neg_mask_loss(lmap, c_d, pt_l, pt_start, pad_hw, C, stride, sqrt_threshold(stride * radius), EPS, True,
                                      prob, p, mask_classes=C)
    pts, valid, bag = ops.bag_sample(lmap, c_d, pt_img, pad_hw, off_d, stride)
    out5, bag_ws = ops.mil_loss(bag.view(G, R * K, J), C, valid.view(G, R * K), lab_b, C, partial, w_mil, W_GT, W_NEG, None,
                                EPS, bags=bags, centres=centres, prob_type=prob, norm_p=p, binary_ins=bi, allpos=allpos,
                                neg_from_gt=not with_mil)
    up = _upstream(len(name)).cuda()

    def bwd(u):
        dmap, dbag = ops.cpr_loss_bwd_general(lmap, mask, out5, bag, valid, lab_b, bag_ws, bags, centres, C, C, Jd, w_mil, W_GT,
                                              W_NEG, eps=EPS, upstream=u, prob_type=prob, norm_p=p, binary_ins=bi,
                                              allpos=allpos, neg_from_gt=not with_mil)
        return ops.bag_gather_bwd(dbag, c_d, pt_img, off_d, dmap, stride, rc), dbag
    dmap, dbag = bwd(up)
    dmap2, dbag2 = bwd(up)
    up2 = up.clone()
    up2[2] *= 3.0
    up2[4] += 1.0
    dmap3, dbag3 = bwd(up2)
    torch.cuda.synchronize()
    assert torch.equal(dmap, dmap2) and torch.equal(dbag, dbag2), 'two launches differ'
    assert torch.equal(dmap, dmap3) and torch.equal(dbag, dbag3), 'upstream[2] / upstream[4] changed the gradient'
    # ---- fp64 options oracle
    rec = _Recorder(O.sample_bilinear)
    monkeypatch.setattr(O, 'sample_bilinear', rec)
    m64 = m.permute(0, 3, 1, 2).double().contiguous().requires_grad_(True)
    boxes = [torch.cat([c, c], dim=1) for c in ctr_l]
    metas = [dict(pad_shape=(pad[0], pad[1], 3))] * N
    losses, per = OO.cpr_loss(_identity_sd(J, C, nins), m64, boxes, labels_l, metas, cfg, W_MIL, W_NEG, W_GT)
    assert torch.equal(valid.cpu().bool(), torch.cat([q['valid'] for q in per]).reshape(G * R, K))
    assert torch.equal(mask.cpu().bool(), torch.cat([q['neg_valid'] for q in per]))
    _check_terms(name, bwd, up, losses, m64, rec, J, neg_bar)
