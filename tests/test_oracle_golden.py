"""The CPU oracle (oracle/cpr_oracle.py) against fixtures produced by the REFERENCE's own classes
(oracle/gen_golden.py).  Runs everywhere (no /root/reference needed, no GPU)."""
import os

import numpy as np
import pytest
import torch

from oracle import cpr_oracle as O
from oracle.gen_golden import CPR_CASES, assigner_inputs, grad_sample_index
from pointtinybenchmark_amd import synthetic


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


@pytest.mark.parametrize('name', list(CPR_CASES))
def test_cpr_path_matches_reference_fixture(golden_dir, name):
    cfg = CPR_CASES[name]
    g = _load(golden_dir, name)
    sd = synthetic.locator_state_dict(cfg['depth'], cfg['num_classes'], cfg['start_level'], 'cpr', cfg['seed'],
                                      cfg['head_std'], num_cls_fcs=cfg.get('num_cls_fcs', 0),
                                      fc_out_channels=cfg.get('fc_out_channels', 1024))
    batch = synthetic.synthetic_batch(cfg['batch'], cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'],
                                      cfg['seed'], cfg.get('ragged', False))
    torch.set_num_threads(8)
    with torch.no_grad():
        c = O.resnet_forward(sd, batch['img'], cfg['depth'])
        feats = O.fpn_forward(sd, c, cfg['start_level'], 1)
        cls_feat, _ = O.cpr_head_forward(sd, feats)
        losses, per = O.cpr_loss(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'],
                                 cfg['stride'], cfg['radius'], cfg['num_classes'])
        ref = O.cpr_refine(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['gt_anns_id'],
                           batch['img_metas'], cfg['stride'], cfg['radius'], cfg['num_classes'])
    # same torch ops in the same order -> these are bit-identical to the reference
    assert np.array_equal(c[0][:, ::37, ::5, ::7].numpy(), g['c2_sample'])
    assert np.array_equal(c[3][:, ::101, ::3, ::3].numpy(), g['c5_sample'])
    assert np.array_equal(feats[0][:, ::17, ::5, ::7].numpy(), g['fpn_sample'])
    assert np.array_equal(cls_feat[0][:, ::13, ::3, ::5].numpy(), g['cls_feat_sample'])
    pts = torch.cat([p['pts'] for p in per])
    assert np.array_equal(pts.numpy(), g['pos_pts'][:, 0, :, :2])
    valid = torch.cat([p['valid'] for p in per])
    assert np.array_equal(valid.numpy(), g['pos_valid'][:, 0, :, 0])
    np.testing.assert_allclose(torch.cat([p['cls_logit'] for p in per]).numpy(), g['pos_cls_logit'][:, 0], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(torch.cat([p['ins_logit'] for p in per]).numpy(), g['pos_ins_logit'][:, 0], atol=2e-5, rtol=1e-5)
    nv = torch.cat([p['neg_valid'] for p in per]).numpy()
    gv = np.unpackbits(g['neg_valid'])[:nv.size].reshape(nv.shape).astype(bool)
    assert np.array_equal(nv, gv)                      # negative mask: bit-exact
    assert int(nv.sum()) == int(g['neg_valid_count'])
    for k in ('gt_loss', 'pos_loss', 'neg_loss', 'bag_acc'):
        np.testing.assert_allclose(float(losses[k]), float(g['loss_' + k]), rtol=2e-6, atol=1e-7)
    dets = torch.cat([r['dets'] for r in ref]).numpy()
    np.testing.assert_allclose(dets, g['dets'], rtol=1e-6, atol=1e-5)
    assert np.array_equal(torch.cat([r['labels'] for r in ref]).numpy(), g['det_labels'])


def _pa_inputs(seed):
    g = torch.Generator().manual_seed(100 + seed)
    pts = []
    for s in (8, 16, 32):
        n = 128 // s * 2
        ys, xs = torch.meshgrid(torch.arange(n), torch.arange(n), indexing='ij')
        pts.append(torch.stack([xs.flatten() * s, ys.flatten() * s, torch.full((n * n,), s)], -1).float())
    pts = torch.cat(pts)
    k = 3 + seed * 2
    xy = torch.rand((k, 2), generator=g) * 200 + 10
    wh = torch.rand((k, 2), generator=g) * 90 + 4
    return pts, torch.cat([xy - wh / 2, xy + wh / 2], 1), torch.randint(0, 5, (k,), generator=g)


@pytest.mark.parametrize('seed', range(6))
def test_point_assigner_matches_reference_fixture(golden_dir, seed):
    g = _load(golden_dir, 'assigners')
    pts, gtb, gl = _pa_inputs(seed)
    inds, lab = O.point_assign(pts, gtb, gl)
    assert np.array_equal(inds.numpy(), g['pa%d_gt_inds' % seed])
    assert np.array_equal(lab.numpy(), g['pa%d_labels' % seed])


@pytest.fixture
def build_host_math(golden_dir):
    """The assigner fixtures hold cost bits of the build host's torch.log / torch.cdist(p=2), which differ in the last bit
    between CPUs (oracle/host_math.py): the oracle evaluates its costs with those recorded primitives, so the bit-exact
    comparisons below hold on every host."""
    from oracle import host_math
    with host_math.replay(os.path.join(golden_dir, 'build_host_math.npz')):
        yield


@pytest.mark.parametrize('case', range(5))
def test_hungarian_v2_matches_reference_fixture(golden_dir, case, build_host_math):
    g = _load(golden_dir, 'assigners')
    n_side, G, C, k = [int(v) for v in g['ha%d_cfg' % case]]
    pred, logits, gt, labels, shp = assigner_inputs(200 + case, n_side, 4, G, C)
    inds, lab, _ = O.hungarian_assign_v2(pred, logits, gt, labels, shp, topk_k=k)
    assert np.array_equal(inds.numpy(), g['ha%d_gt_inds' % case])
    assert np.array_equal(lab.numpy(), g['ha%d_labels' % case])
    assert int((inds > 0).sum()) == min(k, (n_side * n_side) // G) * G


@pytest.mark.parametrize('name', ['cpr_r18_c3_128', 'cpr_r50_c1_160_spread', 'cpr_r50_c80_s8_r8'])
def test_oracle_autograd_matches_reference_autograd(golden_dir, name):
    """Pins the ORACLE's backward: torch autograd over oracle/cpr_oracle.py against loss.backward() through the reference's
    own modules (fixtures from oracle.gen_golden.run_reference_cpr_grads): per-tensor norm, sum and strided samples."""
    from oracle.gen_golden import CPR_CASES, grad_sample_index
    cfg = CPR_CASES[name]
    gold = _load(golden_dir, 'cpr_grads_' + name)
    sd = synthetic.locator_state_dict(cfg['depth'], cfg['num_classes'], cfg['start_level'], 'cpr', cfg['seed'],
                                      cfg['head_std'], num_cls_fcs=cfg.get('num_cls_fcs', 0),
                                      fc_out_channels=cfg.get('fc_out_channels', 1024))
    keys = [k[len('norm:'):] for k in gold.files if k.startswith('norm:')]
    assert len(keys) == int(gold['num_tensors'])
    sd = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        sd[k].requires_grad_(True)
    batch = synthetic.synthetic_batch(cfg['batch'], cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'],
                                      cfg['seed'], cfg.get('ragged', False))
    losses, _, _ = O.locator_forward_train(sd, batch, cfg['depth'], cfg['start_level'], cfg['stride'], cfg['radius'],
                                           cfg['num_classes'])
    total = sum(v for k, v in losses.items() if 'loss' in k)
    assert abs(float(total.detach()) - float(gold['total_loss'])) <= 1e-4 * max(1.0, abs(float(gold['total_loss'])))
    total.backward()
    gmax = max(float(gold['norm:' + k]) for k in keys)
    for k in keys:
        g = sd[k].grad.detach().double().flatten()
        ref_n = float(gold['norm:' + k])
        assert abs(float(g.norm()) - ref_n) <= 1e-3 * ref_n + 1e-7 * gmax, (k, float(g.norm()), ref_n)
        smp = g[torch.from_numpy(grad_sample_index(g.numel()))].numpy()
        ref = gold['sample:' + k].astype(np.float64)
        assert np.abs(smp - ref).max() <= 1e-3 * max(np.abs(ref).max(), 1e-6 * gmax), k


def _refine_names():
    from oracle.gen_golden_r2 import REFINE_CASES
    return list(REFINE_CASES)


@pytest.mark.parametrize('name', _refine_names())
def test_oracle_refine_internals_match_reference(golden_dir, name):
    """PointRefiner internals of the restatement (chosen-point masks, not_refine, refined points, scores) against what the
    reference's own refine_single returned (tests/golden/refine.npz, oracle/gen_golden_r2.py): masks bit-exact.
    ``cpr_r50_c80_s8_r8_live`` is the C = 80 / K = 289 case whose merge branch is not empty (576 chosen points)."""
    from oracle.gen_golden_r2 import REFINE_CASES
    cfg = REFINE_CASES[name]
    g = _load(golden_dir, 'refine')
    p = name + ':'
    sd = synthetic.locator_state_dict(cfg['depth'], cfg['num_classes'], cfg['start_level'], 'cpr', cfg['seed'],
                                      cfg['head_std'], num_cls_fcs=cfg.get('num_cls_fcs', 0),
                                      fc_out_channels=cfg.get('fc_out_channels', 1024))
    batch = synthetic.synthetic_batch(cfg['batch'], cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'],
                                      cfg['seed'], cfg.get('ragged', False))
    torch.set_num_threads(8)
    with torch.no_grad():
        feats = O.fpn_forward(sd, O.resnet_forward(sd, batch['img'], cfg['depth']), cfg['start_level'], 1)
        cls_feat, _ = O.cpr_head_forward(sd, feats)
        ref = O.cpr_refine(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['gt_anns_id'],
                           batch['img_metas'], cfg['stride'], cfg['radius'], cfg['num_classes'])
    mv = torch.cat([r['merge_valid'] for r in ref]).numpy()
    chosen = np.unpackbits(g[p + 'chosen'])[:mv.size].reshape(mv.shape).astype(bool)
    assert np.array_equal(mv, chosen)
    assert np.array_equal(torch.cat([r['not_refine'] for r in ref]).numpy(), g[p + 'not_refine'])
    np.testing.assert_allclose(torch.cat([r['refine_pts'] for r in ref]).numpy(), g[p + 'refine_pts'], rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(torch.cat([r['scores'] for r in ref]).numpy(), g[p + 'scores'], rtol=1e-6, atol=1e-7)


def test_correctly_rounded_log_cost_vs_reference_cost_fixture(golden_dir):
    """The reference's own fp32 cost matrices (tests/golden/assigner_costs.npz, computed by its FocalLossCost/DisCostV2 on
    the build host) against the restated formula with a CORRECTLY ROUNDED log -- what the HIP cost kernel computes and what
    is host independent: at most a handful of entries 1 ulp apart (the build host's MKL log), indices identical."""
    g, gc = _load(golden_dir, 'assigners'), _load(golden_dir, 'assigner_costs')
    total_diff = 0
    for case in range(5):
        n_side, G, C, k = [int(v) for v in g['ha%d_cfg' % case]]
        pred, logits, gt, labels, shp = assigner_inputs(200 + case, n_side, 4, G, C)
        inds, _, cost = O.hungarian_assign_v2(pred, logits, gt, labels, shp, topk_k=k, log_mode='cr')
        ref = gc['ha%d_cost' % case]
        ulp = np.abs(cost.numpy().view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1
        total_diff += int((ulp > 0).sum())
        assert np.array_equal(inds.numpy(), g['ha%d_gt_inds' % case])
    assert total_diff <= 8, total_diff


def _option_names():
    from oracle.gen_golden_r2 import OPTION_CASES, OPTION_CASES_R3
    return list(OPTION_CASES) + list(OPTION_CASES_R3)


@pytest.mark.parametrize('name', _option_names())
def test_option_oracle_matches_reference_fixture(golden_dir, name):
    """oracle/cpr_options_oracle.py (num_refine > 1 bag policies, grid-circle bags, softmax / normed_sigmoid, binary_ins,
    AllPosLoss) against what the reference's own classes computed (tests/golden/cpr_options.npz): bag points, validity,
    negative masks and the refiner's chosen-point masks bit for bit, losses to 3e-6."""
    from oracle import cpr_options_oracle as OO
    from oracle.gen_golden_r2 import OPTION_CASES, case_inputs, option_cfg
    cfg = option_cfg(name)
    g = _load(golden_dir, 'cpr_options' if name in OPTION_CASES else 'cpr_options_r3')
    p = name + ':'
    if (p + 'reference_error') in g.files:
        # AnchorPtFeatGenerator(scale_factor != 1): the reference passes scale_factor as F.interpolate's `size` (cpr_head.py:229)
        assert 'Error' in str(g[p + 'reference_error'])
        return
    sd, batch = case_inputs(cfg)
    torch.set_num_threads(8)
    with torch.no_grad():
        feats = O.fpn_forward(sd, O.resnet_forward(sd, batch['img'], cfg['depth']), cfg['start_level'], 1)
        cls_feat, _ = O.cpr_head_forward(sd, feats)
        ins_feat = OO.ins_tower_forward(sd, feats)[0] if cfg.get('ins_tower') else None
        losses, per = OO.cpr_loss(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'], cfg,
                                  ins_feat=ins_feat)
    pts = torch.cat([q['pts'] for q in per]).numpy()
    assert np.array_equal(pts, g[p + 'pos_pts'])
    assert np.array_equal(torch.cat([q['valid'] for q in per]).numpy(), g[p + 'pos_valid'])
    nv = torch.cat([q['neg_valid'] for q in per]).numpy()
    gv = np.unpackbits(g[p + 'neg_valid'])[:nv.size].reshape(nv.shape).astype(bool)
    assert np.array_equal(nv, gv) and int(nv.sum()) == int(g[p + 'neg_valid_count'])
    np.testing.assert_allclose(torch.cat([q['cls_logit'] for q in per]).numpy(), g[p + 'pos_cls_logit'], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(torch.cat([q['ins_logit'] for q in per]).numpy(), g[p + 'pos_ins_logit'], atol=2e-5, rtol=1e-5)
    for k, v in losses.items():
        np.testing.assert_allclose(float(v), float(g[p + 'loss_' + k]), rtol=3e-6, atol=1e-7)
    assert set('loss_' + k for k in losses) == set(k[len(p):] for k in g.files if k.startswith(p + 'loss_'))
    if (p + 'refine_asserts_in_reference') in g.files:
        with pytest.raises(AssertionError):
            OO.cpr_refine(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'], cfg)
        return
    with torch.no_grad():
        ref = OO.cpr_refine(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'], cfg, ins_feat=ins_feat)
    chosen = torch.cat([r['chosen'] for r in ref]).numpy()
    want = np.unpackbits(g[p + 'chosen'])[:chosen.size].reshape(chosen.shape).astype(bool)
    assert np.array_equal(chosen, want)
    assert np.array_equal(torch.cat([r['not_refine'] for r in ref]).numpy(), g[p + 'not_refine'])
    np.testing.assert_allclose(torch.cat([r['refine_pts'] for r in ref]).numpy(), g[p + 'refine_pts'], rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(torch.cat([r['scores'] for r in ref]).numpy(), g[p + 'scores'], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('name', ['r2_independent', 'ins_tower', 'ins_tower_fc', 'ins_tower_fc_boundary', 'fc2_shared', 'softmax',
                                  'normed_sigmoid_p1', 'normed_sigmoid_p2', 'binary_ins', 'allpos', 'r2_merge_gt', 'r3_only_refine', 'bg_cls',
                                  'no_mil_loss', 'grid_circles', 'grid_circles_r2', 'align_corners', 'align_corners_grid',
                                  'grid_circles_fc', 'no_neg', 'combo_fc_softmax_merge', 'combo_tower_binary_normed'])
def test_option_oracle_autograd_matches_reference_autograd(golden_dir, name):
    """Pins the options oracle's BACKWARD (torch autograd over oracle/cpr_options_oracle.py) to loss.backward() through the
    reference's own modules for the options that gained a hand-written backward in round 5 (tests/golden/cpr_option_grads.npz,
    oracle/gen_golden_r5.py): per-tensor norm and strided samples, 1e-3."""
    from oracle import cpr_options_oracle as OO
    from oracle.gen_golden import grad_sample_index
    from oracle.gen_golden_r2 import case_inputs
    from oracle.gen_golden_r5 import grad_option_cfg
    cfg = grad_option_cfg(name)
    g = _load(golden_dir, 'cpr_option_grads')
    p = name + ':'
    sd, batch = case_inputs(cfg)
    keys = [k[len(p + 'norm:'):] for k in g.files if k.startswith(p + 'norm:')]
    assert len(keys) == int(g[p + 'num_tensors'])
    sd = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        sd[k].requires_grad_(True)
    torch.set_num_threads(8)
    feats = O.fpn_forward(sd, O.resnet_forward(sd, batch['img'], cfg['depth']), cfg['start_level'], 1)
    cls_feat, _ = O.cpr_head_forward(sd, feats)
    ins_feat = OO.ins_tower_forward(sd, feats)[0] if cfg.get('ins_tower') else None
    losses, _ = OO.cpr_loss(sd, cls_feat[0], batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'], cfg, ins_feat=ins_feat)
    total = sum(v for k, v in losses.items() if 'loss' in k)
    assert abs(float(total.detach()) - float(g[p + 'total_loss'])) <= 1e-4 * max(1.0, abs(float(g[p + 'total_loss'])))
    total.backward()
    gmax = max(float(g[p + 'norm:' + k]) for k in keys)
    for k in keys:
        ref_n = float(g[p + 'norm:' + k])
        if sd[k].grad is None:
            # AllPosLoss: the reference computes the instance logits and weights them out, so autograd hands ins_out an exactly
            # zero gradient; the restatement never touches ins_out there
            assert ref_n == 0.0, k
            continue
        gr = sd[k].grad.detach().double().flatten()
        assert abs(float(gr.norm()) - ref_n) <= 1e-3 * ref_n + 1e-7 * gmax, (k, float(gr.norm()), ref_n)
        smp = gr[torch.from_numpy(grad_sample_index(gr.numel()))].numpy()
        ref = g[p + 'sample:' + k].astype(np.float64)
        assert np.abs(smp - ref).max() <= 1e-3 * max(np.abs(ref).max(), 1e-6 * gmax), k


@pytest.mark.parametrize('ci', [0, 1])
def test_oracle_p2p_loss_matches_reference_fixture(golden_dir, ci):
    """oracle.cpr_oracle.p2p_loss (round 4: the restatement bench.py times and gates the P2PNet line with) on the reference's OWN
    tower outputs (tests/golden/p2p.npz, produced by the reference's P2PHead): the Hungarian targets must equal the reference's
    bit for bit and the first image's focal / SmoothL1 losses agree to 2e-6."""
    g = np.load(os.path.join(golden_dir, 'p2p.npz'))
    C, hw, G, std1000 = [int(v) for v in g['p2p%d_cfg' % ci]]
    from pointtinybenchmark_amd import synthetic
    batch = synthetic.synthetic_batch(2, hw * 4, hw * 4, G, C, seed=300 + ci, ragged=True)
    cls_out, pts_out = torch.from_numpy(g['p2p%d_cls_out' % ci]), torch.from_numpy(g['p2p%d_pts_out' % ci])
    with torch.no_grad():
        losses, inds = O.p2p_loss(cls_out, pts_out, batch['gt_bboxes'], batch['gt_labels'], (hw * 4, hw * 4, 3))
    ref_labels = g['p2p%d_target_labels' % ci]
    for b in range(2):
        lab = torch.full((inds[b].shape[0],), C, dtype=torch.long)
        pos = inds[b] > 0
        lab[pos] = batch['gt_labels'][b][inds[b][pos] - 1]
        assert np.array_equal(lab.numpy().astype(np.int32), ref_labels[b]), 'image %d: assignment targets differ' % b
    for key, mine in (('loss_cls', losses['loss_cls'][0]), ('loss_pts', losses['loss_pts'][0])):
        ref = float(g['p2p%d_%s' % (ci, key)])
        assert abs(float(mine) - ref) <= 2e-6 * max(1.0, abs(ref)), (key, float(mine), ref)


# ------------------------------------------------------------------------------------------------ round 6: P2P / assigner options
def _r6():
    from oracle import gen_golden_r6 as R6
    from oracle import p2p_options_oracle as PO
    return R6, PO


@pytest.mark.parametrize('name', ['bce_mse', 'softmax_sl1', 'focal_l1', 'defaults_k4', 'two_levels'])
def test_p2p_option_oracle_matches_reference_fixture(golden_dir, name):
    """oracle/p2p_options_oracle.py (losses, general match costs, multi-level points, the no-NMS branch) on the head outputs the reference
    produced (tests/golden/p2p_options.npz): assignment labels identical, losses to 1e-5, and -- on the cases that carry them -- the oracle's
    autograd against the reference's loss.backward() on the recorded outputs (d loss / d cls_out, pts_out through the head is the product's
    job; here the loss functions' own gradients are pinned through the output-conv parameters' sampled gradients at 1e-4)."""
    R6, PO = _r6()
    g = np.load(os.path.join(golden_dir, 'p2p_options.npz'))
    cfg = R6.HEAD_CASES[name]
    _, batch = R6.head_inputs(cfg)
    L = len(cfg['strides'])
    cls_outs = [torch.from_numpy(g['%s:cls_out%d' % (name, l)]) for l in range(L)]
    pts_outs = [torch.from_numpy(g['%s:pts_out%d' % (name, l)]) for l in range(L)]
    shape = batch['img_metas'][0]['img_shape']
    losses, inds = PO.p2p_loss(cls_outs, pts_outs, batch['gt_bboxes'], batch['gt_labels'], shape, cfg['strides'], cfg['C'], cfg['loss_cls'],
                               cfg['loss_reg'], cfg['assigner'], point_anchor=cfg['anchors'])
    lab = []
    for b, gi in enumerate(inds):
        l = torch.full(gi.shape, cfg['C'], dtype=torch.long)
        l[gi > 0] = batch['gt_labels'][b][gi[gi > 0] - 1]
        lab.append(l)
    assert np.array_equal(torch.stack(lab).numpy().astype(np.int32), g[name + ':target_labels'])
    for key in ('loss_cls', 'loss_pts'):
        np.testing.assert_allclose(np.array([float(v) for v in losses[key]]), g['%s:%s' % (name, key)], rtol=2e-5, atol=1e-8, err_msg=key)
    use_sigmoid = cfg['loss_cls'].get('use_sigmoid', False)
    nco = cfg['C'] if use_sigmoid else cfg['C'] + 1
    pred3, cls = PO.get_pred_points(cls_outs, pts_outs, cfg['strides'], cfg['anchors'], 1.0, nco)
    for b in range(2):
        d, l = PO.p2p_get_bboxes_single(cls[b], pred3[b][:, :2], shape, L, use_sigmoid, nco, R6.TEST_CFG['nms_pre'], R6.TEST_CFG['score_thr'],
                                        0.2, R6.TEST_CFG['max_per_img'])
        rd = g['%s:det%d' % (name, b)]
        assert np.array_equal(l.numpy(), g['%s:detlabel%d' % (name, b)])
        np.testing.assert_allclose(torch.cat([d[:, :2] - 8, d[:, :2] + 8, d[:, 2:]], -1).numpy(), rd, rtol=0, atol=1e-4)
    if not use_sigmoid:
        d, l = PO.p2p_get_bboxes_single(cls[0], pred3[0][:, :2], shape, L, False, nco, R6.TEST_CFG['nms_pre'], R6.TEST_CFG['score_thr'], 0.2,
                                        R6.TEST_CFG['max_per_img'], with_nms=False)
        assert np.array_equal(l.numpy(), g[name + ':nonms_label'])
        np.testing.assert_allclose(d.numpy(), g[name + ':nonms_det'], rtol=0, atol=1e-5)


@pytest.mark.parametrize('name', ['bce_mse', 'softmax_sl1', 'focal_l1'])
def test_p2p_option_oracle_autograd_matches_reference_autograd(golden_dir, name):
    """The whole head (oracle towers + the option losses) differentiated by torch against the reference's loss.backward() (every head
    parameter + the input feature map, norm and strided sample)."""
    from oracle import cpr_oracle as O
    R6, PO = _r6()
    g = np.load(os.path.join(golden_dir, 'p2p_options.npz'))
    cfg = R6.HEAD_CASES[name]
    feats, batch = R6.head_inputs(cfg)
    sd = {k: v.clone().requires_grad_(True) for k, v in R6.head_state_dict(cfg).items()}
    feat = feats[0].clone().requires_grad_(True)
    cls_outs, pts_outs = O.p2p_head_forward(sd, (feat,))
    losses, _ = PO.p2p_loss(cls_outs, pts_outs, batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'][0]['img_shape'], cfg['strides'], cfg['C'],
                            cfg['loss_cls'], cfg['loss_reg'], cfg['assigner'], point_anchor=cfg['anchors'])
    total = sum(sum(v) for v in losses.values())
    total.backward()
    assert abs(float(total.detach()) - float(g[name + ":total_loss"])) <= 1e-5 * max(1.0, abs(float(g[name + ':total_loss'])))
    got = dict(sd)
    got['feat'] = feat
    keys = [k.split(':', 2)[2] for k in g.files if k.startswith(name + ':norm:')]
    gmax = max(float(g['%s:norm:%s' % (name, k)]) for k in keys)
    for k in keys:
        gr = got[k].grad.detach().double().flatten()
        ref = g['%s:sample:%s' % (name, k)].astype(np.float64)
        smp = gr[torch.from_numpy(grad_sample_index(gr.numel()))].numpy()
        assert np.linalg.norm(smp - ref) <= 1e-4 * max(np.linalg.norm(ref), 1e-4 * gmax), k
        assert abs(float(gr.norm()) - float(g['%s:norm:%s' % (name, k)])) <= 1e-4 * float(g['%s:norm:%s' % (name, k)]) + 1e-7 * gmax, k


@pytest.mark.parametrize('ci', range(5))
def test_general_match_cost_oracle_matches_reference(golden_dir, ci, build_host_math):
    from oracle.gen_golden import assigner_inputs
    R6, PO = _r6()
    g = np.load(os.path.join(golden_dir, 'p2p_options.npz'))
    seed, n_side, G, C, cc, rc, k = R6.COST_CASES[ci]
    pred, logits, gt, labels, shape = assigner_inputs(seed, n_side, 4, G, C)
    cc = cc if isinstance(cc, list) else [cc]
    rc = rc if isinstance(rc, list) else [rc]
    inds, lab, cost = PO.hungarian_assign_v2(cc, rc, k, pred, logits, gt, labels, shape)
    assert np.array_equal(cost.numpy().astype(np.float32), g['cost%d:cost' % ci]), 'the restated cost must carry the reference bits (build-host log / cdist)'
    assert np.array_equal(inds.numpy().astype(np.int32), g['cost%d:gt_inds' % ci])
    assert np.array_equal(lab.numpy().astype(np.int32), g['cost%d:labels' % ci])


def test_hungarian_v1_oracle_matches_reference(golden_dir):
    R6, PO = _r6()
    g = np.load(os.path.join(golden_dir, 'p2p_options.npz'))
    for vi, seed in enumerate((41, 42, 43)):
        bp, lg, gts, lbl, meta = R6.v1_inputs(seed, C=4 if vi < 2 else 1)
        kw = {} if vi != 1 else dict(reg_w=5.0, iou_w=2.0, iou_mode='iou')
        inds, lab = PO.hungarian_assign_v1(bp, lg, gts, lbl, meta['img_shape'], **kw)
        assert np.array_equal(inds.numpy().astype(np.int32), g['v1_%d:gt_inds' % vi]), vi
        assert np.array_equal(lab.numpy().astype(np.int32), g['v1_%d:labels' % vi]), vi
