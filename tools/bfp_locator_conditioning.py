"""Which data seeds the whole-locator gradient test of the BFP neck may use (CPU, needs no reference tree):
  python tools/bfp_locator_conditioning.py [--seeds 4,5,6,7,8 | --seeds 1-400 --exposure-only]
tests/test_gpu_bfp.py::test_locator_gradients_vs_fp64_autograd holds the HIP step to fp64 autograd of the oracle network at 2e-3 per
tensor.  The rule is tools/pafpn_locator_conditioning.py's (see there), with tests/bfp_ref.bfp_forward behind the oracle's FPN / PAFPN:
the oracle network run in fp32 on the CPU against its fp64 run, on the fp64 run's assignment, must keep every tensor within a quarter of
the bar, and the fp64 run's kink exposure -- what ONE head-tower ReLU input within fp32 rounding of zero moves when it flips -- must stay
below the bar.  BFP adds kinks of its own, the max-pool selections and the refine layer's ReLU; a selection that flips between two nearly
equal values only moves one cell's gradient to a neighbour carrying nearly the same value, and the fp32 run crosses the same kinks, so
they are covered by the first condition."""
import argparse
import os
import sys

import torch

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (ROOT, TOOLS):
    if p not in sys.path:
        sys.path.insert(0, p)
from bench import p2p_model_cfg  # noqa: E402
from fpn_extra_locator_conditioning import ADMIT, FROZEN, GRID4  # noqa: E402
from oracle import cpr_oracle as O  # noqa: E402
from oracle import p2p_options_oracle as PO  # noqa: E402
from pafpn_locator_conditioning import ADMIT_EXPOSURE, _TowerRelus  # noqa: E402
from pointtinybenchmark_amd import synthetic  # noqa: E402
from tests import bfp_ref as BR  # noqa: E402
from tests import pafpn_ref as PR  # noqa: E402
from tests.fpn_extra_ref import fpn_forward  # noqa: E402

#            inner neck, start_level, num_outs, add_extra_convs, strides, refine_level, refine_type
LOCATORS = {'fpn_conv': ('FPN', 0, 4, False, [4, 8, 16, 32], 1, 'conv'),
            'pafpn_none': ('PAFPN', 1, 5, 'on_input', [8, 16, 32, 64, 128], 2, None)}


def locator_state_dict(kind, wseed=3, C=2):
    inner, start, num_outs, extra, _, _, refine = LOCATORS[kind]
    sd = synthetic.locator_state_dict(18, C, start, 'p2p', wseed, head_std=0.05, num_points=4)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    make = synthetic.pafpn_state_dict if inner == 'PAFPN' else synthetic.fpn_state_dict
    sd.update(make(synthetic.backbone_out_channels(18), 256, start, num_outs, wseed + 1, prefix='neck.0.', add_extra_convs=extra))
    sd.update(synthetic.bfp_state_dict(256, refine, wseed + 2, prefix='neck.1.'))
    return sd


def neck_forward(kind, sd, feats):
    inner, start, num_outs, extra, _, r, refine = LOCATORS[kind]
    mid = (PR.pafpn_forward if inner == 'PAFPN' else fpn_forward)(sd, list(feats), num_outs, start, extra, prefix='neck.0.')
    return BR.bfp_forward(sd, list(mid), r, refine, prefix='neck.1.')


def run(kind, seed, dtype, gt_inds=None, hw=(128, 160), C=2):
    strides = LOCATORS[kind][4]
    sd = locator_state_dict(kind, C=C)
    batch = synthetic.synthetic_batch(2, hw[0], hw[1], 6, C, seed=seed)
    sdd = {k: (v.to(dtype).requires_grad_(not k.startswith(FROZEN) and 'running_' not in k) if v.is_floating_point() else v)
           for k, v in sd.items()}
    feats = O.resnet_forward(sdd, batch['img'].to(dtype), depth=18)
    co, po = O.p2p_head_forward(sdd, neck_forward(kind, sdd, feats))
    pred, cls = PO.get_pred_points(co, po, strides, GRID4, 1, C)
    ctr = [(b[:, :2] + b[:, 2:]) / 2 for b in batch['gt_bboxes']]
    if gt_inds is None:
        a = p2p_model_cfg(18, C)['train_cfg']['assigner']
        gt_inds = torch.stack([PO.hungarian_assign_v2([a['cls_costs']], [a['reg_costs']], a['topk_k'], pred[b, :, :2].detach(),
                                                      cls[b].detach(), ctr[b].to(dtype), batch['gt_labels'][b], hw + (3,))[0]
                               for b in range(2)])
    counts = [len(c) for c in ctr]
    rc, rp = PO.p2p_loss_from_assignment(cls, pred, gt_inds, torch.cat(ctr).to(dtype), torch.cat(list(batch['gt_labels'])),
                                         torch.tensor([0] + counts[:-1]).cumsum(0), 0.25, 2.0, 1.0 / 9.0, 1.0, 1.0, 1, 1.0, 0.5, 0, 0)
    (rc.sum() + rp.sum()).backward()
    return {k: v.grad for k, v in sdd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}, gt_inds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', default='4,5,6,7,8', help='a list 4,5,6 or a range 1-400')
    ap.add_argument('--kinds', default=','.join(LOCATORS))
    ap.add_argument('--exposure-only', action='store_true', help='the fp64 run alone: kink exposure per seed')
    args = ap.parse_args()
    torch.set_num_threads(8)
    lo, _, hi = args.seeds.partition('-')
    seeds = list(range(int(lo), int(hi) + 1)) if hi else [int(s) for s in args.seeds.split(',')]
    for kind in args.kinds.split(','):
        for seed in seeds:
            with _TowerRelus() as relus:
                g64, inds = run(kind, seed, torch.float64)
            kink = relus.exposure()
            if args.exposure_only:
                print('%-12s seed %d: kink exposure %.2e' % (kind, seed, kink), flush=True)
                continue
            g32, _ = run(kind, seed, torch.float32, inds)
            gmax = max(float(v.norm()) for v in g64.values())
            worst, name = max((float((g32[k].double() - g64[k]).norm()) / max(float(g64[k].norm()), 1e-5 * gmax), k) for k in g64)
            print('%-12s seed %d: %d positives, worst tensor fp32 vs fp64 %.2e (%s), kink exposure %.2e -> %s' % (
                kind, seed, int((inds > 0).sum()), worst, name, kink, 'admitted' if worst <= ADMIT and kink <= ADMIT_EXPOSURE else 'refused'), flush=True)


if __name__ == '__main__':
    main()
