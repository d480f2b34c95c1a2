"""Which data seeds the whole-locator gradient test of the PAFPN neck may use (CPU, needs no reference tree):
  python tools/pafpn_locator_conditioning.py [--seeds 4,5,6,7,8 | --seeds 1-400 --exposure-only]
tests/test_gpu_pafpn.py::test_locator_gradients_vs_fp64_autograd holds the HIP step to fp64 autograd of the oracle network at 2e-3
per tensor.  The rule is tools/fpn_extra_locator_conditioning.py's (see there): the same oracle network -- here with
tests/pafpn_ref.pafpn_forward as its neck -- run in fp32 on the CPU against its fp64 run, on the fp64 run's assignment, must keep
every tensor within a quarter of the bar.
One more condition, also from the reference alone.  Whether an fp32 evaluation lands on the wrong side of a ReLU that sits within fp32
rounding of zero is a matter of ITS rounding, not of the network: the CPU's fp32 run may pass where another correct fp32 evaluation
flips it (pa4, seed 7: a reg_convs.2 input of 5.96e-7 carrying 4.7e-3 of that layer's GroupNorm-bias gradient; the CPU fp32 run stays
at 2.9e-5, the HIP step moves by 4.7e-3 from reg_convs.2 down; pa_on_input, seed 17: a cls_convs.3 input of 6.2e-6).  So the fp64
run also reports its kink exposure: over the head towers' ReLU inputs with |y| < NEAR, the largest |dL/dReLU(y)| relative to the norm
of that layer's GroupNorm-bias gradient (summed over the levels, as the parameter's is) -- what ONE flipped element moves.  NEAR is
the reference's own fp32 error on those inputs: the CPU fp32 run against the fp64 run
measures a median of 5.5e-7, a 99th percentile of 2.9e-6 and a maximum of 8.4e-6 .. 9.6e-6 (pa4 seeds 7 / 40, pa_on_input seed 4).
These maps are dense in such inputs (a third of the elements of a tower map carry more than 1e-3 of their layer's bias gradient), so no
seed of the 400 / 240 scanned keeps the exposure within a quarter of the bar; a seed is admitted when one flipped element alone cannot
exceed the bar (exposure <= 2e-3), and the test takes the admitted seed with the least exposure of the scan (--exposure-only: the
fp64 run alone): pa4 119 (1.4e-3; then 131, 84), pa_on_input 74 (9.2e-4; then 116)."""
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
from pointtinybenchmark_amd import synthetic  # noqa: E402
from tests import pafpn_ref as PR  # noqa: E402

NEAR, ADMIT_EXPOSURE = 1e-5, 2e-3
LOCATORS = {'pa4': (0, 4, False, [4, 8, 16, 32]), 'pa_on_input': (1, 5, 'on_input', [8, 16, 32, 64, 128])}


class _TowerRelus:
    """Records (pre-activation, activated) of every conv + GN + ReLU layer the oracle head runs."""

    def __enter__(self):
        self.held, self._orig = [], O._conv_gn

        def conv_gn(x, sd, prefix, pad, relu, *a, **k):
            y = self._orig(x, sd, prefix, pad, False, *a, **k)
            if not relu:
                return y
            z = torch.relu(y)
            if z.requires_grad:
                z.retain_grad()
                self.held.append((prefix, y.detach(), z))
            return z
        O._conv_gn = conv_gn
        return self

    def __exit__(self, *exc):
        O._conv_gn = self._orig

    def exposure(self):
        bias = {}       # layer -> its GroupNorm-bias gradient, summed over the levels
        for prefix, y, z in self.held:
            if z.grad is not None:
                bias[prefix] = bias.get(prefix, 0) + (z.grad * (y > 0)).sum((0, 2, 3))
        worst = 0.0
        for prefix, y, z in self.held:
            near = y.abs() < NEAR
            if z.grad is not None and bool(near.any()):
                worst = max(worst, float((z.grad.abs() * near).max()) / max(float(bias[prefix].norm()), 1e-30))
        return worst


def run(kind, seed, dtype, gt_inds=None, wseed=3, hw=(128, 160), C=2):
    start, num_outs, extra, strides = LOCATORS[kind]
    sd = synthetic.locator_state_dict(18, C, start, 'p2p', wseed, head_std=0.05, num_points=4)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.pafpn_state_dict(synthetic.backbone_out_channels(18), 256, start, num_outs, wseed + 1, add_extra_convs=extra))
    batch = synthetic.synthetic_batch(2, hw[0], hw[1], 6, C, seed=seed)
    sdd = {k: (v.to(dtype).requires_grad_(not k.startswith(FROZEN) and 'running_' not in k) if v.is_floating_point() else v)
           for k, v in sd.items()}
    feats = O.resnet_forward(sdd, batch['img'].to(dtype), depth=18)
    outs = PR.pafpn_forward(sdd, list(feats), num_outs, start, extra, prefix='neck.')
    co, po = O.p2p_head_forward(sdd, outs)
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
    ap.add_argument('--exposure-only', action='store_true', help='the fp64 run alone: kink exposure per seed')
    args = ap.parse_args()
    torch.set_num_threads(8)
    lo, _, hi = args.seeds.partition('-')
    seeds = list(range(int(lo), int(hi) + 1)) if hi else [int(s) for s in args.seeds.split(',')]
    for kind in LOCATORS:
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
