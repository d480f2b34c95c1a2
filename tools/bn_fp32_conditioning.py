"""How far the backbone gradient of a ResNet with training-mode BatchNorm (norm_eval=False) can be pinned by ANY fp32
implementation: the CPU oracle (oracle/cpr_oracle.py, its BatchNorm switched to batch statistics for the stages above
frozen_stages) run in fp32 and in fp64 on the same weights, image and fixed upstream gradients, per-tensor rel-L2 of the fp32
gradients against the fp64 ones.  With batch statistics a ReLU whose pre-activation lies within rounding of 0 moves the backward of
its whole BatchNorm channel, so the fp32 / fp64 gap is set by the network, not by the kernels.  CPU only; prints one line per case."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpr_oracle as O          # noqa: E402
from pointtinybenchmark_amd import synthetic  # noqa: E402


def batch_stats_bn(frozen_stages, orig):
    def bn(x, sd, p, eps=1e-5):
        q = p[len('backbone.'):]
        stage = 0 if q.startswith('bn1') else int(q.split('.')[0][len('layer'):])
        if stage <= frozen_stages:
            return orig(x, sd, p, eps)
        return F.batch_norm(x, None, None, sd[p + '.weight'], sd[p + '.bias'], True, 0.1, eps)
    return bn


def case(depth, frozen_stages, hw=(160, 192), seed=3):
    orig = O._bn_eval
    O._bn_eval = batch_stats_bn(frozen_stages, orig)
    try:
        sd = {k: v for k, v in synthetic.locator_state_dict(depth, 1, 0, 'cpr', seed, 0.3).items() if k.startswith('backbone.')}
        g = torch.Generator().manual_seed(seed)
        img = torch.randn((2, 3) + tuple(hw), generator=g)
        trained = [k for k, v in sd.items() if v.is_floating_point() and 'running' not in k and
                   any(k.startswith('backbone.layer%d.' % i) for i in range(frozen_stages + 1, 5))]
        grads, ups = {}, None
        for dt in (torch.float32, torch.float64):
            osd = {k: v.detach().to(dt).clone() if v.is_floating_point() else v for k, v in sd.items()}
            for k in trained:
                osd[k].requires_grad_(True)
            outs = O.resnet_forward(osd, img.to(dt), depth)
            if ups is None:
                ups = [torch.randn(tuple(o.shape), generator=g, dtype=torch.float64) for o in outs]
            sum((outs[i] * ups[i].to(dt)).sum() for i in range(max(frozen_stages, 0), len(outs))).backward()
            grads[dt] = {k: osd[k].grad.double() for k in trained}
    finally:
        O._bn_eval = orig
    errs = sorted(float((grads[torch.float32][k] - grads[torch.float64][k]).norm() / grads[torch.float64][k].norm()) for k in trained)
    return dict(depth=depth, frozen_stages=frozen_stages, hw=hw, tensors=len(errs), median=errs[len(errs) // 2], worst=errs[-1])


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    for depth, fr in ((18, 1), (18, 2), (50, 1), (50, 2)):
        r = case(depth, fr)
        print('R%d frozen_stages=%d %dx%d B=2: fp32 oracle vs fp64 oracle, backbone gradients rel-L2 over %d tensors: median %.2e, worst %.2e'
              % (depth, fr, r['hw'][0], r['hw'][1], r['tensors'], r['median'], r['worst']), flush=True)


if __name__ == '__main__':
    main()
