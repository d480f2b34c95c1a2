"""What a MobileNetV2 backbone costs next to R50, and what its depthwise kernels reach, all lines in the same run:

  locators   BasicLocator(backbone, FPN, CPRHead) at 640^2, B = 64: forward + loss img/s and full training-step img/s with R50
             (frozen_stages=1) and MobileNetV2 (out_indices (1, 2, 4, 7), neck.in_channels [24, 32, 96, 1280]) twice: frozen_stages=1,
             the like-for-like line (stem and layer1 frozen as R50's stem and layer1 are), and frozen_stages=-1 (everything trains).
  layers     the depthwise 3x3 of the first block of each of the seven layers (mid channels, input map, stride) at 640 x 640, B = 64, at the pitch
             the backbone keeps them at -- forward (in_clamp6, scale / bias / relu6), data gradient (mask6 + column sums), weight
             gradient (in_clamp6): time per launch and achieved TB/s against the ALGORITHMIC bytes -- forward and data gradient: read
             the input map once, write the output once (+ the mask map for the data gradient); weight gradient: read dy and x once.
  gn_apply   the streaming reference of this repository (one read, one write per element) on a map of each layer's input size, in the
             same loop, so the depthwise rates stand next to what a pure streaming kernel reaches on the same box in the same run.

No rate is fixed in advance: the result records what was measured.  Device-event medians.  Prints one JSON object (--out FILE also
writes it: profiles/mobilenet_v2_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.resnext_bench import med, timed  # noqa: E402

# (mid channels, stride of the input map relative to the image, conv stride): the depthwise conv of the first block of layer1 .. layer7
LAYERS = [(32, 2, 1), (96, 2, 2), (144, 4, 2), (192, 8, 2), (384, 16, 1), (576, 16, 2), (960, 32, 1)]


def bench_layers(args):
    import torch
    from pointtinybenchmark_amd import ops
    B, recs = args.batch, []
    for C, div, s in LAYERS:
        H = args.size // div
        OH = (H - 1) // s + 1
        Cp = ops.pad32(C)
        gen = torch.Generator(device='cuda').manual_seed(C + s)
        xs = [torch.randn((B, H, H, Cp), device='cuda', generator=gen).mul_(4).clamp_(min=0) for _ in range(2)]
        dys = [torch.randn((B, OH, OH, Cp), device='cuda', generator=gen) for _ in range(2)]
        for t in xs + dys:
            t[..., C:] = 0
        w = torch.randn((C, 1, 3, 3), device='cuda', generator=gen) * 0.3
        sc, bi = torch.rand((C,), device='cuda') + 0.5, torch.randn((C,), device='cuda')
        a, b = torch.rand((B, Cp), device='cuda') + 0.5, torch.randn((B, Cp), device='cuda')
        pack, packt = ops.DwPack(w), ops.DwPack(w, sc)
        lines = {'fwd': lambda j: ops.dw_conv(xs[j], pack, s, scale=sc, bias=bi, in_clamp6=True, relu6=True),
                 'dgrad': lambda j: ops.dw_dgrad(dys[j], packt, (H, H), s, mask6=xs[j], colsum=True),
                 'wgrad': lambda j: ops.dw_wgrad(dys[j], xs[j], C, s, in_clamp6=True),
                 'gn_apply': lambda j: ops.gn_apply(xs[j], a, b, relu=True)}
        ts = {k: [] for k in lines}
        for it in range(args.warmup + args.iters):
            for k, fn in lines.items():
                t = timed(lambda: fn(it % 2))
                if it >= args.warmup:
                    ts[k].append(t)
        n_in, n_out = B * H * H * Cp * 4, B * OH * OH * Cp * 4
        nbytes = dict(fwd=n_in + n_out, dgrad=n_out + 2 * n_in, wgrad=n_in + n_out, gn_apply=2 * n_in)
        rec = dict(map=[B, H, H, C], pitch=Cp, stride=s)
        for k in lines:
            rec[k] = dict(med(ts[k]), bytes=nbytes[k], TBps=nbytes[k] / statistics.median(ts[k]) / 1e9)
        for k in ('fwd', 'dgrad', 'wgrad'):
            rec[k]['of_gn_apply'] = rec[k]['TBps'] / rec['gn_apply']['TBps']
        recs.append(rec)
        del xs, dys
        torch.cuda.empty_cache()
    return recs


def bench_locators(args):
    import torch
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import CprTrainer
    B, S = args.batch, args.size
    batch = synthetic.synthetic_batch(B, S, S, 32, 1, seed=123)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    out = dict(shape=[B, 3, S, S], backbones={})
    for name in ('r50', 'mobilenet_v2_fs1', 'mobilenet_v2'):
        cfg = model_cfg(50, 1)
        if name != 'r50':
            cfg['backbone'] = dict(type='MobileNetV2', out_indices=(1, 2, 4, 7), frozen_stages=1 if name.endswith('fs1') else -1, norm_eval=True)
            cfg['neck'] = dict(cfg['neck'], in_channels=[24, 32, 96, 1280])
            sd = synthetic.locator_state_dict(num_classes=1, head='cpr', seed=0, arch='mobilenet_v2')
        else:
            sd = synthetic.locator_state_dict(50, 1, 0, 'cpr', 0)
        m = P.build_detector(cfg).cuda()
        m.load_state_dict(sd, strict=True)
        m.train()
        ts = []
        with torch.no_grad():
            for it in range(args.warmup + args.steps):
                t = timed(lambda: m.forward_train(**data))
                if it >= args.warmup:
                    ts.append(t)
        rec = dict(forward_loss=dict(med(ts), img_per_s=B / statistics.median(ts) * 1e3))
        tr = CprTrainer(m, lr=1e-3)
        ts = []
        for it in range(args.warmup + args.steps):
            t = timed(lambda: tr.train_step(dict(data)))
            if it >= args.warmup:
                ts.append(t)
        rec['train_step'] = dict(med(ts), img_per_s=B / statistics.median(ts) * 1e3)
        out['backbones'][name] = rec
        del tr, m
        torch.cuda.empty_cache()
    for name in ('mobilenet_v2_fs1', 'mobilenet_v2'):      # (only the frozen_stages=1 line is like for like with R50's training step)
        out['backbones'][name]['ratio_to_r50'] = {k: out['backbones'][name][k]['ms'] / out['backbones']['r50'][k]['ms']
                                                  for k in ('forward_loss', 'train_step')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--parts', default='layers,locators')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mobilenet_v2_bench.py measures on the GPU; none is visible')
    result = dict(iters=args.iters, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    for part, fn in (('layers', bench_layers), ('locators', bench_locators)):
        if part in args.parts.split(','):
            result[part] = fn(args)
            if args.out:        # (kept as it grows: a later part that fails leaves the earlier ones on disk)
                with open(args.out, 'w') as f:
                    f.write(json.dumps(result) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
