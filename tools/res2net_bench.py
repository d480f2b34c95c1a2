"""What the Res2Net slice convs (csrc/res2net.hip) cost, and the Res2Net-50 26w4s forward beside R50 and x50_32x4d, all lines in the same
run:

  layers     every slice-conv launch shape of Res2Net-50 26w4s at 640 x 640, B = 64 (per stage: the stride-1 'normal' launch, which
             sums slice i of conv1's output and slice i - 1 of the concatenated map on load, and from layer2 on the stride-2 'stage'
             launch), on maps at the block's pitch roundup(4 * width, 32) -- forward (scale / bias / ReLU), data gradient, weight
             gradient: time and executed TFLOP/s (2 * 9 * width FMAs per output; the data gradient of a stride-2 layer runs in gather
             form over every tap and is charged what it executes), alternating over two sets of maps.
  locators   BasicLocator(backbone, FPN, CPRHead) at 640^2, B = 64: forward + loss img/s and full training-step img/s (CprTrainer) with
             R50, x50_32x4d and Res2Net-50 26w4s.

Device-event medians.  Prints one JSON object (--out FILE also writes it: profiles/res2net_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.resnext_bench import med, timed  # noqa: E402


def layer_shapes(size, base_width=26, scales=4):
    """(stage, H, width, pitch, stride, add) of every distinct slice-conv launch on a size x size image (H = the conv's input map)."""
    out = []
    for i in range(4):
        w = base_width * 2 ** i
        pitch = (w * scales + 31) // 32 * 32
        H = size // 4 // 2 ** i
        if i > 0:
            out.append((i + 1, 2 * H, w, pitch, 2, False))
        out.append((i + 1, H, w, pitch, 1, True))
    return out


def bench_layers(args):
    import torch
    from pointtinybenchmark_amd import ops
    B = args.batch
    recs = []
    for stage, H, w, pitch, stride, add in layer_shapes(args.size):
        OH = (H - 1) // stride + 1
        gen = torch.Generator(device='cuda').manual_seed(stage * 10 + stride)
        # (conv1's output, the concatenated map / its gradient): the conv reads slice 1 of the first (+ slice 0 of the second) and
        # writes slice 1 of the second, as convs[1] of a block does
        sets = [(torch.randn((B, H, H, pitch), device='cuda', generator=gen), torch.randn((B, OH, OH, pitch), device='cuda', generator=gen),
                 torch.empty((B, H, H, pitch), device='cuda')) for _ in range(2)]
        wt = torch.randn((w, w, 3, 3), device='cuda', generator=gen) * 0.05
        sc, bi = torch.rand((w,), device='cuda') + 0.5, torch.randn((w,), device='cuda')
        pk, pt = ops.Res2Pack(wt), ops.Res2Pack(wt, scale=sc, transpose=True)
        lines = {
            'fwd': lambda i: ops.res2_conv(sets[i][0], w, pk, sets[i][1], w, stride=stride, add=sets[i][1] if add else None, add_off=0,
                                           scale=sc, bias=bi, relu=True),
            'dgrad': lambda i: ops.res2_conv(sets[i][1], w, pt, sets[i][2], w, stride=stride, transposed=True),
            'wgrad': lambda i: ops.res2_wgrad(sets[i][1], w, sets[i][0], w, w, stride, add=sets[i][1] if add else None, add_off=0),
        }
        ts = {k: [] for k in lines}
        for it in range(args.warmup + args.iters):
            for k, fn in lines.items():
                t = timed(lambda: fn(it % 2))
                if it >= args.warmup:
                    ts[k].append(t)
        flop = dict(fwd=2.0 * B * OH * OH * w * w * 9, dgrad=2.0 * B * H * H * w * w * 9, wgrad=2.0 * B * OH * OH * w * w * 9)
        rec = dict(stage=stage, map=[B, H, H, pitch], width=w, stride=stride, add=add)
        for k in lines:
            g = med(ts[k])
            g.update(executed_TFLOPs=flop[k] / g['ms'] / 1e9)
            rec[k] = g
        recs.append(rec)
        del sets
        torch.cuda.empty_cache()
    return recs


BACKBONES = {'r50': dict(type='ResNet'), 'x50_32x4d': dict(type='ResNeXt', groups=32, base_width=4),
             'res2net50_26w4s': dict(type='Res2Net', scales=4, base_width=26)}


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
    for name, kw in BACKBONES.items():
        cfg = model_cfg(50, 1)
        cfg['backbone'] = dict(cfg['backbone'], **kw)
        m = P.build_detector(cfg).cuda()
        if kw['type'] == 'Res2Net':
            sd = {k: v for k, v in synthetic.locator_state_dict(50, 1, 0, 'cpr', 0).items() if not k.startswith('backbone.')}
            sd.update(synthetic.res2net_state_dict(50, kw['scales'], kw['base_width'], 0))
        else:
            sd = synthetic.locator_state_dict(50, 1, 0, 'cpr', 0, **{k: v for k, v in kw.items() if k != 'type'})
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
    for name in ('x50_32x4d', 'res2net50_26w4s'):
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
        raise SystemExit('res2net_bench.py measures on the GPU; none is visible')
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
