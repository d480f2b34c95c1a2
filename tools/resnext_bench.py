"""What the grouped 3x3 layers of ResNeXt cost next to R50's dense 3x3 of the same stage, all lines in the same run:

  layers     every grouped-conv launch shape of x50_32x4d at 640 x 640, B = 64 (per stage: the stride-1 blocks and, from layer2 on, the
             stride-2 first block) -- forward (scale / bias / ReLU), data gradient, weight gradient: time, bytes moved, GB/s and
             executed TFLOP/s (2 * 9 * cg FMAs per output; the data gradient of a stride-2 layer runs over the zero-inserted map and
             is charged what it executes), next to R50's dense 3x3 of that stage (half the channels, same map) in the same loop,
             alternating over two sets of maps.
  locators   BasicLocator(backbone, FPN, CPRHead) at 640^2, B = 64: forward + loss img/s and full training-step img/s with
             x50_32x4d and x101_64x4d beside R50 and R101.

The comparison is the dense layer on the same box, never a target.  Device-event medians.  Prints one JSON object (--out FILE also
writes it: profiles/resnext_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(ts):
    return dict(ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def layer_shapes(size, groups=32, base_width=4):
    """(stage, H, C, cg, stride) of every distinct grouped launch of a 32x4d net on a size x size image (H = the conv's input map)."""
    out = []
    for i in range(4):
        cg = 64 * 2 ** i * base_width // 64
        C = cg * groups
        H = size // 4 // 2 ** i
        if i > 0:
            out.append((i + 1, 2 * H, C, cg, 2))
        out.append((i + 1, H, C, cg, 1))
    return out


def bench_layers(args):
    import torch
    from pointtinybenchmark_amd import ops
    B = args.batch
    recs = []
    for stage, H, C, cg, stride in layer_shapes(args.size):
        OH = (H - 1) // stride + 1
        G = C // cg
        Cd = C // 2            # R50's conv2 of this stage
        gen = torch.Generator(device='cuda').manual_seed(stage * 10 + stride)

        def maps(c):
            return [(torch.randn((B, H, H, c), device='cuda', generator=gen), torch.randn((B, OH, OH, c), device='cuda', generator=gen))
                    for _ in range(2)]
        gm, dm = maps(C), maps(Cd)
        wg = torch.randn((C, cg, 3, 3), device='cuda', generator=gen) * 0.05
        wd = torch.randn((Cd, Cd, 3, 3), device='cuda', generator=gen) * 0.05
        sg, bg = torch.rand((C,), device='cuda') + 0.5, torch.randn((C,), device='cuda')
        sd, bd = torch.rand((Cd,), device='cuda') + 0.5, torch.randn((Cd,), device='cuda')
        pg, pd = ops.PackedConv(wg, stride, 1, groups=G), ops.PackedConv(wd, stride, 1)
        tg, td = ops.dgrad_pack(wg, stride, 1, scale=sg, groups=G), ops.dgrad_pack(wd, stride, 1, scale=sd)
        lines = {
            'fwd': (lambda i: ops.conv2d(gm[i][0], pg, scale=sg, bias=bg, relu=True), lambda i: ops.conv2d(dm[i][0], pd, scale=sd, bias=bd, relu=True)),
            'dgrad': (lambda i: ops.conv2d_dgrad(gm[i][1], tg, (H, H), stride), lambda i: ops.conv2d_dgrad(dm[i][1], td, (H, H), stride)),
            'wgrad': (lambda i: ops.conv2d_wgrad(gm[i][1], gm[i][0], (C, cg, 3, 3), stride, 1, groups=G),
                      lambda i: ops.conv2d_wgrad(dm[i][1], dm[i][0], (Cd, Cd, 3, 3), stride, 1)),
        }
        ts = {k: ([], []) for k in lines}
        for it in range(args.warmup + args.iters):
            for k, fns in lines.items():
                for j, fn in enumerate(fns):
                    t = timed(lambda: fn(it % 2))
                    if it >= args.warmup:
                        ts[k][j].append(t)
        n_in, n_out = B * H * H * C * 4, B * OH * OH * C * 4
        n_w = C * cg * 9 * 4
        ws = ops._lib.call('cpr_conv_group_wgrad_workspace', B, OH, OH, C, cg, positive=True) * 4
        nbytes = dict(fwd=n_in + n_out + n_w,
                      dgrad=n_in + n_out + n_w + (2 * n_in if stride > 1 else 0),        # the zero-inserted map: written, then read
                      wgrad=n_in + n_out + 2 * ws + n_w)
        flop = dict(fwd=2.0 * B * OH * OH * C * cg * 9, dgrad=2.0 * B * H * H * C * cg * 9, wgrad=2.0 * B * OH * OH * C * cg * 9)
        rec = dict(stage=stage, map=[B, H, H, C], group_width=cg, groups=G, stride=stride, dense_channels=Cd)
        for k in lines:
            g, d = med(ts[k][0]), med(ts[k][1])
            g.update(bytes=nbytes[k], GBps=nbytes[k] / g['ms'] / 1e6, executed_TFLOPs=flop[k] / g['ms'] / 1e9)
            rec[k] = dict(grouped=g, dense_r50=d, ratio_to_dense=g['ms'] / d['ms'])
        recs.append(rec)
        del gm, dm
        torch.cuda.empty_cache()
    return recs


BACKBONES = {'r50': dict(depth=50), 'x50_32x4d': dict(depth=50, groups=32, base_width=4), 'r101': dict(depth=101),
             'x101_64x4d': dict(depth=101, groups=64, base_width=4)}


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
        cfg = model_cfg(kw['depth'], 1)
        grouped = {k: v for k, v in kw.items() if k != 'depth'}
        cfg['backbone'] = dict(cfg['backbone'], type='ResNeXt' if grouped else 'ResNet', **grouped)
        m = P.build_detector(cfg).cuda()
        m.load_state_dict(synthetic.locator_state_dict(kw['depth'], 1, 0, 'cpr', 0, **grouped), strict=True)
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
    for name, base in (('x50_32x4d', 'r50'), ('x101_64x4d', 'r101')):
        out['backbones'][name]['ratio_to_' + base] = {k: out['backbones'][name][k]['ms'] / out['backbones'][base][k]['ms']
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
        raise SystemExit('resnext_bench.py measures on the GPU; none is visible')
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
