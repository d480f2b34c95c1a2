"""What the ResNet variants cost next to the standard net, all lines in the same run:

  stem        the deep stem (csrc/stem_deep.hip, three launches) against the standard stem (csrc/stem_f32.hip / stem_bf16.hip, unchanged
              code) at 64 x 3 x 640 x 640, fp32 and bf16 mode, the two alternating over a ring of distinct images larger than 1 GiB.
              Target: time <= 3.03 x the standard stem's x 1.25 (3.03 = the multiply ratio, 28 512 against 9 408 per output position).
  avgpool     ops.avgpool / ops.avgpool_bwd (with and without ``add``) on maps larger than 1 GiB, fp32 and bf16; bytes = every
              element read once + every element written once.  Target: >= 4.5 TB/s.
  r50         BasicLocator(R50, FPN, CPRHead) at 640^2, B = 64: backbone forward (stem and each stage bracketed by device events),
              the fp32 training step and the mixed-precision step for style pytorch / caffe / avg_down / ResNetV1d.  No target: ratios.

Device-event medians.  Prints one JSON object (--out FILE also writes it: profiles/resnet_variants_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RING_BYTES = 1.25 * (1 << 30)


def timed(fn, sync):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(ts):
    return dict(ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def bench_stem(args):
    import torch
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.backbones.resnet import ResNet
    B, S = args.batch, args.size
    std = ResNet(50, frozen_stages=1).cuda()
    std.load_state_dict(synthetic.resnet_state_dict(50, 0, prefix=''), strict=True)
    deep = ResNet(50, frozen_stages=1, deep_stem=True, avg_down=True).cuda()
    deep.load_state_dict(synthetic.resnet_state_dict(50, 0, prefix='', deep_stem=True, avg_down=True), strict=True)
    std.eval(), deep.eval()
    n_img = int(RING_BYTES // (B * 3 * S * S * 4)) + 2
    ring = [torch.randn((B, 3, S, S), device='cuda', generator=torch.Generator(device='cuda').manual_seed(k)) for k in range(n_img)]
    out = dict(shape=[B, 3, S, S], ring_images=n_img, multiply_ratio=28512 / 9408, allowance=1.25)
    for mode, dt in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        std.compute_dtype = deep.compute_dtype = dt
        ts = dict(std=[], deep=[])
        with torch.no_grad():
            for it in range(args.warmup + args.iters):
                for which, m in (('std', std), ('deep', deep)):
                    x = ring[(2 * it + (which == 'deep')) % n_img]
                    t = timed(lambda: m.run_stem(x), True)
                    if it >= args.warmup:
                        ts[which].append(t)
        r = dict(standard=med(ts['std']), deep=med(ts['deep']))
        r['ratio'] = r['deep']['ms'] / r['standard']['ms']
        r['target_ratio'] = 3.03 * 1.25
        r['within_target'] = r['ratio'] <= r['target_ratio']
        OH = (S - 1) // 2 + 1
        flop = 2.0 * B * OH * OH * (27 * 32 + 288 * 32 + 288 * 64)
        r['deep_TFLOPs'] = flop / r['deep']['ms'] / 1e9
        r['deep_map_bytes'] = B * OH * OH * 32 * 4 * 4 + B * 3 * S * S * 4        # two 32-channel maps written and read, the image read
        out[mode] = r
    return out


def bench_avgpool(args):
    import torch
    from pointtinybenchmark_amd import ops
    out = {}
    for mode, dt, shape in (('fp32', torch.float32, (64, 160, 160, 256)), ('bf16', torch.bfloat16, (64, 160, 160, 512))):
        es = 4 if dt == torch.float32 else 2
        xs = [torch.randn(shape, device='cuda', dtype=dt) for _ in range(2)]
        gs = [torch.randn((shape[0], shape[1] // 2, shape[2] // 2, shape[3]), device='cuda', dtype=dt) for _ in range(2)]
        n_in, n_out = xs[0].numel(), gs[0].numel()
        assert n_in * es > (1 << 30)
        lines = dict(fwd=(lambda i: ops.avgpool(xs[i], 2), (n_in + n_out) * es),
                     bwd=(lambda i: ops.avgpool_bwd(gs[i], shape[1:3], 2), (n_in + n_out) * es),
                     bwd_add=(lambda i: ops.avgpool_bwd(gs[i], shape[1:3], 2, add=xs[i]), (2 * n_in + n_out) * es))
        ts = {k: [] for k in lines}
        for it in range(args.warmup + args.iters):
            for k, (fn, _) in lines.items():
                t = timed(lambda: fn(it % 2), True)
                if it >= args.warmup:
                    ts[k].append(t)
        rec = dict(shape=list(shape), window=2)
        for k, (_, nbytes) in lines.items():
            m = med(ts[k])
            m.update(bytes=nbytes, TBps=nbytes / m['ms'] / 1e9, target_TBps=4.5, within_target=nbytes / m['ms'] / 1e9 >= 4.5)
            rec[k] = m
        out[mode] = rec
        del xs, gs
        torch.cuda.empty_cache()
    return out


VARIANTS = {'pytorch': dict(), 'caffe': dict(style='caffe'), 'avg_down': dict(avg_down=True), 'v1d': dict(deep_stem=True, avg_down=True)}


def bench_r50(args):
    import torch
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import CprTrainer
    B, S = args.batch, args.size
    batch = synthetic.synthetic_batch(B, S, S, 32, 1, seed=123)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    out = dict(shape=[B, 3, S, S], variants={})
    for name, kw in VARIANTS.items():
        cfg = model_cfg(50, 1)
        cfg['backbone'] = dict(cfg['backbone'], **kw)
        m = P.build_detector(cfg).cuda()
        m.load_state_dict(synthetic.locator_state_dict(50, 1, 0, 'cpr', 0, deep_stem=kw.get('deep_stem', False),
                                                       avg_down=kw.get('avg_down', False)), strict=True)
        rec = {}
        bb = m.backbone
        for mode in ('fp32', 'bf16'):
            m.set_compute_dtype(mode)
            m.eval()
            parts = {k: [] for k in ('stem', 'layer1', 'layer2', 'layer3', 'layer4', 'forward')}
            with torch.no_grad():
                for it in range(args.warmup + args.steps):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                    ev[0].record()
                    x = bb.run_stem(data['img'])
                    ev[1].record()
                    for i in range(4):
                        x = bb.run_stage(i, x)
                        ev[2 + i].record()
                    ev[5].synchronize()
                    if it >= args.warmup:
                        for j, k in enumerate(('stem', 'layer1', 'layer2', 'layer3', 'layer4')):
                            parts[k].append(ev[j].elapsed_time(ev[j + 1]))
                        parts['forward'].append(ev[0].elapsed_time(ev[5]))
            rec['backbone_forward_' + mode] = {k: statistics.median(v) for k, v in parts.items()}
            m.train()
            tr = CprTrainer(m, lr=1e-3)
            ts = []
            for it in range(args.warmup + args.steps):
                t = timed(lambda: tr.train_step(dict(data)), True)
                if it >= args.warmup:
                    ts.append(t)
            rec['train_step_' + ('fp32' if mode == 'fp32' else 'mixed')] = dict(med(ts), img_per_s=B / statistics.median(ts) * 1e3)
            del tr
            torch.cuda.empty_cache()
        out['variants'][name] = rec
        del m
        torch.cuda.empty_cache()
    base = out['variants']['pytorch']
    for name, rec in out['variants'].items():
        rec['ratio_to_pytorch'] = {k: (rec[k]['forward'] / base[k]['forward'] if 'forward' in rec[k] else rec[k]['ms'] / base[k]['ms'])
                                   for k in base if k != 'ratio_to_pytorch'}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--parts', default='stem,avgpool,r50')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('resnet_variants_bench.py measures on the GPU; none is visible')
    result = dict(iters=args.iters, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    for part, fn in (('stem', bench_stem), ('avgpool', bench_avgpool), ('r50', bench_r50)):
        if part in args.parts.split(','):
            result[part] = fn(args)
            if args.out:        # (kept as it grows: a later part that fails leaves the earlier ones on disk)
                with open(args.out, 'w') as f:
                    f.write(json.dumps(result) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
