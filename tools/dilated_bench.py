"""What dilated stages cost, all lines in the same run:

  locators   BasicLocator(backbone, FPN, CPRHead) at 640^2 with frozen_stages=1: forward + loss img/s and full training-step img/s with
             R50 beside R50 DC5 (strides (1, 2, 2, 1), dilations (1, 1, 1, 2): layer4 at 4x the pixels) and R50 OS8 (strides (1, 2, 1, 1),
             dilations (1, 1, 2, 4): layer3 at 4x, layer4 at 16x), and x50_32x4d beside its DC5 form.  One batch size for all five: the
             largest of --batches at which the heaviest net (R50 OS8) trains; it is recorded.
  layers     the dilated dense 3x3 launches of those nets -- 512 -> 512 (layer4: 40 x 40 at d = 2, 80 x 80 at d = 4) and 256 -> 256 (layer3 of
             OS8: 80 x 80 at d = 2) -- forward (scale / bias / ReLU), data gradient, weight gradient, and beside each the UNDILATED layer
             on the same map on the direct kernel (ops.WINOGRAD off) and on Winograd, with the executed TFLOP/s of each (direct and
             dilated execute 2 * 9 * Cin * Cout per output, Winograd F(2x2, 3x3) 1 / 2.25 of that).

The comparison is the undilated layer / net on the same box, never a target.  Device-event medians, warm-up, one run.  Prints one JSON
object (--out FILE also writes it: profiles/dilated_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DC5 = dict(strides=(1, 2, 2, 1), dilations=(1, 1, 1, 2))
OS8 = dict(strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4))
BACKBONES = {'r50': dict(), 'r50_dc5': dict(DC5), 'r50_os8': dict(OS8), 'x50_32x4d': dict(groups=32, base_width=4),
             'x50_32x4d_dc5': dict(groups=32, base_width=4, **DC5)}
# (name, H = W of the map at a 640 x 640 input, channels, dilation)
LAYERS = [('layer4_dc5', 40, 512, 2), ('layer4_os8', 80, 512, 4), ('layer3_os8', 80, 256, 2)]


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


def _locator(kw):
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = model_cfg(50, 1)
    grouped = {k: v for k, v in kw.items() if k in ('groups', 'base_width')}
    cfg['backbone'] = dict(cfg['backbone'], type='ResNeXt' if grouped else 'ResNet', frozen_stages=1, **kw)
    m = P.build_detector(cfg).cuda()
    m.load_state_dict(synthetic.locator_state_dict(50, 1, 0, 'cpr', 0, **grouped), strict=True)
    m.train()
    return m


def _data(B, S):
    from pointtinybenchmark_amd import synthetic
    batch = synthetic.synthetic_batch(B, S, S, 32, 1, seed=123)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def pick_batch(args):
    """The largest of --batches at which R50 OS8 runs one training step (an allocation failure moves on to the next)."""
    import torch
    from pointtinybenchmark_amd.training import CprTrainer
    tried = []
    for B in [int(b) for b in args.batches.split(',')]:
        m = tr = data = None
        try:
            m = _locator(BACKBONES['r50_os8'])
            data = _data(B, args.size)
            tr = CprTrainer(m, lr=1e-3)
            tr.train_step(dict(data))
            torch.cuda.synchronize()
            tried.append(dict(batch=B, fits=True, peak_GiB=torch.cuda.max_memory_allocated() / 2 ** 30))
            return B, tried
        except torch.cuda.OutOfMemoryError:
            tried.append(dict(batch=B, fits=False))
        finally:
            del m, tr, data
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
    raise SystemExit('R50 OS8 fits at none of --batches %s' % args.batches)


def bench_locators(args):
    import torch
    from pointtinybenchmark_amd.training import CprTrainer
    B, tried = pick_batch(args)
    S = args.size
    data = _data(B, S)
    out = dict(shape=[B, 3, S, S], frozen_stages=1, batches_tried=tried, backbones={})
    for name, kw in BACKBONES.items():
        m = _locator(kw)
        torch.cuda.reset_peak_memory_stats()
        ts = []
        with torch.no_grad():
            for it in range(args.warmup + args.steps):
                t = timed(lambda: m.forward_train(**data))
                if it >= args.warmup:
                    ts.append(t)
        rec = dict(strides=list(m.backbone.strides), dilations=list(m.backbone.dilations),
                   forward_loss=dict(med(ts), img_per_s=B / statistics.median(ts) * 1e3))
        tr = CprTrainer(m, lr=1e-3)
        ts = []
        for it in range(args.warmup + args.steps):
            t = timed(lambda: tr.train_step(dict(data)))
            if it >= args.warmup:
                ts.append(t)
        rec['train_step'] = dict(med(ts), img_per_s=B / statistics.median(ts) * 1e3)
        rec['peak_GiB'] = torch.cuda.max_memory_allocated() / 2 ** 30
        out['backbones'][name] = rec
        del tr, m
        torch.cuda.empty_cache()
    for name, base in (('r50_dc5', 'r50'), ('r50_os8', 'r50'), ('x50_32x4d_dc5', 'x50_32x4d')):
        out['backbones'][name]['ratio_to_' + base] = {k: out['backbones'][name][k]['ms'] / out['backbones'][base][k]['ms']
                                                      for k in ('forward_loss', 'train_step')}
    return out


def bench_layers(args, B):
    import torch
    from pointtinybenchmark_amd import ops
    recs = []
    for name, H, C, d in LAYERS:
        gen = torch.Generator(device='cuda').manual_seed(H + C + d)
        maps = [(torch.randn((B, H, H, C), device='cuda', generator=gen), torch.randn((B, H, H, C), device='cuda', generator=gen))
                for _ in range(2)]
        w = torch.randn((C, C, 3, 3), device='cuda', generator=gen) * 0.02
        s, b = torch.rand((C,), device='cuda') + 0.5, torch.randn((C,), device='cuda')
        forms = {'dilated': (ops.PackedConv(w, 1, d, dilation=d), ops.dgrad_pack(w, 1, d, scale=s, dilation=d), d, True),
                 'undilated_direct': (ops.PackedConv(w, 1, 1), ops.dgrad_pack(w, 1, 1, scale=s), 1, False),
                 'undilated_winograd': (ops.PackedConv(w, 1, 1), ops.dgrad_pack(w, 1, 1, scale=s), 1, True)}
        flop = 2.0 * B * H * H * 9 * C * C
        rec = dict(layer=name, map=[B, H, H, C], dilation=d, direct_GFLOP=flop / 1e9)
        for form, (pc, pt, dil, wino) in forms.items():
            lines = dict(fwd=lambda i: ops.conv2d(maps[i][0], pc, scale=s, bias=b, relu=True),
                         dgrad=lambda i: ops.conv2d_dgrad(maps[i][1], pt, (H, H), 1),
                         wgrad=lambda i: ops.conv2d_wgrad(maps[i][1], maps[i][0], (C, C, 3, 3), 1, dil, dilation=dil))
            ts = {k: [] for k in lines}
            variants = {}
            ops.WINOGRAD[0] = wino
            try:
                for it in range(args.warmup + args.iters):
                    for k, fn in lines.items():
                        ops.TRACE_CONV_VARIANT[0] = k != 'wgrad'
                        t = timed(lambda: fn(it % 2))
                        if k != 'wgrad':
                            variants[k] = list(ops.TRACE_CONV_VARIANT[1] or ())
                        if it >= args.warmup:
                            ts[k].append(t)
            finally:
                ops.WINOGRAD[0] = True
                ops.TRACE_CONV_VARIANT[0] = False
            executed = flop / 2.25 if form == 'undilated_winograd' else flop
            rec[form] = {k: dict(med(v), executed_TFLOPs=executed / statistics.median(v) / 1e9, kernel=variants.get(k)) for k, v in ts.items()}
        for k in ('fwd', 'dgrad', 'wgrad'):
            rec.setdefault('ratio_dilated_to', {})[k] = {f: rec['dilated'][k]['ms'] / rec[f][k]['ms']
                                                         for f in ('undilated_direct', 'undilated_winograd')}
        recs.append(rec)
        del maps
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', default='64,32,16,8', help='batch sizes to try, largest first')
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--parts', default='locators,layers')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('dilated_bench.py measures on the GPU; none is visible')
    result = dict(iters=args.iters, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    parts = args.parts.split(',')
    B = int(args.batches.split(',')[-1])
    if 'locators' in parts:
        result['locators'] = bench_locators(args)
        B = result['locators']['shape'][0]
    if args.out:        # (kept as it grows: a later part that fails leaves the earlier ones on disk)
        with open(args.out, 'w') as f:
            f.write(json.dumps(result) + '\n')
    if 'layers' in parts:
        result['layers'] = bench_layers(args, B)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
