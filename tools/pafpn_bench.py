"""What the PAFPN neck costs (writes profiles/pafpn_bench.json with --out):
  python tools/pafpn_bench.py --out profiles/pafpn_bench.json

1. The two-source GroupNorm apply (ops.gn_apply2, csrc/pafpn.hip) next to ops.gn_apply on the same maps: 160x160 and 80x80 x 256
   channels at B=16, fp32 and bf16.  Device events around --launches back-to-back launches, the variants alternating within each of
   --reps rounds, the median round reported.  Bytes are the algorithm's: three maps for gn_apply2 (two reads, one write), two for
   gn_apply; the (N, C) affines are negligible.  fp32 also times the route the kernel replaces: gn_apply, gn_apply, axpby (seven maps).
2. The P2P line: BasicLocator(R50, P2PHead C=1), 640x640, B=16, start_level=1, num_outs=5, 'on_input', strides [8, 16, 32, 64, 128],
   under FPN and under PAFPN -- forward + loss (forward_train under no_grad) and P2PTrainer.train_step, fp32 and bf16 compute mode.
   Host clock around a step that ends in a device synchronise; the two necks alternate step by step, medians over --steps after
   --warmup."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STRIDES = [8, 16, 32, 64, 128]


def bench_kernel(args):
    import torch
    from pointtinybenchmark_amd import ops
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for hw in (160, 80):
            N, C = args.batch, 256
            g = torch.Generator().manual_seed(1)
            x1, x2 = (torch.randn((N, hw, hw, C), generator=g).to(dtype).cuda() for _ in range(2))
            a1, b1, a2, b2 = (torch.randn((N, C), generator=g).cuda() for _ in range(4))
            out = torch.empty_like(x1)
            map_bytes = x1.numel() * x1.element_size()
            variants = {'gn_apply2': (lambda: ops.gn_apply2(x1, a1, b1, x2, a2, b2, out=out), 3),
                        'gn_apply': (lambda: ops.gn_apply(x1, a1, b1, out=out), 2)}
            if dtype == torch.float32:
                tmp = torch.empty_like(x1)

                def composed():
                    ops.gn_apply(x1, a1, b1, out=out)
                    ops.gn_apply(x2, a2, b2, out=tmp)
                    ops.axpby(out, tmp, 1.0, 1.0)
                variants['gn_apply+gn_apply+axpby'] = (composed, 7)
            for fn, _ in variants.values():       # warm up: code objects, allocator
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, (fn, _) in variants.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(args.launches):
                        fn()
                    e.record()
                    torch.cuda.synchronize()
                    times[k].append(s.elapsed_time(e) / args.launches)
            for k, (_, maps) in variants.items():
                ms = statistics.median(times[k])
                rows.append(dict(op=k, dtype=str(dtype).split('.')[1], shape=[N, hw, hw, C], maps_moved=maps,
                                 ms_median=round(ms, 4), ms_min=round(min(times[k]), 4), ms_max=round(max(times[k]), 4),
                                 tb_per_s=round(maps * map_bytes / (ms * 1e-3) / 1e12, 3)))
                print(json.dumps(rows[-1]), flush=True)
            del x1, x2, out
            torch.cuda.empty_cache()
    return rows


def build(neck_type, dtype, depth=50):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(depth, 1)
    cfg['neck'] = dict(cfg['neck'], type=neck_type, num_outs=5, start_level=1, add_extra_convs='on_input')
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=STRIDES)
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, 1, 1, 'p2p', 3, head_std=0.05, num_points=1)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    make = synthetic.pafpn_state_dict if neck_type == 'PAFPN' else synthetic.fpn_state_dict
    sd.update(make(synthetic.backbone_out_channels(depth), 256, 1, 5, 4, add_extra_convs='on_input'))
    m.load_state_dict(sd, strict=True)
    m.train()
    m.set_compute_dtype(dtype)
    return m


def bench_locator(args):
    import torch
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import P2PTrainer
    batch = synthetic.synthetic_batch(args.batch, args.size, args.size, args.gts, 1, seed=61)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    rows = []
    for dtype in args.dtypes.split(','):
        models = {k: build(k, dtype) for k in ('FPN', 'PAFPN')}

        def forward_loss(m):
            with torch.no_grad():
                m.forward_train(**data)
        trainers = {}
        for mode in ('forward_loss', 'train_step'):
            if mode == 'train_step':
                trainers = {k: P2PTrainer(m, optimizer=dict(type='Adam', lr=1e-4), max_norm=35.0) for k, m in models.items()}
            times = {k: [] for k in models}
            for i in range(args.warmup + args.steps):
                for k, m in models.items():       # the two necks alternate step by step
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if mode == 'train_step':
                        trainers[k].train_step(dict(data))
                    else:
                        forward_loss(m)
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3)
            for k in models:
                med = statistics.median(times[k])
                rows.append(dict(neck=k, compute=dtype, mode=mode, ms_median=round(med, 2), ms=[round(v, 2) for v in times[k]],
                                 img_per_s=round(args.batch * 1e3 / med, 1)))
                print(json.dumps(rows[-1]), flush=True)
            rows[-1]['delta_vs_fpn_ms'] = round(rows[-1]['ms_median'] - rows[-2]['ms_median'], 2)
            rows[-1]['delta_vs_fpn'] = round(rows[-1]['ms_median'] / rows[-2]['ms_median'] - 1, 4)
        del trainers, models
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--gts', type=int, default=32)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dtypes', default='fp32,bf16')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch,
               kernel=dict(method='device events around %d back-to-back launches, variants alternating, median of %d rounds; bytes = '
                           'maps moved x map size' % (args.launches, args.reps), rows=bench_kernel(args)),
               locator=dict(workload='BasicLocator(R50, P2PHead C=1), %dx%d, B=%d, %d gts/image, start_level=1, num_outs=5, on_input, '
                            'strides %s; train_step: P2PTrainer, Adam' % (args.size, args.size, args.batch, args.gts, STRIDES),
                            method='host clock around a step ending in a device synchronise, necks alternating, median of %d steps '
                            'after %d warm-up steps' % (args.steps, args.warmup), rows=bench_locator(args)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
