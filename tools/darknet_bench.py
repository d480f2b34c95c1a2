"""What the Darknet passes cost (writes profiles/darknet_bench.json with --out; needs the GPU):
  python tools/darknet_bench.py --out profiles/darknet_bench.json

1. The three kernels of csrc/darknet.hip on full-size maps of a 16 x 640^2 batch: ops.leaky (in place, and with the shortcut sum
   into a second buffer) and ops.leaky_bwd_colsum (with and without ``add``) at 16 x 320^2 x 64 (stage 1) and 16 x 80^2 x 256 (stage 3);
   ops.leaky in place and ops.stem3x3s1_wgrad at 16 x 640^2 x 32 (conv1's map).  Beside them, in the same run: ops.gn_apply2 at
   16 x 160^2 x 256 x 3 maps = 1.26 GB (the yardstick: a two-input streaming pass at HBM speed).  Device events around --launches
   back-to-back launches, the variants alternating within each of --reps rounds, the median round reported.  Bytes are the
   algorithm's: every operand map read once, every result map written once (the column-sum partials and the 864-float weight gradient
   are left out: they are below 1 % of the maps).  Every variant relaunches on the same buffers, so a working set below the 256 MB
   Infinity Cache is measured cache-resident, not at HBM speed; ``fits_infinity_cache`` says which.
2. The P2P line: BasicLocator(P2PHead C=1), 640 x 640, B=16, fp32: ResNet-50 + FPN(num_outs=3, strides [4, 8, 16]) against Darknet-53 +
   FPN(num_outs=3, in_channels [256, 512, 1024], strides [8, 16, 32]) -- forward + loss (forward_train under no_grad) and
   P2PTrainer.train_step.  Host clock around a step that ends in a device synchronise; the two models alternate step by step, medians
   over --steps after --warmup.  The share of the Darknet step that the leaky passes and the stem weight gradient take: device-event
   brackets around every ops.leaky / ops.leaky_bwd_colsum / ops.stem3x3s1_wgrad launch in --share-steps further steps (not in the timed
   steps), their sum over the unbracketed step's median.  That share is the price of leaving the conv epilogues alone."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NECK_IN = [256, 512, 1024]
INFINITY_CACHE = 256 << 20


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def bench_kernel(args):
    import torch
    from pointtinybenchmark_amd import ops
    N, S = args.batch, args.size
    g = torch.Generator().manual_seed(1)
    variants = {}

    def rand(shape):
        return torch.randn(shape, generator=g).cuda()
    for H, C in ((S // 2, 64), (S // 8, 256)):
        shape = (N, H, H, C)
        z, res, dy, add = rand(shape), rand(shape), rand(shape), rand(shape)
        out, gbuf = torch.empty_like(z), torch.empty_like(z)
        tag = '%dx%d^2x%d' % (N, H, C)
        # (in place on the same buffer again and again: the values shrink towards zero, the traffic does not change)
        variants['leaky in place ' + tag] = (lambda z=z: ops.leaky(z, 0.1), 2 * nbytes([z]), dict(shape=list(shape)))
        variants['leaky + shortcut ' + tag] = (lambda z=z, res=res, out=out: ops.leaky(z, 0.1, res=res, out=out), 3 * nbytes([z]),
                                               dict(shape=list(shape)))
        variants['leaky_bwd_colsum ' + tag] = (lambda dy=dy, z=z, gbuf=gbuf: ops.leaky_bwd_colsum(dy, z, 0.1, out=gbuf), 3 * nbytes([z]),
                                               dict(shape=list(shape)))
        variants['leaky_bwd_colsum + add ' + tag] = (lambda dy=dy, z=z, add=add, gbuf=gbuf: ops.leaky_bwd_colsum(dy, z, 0.1, add=add, out=gbuf),
                                                     4 * nbytes([z]), dict(shape=list(shape)))
    shape = (N, S, S, 32)
    z0, x4 = rand(shape), rand((N, S, S, 4))
    gw = torch.empty((32, 3, 3, 3), device='cuda')
    tag = '%dx%d^2x32' % (N, S)
    variants['leaky in place ' + tag] = (lambda: ops.leaky(z0, 0.1), 2 * nbytes([z0]), dict(shape=list(shape)))
    variants['stem3x3s1_wgrad ' + tag] = (lambda: ops.stem3x3s1_wgrad(z0, x4, planar=False, out=gw), nbytes([z0, x4]), dict(shape=list(shape)))
    C, Hy = 256, S // 4
    x, x2 = rand((N, Hy, Hy, C)), rand((N, Hy, Hy, C))
    a, b = rand((N, C)), rand((N, C))
    yo = torch.empty_like(x)
    variants['gn_apply2'] = (lambda: ops.gn_apply2(x, a, b, x2, a, b, out=yo), 3 * nbytes([x]), dict(shape=[N, Hy, Hy, C]))
    for fn, _, _ in variants.values():       # warm up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, (fn, _, _) in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.launches):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / args.launches)
    rows, yard = [], None
    for k, (_, moved, info) in variants.items():
        ms = statistics.median(times[k])
        rows.append(dict(op=k, bytes_moved=moved, gb_moved=round(moved / 1e9, 4), fits_infinity_cache=moved <= INFINITY_CACHE,
                         ms_median=round(ms, 4), ms_min=round(min(times[k]), 4), ms_max=round(max(times[k]), 4),
                         tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3), **info))
        if k == 'gn_apply2':
            yard = rows[-1]['tb_per_s']
    for r in rows:
        r['rate_vs_gn_apply2'] = round(r['tb_per_s'] / yard, 3)
        print(json.dumps(r), flush=True)
    return rows


def build(darknet):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(50, 1)
    if darknet:
        cfg['backbone'] = dict(type='Darknet', depth=53)
        cfg['neck'] = dict(cfg['neck'], in_channels=NECK_IN, num_outs=3, add_extra_convs=False)
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[8, 16, 32])
        sd = synthetic.darknet_state_dict(53, 3, prefix='backbone.')
        sd.update(synthetic.fpn_state_dict(NECK_IN, 256, 0, 3, 4))
        sd.update(synthetic.p2p_head_state_dict(1, seed=6, std=0.05))
    else:
        cfg['neck'] = dict(cfg['neck'], num_outs=3)
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16])
        chans = synthetic.backbone_out_channels(50)
        sd = synthetic.locator_state_dict(50, 1, 0, 'p2p', 3, head_std=0.05, num_points=1)
        sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
        sd.update(synthetic.fpn_state_dict(chans, 256, 0, 3, 4))
    m = P.build_detector(cfg).cuda()
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def bench_locator(args):
    import torch
    from pointtinybenchmark_amd import ops, synthetic
    from pointtinybenchmark_amd.training import P2PTrainer
    batch = synthetic.synthetic_batch(args.batch, args.size, args.size, args.gts, 1, seed=61)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    models = {'R50+FPN': build(False), 'Darknet-53+FPN': build(True)}
    names = ('leaky', 'leaky_bwd_colsum', 'stem3x3s1_wgrad')
    real = {k: getattr(ops, k) for k in names}
    rows, trainers, shares = [], {}, {}
    for mode in ('forward_loss', 'train_step'):
        if mode == 'train_step':
            trainers = {k: P2PTrainer(m, optimizer=dict(type='Adam', lr=1e-4), max_norm=35.0) for k, m in models.items()}

        def step(k):
            if mode == 'train_step':
                out = trainers[k].train_step(dict(data))
                assert all(v == v and abs(v) < float('inf') for v in out['log_vars'].values()), out['log_vars']
            else:
                with torch.no_grad():
                    models[k].forward_train(**data)
        times = {k: [] for k in models}
        for i in range(args.warmup + args.steps):
            for k in models:       # the two models alternate step by step
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(k)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        for k in models:
            med = statistics.median(times[k])
            rows.append(dict(model=k, compute='fp32', mode=mode, ms_median=round(med, 2), ms=[round(v, 2) for v in times[k]],
                             img_per_s=round(args.batch * 1e3 / med, 1)))
            print(json.dumps(rows[-1]), flush=True)
        # the share of the Darknet step that the new passes take
        step_ms = rows[-1]['ms_median']
        events = {k: [] for k in names}

        def bracket(name):
            def fn(*a, **kw):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = real[name](*a, **kw)
                e.record()
                events[name].append((s, e))
                return r
            return fn
        for k in names:
            setattr(ops, k, bracket(k))
        try:
            for _ in range(args.share_steps):
                step('Darknet-53+FPN')
            torch.cuda.synchronize()
        finally:
            for k in names:
                setattr(ops, k, real[k])
        share = {}
        for k, ev in events.items():
            ms = sum(s.elapsed_time(e) for s, e in ev) / args.share_steps
            share[k] = dict(launches_per_step=len(ev) // args.share_steps, ms_per_step=round(ms, 3), share_of_step=round(ms / step_ms, 4))
        share['all'] = dict(ms_per_step=round(sum(v['ms_per_step'] for v in share.values()), 3),
                            share_of_step=round(sum(v['share_of_step'] for v in share.values()), 4))
        shares[mode] = share
        print(json.dumps({mode: share}), flush=True)
    return rows, shares


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--gts', type=int, default=32)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--share-steps', type=int, default=3)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-locator', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch,
               kernel=dict(method='device events around %d back-to-back launches, variants alternating, median of %d rounds; bytes = every '
                           'operand map read once and every result map written once' % (args.launches, args.reps), rows=bench_kernel(args)))
    if not args.skip_locator:
        rows, shares = bench_locator(args)
        res['locator'] = dict(workload='BasicLocator(P2PHead C=1), %dx%d, B=%d, %d gts/image, fp32: ResNet-50 + FPN(num_outs=3, strides '
                              '[4, 8, 16]) against Darknet-53 + FPN(num_outs=3, strides [8, 16, 32]); train_step: P2PTrainer, Adam'
                              % (args.size, args.size, args.batch, args.gts),
                              method='host clock around a step ending in a device synchronise, models alternating, median of %d steps '
                              'after %d warm-up steps' % (args.steps, args.warmup), rows=rows,
                              darknet_pass_share=dict(method='device-event brackets around every launch of the three ops in %d further '
                                                      'steps, summed per step, over the unbracketed median of that mode (the weight '
                                                      'gradient runs on the side stream: its time overlaps the main stream\'s)'
                                                      % args.share_steps, **shares))
    res['not_measured'] = ['the bf16 compute mode (refused for Darknet)', 'CprTrainer at full size', 'hardware counters of the three kernels',
                           'multi-GPU training']
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
