"""What the HRFPN neck costs (writes profiles/hrfpn_bench.json with --out; needs the GPU):
  python tools/hrfpn_bench.py --out profiles/hrfpn_bench.json

1. The four streaming kernels of csrc/hrfpn.hip at 16 x 160^2 x 256 (4 inputs, 5 outputs): ops.hrfpn_fuse and ops.hrfpn_pool in fp32 and
   bf16, ops.hrfpn_pool_bwd and ops.hrfpn_fuse_bwd in fp32, beside ops.gn_apply and ops.gn_apply2 on the same level-0 map in the same run
   (the yardsticks: one-input and two-input streaming passes at HBM speed).  Device events around --launches back-to-back launches, the
   variants alternating within each of --reps rounds, the median round reported.  Bytes are the algorithm's: the fuse reads every level
   once and writes out; the pool reads out once and writes the pooled levels; pool_bwd reads every g_k once and writes d_out; fuse_bwd
   reads d_out once per level and writes dy_i.  (What the kernels actually fetch is more: the pool reads out once PER pooled level, the
   fuse_bwd tiles carry a halo -- DESIGN 8d counts it.)
2. The P2P line: BasicLocator(R50, P2PHead C=1), 640x640, B=16, strides [4, 8, 16], under FPN(num_outs=3) and under HRFPN(num_outs=3) --
   forward + loss (forward_train under no_grad) and P2PTrainer.train_step, fp32 and bf16 compute mode.  Host clock around a step that
   ends in a device synchronise; the two necks alternate step by step, medians over --steps after --warmup."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STRIDES = [4, 8, 16]


def bench_kernel(args):
    import torch
    from pointtinybenchmark_amd import ops
    rows = []
    N, S, C, L, K = args.batch, args.side, 256, 4, 5
    for dtype in (torch.float32, torch.bfloat16):
        name = str(dtype).split('.')[1]
        g = torch.Generator().manual_seed(1)
        ys = [torch.randn((N, S >> i, S >> i, C), generator=g).to(dtype).cuda() for i in range(L)]
        bias = torch.randn((C,), generator=g).cuda()
        a, b = torch.randn((N, C), generator=g).cuda(), torch.randn((N, C), generator=g).cuda()
        out = ops.hrfpn_fuse(ys, bias)
        pooled = ops.hrfpn_pool(out, K)
        nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)      # noqa: E731
        yo = torch.empty_like(out)
        variants = {'hrfpn_fuse': (lambda: ops.hrfpn_fuse(ys, bias), nbytes(ys) + nbytes([out])),
                    'hrfpn_pool': (lambda: ops.hrfpn_pool(out, K), nbytes([out]) + nbytes(pooled)),
                    'gn_apply': (lambda: ops.gn_apply(ys[0], a, b, out=yo), 2 * nbytes([out])),
                    'gn_apply2': (lambda: ops.gn_apply2(ys[0], a, b, out, a, b, out=yo), 3 * nbytes([out]))}
        if dtype == torch.float32:
            gs = [torch.randn(t.shape, generator=g).cuda() for t in [out] + pooled]
            d_out, _ = ops.hrfpn_pool_bwd(gs)
            sizes = [tuple(y.shape[1:3]) for y in ys[1:]]
            dys = ops.hrfpn_fuse_bwd(d_out, sizes)
            variants['hrfpn_pool_bwd'] = (lambda: ops.hrfpn_pool_bwd(gs), nbytes(gs) + nbytes([d_out]))
            variants['hrfpn_fuse_bwd'] = (lambda: ops.hrfpn_fuse_bwd(d_out, sizes), len(sizes) * nbytes([d_out]) + nbytes(dys))
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
        for k, (_, moved) in variants.items():
            ms = statistics.median(times[k])
            rows.append(dict(op=k, dtype=name, level0=[N, S, S, C], inputs=L, outputs=K, bytes_moved=moved, ms_median=round(ms, 4),
                             ms_min=round(min(times[k]), 4), ms_max=round(max(times[k]), 4),
                             tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3)))
        by = {r['op']: r for r in rows if r['dtype'] == name}
        for k in by:
            if k.startswith('hrfpn_'):
                by[k]['rate_vs_gn_apply2'] = round(by[k]['tb_per_s'] / by['gn_apply2']['tb_per_s'], 3)
            print(json.dumps(by[k]), flush=True)
        del variants, ys, out, pooled
        torch.cuda.empty_cache()
    return rows


def build(hrfpn, dtype, depth=50):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(depth, 1)
    chans = synthetic.backbone_out_channels(depth)
    cfg['neck'] = dict(type='HRFPN', in_channels=chans, out_channels=256, num_outs=3) if hrfpn else dict(cfg['neck'], num_outs=3)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=STRIDES)
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, 1, 0, 'p2p', 3, head_std=0.05, num_points=1)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.hrfpn_state_dict(chans, 256, 3, 4) if hrfpn else synthetic.fpn_state_dict(chans, 256, 0, 3, 4))
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
        models = {'FPN': build(False, dtype), 'HRFPN': build(True, dtype)}
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
                        with torch.no_grad():
                            m.forward_train(**data)
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
    ap.add_argument('--side', type=int, default=160)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--gts', type=int, default=32)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dtypes', default='fp32,bf16')
    ap.add_argument('--skip-locator', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch,
               kernel=dict(method='device events around %d back-to-back launches, variants alternating, median of %d rounds; bytes = what '
                           'the algorithm must move' % (args.launches, args.reps), rows=bench_kernel(args)))
    if not args.skip_locator:
        res['locator'] = dict(workload='BasicLocator(R50, P2PHead C=1), %dx%d, B=%d, %d gts/image, strides %s; FPN(num_outs=3) against '
                              'HRFPN(num_outs=3); train_step: P2PTrainer, Adam' % (args.size, args.size, args.batch, args.gts, STRIDES),
                              method='host clock around a step ending in a device synchronise, necks alternating, median of %d steps '
                              'after %d warm-up steps' % (args.steps, args.warmup), rows=bench_locator(args))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
