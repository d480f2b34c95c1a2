"""What the BFP neck costs (writes profiles/bfp_bench.json with --out):
  python tools/bfp_bench.py --out profiles/bfp_bench.json

1. The two streaming passes (ops.bfp_gather / ops.bfp_scatter, csrc/bfp.hip) at 16 x (80^2, 40^2, 20^2, 10^2, 5^2) x 256, refine_level 2,
   levels raw under pending affines, fp32 and bf16, next to ops.gn_apply on ONE map of the same total bytes (the yardstick: a streaming
   pass at HBM speed).  The level tables are built once and the entry points called directly, so the host does not pace the launches;
   device events around --launches back-to-back launches, the variants alternating within each of --reps rounds, the median round
   reported.  Bytes are the algorithm's: the gather reads every level once and writes bsf; the scatter reads every level and the refined
   map once and writes every level; gn_apply reads and writes its map; the (N, C) affines are negligible.
2. The P2P line: BasicLocator(R50, P2PHead C=1), 640x640, B=16, start_level=1, num_outs=5, 'on_input', strides [8, 16, 32, 64, 128],
   under FPN and under [FPN, BFP(refine_level=1, 'conv')] -- forward + loss (forward_train under no_grad) and P2PTrainer.train_step,
   fp32 and bf16 compute mode.  Host clock around a step that ends in a device synchronise; the two necks alternate step by step,
   medians over --steps after --warmup."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STRIDES = [8, 16, 32, 64, 128]
SIDES = [80, 40, 20, 10, 5]


def bench_kernel(args):
    import torch
    from pointtinybenchmark_amd import _lib, ops
    rows, r = [], 2
    for dtype in (torch.float32, torch.bfloat16):
        N, C = args.batch, 256
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn((N, s, s, C), generator=g).to(dtype).cuda() for s in SIDES]
        abs_ = [(torch.randn((N, C), generator=g).cuda(), torch.randn((N, C), generator=g).cuda()) for _ in SIDES]
        levels = [(x, ab) for x, ab in zip(xs, abs_)]
        h = w = SIDES[r]
        bsf = ops.bfp_gather(levels, r)
        outs = ops.bfp_scatter(levels, r, bsf, abs_[r])
        sfx = '_bf16' if dtype == torch.bfloat16 else ''
        gather_t = ops._bfp_table([(x, a, b, None, None, x.shape[1], x.shape[2], ops.nearest_scale(x.shape[1], h), ops.nearest_scale(x.shape[2], w))
                                   for x, (a, b) in zip(xs, abs_)])
        scatter_t = ops._bfp_table([(x, a, b, y, None, x.shape[1], x.shape[2], ops.nearest_scale(h, x.shape[1]), ops.nearest_scale(w, x.shape[2]))
                                    for x, (a, b), y in zip(xs, abs_, outs)])
        level_bytes = sum(x.numel() * x.element_size() for x in xs)
        bsf_bytes = bsf.numel() * bsf.element_size()
        moved = {'bfp_gather': level_bytes + bsf_bytes, 'bfp_scatter': 2 * level_bytes + bsf_bytes}
        stream = ops._stream
        variants = {
            'bfp_gather': lambda: _lib.call('cpr_bfp_gather' + sfx, gather_t, len(xs), r, ops._ptr(bsf), N, C, 0, stream()),
            'bfp_scatter': lambda: _lib.call('cpr_bfp_scatter' + sfx, scatter_t, len(xs), r, ops._ptr(bsf), ops._ptr(abs_[r][0]),
                                             ops._ptr(abs_[r][1]), N, C, 0, stream()),
        }
        yard = {}
        for k, nbytes in list(moved.items()):       # gn_apply on one (N, P, 1, C) map moving the same bytes
            P = nbytes // 2 // (N * C * xs[0].element_size())
            ym = torch.randn((N, P, 1, C), generator=torch.Generator('cuda').manual_seed(2), device='cuda').to(dtype)
            yo = torch.empty_like(ym)
            yard[k] = 2 * ym.numel() * ym.element_size()
            variants['gn_apply@' + k] = (lambda ym=ym, yo=yo: ops.gn_apply(ym, abs_[0][0], abs_[0][1], out=yo))
            moved['gn_apply@' + k] = yard[k]
        for fn in variants.values():       # warm up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(args.launches):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[k].append(s.elapsed_time(e) / args.launches)
        for k in variants:
            ms = statistics.median(times[k])
            rows.append(dict(op=k, dtype=str(dtype).split('.')[1], levels=[[N, s, s, C] for s in SIDES], refine_level=r,
                             bytes_moved=moved[k], ms_median=round(ms, 4), ms_min=round(min(times[k]), 4),
                             ms_max=round(max(times[k]), 4), tb_per_s=round(moved[k] / (ms * 1e-3) / 1e12, 3)))
            print(json.dumps(rows[-1]), flush=True)
        by = {row['op']: row for row in rows if row['dtype'] == str(dtype).split('.')[1]}
        for k in ('bfp_gather', 'bfp_scatter'):
            by[k]['rate_vs_gn_apply'] = round(by[k]['tb_per_s'] / by['gn_apply@' + k]['tb_per_s'], 3)
        del xs, outs, bsf, variants
        torch.cuda.empty_cache()
    return rows


def build(with_bfp, dtype, depth=50):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(depth, 1)
    fpn = dict(cfg['neck'], num_outs=5, start_level=1, add_extra_convs='on_input')
    cfg['neck'] = [fpn, dict(type='BFP', in_channels=256, num_levels=5, refine_level=1, refine_type='conv',
                             norm_cfg=dict(type='GN', num_groups=32))] if with_bfp else fpn
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=STRIDES)
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, 1, 1, 'p2p', 3, head_std=0.05, num_points=1)
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.fpn_state_dict(synthetic.backbone_out_channels(depth), 256, 1, 5, 4, prefix='neck.0.' if with_bfp else 'neck.',
                                       add_extra_convs='on_input'))
    if with_bfp:
        sd.update(synthetic.bfp_state_dict(256, 'conv', 5))
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
        models = {'FPN': build(False, dtype), 'FPN+BFP': build(True, dtype)}

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
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--dtypes', default='fp32,bf16')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch,
               kernel=dict(method='device events around %d back-to-back launches on prebuilt level tables, variants alternating, median of '
                           '%d rounds; bytes = what the algorithm must move' % (args.launches, args.reps), rows=bench_kernel(args)),
               locator=dict(workload='BasicLocator(R50, P2PHead C=1), %dx%d, B=%d, %d gts/image, start_level=1, num_outs=5, on_input, '
                            'strides %s; FPN+BFP: BFP(256, 5, refine_level=1, conv, GN); train_step: P2PTrainer, Adam'
                            % (args.size, args.size, args.batch, args.gts, STRIDES),
                            method='host clock around a step ending in a device synchronise, necks alternating, median of %d steps '
                            'after %d warm-up steps' % (args.steps, args.warmup), rows=bench_locator(args)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
