"""What the HRNet exchange costs (writes profiles/hrnet_bench.json with --out; needs the GPU):
  python tools/hrnet_bench.py --out profiles/hrnet_bench.json

1. The two streaming kernels of csrc/hrnet.hip on the four W32 branch shapes of a 16 x 640^2 batch -- 160^2 x 32, 80^2 x 64, 40^2 x 128,
   20^2 x 256 -- each with the term table of its stage4 exchange (output branch i: i down-chain outputs and the identity at its own
   size, then the coarser branches' 1x1 outputs at k = 1 .. 3 - i) and, for the adjoint, K = 3 - i pooled maps.  Beside them, in the same
   run: ops.gn_apply2 at 16 x 160^2 x 256 (the yardstick: a two-input streaming pass at HBM speed) and the route the forward kernel
   replaces -- torch's nearest upsample of every coarse term, the adds and the ReLU on the same maps (channels-last views).  Device events
   around --launches back-to-back launches, the variants alternating within each of --reps rounds, the median round reported.  Bytes
   are the algorithm's: the fuse reads every term once at its own size and writes out; the adjoint reads dy and y once and writes g, the
   K pooled maps and the column-sum partials.  Every variant relaunches on the same buffers: the branch working sets (20 .. 175 MB) fit the 256 MB
   Infinity Cache and the yardstick's 1.26 GB does not, so their TB/s are cache-resident rates, not HBM rates.
2. The P2P line: BasicLocator(P2PHead C=1), 640 x 640, B=16, strides [4, 8, 16]: ResNet-50 + FPN(num_outs=3) against HRNetV2p-W32 +
   HRFPN(num_outs=3), fp32 -- forward + loss (forward_train under no_grad) and P2PTrainer.train_step.  Host clock around a step that ends
   in a device synchronise; the two models alternate step by step, medians over --steps after --warmup.  The exchange kernels' share of
   the HRNet step: device-event brackets around every ops.hrnet_fuse / ops.hrnet_fuse_bwd launch in --share-steps further steps (the
   brackets serialise nothing -- one stream -- but are not in the timed steps), their sum over the unbracketed step's median."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STRIDES = [4, 8, 16]
from tests.hrnet_ref import W32_EXTRA  # noqa: E402  (the reference's HRNetV2p-W32 ``extra``)

WIDTHS = [32, 64, 128, 256]


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def bench_kernel(args):
    import torch
    import torch.nn.functional as F
    from pointtinybenchmark_amd import ops
    N, S = args.batch, args.side
    g = torch.Generator().manual_seed(1)
    variants = {}
    for i, C in enumerate(WIDTHS):
        H = S >> i
        ks = [0] * (i + 1) + list(range(1, 4 - i))
        terms = [(torch.randn((N, H >> k, H >> k, C), generator=g).cuda(), k) for k in ks]
        out = ops.hrnet_fuse(terms, (H, H))
        dy = torch.randn((N, H, H, C), generator=g).cuda()
        K = 3 - i
        gg, pools, part = ops.hrnet_fuse_bwd(dy, out, K)
        nchw = [(t.permute(0, 3, 1, 2), k) for t, k in terms]      # channels-last views of the same maps

        def torch_route(nchw=nchw):
            acc = nchw[0][0]
            for t, k in nchw[1:]:
                acc = acc + (F.interpolate(t, scale_factor=2 ** k, mode='nearest') if k else t)
            return torch.relu(acc)
        assert torch.equal(torch_route().permute(0, 2, 3, 1), out)
        shape = [N, H, H, C]
        variants['hrnet_fuse b%d' % i] = (lambda terms=terms, H=H: ops.hrnet_fuse(terms, (H, H)), nbytes([t for t, _ in terms]) + nbytes([out]),
                                          dict(shape=shape, terms=ks))
        variants['torch upsample+add+relu b%d' % i] = (torch_route, nbytes([t for t, _ in terms]) + nbytes([out]), dict(shape=shape, terms=ks))
        variants['hrnet_fuse_bwd b%d' % i] = (lambda dy=dy, out=out, K=K: ops.hrnet_fuse_bwd(dy, out, K),
                                              nbytes([dy, out, gg, part.part]) + nbytes(pools), dict(shape=shape, K=K))
    C = 256
    x, x2 = torch.randn((N, S, S, C), generator=g).cuda(), torch.randn((N, S, S, C), generator=g).cuda()
    a, b = torch.randn((N, C), generator=g).cuda(), torch.randn((N, C), generator=g).cuda()
    yo = torch.empty_like(x)
    variants['gn_apply2'] = (lambda: ops.gn_apply2(x, a, b, x2, a, b, out=yo), 3 * nbytes([x]), dict(shape=[N, S, S, C]))
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
    rows = []
    yard = None
    for k, (_, moved, info) in variants.items():
        ms = statistics.median(times[k])
        rows.append(dict(op=k, bytes_moved=moved, gb_moved=round(moved / 1e9, 4), ms_median=round(ms, 4), ms_min=round(min(times[k]), 4),
                         ms_max=round(max(times[k]), 4), tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3), **info))
        if k == 'gn_apply2':
            yard = rows[-1]['tb_per_s']
    for r in rows:
        r['rate_vs_gn_apply2'] = round(r['tb_per_s'] / yard, 3)
        print(json.dumps(r), flush=True)
    return rows


def build(hrnet):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(50, 1)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=STRIDES)
    if hrnet:
        cfg['backbone'] = dict(type='HRNet', extra=W32_EXTRA)
        cfg['neck'] = dict(type='HRFPN', in_channels=WIDTHS, out_channels=256, num_outs=3)
        sd = synthetic.hrnet_state_dict(W32_EXTRA, 3, prefix='backbone.')
        sd.update(synthetic.hrfpn_state_dict(WIDTHS, 256, 3, 4))
        sd.update(synthetic.p2p_head_state_dict(1, seed=6, std=0.05))
    else:
        cfg['neck'] = dict(cfg['neck'], num_outs=3)
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
    models = {'R50+FPN': build(False), 'HRNetV2p-W32+HRFPN': build(True)}
    rows, trainers = [], {}
    for mode in ('forward_loss', 'train_step'):
        if mode == 'train_step':
            trainers = {k: P2PTrainer(m, optimizer=dict(type='Adam', lr=1e-4), max_norm=35.0) for k, m in models.items()}
        times = {k: [] for k in models}
        for i in range(args.warmup + args.steps):
            for k, m in models.items():       # the two models alternate step by step
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == 'train_step':
                    out = trainers[k].train_step(dict(data))
                    assert all(v == v and abs(v) < float('inf') for v in out['log_vars'].values()), out['log_vars']
                else:
                    with torch.no_grad():
                        m.forward_train(**data)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        for k in models:
            med = statistics.median(times[k])
            rows.append(dict(model=k, compute='fp32', mode=mode, ms_median=round(med, 2), ms=[round(v, 2) for v in times[k]],
                             img_per_s=round(args.batch * 1e3 / med, 1)))
            print(json.dumps(rows[-1]), flush=True)
    # the exchange kernels' share of the HRNet training step
    step_ms = rows[-1]['ms_median']
    events = {'hrnet_fuse': [], 'hrnet_fuse_bwd': []}
    real = {k: getattr(ops, k) for k in events}

    def bracket(name):
        def fn(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = real[name](*a, **kw)
            e.record()
            events[name].append((s, e))
            return r
        return fn
    for k in events:
        setattr(ops, k, bracket(k))
    try:
        for _ in range(args.share_steps):
            trainers['HRNetV2p-W32+HRFPN'].train_step(dict(data))
        torch.cuda.synchronize()
    finally:
        for k in events:
            setattr(ops, k, real[k])
    share = {}
    for k, ev in events.items():
        ms = sum(s.elapsed_time(e) for s, e in ev) / args.share_steps
        share[k] = dict(launches_per_step=len(ev) // args.share_steps, ms_per_step=round(ms, 3), share_of_step=round(ms / step_ms, 4))
    print(json.dumps(share), flush=True)
    return rows, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--side', type=int, default=160)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--gts', type=int, default=32)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--share-steps', type=int, default=3)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-locator', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch,
               kernel=dict(method='device events around %d back-to-back launches, variants alternating, median of %d rounds; bytes = what '
                           'the algorithm must move' % (args.launches, args.reps), rows=bench_kernel(args)))
    if not args.skip_locator:
        rows, share = bench_locator(args)
        res['locator'] = dict(workload='BasicLocator(P2PHead C=1), %dx%d, B=%d, %d gts/image, strides %s, fp32: ResNet-50 + FPN(num_outs=3) '
                              'against HRNetV2p-W32 + HRFPN(num_outs=3); train_step: P2PTrainer, Adam'
                              % (args.size, args.size, args.batch, args.gts, STRIDES),
                              method='host clock around a step ending in a device synchronise, models alternating, median of %d steps '
                              'after %d warm-up steps' % (args.steps, args.warmup), rows=rows,
                              exchange_share=dict(method='device-event brackets around every exchange launch in %d further steps, summed per '
                                                  'step, over the unbracketed train_step median' % args.share_steps, **share))
    res['not_measured'] = ['the bf16 compute mode (refused for HRNet)', 'CprTrainer at full size', 'hardware counters of the two kernels',
                           'multi-GPU training']
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
