"""What the native Adam step costs (csrc/optim.hip, ``CprTrainer(optimizer=dict(type='Adam', ...))``).

  --mode kernels  clip-norm + Adam (``cpr_grad_sumsq`` + ``cpr_adam_step``) and the SGD step (``cpr_sgd_step``) on flat fp32
                  buffers of the R50 P2P trainable size, rotating over > 1 GiB of distinct buffer sets so that the 256 MiB
                  Infinity Cache cannot serve re-reads; device-event time per launch (median) and TB/s at 28 B
                  (Adam: reads p, g, m, v, writes p, m, v) and 20 B (SGD: reads p, g, buf, writes p, buf) per parameter.  Next to
                  them torch.optim.Adam (foreach=True, and fused=True when the installed torch takes it) over the model's
                  trainable tensors.  Run it alone under ``rocprofv3 --kernel-trace --stats`` for the per-kernel table.
  --mode step     P2PTrainer R50 640x640 B=--batch (BASELINE.json configs[3]): the SGD step against the Adam step, fp32 and bf16,
                  alternating the two every round; per-round medians and the spread over rounds.
Every mode prints one JSON object (--out FILE also writes it)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trainable_shapes(depth=50):
    """Shapes of the trainable tensors of the P2P model (built on the CPU: no kernel runs)."""
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    model = P.build_detector(p2p_model_cfg(depth))
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


def _events_ms(fn, iters):
    import torch
    times = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def kernels_mode(args):
    import torch
    from pointtinybenchmark_amd import ops
    shapes = trainable_shapes()
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    sets = []
    for k in range(args.sets):      # Adam: 4 buffers of n floats per set
        g = torch.Generator(device='cuda').manual_seed(k)
        sets.append(dict(p=torch.randn(n, device='cuda', generator=g), g=torch.randn(n, device='cuda', generator=g) * 1e-2,
                         m=torch.zeros(n, device='cuda'), v=torch.zeros(n, device='cuda')))
    norm2 = torch.zeros((1,), device='cuda', dtype=torch.float64)
    ws = torch.empty((1024,), device='cuda', dtype=torch.float64)
    step = [0]

    def adam(i, clip):
        s = sets[i % len(sets)]
        if clip:
            ops.grad_sumsq(s['g'], norm2, ws, accumulate=False)
        step[0] += 1
        ops.adam_step(s['p'], s['g'], s['m'], s['v'], norm2, 1e-4, (0.9, 0.999), 1e-8, 0.0, step[0], 35.0 if clip else 0.0, 1.0)

    def sgd(i):
        s = sets[i % len(sets)]
        ops.sgd_step(s['p'], s['g'], s['m'], norm2, 1e-4, 0.9, 1e-4, 0.0, 1.0, first=False)

    def sumsq(i):
        ops.grad_sumsq(sets[i % len(sets)]['g'], norm2, ws, accumulate=False)

    res = dict(params=n, tensors=len(shapes), sets=args.sets, rotated_gib=round(args.sets * 16 * n / 2 ** 30, 2),
               iters=args.iters, cases={})
    for name, fn, bpp in (('adam_step', lambda i: adam(i, False), 28), ('sgd_step', sgd, 20), ('grad_sumsq', sumsq, 4),
                          ('grad_sumsq+adam_step', lambda i: adam(i, True), 32)):
        _events_ms(fn, 2 * args.sets)                          # warm-up
        t = sorted(_events_ms(fn, args.iters))
        med = statistics.median(t)
        res['cases'][name] = dict(ms_median=round(med, 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4),
                                  bytes_per_param=bpp, mbytes=round(bpp * n / 1e6, 1), tbps=round(bpp * n / med / 1e9, 2))
    # torch.optim.Adam over the model's trainable tensors (one set: 169 tensors, > 256 MiB per step)
    g = torch.Generator(device='cuda').manual_seed(99)
    params = [torch.randn(s, device='cuda', generator=g).requires_grad_(True) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 1e-2
    for kw in (dict(foreach=True), dict(fused=True)):
        key = 'torch_adam_' + next(iter(kw))
        try:
            opt = torch.optim.Adam(params, lr=1e-4, **kw)
            _events_ms(lambda i: opt.step(), 3)
        except (RuntimeError, ValueError) as e:
            res['cases'][key] = dict(unsupported=str(e)[:200])
            continue
        t = sorted(_events_ms(lambda i: opt.step(), args.iters))
        med = statistics.median(t)
        res['cases'][key] = dict(ms_median=round(med, 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4),
                                 tbps_at_28B=round(28 * n / med / 1e9, 2))
    return res


def step_mode(args):
    import torch
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import P2PTrainer
    batch = synthetic.synthetic_batch(args.batch, 640, 640, 30, 1, seed=0)
    img = batch['img'].cuda()
    gtb = [b.cuda() for b in batch['gt_bboxes']]
    gtl = [l.cuda() for l in batch['gt_labels']]
    metas = batch['img_metas']
    res = dict(batch=args.batch, steps_per_round=args.steps, rounds=args.rounds, modes={})
    for dtype in ('fp32', 'bf16'):
        trainers = {}
        for kind, opt in (('sgd', dict(type='SGD', lr=1e-4, momentum=0.9, weight_decay=1e-4)), ('adam', dict(type='Adam', lr=1e-4))):
            model = P.build_detector(p2p_model_cfg(50)).cuda()
            model.load_state_dict(synthetic.locator_state_dict(50, 1, 0, 'p2p', 0, head_std=0.05), strict=True)
            model.train()
            model.set_compute_dtype(dtype)
            trainers[kind] = P2PTrainer(model, optimizer=opt, max_norm=35.0)

        def run(kind, k):
            tr = trainers[kind]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(k):
                tr.forward_backward(img, metas, gtb, gtl)
                tr.step()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / k
        for kind in trainers:
            run(kind, args.warmup)
        per = {kind: [] for kind in trainers}
        for r in range(args.rounds):
            for kind in (('sgd', 'adam') if r % 2 == 0 else ('adam', 'sgd')):
                per[kind].append(run(kind, args.steps))
        s, a = statistics.median(per['sgd']), statistics.median(per['adam'])
        ratios = [x / y for x, y in zip(per['adam'], per['sgd'])]
        res['modes'][dtype] = dict(sgd_ms=[round(x, 3) for x in per['sgd']], adam_ms=[round(x, 3) for x in per['adam']],
                                   sgd_median_ms=round(s, 3), adam_median_ms=round(a, 3),
                                   adam_over_sgd_median=round(a / s, 4),
                                   adam_over_sgd_round_range=[round(min(ratios), 4), round(max(ratios), 4)],
                                   sgd_round_spread=round((max(per['sgd']) - min(per['sgd'])) / s, 4),
                                   img_per_s=dict(sgd=round(args.batch * 1e3 / s, 1), adam=round(args.batch * 1e3 / a, 1)))
        del trainers
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['kernels', 'step'], required=True)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'optim_bench measures on the GPU'
    res = dict(mode=args.mode, device=torch.cuda.get_device_name(0))
    res.update(kernels_mode(args) if args.mode == 'kernels' else step_mode(args))
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
