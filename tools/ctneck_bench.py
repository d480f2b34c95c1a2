"""What the transposed-conv kernel and the CTResNetNeck cost (writes profiles/ctneck_bench.json with --out; needs the GPU):
  python tools/ctneck_bench.py --out profiles/ctneck_bench.json

1. ops.deconv4x4s2 (csrc/deconv.hip) and its two gradients (the dense-conv entries with the roles swapped) at the three stages of
   CTResNetNeck(512, (256, 128, 64)) behind a ResNet-18 at B = 16, 640^2 -- 16 x 20^2 x 256, 16 x 40^2 x 128, 16 x 80^2 x 64 -- beside the
   COMPOSED route, what the project could assemble before from public ops, as ops.PhasedDgrad assembles a stride-2 data gradient: per
   output-parity class a 2x2 / padding 1 sub-convolution, and cpr_phase_scatter_add to the strided positions (forward); the adjoint of
   that, class by class, for the gradients (a zero-embedded copy of the class's gradient pixels -- two torch passes per class, timed
   with the route: it cannot run without them -- then the sub-convolution's data / weight gradient; the weight gradient is timed up to its
   four (Cout, Cin, 2, 2) pieces, their placement into (Cin, Cout, 4, 4) is not).  Both routes are checked against each other first.
   Device events around --launches back-to-back launches; the launches walk a ring of R sets of EVERY large map a variant touches (x, the
   doubled output, dy), R chosen so that R * (|x| + |out|) exceeds the 256 MB Infinity Cache (``ring_mb``): no launch finds a map it
   touched before in cache; the variants alternate within each of --reps rounds, the median round is
   reported with the spread of the rounds.  TFLOP/s: the multiply-adds the fused kernel executes, 2 * N*H*W * 4 * Cout * 4*Cin.
   ops.gn_apply2 on the neck's 16 x 160^2 x 64 output map is timed in the same rounds (the project's streaming yardstick).
2. Whole model, BasicLocator(R18, .., C=1), 640 x 640, B = 16, strides=[4]: CTResNetNeck + P2PHead and + CPRHead (in_channels 64) against
   FPN(num_outs=1) + the same head (in_channels 256) -- forward + loss (forward_train under no_grad) and the trainer's train_step.  Host
   clock around a step that ends in a device synchronise; the models alternate step by step, medians over --steps after --warmup."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(20, 256), (40, 128), (80, 64)]
NECK = dict(type='CTResNetNeck', in_channel=512, num_deconv_filters=(256, 128, 64), num_deconv_kernels=(4, 4, 4), use_dcn=False)
RING_BYTES = 320 << 20


class Composed:
    """The four-sub-convolution route over one weight (Cin, Cout, 4, 4)."""

    def __init__(self, w):
        from pointtinybenchmark_amd import ops
        self.Cin, self.Cout = w.shape[:2]
        self.classes = []
        for a in range(2):
            for b in range(2):
                khs, kws = [3 - a, 1 - a], [3 - b, 1 - b]
                sub = w[:, :, khs][:, :, :, kws].permute(1, 0, 2, 3).contiguous()      # (Cout, Cin, 2, 2); class (a, b) is out[i + a, j + b]
                self.classes.append((a, b, khs, kws, sub, ops.PackedConv(sub, 1, 1), ops.PackedConv.for_dgrad(sub, 1)))

    def forward(self, x, y):
        from pointtinybenchmark_amd import _lib, ops
        N, H, W, _ = x.shape
        y.zero_()
        for a, b, _, _, _, pc, _ in self.classes:
            o = ops.conv2d(x, pc)
            _lib.call('cpr_phase_scatter_add', ops._ptr(o), ops._ptr(y), N, H + 1, W + 1, self.Cout, 2 * H, 2 * W, a, b, a, b, 2, ops._stream())
        return y

    def _embedded(self, dy, a, b):
        import torch
        N, H2, W2, C = dy.shape
        d = torch.zeros((N, H2 // 2 + 1, W2 // 2 + 1, C), device=dy.device, dtype=dy.dtype)
        d[:, a:a + H2 // 2, b:b + W2 // 2] = dy[:, a::2, b::2]
        return d

    def dgrad(self, dy):
        from pointtinybenchmark_amd import ops
        N, H2, W2, _ = dy.shape
        dx = None
        for a, b, _, _, _, _, pt in self.classes:
            dx = ops.conv2d_dgrad(self._embedded(dy, a, b), pt, (H2 // 2, W2 // 2), 1, add=dx)
        return dx

    def wgrad(self, dy, x):
        """-> the four sub-convolutions' weight gradients (Cout, Cin, 2, 2), one per class; ``assemble`` places them."""
        from pointtinybenchmark_amd import ops
        return [ops.conv2d_wgrad(self._embedded(dy, a, b), x, tuple(sub.shape), 1, 1) for a, b, _, _, sub, _, _ in self.classes]

    def assemble(self, gs, out):
        """The (Cin, Cout, 4, 4) gradient from ``wgrad``'s four pieces (not timed: sixteen tiny strided copies)."""
        for (_, _, khs, kws, _, _, _), g in zip(self.classes, gs):
            g = g.permute(1, 0, 2, 3)
            for r, kh in enumerate(khs):
                for s, kw in enumerate(kws):
                    out[:, :, kh, kw] = g[:, :, r, s]
        return out


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def bench_kernels(args):
    import torch
    from pointtinybenchmark_amd import ops
    rows = []
    N = args.batch
    g = torch.Generator().manual_seed(1)
    ya = torch.randn((N, 160, 160, 64), generator=g).cuda()
    yb, yo = torch.randn((N, 160, 160, 64), generator=g).cuda(), torch.empty((N, 160, 160, 64)).cuda()
    ab = torch.randn((N, 64), generator=g).cuda()
    for S, C in SHAPES:
        w = (torch.randn((C, C, 4, 4), generator=g) * (4 * C) ** -0.5).cuda()
        per = (N * S * S * C + N * 4 * S * S * C) * 4
        R = max(2, -(-RING_BYTES // per))
        xs = [torch.randn((N, S, S, C), generator=g).cuda() for _ in range(R)]
        dys = [torch.randn((N, 2 * S, 2 * S, C), generator=g).cuda() for _ in range(R)]
        outs = [torch.empty((N, 2 * S, 2 * S, C)).cuda() for _ in range(R)]      # ringed too: a forward launch touches x AND out
        gw = [torch.empty((C, C, 4, 4)).cuda() for _ in range(2)]
        pack, pdg, comp = ops.DeconvPack(w), ops.deconv4x4s2_dgrad_pack(w), Composed(w)
        agree = dict(forward=rel(comp.forward(xs[0], outs[1]), ops.deconv4x4s2(xs[0], pack, out=outs[0])),
                     dgrad=rel(comp.dgrad(dys[0]), ops.conv2d(dys[0], pdg)),
                     wgrad=rel(comp.assemble(comp.wgrad(dys[0], xs[0]), gw[1]), ops.deconv4x4s2_wgrad(dys[0], xs[0], tuple(w.shape), out=gw[0])))
        assert max(agree.values()) < 1e-5, agree
        variants = {'forward fused': lambda i: ops.deconv4x4s2(xs[i % R], pack, out=outs[i % R]),
                    'forward composed': lambda i: comp.forward(xs[i % R], outs[i % R]),
                    'dgrad fused': lambda i: ops.conv2d(dys[i % R], pdg),
                    'dgrad composed': lambda i: comp.dgrad(dys[i % R]),
                    'wgrad fused': lambda i: ops.deconv4x4s2_wgrad(dys[i % R], xs[i % R], tuple(w.shape), out=gw[0]),
                    'wgrad composed': lambda i: comp.wgrad(dys[i % R], xs[i % R]),
                    'gn_apply2': lambda i: ops.gn_apply2(ya, ab, ab, yb, ab, ab, out=yo)}
        for fn in variants.values():
            for i in range(3):
                fn(i)
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for i in range(args.launches):
                    fn(i)
                e.record()
                torch.cuda.synchronize()
                times[k].append(s.elapsed_time(e) / args.launches)
        flop = 2.0 * N * S * S * 4 * C * 4 * C
        for k in variants:
            ms = statistics.median(times[k])
            row = dict(op=k, shape=[N, S, S, C], cout=C, ring_sets=R, ring_mb=round(R * per / 2 ** 20, 1), ms_median=round(ms, 4),
                       ms_min=round(min(times[k]), 4), ms_max=round(max(times[k]), 4))
            if k == 'gn_apply2':
                row.update(shape=[N, 160, 160, 64], ring_sets=1, ring_mb=round(3 * ya.numel() * 4 / 2 ** 20, 1),
                           tb_per_s=round(3 * ya.numel() * 4 / (ms * 1e-3) / 1e12, 3))
            elif k.endswith('fused'):
                row['tflops_executed'] = round(flop / (ms * 1e-3) / 1e12, 2)
            rows.append(row)
        by = {r['op']: r for r in rows[-len(variants):]}
        for kind in ('forward', 'dgrad', 'wgrad'):
            f, c = by[kind + ' fused'], by[kind + ' composed']
            f['composed_over_fused'] = round(c['ms_median'] / f['ms_median'], 3)
            f['routes_rel_l2'] = agree[kind]
        for r in by.values():
            print(json.dumps(r), flush=True)
        del variants, xs, dys, outs, comp
        torch.cuda.empty_cache()
    return rows


def build(neck, head):
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(18, 1) if head == 'p2p' else model_cfg(18, 1)
    ct = neck == 'CTResNetNeck'
    if ct:
        cfg['neck'] = dict(NECK)
        cfg['bbox_head'] = dict(cfg['bbox_head'], in_channels=64)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4])
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(18, 1, 0, head, 3, **(dict(head_std=0.05) if head == 'p2p' else dict(head_std=0.3)))
    if ct:
        sd = {k: (v[:, :64].contiguous() if k.endswith('_convs.0.conv.weight') else v) for k, v in sd.items() if not k.startswith('neck.')}
        sd.update(synthetic.ctneck_state_dict(512, (256, 128, 64), 4))
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def bench_locator(args):
    import torch
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    batch = synthetic.synthetic_batch(args.batch, args.size, args.size, args.gts, 1, seed=61)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    rows = []
    for head, Trainer in (('p2p', P2PTrainer), ('cpr', CprTrainer)):
        models = {'FPN': build('FPN', head), 'CTResNetNeck': build('CTResNetNeck', head)}
        trainers = {}
        for mode in ('forward_loss', 'train_step'):
            if mode == 'train_step':
                trainers = {k: Trainer(m, optimizer=dict(type='Adam', lr=1e-5), max_norm=35.0) for k, m in models.items()}
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
                rows.append(dict(neck=k, head=head, mode=mode, ms_median=round(med, 2), ms=[round(v, 2) for v in times[k]],
                                 img_per_s=round(args.batch * 1e3 / med, 1)))
                print(json.dumps(rows[-1]), flush=True)
            rows[-1]['delta_vs_fpn_ms'] = round(rows[-1]['ms_median'] - rows[-2]['ms_median'], 2)
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
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-locator', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), batch=args.batch,
               kernel=dict(method='device events around %d back-to-back launches walking a ring of ring_sets sets of every large map a variant touches '
                           '(x and the doubled output: ring_mb MiB together; dy: 4/5 of that), each ring > the 256 MB Infinity Cache; the composed '
                           'weight gradient is timed up to its four 2x2 pieces; variants alternating, median / min / max of %d rounds; tflops_executed = 2 N H W 4 Cout 4 Cin / '
                           'time; gn_apply2 reads two 16 x 160^2 x 64 maps and writes one (a working set of 300 MiB, larger than the '
                           'cache too)' % (args.launches, args.reps), rows=bench_kernels(args)))
    if not args.skip_locator:
        res['locator'] = dict(workload='BasicLocator(R18, head C=1), %dx%d, B=%d, %d gts/image, strides [4]; FPN(num_outs=1, 256 channels) '
                              'against CTResNetNeck(512, (256, 128, 64)) (64 channels); train_step: the native trainer, Adam'
                              % (args.size, args.size, args.batch, args.gts),
                              method='host clock around a step ending in a device synchronise, necks alternating, median of %d steps '
                              'after %d warm-up steps' % (args.steps, args.warmup), rows=bench_locator(args))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
