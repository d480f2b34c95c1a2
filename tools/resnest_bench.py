"""What the split-attention kernels (csrc/splat.hip) and the block-diagonal dense conv2 cost, and the ResNeSt-50 forward and training step
beside R50 and x50_32x4d, all lines in the same run:

  kernels    the six kernels at every launch shape of ResNeSt-50 at 640 x 640, B = 64 (per stage the unpooled block, and from layer2 on the
             pooled first block whose conv2 runs on the 2x map): time per launch and, for the four map kernels, achieved TB/s over the
             bytes they must move (u read once, the gradient / output maps once) -- beside gn_apply (one read, one write) and
             relu_bwd_colsum (two reads, one write) on a map of u's size.
  conv2      the dense w -> 2w 3x3 (block-diagonal pack) forward with scale / bias / ReLU, data gradient and dense weight gradient,
             beside R50's conv2 (w -> w) of the same stage and map.
  locators   BasicLocator(backbone, FPN, CPRHead) at 640^2, B = 64, frozen_stages=1: forward + loss img/s and full training-step img/s
             (CprTrainer) with R50, x50_32x4d and ResNeSt-50.

Device-event medians, alternating over two sets of maps.  Prints one JSON object (--out FILE also writes it: profiles/resnest_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.resnext_bench import med, timed  # noqa: E402


def block_shapes(size):
    """(stage, H, w, pool) of every distinct split-attention launch shape on a size x size image (H = conv2's map)."""
    out = []
    for i in range(4):
        w, H = 64 * 2 ** i, size // 4 // 2 ** i
        if i > 0:
            out.append((i + 1, 2 * H, w, True))
        out.append((i + 1, H, w, False))
    return out


def _run(lines, args):
    ts = {k: [] for k in lines}
    for it in range(args.warmup + args.iters):
        for k, fn in lines.items():
            t = timed(lambda: fn(it % 2))
            if it >= args.warmup:
                ts[k].append(t)
    return {k: med(v) for k, v in ts.items()}


def bench_kernels(args):
    import torch
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.backbones.resnest import inter_channels
    B = args.batch
    recs = []
    for stage, H, w, pool in block_shapes(args.size):
        OH = (H - 1) // 2 + 1 if pool else H
        inter = inter_channels(w)
        gen = torch.Generator(device='cuda').manual_seed(stage * 10 + pool)

        def rn(*s):
            return torch.randn(s, device='cuda', generator=gen)
        sets = [dict(u=torch.relu(rn(B, H, H, 2 * w)), dout=rn(B, OH, OH, w), big=rn(B, H, H, 2 * w), out=torch.empty((B, H, H, 2 * w), device='cuda'))
                for _ in range(2)]
        fc1_w, fc1_b, fc2_w, fc2_b = rn(inter, w, 1, 1) * 0.05, rn(inter) * 0.1, rn(2 * w, inter, 1, 1) * 0.05, rn(2 * w) * 0.1
        s1, t1, mean, inv = torch.rand((inter,), device='cuda') + 0.5, rn(inter) * 0.1, rn(inter) * 0.1, torch.rand((inter,), device='cuda') + 0.5
        a, b = torch.rand((B, 2 * w), device='cuda') + 0.5, rn(B, 2 * w)
        g = ops.splat_gap(sets[0]['u'])
        att, z = ops.splat_attn(g, fc1_w, fc1_b, s1, t1, fc2_w, fc2_b, record=True)
        datt, dg = rn(B, 2, w), rn(B, w)
        grads = dict(fc1_w=torch.empty_like(fc1_w), fc1_b=torch.empty_like(fc1_b), bn_w=torch.empty_like(s1), bn_b=torch.empty_like(s1),
                     fc2_w=torch.empty_like(fc2_w), fc2_b=torch.empty_like(fc2_b))
        lines = {
            'splat_gap': lambda i: ops.splat_gap(sets[i]['u']),
            'splat_attn': lambda i: ops.splat_attn(g, fc1_w, fc1_b, s1, t1, fc2_w, fc2_b, record=True),
            'splat_apply': lambda i: ops.splat_apply(sets[i]['u'], att, pool=pool),
            'splat_attn_grad': lambda i: ops.splat_attn_grad(sets[i]['dout'], sets[i]['u'], pool=pool),
            'splat_attn_bwd': lambda i: ops.splat_attn_bwd(att, datt, z, g, fc1_w, fc1_b, s1, mean, inv, fc2_w, grads=grads),
            'splat_apply_bwd': lambda i: ops.splat_apply_bwd(sets[i]['dout'], sets[i]['u'], att, dg, pool=pool),
            'gn_apply': lambda i: ops.gn_apply(sets[i]['big'], a, b, out=sets[i]['out']),
            'relu_bwd_colsum': lambda i: ops.relu_bwd_colsum(sets[i]['big'], sets[i]['u']),
        }
        res = _run(lines, args)
        m_u, m_o = 4.0 * B * H * H * 2 * w, 4.0 * B * OH * OH * w
        nbytes = dict(splat_gap=m_u, splat_apply=m_u + m_o, splat_attn_grad=m_u + m_o, splat_apply_bwd=2 * m_u + m_o, gn_apply=2 * m_u,
                      relu_bwd_colsum=3 * m_u)
        for k, nb in nbytes.items():
            res[k].update(bytes=nb, TB_per_s=nb / res[k]['ms'] / 1e9)
        recs.append(dict(stage=stage, u=[B, H, H, 2 * w], pool=pool, inter=inter, **res))
        del sets
        torch.cuda.empty_cache()
    return recs


def bench_conv2(args):
    import torch
    from pointtinybenchmark_amd import ops
    B = args.batch
    recs = []
    for stage, H, w, pool in block_shapes(args.size):
        gen = torch.Generator(device='cuda').manual_seed(stage * 10 + pool + 100)

        def rn(*s):
            return torch.randn(s, device='cuda', generator=gen)
        xs = [rn(B, H, H, w) for _ in range(2)]
        rec = dict(stage=stage, map=[B, H, H, w], pool=pool)
        for name, cout, wt in (('resnest', 2 * w, ops.splat_dense_weight(rn(2 * w, w // 2, 3, 3) * 0.05)), ('r50', w, rn(w, w, 3, 3) * 0.05)):
            sc, bi = torch.rand((cout,), device='cuda') + 0.5, rn(cout)
            dys = [rn(B, H, H, cout) for _ in range(2)]
            pc, pt = ops.PackedConv(wt, 1, 1), ops.dgrad_pack(wt, 1, 1, scale=sc)
            lines = {
                'fwd': lambda i: ops.conv2d(xs[i], pc, scale=sc, bias=bi, relu=True),
                'dgrad': lambda i: ops.conv2d_dgrad(dys[i], pt, (H, H), 1),
                'wgrad': lambda i: ops.conv2d_wgrad(dys[i], xs[i], tuple(wt.shape), 1, 1),
            }
            res = _run(lines, args)
            flop = 2.0 * B * H * H * cout * w * 9
            for k in res:
                res[k].update(executed_TFLOPs=flop / res[k]['ms'] / 1e9)
            rec[name] = res
            del dys
        rec['ratio_to_r50'] = {k: rec['resnest'][k]['ms'] / rec['r50'][k]['ms'] for k in ('fwd', 'dgrad', 'wgrad')}
        recs.append(rec)
        del xs
        torch.cuda.empty_cache()
    return recs


BACKBONES = {'r50': dict(type='ResNet'), 'x50_32x4d': dict(type='ResNeXt', groups=32, base_width=4), 'resnest50': dict(type='ResNeSt')}


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
        cfg = model_cfg(50, 1)
        cfg['backbone'] = dict(cfg['backbone'], frozen_stages=1, **kw)
        m = P.build_detector(cfg).cuda()
        if kw['type'] == 'ResNeSt':
            sd = {k: v for k, v in synthetic.locator_state_dict(50, 1, 0, 'cpr', 0).items() if not k.startswith('backbone.')}
            sd.update(synthetic.resnest_state_dict(50, 0))
        else:
            sd = synthetic.locator_state_dict(50, 1, 0, 'cpr', 0, **{k: v for k, v in kw.items() if k != 'type'})
        m.load_state_dict(sd, strict=True)
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
    for name in ('x50_32x4d', 'resnest50'):
        out['backbones'][name]['ratio_to_r50'] = {k: out['backbones'][name][k]['ms'] / out['backbones']['r50'][k]['ms']
                                                  for k in ('forward_loss', 'train_step')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--parts', default='kernels,conv2,locators')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('resnest_bench.py measures on the GPU; none is visible')
    result = dict(iters=args.iters, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    for part, fn in (('kernels', bench_kernels), ('conv2', bench_conv2), ('locators', bench_locators)):
        if part in args.parts.split(','):
            result[part] = fn(args)
            if args.out:        # (kept as it grows: a later part that fails leaves the earlier ones on disk)
                with open(args.out, 'w') as f:
                    f.write(json.dumps(result) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
