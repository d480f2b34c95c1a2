"""What a RegNetX backbone costs next to R50 and x50_32x4d, all lines in the same run:

  locators   BasicLocator(backbone, FPN, CPRHead) at 640^2, B = 64: forward + loss img/s and full training-step img/s with R50,
             x50_32x4d, regnetx_800mf (group width 16, no padded map) and regnetx_3.2gf (group width 48, stages 3 - 4 at a padded pitch),
             every backbone with frozen_stages=1.
  layers     the stride-1 grouped 3x3 layer of every stage of regnetx_800mf (cg 16) and regnetx_3.2gf (cg 48) at 640 x 640, B = 64, at
             the pitch the backbone keeps it at -- forward (scale / bias / ReLU), data gradient, weight gradient: time per launch and
             executed TFLOP/s (2 * 9 * cg FMAs per output).
  stem       the 3x3 / 2 stem conv 3 -> 32 (+ BN + ReLU) forward in both input layouts and its weight gradient, B = 64 at 640^2.

Nothing here replaces an existing path: the comparison is the other backbones on the same box, never a target.  Device-event medians.
Prints one JSON object (--out FILE also writes it: profiles/regnet_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.resnext_bench import med, timed  # noqa: E402

BACKBONES = {'r50': dict(type='ResNet', depth=50), 'x50_32x4d': dict(type='ResNeXt', depth=50, groups=32, base_width=4),
             'regnetx_800mf': dict(type='RegNet', arch='regnetx_800mf'), 'regnetx_3.2gf': dict(type='RegNet', arch='regnetx_3.2gf')}


def bench_layers(args):
    import torch
    from pointtinybenchmark_amd import ops
    from pointtinybenchmark_amd.backbones.regnet import RegNet, stage_layout
    B, recs = args.batch, []
    for arch in ('regnetx_800mf', 'regnetx_3.2gf'):
        widths, gws, _ = stage_layout(RegNet.arch_settings[arch])
        for i, (C, cg) in enumerate(zip(widths, gws)):
            H = args.size // 4 // 2 ** i
            Cp, G = ops.pad32(C), C // cg
            gen = torch.Generator(device='cuda').manual_seed(10 * i + cg)
            maps = [(torch.randn((B, H, H, Cp), device='cuda', generator=gen), torch.randn((B, H, H, Cp), device='cuda', generator=gen))
                    for _ in range(2)]
            w = torch.randn((C, cg, 3, 3), device='cuda', generator=gen) * 0.05
            s, b = torch.rand((C,), device='cuda') + 0.5, torch.randn((C,), device='cuda')
            pc, pt = ops.PackedConv(w, 1, 1, groups=G, pitch=Cp), ops.dgrad_pack(w, 1, 1, scale=s, groups=G, pitch=Cp)
            lines = {'fwd': lambda j: ops.conv2d(maps[j][0], pc, scale=s, bias=b, relu=True),
                     'dgrad': lambda j: ops.conv2d_dgrad(maps[j][1], pt, (H, H), 1),
                     'wgrad': lambda j: ops.conv2d_wgrad(maps[j][1], maps[j][0], (C, cg, 3, 3), 1, 1, groups=G)}
            ts = {k: [] for k in lines}
            for it in range(args.warmup + args.iters):
                for k, fn in lines.items():
                    t = timed(lambda: fn(it % 2))
                    if it >= args.warmup:
                        ts[k].append(t)
            flop = 2.0 * B * H * H * C * cg * 9
            rec = dict(arch=arch, stage=i + 1, map=[B, H, H, C], pitch=Cp, group_width=cg, groups=G, flop=flop)
            for k in lines:
                rec[k] = dict(med(ts[k]), executed_TFLOPs=flop / statistics.median(ts[k]) / 1e9)
            recs.append(rec)
            del maps
            torch.cuda.empty_cache()
    return recs


def bench_stem(args):
    import torch
    from pointtinybenchmark_amd import ops
    B, S = args.batch, args.size
    gen = torch.Generator(device='cuda').manual_seed(5)
    x = torch.randn((B, 3, S, S), device='cuda', generator=gen)
    x4 = ops.nchw_to_nhwc(x)
    w = torch.randn((32, 3, 3, 3), device='cuda', generator=gen) * 0.2
    s, b = torch.rand((32,), device='cuda') + 0.5, torch.randn((32,), device='cuda')
    pc = ops.PackedConv(w, 2, 1)
    dy = torch.randn((B, S // 2, S // 2, 32), device='cuda', generator=gen)
    lines = {'fwd_planar': lambda: ops.stem3x3s2(x, pc, s, b, planar=True), 'fwd_nhwc4': lambda: ops.stem3x3s2(x4, pc, s, b, planar=False),
             'wgrad_planar': lambda: ops.stem3x3s2_wgrad(dy, x, planar=True), 'wgrad_nhwc4': lambda: ops.stem3x3s2_wgrad(dy, x4, planar=False)}
    ts = {k: [] for k in lines}
    for it in range(args.warmup + args.iters):
        for k, fn in lines.items():
            t = timed(fn)
            if it >= args.warmup:
                ts[k].append(t)
    flop = 2.0 * B * (S // 2) ** 2 * 32 * 27
    nbytes = dict(fwd_planar=x.numel() * 4 + dy.numel() * 4, fwd_nhwc4=x4.numel() * 4 + dy.numel() * 4,
                  wgrad_planar=x.numel() * 4 + dy.numel() * 4, wgrad_nhwc4=x4.numel() * 4 + dy.numel() * 4)
    return dict(shape=[B, 3, S, S], flop=flop,
                **{k: dict(med(ts[k]), TFLOPs=flop / statistics.median(ts[k]) / 1e9, bytes=nbytes[k], GBps=nbytes[k] / statistics.median(ts[k]) / 1e6)
                   for k in lines})


def bench_locators(args):
    import torch
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.backbones.regnet import RegNet, stage_layout
    from pointtinybenchmark_amd.training import CprTrainer
    B, S = args.batch, args.size
    batch = synthetic.synthetic_batch(B, S, S, 32, 1, seed=123)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    out = dict(shape=[B, 3, S, S], backbones={})
    for name, kw in BACKBONES.items():
        cfg = model_cfg(50, 1)
        if kw['type'] == 'RegNet':
            keep = {k: cfg['backbone'][k] for k in ('out_indices', 'frozen_stages', 'norm_cfg', 'norm_eval', 'style')}
            cfg['backbone'] = dict(keep, **kw)
            cfg['neck'] = dict(cfg['neck'], in_channels=stage_layout(RegNet.arch_settings[kw['arch']])[0])
            sd = synthetic.locator_state_dict(num_classes=1, head='cpr', seed=0, arch=kw['arch'])
        else:
            extra = {k: v for k, v in kw.items() if k not in ('type', 'depth')}
            cfg['backbone'] = dict(cfg['backbone'], **kw)
            sd = synthetic.locator_state_dict(50, 1, 0, 'cpr', 0, **extra)
        m = P.build_detector(cfg).cuda()
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
    for name in ('x50_32x4d', 'regnetx_800mf', 'regnetx_3.2gf'):
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
    ap.add_argument('--parts', default='stem,layers,locators')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('regnet_bench.py measures on the GPU; none is visible')
    result = dict(iters=args.iters, steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    for part, fn in (('stem', bench_stem), ('layers', bench_layers), ('locators', bench_locators)):
        if part in args.parts.split(','):
            result[part] = fn(args)
            if args.out:        # (kept as it grows: a later part that fails leaves the earlier ones on disk)
                with open(args.out, 'w') as f:
                    f.write(json.dumps(result) + '\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
