"""Trainable stem (frozen_stages=-1): the two backward kernels of csrc/stem_bwd.hip at R50 640^2 B=64 (HIP events) and the native
training step with frozen_stages = -1 / 0 / 1 in fp32 and in the mixed-precision mode, plus the batch-statistics stem in fp32.

    python tools/stem_train_bench.py [--out profiles/stem_train_bench.json] [--part kernels|steps|all]

Kernel numbers: stem_pool_bwd in TB/s on its algorithmic bytes (pooled gradient + byte map read, dy written); stem_wgrad_f32 in
TFLOP/s on the 147-product count (2 * 64 * 147 * N * OH * OW) and as a fraction of the 157.3 TF fp32-MFMA peak."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pointtinybenchmark_amd as P  # noqa: E402
from pointtinybenchmark_amd import ops, synthetic  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def _events(fn, warmup=3, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def kernels(N=64, H=640, W=640):
    torch.manual_seed(0)
    x = torch.randn((N, 3, H, W), device='cuda')
    w = torch.randn((64, 3, 7, 7), device='cuda') * (2.0 / 147) ** 0.5
    scale, shift = torch.ones(64, device='cuda'), 0.1 * torch.randn(64, device='cuda')
    out, arg = ops.stem7x7s2_pool_f32(x, ops.stem_weight_f32(w), scale, shift, planar=True, record=True)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dp = torch.randn(out.shape, device='cuda')
    dy, _ = ops.stem_pool_bwd(dp, arg, (OH, OW))
    gw = torch.empty((64, 3, 7, 7), device='cuda')
    t_pool = _events(lambda: ops.stem_pool_bwd(dp, arg, (OH, OW)))
    res = {}
    for planar in (True, False):
        xin = x if planar else ops.nchw_to_nhwc(x)
        res['stem_wgrad_f32_ms_' + ('planar' if planar else 'nhwc4')] = _events(lambda: ops.stem_wgrad_f32(dy, xin, planar=planar, out=gw))
    pool_bytes = dp.numel() * 4 + arg.numel() + dy.numel() * 4
    flops = 2.0 * 64 * 147 * N * OH * OW
    t_w = res['stem_wgrad_f32_ms_planar']
    res.update(shape=[N, 3, H, W], stem_pool_bwd_ms=t_pool, stem_pool_bwd_tbps=pool_bytes / (t_pool * 1e-3) / 1e12,
               stem_pool_bwd_bytes=pool_bytes, stem_wgrad_f32_tflops=flops / (t_w * 1e-3) / 1e12,
               stem_wgrad_f32_frac_peak=flops / (t_w * 1e-3) / PEAK_F32_MFMA, stem_wgrad_flops=flops,
               byte_map_mb=arg.numel() / 1e6)
    return res


def _model(frozen_stages, bf16, norm_eval=True, depth=50):
    from bench import model_cfg
    cfg = model_cfg(depth)
    cfg['backbone'].update(frozen_stages=frozen_stages, norm_eval=norm_eval)
    m = P.build_detector(cfg).cuda()
    m.load_state_dict(synthetic.locator_state_dict(depth, 1, 0, 'cpr', 0), strict=True)
    if bf16:
        m.set_compute_dtype('bf16')
    m.train()
    return m


def step_time(frozen_stages, bf16, norm_eval=True, N=64, size=640, steps=6, warmup=2):
    from pointtinybenchmark_amd.training import CprTrainer
    m = _model(frozen_stages, bf16, norm_eval)
    b = synthetic.synthetic_batch(N, size, size, 10, 1, seed=123)
    data = dict(img=b['img'].cuda(), img_metas=b['img_metas'], gt_bboxes=[t.cuda() for t in b['gt_bboxes']],
                gt_labels=[t.cuda() for t in b['gt_labels']])
    tr = CprTrainer(m, lr=1e-4)
    for _ in range(warmup):
        tr.train_step(dict(data))
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        tr.train_step(dict(data))
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    del tr, m
    torch.cuda.empty_cache()
    return ts[len(ts) // 2]


def steps():
    out = {}
    for bf16 in (False, True):
        mode = 'mixed' if bf16 else 'fp32'
        for fs in (-1, 0, 1):
            out['step_ms_%s_frozen%d' % (mode, fs)] = step_time(fs, bf16)
            print(mode, fs, out['step_ms_%s_frozen%d' % (mode, fs)], flush=True)
        out['ratio_%s_m1_over_0' % mode] = out['step_ms_%s_frozen-1' % mode] / out['step_ms_%s_frozen0' % mode]
    out['step_ms_fp32_batch_stats_frozen-1'] = step_time(-1, False, norm_eval=False)
    out['step_ms_fp32_batch_stats_frozen0'] = step_time(0, False, norm_eval=False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--part', default='all', choices=['kernels', 'steps', 'all'])
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), config='R50 640^2 B=64, CPR locator, native CprTrainer step')
    if a.part in ('kernels', 'all'):
        res['kernels'] = kernels()
        print(json.dumps(res['kernels']), flush=True)
    if a.part in ('steps', 'all'):
        res['steps'] = steps()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
