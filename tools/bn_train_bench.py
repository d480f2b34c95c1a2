"""Training-mode BatchNorm (ResNet norm_eval=False) costs.

  --mode step     the fp32 CPR training step (R50, 640x640, B=64, frozen_stages=1: forward_backward + SGD step) with norm_eval=True and
                  norm_eval=False alternating in one process: warm-up, then device-event timing of each mode, peak memory of each mode.
  --mode kernels  the csrc/bn_train.hip kernels on one large map, for a separate ``rocprofv3 --kernel-trace --stats`` run; writes the
                  bytes each kernel moves per call to --out.
  --mode report   joins the bytes of --bytes with the per-kernel average times of the rocprofv3 --stats CSV (--stats): TB/s per kernel;
                  --step FILE adds the output of a --mode step run, --out FILE writes the combined object (profiles/bn_train_bench.json).
Every mode prints one JSON object."""
import argparse
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def step_mode(args):
    import torch
    import pointtinybenchmark_amd as P
    from bench import model_cfg
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = model_cfg(50)
    m = P.build_detector(cfg).cuda()
    m.load_state_dict(synthetic.locator_state_dict(50, 1, 0, 'cpr', 0), strict=True)
    b = synthetic.synthetic_batch(args.batch, args.size, args.size, 32, 1, seed=0)
    data = dict(img=b['img'].cuda(), img_metas=b['img_metas'], gt_bboxes=[x.cuda() for x in b['gt_bboxes']],
                gt_labels=[x.cuda() for x in b['gt_labels']])

    def set_mode(norm_eval):
        m.backbone.norm_eval = norm_eval
        m.train()
    set_mode(True)
    tr = CprTrainer(m, lr=1e-4)

    def step():
        tr.forward_backward(**data)
        tr.step()
    res = {True: [], False: []}
    peak = {}
    for ne in (True, False):                 # warm-up of both modes; peak memory of one step each
        set_mode(ne)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[ne] = torch.cuda.max_memory_allocated() / 2 ** 30
    for _ in range(args.rounds):             # alternate: drift of clocks / temperature hits both modes alike
        for ne in (True, False):
            set_mode(ne)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            res[ne].append(e0.elapsed_time(e1) / args.steps)
    med = {ne: sorted(v)[len(v) // 2] for ne, v in res.items()}
    return dict(mode='step', depth=50, size=args.size, batch=args.batch, frozen_stages=1, steps_per_round=args.steps,
                rounds=args.rounds, ms_per_step_norm_eval_true=med[True], ms_per_step_norm_eval_false=med[False],
                all_ms_true=res[True], all_ms_false=res[False],
                img_per_s_norm_eval_true=args.batch * 1000.0 / med[True], img_per_s_norm_eval_false=args.batch * 1000.0 / med[False],
                throughput_ratio_false_over_true=med[True] / med[False],
                peak_gib_norm_eval_true=peak[True], peak_gib_norm_eval_false=peak[False],
                device=torch.cuda.get_device_name(0))


def kernels_mode(args):
    import torch
    from pointtinybenchmark_amd import ops
    N, H, W, C = args.shape
    M = N * H * W
    S = 4 * M * C
    torch.manual_seed(0)
    y = torch.randn((N, H, W, C), device='cuda')
    dout = torch.randn_like(y)
    gamma, beta = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    nbt = torch.zeros((), device='cuda', dtype=torch.int64)
    for _ in range(args.reps):
        st = ops.bn_batch_stats(y, gamma, beta, rm, rv, nbt, 0.1, 1e-5)
        z = ops.bn_apply(y, st.scale, st.cshift, center=st.center, relu=True)
        ops.bn_train_bwd(dout, y, st.cmean, st.rstd, gamma, mask=z, center=st.center)
        del z
    torch.cuda.synchronize()
    out = dict(mode='kernels', shape=list(args.shape), map_mbytes=S / 1e6, reps=args.reps,
               bytes={'bn_stats_part_kernel': S, 'bn_apply_kernel': 2 * S, 'bn_bwd_part_kernel': 3 * S, 'bn_bwd_apply_kernel': 4 * S})
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    return out


def report_mode(args):
    with open(args.bytes) as f:
        info = json.load(f)
    paths = [args.stats] if os.path.isfile(args.stats) else glob.glob(os.path.join(args.stats, '**', '*kernel_stats.csv'), recursive=True)
    assert paths, 'no kernel_stats.csv under %s' % args.stats
    import csv
    rows = list(csv.DictReader(open(paths[0])))
    out = dict(mode='report', shape=info['shape'], map_mbytes=info['map_mbytes'], stats_csv=os.path.basename(paths[0]), kernels={})
    for name, nbytes in info['bytes'].items():
        hit = [r for r in rows if name in r['Name'] and 'finalize' not in r['Name']]
        assert hit, name
        avg_ns = float(hit[0]['AverageNs'])
        out['kernels'][name] = dict(calls=int(hit[0]['Calls']), avg_us=avg_ns / 1e3, mbytes=nbytes / 1e6, tb_per_s=nbytes / avg_ns / 1e3)
    for name in ('bn_stats_finalize_kernel', 'bn_bwd_finalize_kernel'):
        for r in rows:
            if name in r['Name']:
                out['kernels'][name] = dict(calls=int(r['Calls']), avg_us=float(r['AverageNs']) / 1e3)
    if args.step:
        with open(args.step) as f:
            step = json.loads([ln for ln in f.read().splitlines() if ln.startswith('{')][-1])
        out = dict(step=step, kernels=out, targets=dict(kernel_tb_per_s_min=4.5, throughput_ratio_false_over_true_min=0.85),
                   met=dict(kernels=all(v['tb_per_s'] >= 4.5 for v in out['kernels'].values() if 'tb_per_s' in v),
                            step=step['throughput_ratio_false_over_true'] >= 0.85))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', choices=('step', 'kernels', 'report'), default='step')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shape', type=int, nargs=4, default=(64, 160, 160, 256))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--bytes', default=None)
    ap.add_argument('--stats', default=None)
    ap.add_argument('--step', default=None)
    args = ap.parse_args()
    t0 = time.time()
    res = {'step': step_mode, 'kernels': kernels_mode, 'report': report_mode}[args.mode](args)
    res['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
