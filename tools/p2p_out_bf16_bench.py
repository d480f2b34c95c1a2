"""P2PNet in the bf16 compute mode: what the output-conv kernels (csrc/p2p_out_bf16.hip) and the mixed-precision step cost.

  --mode kernels  the forward (taps + tap sum), data gradient (fp32 and bf16 out) and weight gradient kernels on the configs[3] map
                  (B x 160 x 160 x 256 bf16, J = 1 and 2), each launched --iters times in a row: device-event time per call and TB/s on
                  the algorithmic bytes (forward: map + a/b + output; dgrad: dout + dx; wgrad: map + dout).  Run it alone under
                  ``rocprofv3 --kernel-trace --stats`` for the per-kernel table.
  --mode step     P2PNet R50 640x640, B = --batch, in one process: the fp32 training step against the mixed-precision step, and fp32
                  inference (forward + top-k + pseudo-box NMS) against bf16 inference, alternating the two versions every round.
Every mode prints one JSON object (--out FILE also writes it)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters       # ms per call


def kernels_mode(args):
    import torch
    from pointtinybenchmark_amd import ops
    N, H, W, C = args.batch, 160, 160, 256
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn((N, H, W, C), device='cuda', generator=g).bfloat16()
    a = torch.rand((N, C), device='cuda', generator=g) + 0.5
    b = torch.randn((N, C), device='cuda', generator=g) * 0.5
    res = dict(map=[N, H, W, C], iters=args.iters, kernels={})
    px = N * H * W
    for J in (1, 2):
        w = torch.randn((J, C, 3, 3), device='cuda', generator=g) * 0.02
        bias = torch.zeros((J,), device='cuda')
        dout = torch.randn((N, H, W, 4), device='cuda', generator=g)
        gw, gb = torch.empty_like(w), torch.empty_like(bias)
        cases = {
            'fwd': (lambda: ops.p2p_out_bf16(x, (a, b), w, bias), px * (2 * C + 4 * J) + 2 * N * C * 4),
            'dgrad_f32': (lambda: ops.p2p_out_bf16_dgrad(dout, w, (N, H, W, C)), px * (4 * J + 4 * C)),
            'dgrad_bf16': (lambda: ops.p2p_out_bf16_dgrad(dout, w, (N, H, W, C), torch.bfloat16), px * (4 * J + 2 * C)),
            'wgrad': (lambda: ops.p2p_out_bf16_wgrad(dout, x, (a, b), tuple(w.shape), out_w=gw, out_b=gb), px * (2 * C + 4 * J)),
        }
        for name, (fn, nbytes) in cases.items():
            ms = _time(fn, args.iters)
            res['kernels']['%s_J%d' % (name, J)] = dict(us=round(ms * 1e3, 2), bytes=nbytes, tb_s=round(nbytes / (ms * 1e-3) / 1e12, 3))
    return res


def step_mode(args):
    import torch
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    from pointtinybenchmark_amd.training import P2PTrainer
    m = P.build_detector(p2p_model_cfg(50)).cuda()
    m.load_state_dict(synthetic.locator_state_dict(50, 1, 0, 'p2p', 0, head_std=0.05), strict=True)
    m.train()
    bt = synthetic.synthetic_batch(args.batch, 640, 640, 32, 1, seed=0)
    data = dict(img=bt['img'].cuda(), img_metas=bt['img_metas'], gt_bboxes=[t.cuda() for t in bt['gt_bboxes']],
                gt_labels=[t.cuda() for t in bt['gt_labels']])
    tr = P2PTrainer(m, lr=1e-5)

    def train():
        tr.forward_backward(**data)
        tr.step()

    def infer():
        with torch.no_grad():
            m.simple_test(data['img'], data['img_metas'])
    out = dict(batch=args.batch, rounds=args.rounds, iters=args.iters)
    for what, fn in (('train', train), ('infer', infer)):
        times = {'fp32': [], 'bf16': []}
        for _ in range(args.rounds):
            for dt in ('fp32', 'bf16'):
                m.set_compute_dtype(dt)
                if what == 'infer':
                    m.eval()
                else:
                    m.train()
                fn()
                times[dt].append(_time(fn, args.iters))
        best = {k: min(v) for k, v in times.items()}
        out[what] = dict(ms=times, img_s={k: round(args.batch / (v * 1e-3), 1) for k, v in best.items()},
                         speedup=round(best['fp32'] / best['bf16'], 3))
    out['peak_mem_gib'] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['kernels', 'step'], required=True)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    res = kernels_mode(args) if args.mode == 'kernels' else step_mode(args)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
