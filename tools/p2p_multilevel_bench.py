"""What training P2PNet on several FPN levels / points per cell costs: P2PTrainer.train_step on BasicLocator(R50, P2PHead) at the
BASELINE.json configs[3] shape (640x640, B=16) for strides [4] / [4, 8, 16, 32] (FPN num_outs 1 / 4) x point_anchor (0, 0) / the
4-point grid, in the fp32 and the bf16 compute mode.  Per setting: proposals per image, the median step time over --steps timed steps
(after --warmup), and the share of it spent in the batched device LSA (ops.lsa_topk bracketed by device events; the LSA runs one
workgroup per image problem, so its cost grows with the proposal count -- measured here, not changed).  One JSON object (--out FILE
also writes it, after every setting, so a partial run leaves what it measured)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID4 = [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]
SETTINGS = [('[4]/P=1', 1, [(0., 0.)]), ('[4,8,16,32]/P=1', 4, [(0., 0.)]), ('[4]/P=4', 1, GRID4), ('[4,8,16,32]/P=4', 4, GRID4)]


def build(num_outs, anchors, dtype, depth=50):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(depth, 1)
    cfg['neck'] = dict(cfg['neck'], num_outs=num_outs)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4, 8, 16, 32][:num_outs], point_anchor=list(anchors))
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, 1, 0, 'p2p', 3, head_std=0.05, num_points=len(anchors))
    sd.update(synthetic.fpn_state_dict(synthetic.backbone_out_channels(depth), 256, 0, num_outs, 4))
    m.load_state_dict(sd, strict=True)
    m.train()
    m.set_compute_dtype(dtype)
    return m


class LsaTimer:
    """Device-event brackets around every ops.lsa_topk call (the head's batched assignment)."""

    def __init__(self, ops):
        self.ops, self.orig, self.pairs = ops, ops.lsa_topk, []

    def __enter__(self):
        import torch

        def timed(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = self.orig(*a, **k)
            e.record()
            self.pairs.append((s, e))
            return out
        self.ops.lsa_topk = timed
        return self

    def __exit__(self, *exc):
        self.ops.lsa_topk = self.orig

    def take_ms(self):
        ms = sum(s.elapsed_time(e) for s, e in self.pairs)
        self.pairs = []
        return ms


def run_setting(label, num_outs, anchors, dtype, args):
    import torch
    from pointtinybenchmark_amd import ops, synthetic
    from pointtinybenchmark_amd.training import P2PTrainer
    m = build(num_outs, anchors, dtype)
    batch = synthetic.synthetic_batch(args.batch, args.size, args.size, args.gts, 1, seed=61)
    data = dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])
    tr = P2PTrainer(m, optimizer=dict(type='Adam', lr=1e-4), max_norm=35.0)
    steps, lsa = [], []
    with LsaTimer(ops) as lt:
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train_step(dict(data))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            l_ms = lt.take_ms()
            if i >= args.warmup:
                steps.append(dt)
                lsa.append(l_ms)
    s = sum(args.size // st * (args.size // st) for st in [4, 8, 16, 32][:num_outs])
    med, lmed = statistics.median(steps), statistics.median(lsa)
    row = dict(setting=label, compute=dtype, num_outs=num_outs, num_points=len(anchors), proposals_per_image=s * len(anchors),
               step_ms_median=round(med, 2), step_ms=[round(v, 2) for v in steps], img_per_s=round(args.batch * 1e3 / med, 1),
               lsa_ms_median=round(lmed, 2), lsa_share=round(lmed / med, 4))
    del tr, m
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--gts', type=int, default=32)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--dtypes', default='fp32,bf16')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    res = dict(workload='P2PTrainer.train_step, BasicLocator(R50, P2PHead C=1), %dx%d, B=%d, %d gts/image, Adam' % (
        args.size, args.size, args.batch, args.gts), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
        rows=[])
    for dtype in args.dtypes.split(','):
        for label, num_outs, anchors in SETTINGS:
            row = run_setting(label, num_outs, anchors, dtype, args)
            print(json.dumps(row), flush=True)
            res['rows'].append(row)
            if args.out:
                with open(args.out, 'w') as f:
                    json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
