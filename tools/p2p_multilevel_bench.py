"""What training P2PNet on several FPN levels / points per cell costs: P2PTrainer.train_step on BasicLocator(R50, P2PHead) at the
BASELINE.json configs[3] shape (640x640, B=16) for strides [4] / [4, 8, 16, 32] (FPN num_outs 1 / 4) x point_anchor (0, 0) / the
4-point grid, in the fp32 and the bf16 compute mode.  Per setting: proposals per image, the median step time over --steps timed steps
(after --warmup), and the share of it spent in the batched device LSA (ops.lsa_topk bracketed by device events; the LSA runs one
workgroup per image problem, so its cost grows with the proposal count -- measured here, not changed).  One JSON object (--out FILE
also writes it, after every setting, so a partial run leaves what it measured).

--extra-levels: what the two extra pyramid levels cost (profiles/fpn_extra_levels_bench.json): start_level=1, num_outs=5, 'on_input',
strides [8 .. 128] beside the three-level line (start_level=1, num_outs=3, strides [8, 16, 32]) it extends, P = 1 and P = 4, and one
max-pool line (add_extra_convs=False) for the subsample kernels.  After the timed steps of a five-level setting, --breakdown-steps
further steps run with device-event brackets (main stream; the weight gradients run beside it on the side stream) around what
the extras add: their convs forward / backward, the subsample kernels, the two towers' forward and backward passes on the two
extra maps, the LSA."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID4 = [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]
SETTINGS = [('[4]/P=1', 1, [(0., 0.)]), ('[4,8,16,32]/P=1', 4, [(0., 0.)]), ('[4]/P=4', 1, GRID4), ('[4,8,16,32]/P=4', 4, GRID4)]


ALL_STRIDES = [4, 8, 16, 32, 64, 128]
EXTRA_SETTINGS = [('[8,16,32]/P=1', 3, [(0., 0.)], 'on_input'), ('[8..128]/P=1', 5, [(0., 0.)], 'on_input'),
                  ('[8..128] max-pool/P=1', 5, [(0., 0.)], False),
                  ('[8,16,32]/P=4', 3, GRID4, 'on_input'), ('[8..128]/P=4', 5, GRID4, 'on_input')]


def build(num_outs, anchors, dtype, depth=50, start_level=0, extra='on_input'):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    cfg = p2p_model_cfg(depth, 1)
    cfg['neck'] = dict(cfg['neck'], num_outs=num_outs, start_level=start_level, add_extra_convs=extra)
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=ALL_STRIDES[start_level:start_level + num_outs], point_anchor=list(anchors))
    m = P.build_detector(cfg).cuda()
    sd = synthetic.locator_state_dict(depth, 1, start_level, 'p2p', 3, head_std=0.05, num_points=len(anchors))
    sd = {k: v for k, v in sd.items() if not k.startswith('neck.')}
    sd.update(synthetic.fpn_state_dict(synthetic.backbone_out_channels(depth), 256, start_level, num_outs, 4, add_extra_convs=extra))
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


class Brackets:
    """Device-event brackets around the calls that only the extra levels make (see the module docstring): patched in for the
    breakdown steps, removed afterwards."""

    def __init__(self, model, trainer, ops, max_pixels):
        self.m, self.tr, self.ops, self.max_pixels = model, trainer, ops, max_pixels
        self.pairs, self.undo = [], []

    def _wrap(self, owner, name, key):
        import torch
        orig = getattr(owner, name)

        def timed(*a, **k):
            kk = key(*a, **k) if callable(key) else key
            if kk is None:
                return orig(*a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = orig(*a, **k)
            e.record()
            self.pairs.append((kk, s, e))
            return out
        setattr(owner, name, timed)
        self.undo.append((owner, name, orig))

    def __enter__(self):
        head_mods = {id(cm) for cm in list(self.m.bbox_head.cls_convs) + list(self.m.bbox_head.reg_convs)}
        small = lambda t: t.shape[1] * t.shape[2] <= self.max_pixels                       # noqa: E731
        self._wrap(self.m.neck, 'run_extras', 'extras_conv_fwd')
        self._wrap(self.tr, '_backward_extras', 'extras_conv_bwd')
        self._wrap(self.ops, 'subsample2', 'subsample')
        self._wrap(self.ops, 'subsample2_bwd_add', 'subsample')
        self._wrap(self.m.bbox_head, '_tower', lambda convs, out_conv, x, tape=None: 'extra_towers_fwd' if small(x) else None)
        self._wrap(self.tr, '_gn_conv_backward', lambda rec, *a, **k: 'extra_towers_bwd'
                   if id(rec['module']) in head_mods and small(rec['raw']) else None)
        self._wrap(self.tr, '_out_conv_backward', lambda rec, *a, **k: 'extra_towers_bwd' if small(rec['x']) else None)
        self._wrap(self.tr, '_p2p_out_conv_backward_mixed', lambda tape, *a, **k: 'extra_towers_bwd' if small(tape[-1]['x']) else None)
        self._wrap(self.ops, 'lsa_topk', 'lsa')
        return self

    def __exit__(self, *exc):
        for owner, name, orig in reversed(self.undo):
            setattr(owner, name, orig)

    def take_ms(self):
        out = {}
        for k, s, e in self.pairs:
            out[k] = out.get(k, 0.0) + s.elapsed_time(e)
        self.pairs = []
        return out


def run_setting(label, num_outs, anchors, dtype, args, start_level=0, extra='on_input'):
    import torch
    from pointtinybenchmark_amd import ops, synthetic
    from pointtinybenchmark_amd.training import P2PTrainer
    m = build(num_outs, anchors, dtype, start_level=start_level, extra=extra)
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
    strides = ALL_STRIDES[start_level:start_level + num_outs]
    s = sum(-(-args.size // st) * -(-args.size // st) for st in strides)
    med, lmed = statistics.median(steps), statistics.median(lsa)
    row = dict(setting=label, compute=dtype, num_outs=num_outs, num_points=len(anchors), proposals_per_image=s * len(anchors),
               step_ms_median=round(med, 2), step_ms=[round(v, 2) for v in steps], img_per_s=round(args.batch * 1e3 / med, 1),
               lsa_ms_median=round(lmed, 2), lsa_share=round(lmed / med, 4))
    if m.neck.extra_levels and args.breakdown_steps:
        # the extra maps are the two coarsest: everything at most as large as the first of them
        first = strides[len(m.neck.lateral_convs)]
        acc = []
        with Brackets(m, tr, ops, (-(-args.size // first)) ** 2) as br:
            for _ in range(args.breakdown_steps):
                tr.train_step(dict(data))
                torch.cuda.synchronize()
                acc.append(br.take_ms())
        keys = sorted({k for a in acc for k in a})
        row['extras_breakdown_ms'] = {k: round(statistics.median(a.get(k, 0.0) for a in acc), 3) for k in keys}
        row['extras_cells_share'] = round(sum((-(-args.size // st)) ** 2 for st in strides[len(m.neck.lateral_convs):]) / s, 4)
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
    ap.add_argument('--extra-levels', action='store_true', help='the FPN extra-levels lines instead of the multi-level ones')
    ap.add_argument('--breakdown-steps', type=int, default=3)
    args = ap.parse_args()
    import torch
    res = dict(workload='P2PTrainer.train_step, BasicLocator(R50, P2PHead C=1), %dx%d, B=%d, %d gts/image, Adam' % (
        args.size, args.size, args.batch, args.gts), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
        rows=[])
    settings = [(l, n, a, dict(start_level=1, extra=e)) for l, n, a, e in EXTRA_SETTINGS] if args.extra_levels else \
        [(l, n, a, {}) for l, n, a in SETTINGS]
    for dtype in args.dtypes.split(','):
        for label, num_outs, anchors, kw in settings:
            row = run_setting(label, num_outs, anchors, dtype, args, **kw)
            print(json.dumps(row), flush=True)
            res['rows'].append(row)
            if args.extra_levels and num_outs == 5:       # the delta against the three-level line of the same P and compute mode
                base = [r for r in res['rows'] if r['compute'] == dtype and r['num_outs'] == 3 and r['num_points'] == len(anchors)]
                if base:
                    row['delta_vs_three_levels_ms'] = round(row['step_ms_median'] - base[-1]['step_ms_median'], 2)
                    row['delta_vs_three_levels'] = round(row['step_ms_median'] / base[-1]['step_ms_median'] - 1, 4)
            if args.out:
                with open(args.out, 'w') as f:
                    json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
