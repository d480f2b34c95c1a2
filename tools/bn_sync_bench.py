"""SyncBN: what splitting the two BatchNorm finalize steps costs (csrc/bn_train.hip).

Times, with device events in ONE process, the four split kernels (bn_stats_local / bn_stats_merge / bn_bwd_local / bn_bwd_merge) and
the two single-rank finalize kernels they stand in for (bn_stats_finalize / bn_bwd_finalize) on the map tools/bn_train_bench.py uses.
The measurement build's ``cpr_bn_set_finalize_only(1)`` makes every bn_train.hip entry skip its streaming passes, so each entry is
exactly one of these launches; the row-block partials they read are left in the workspace by one full call before.  Each figure is the
interval between back-to-back launches of the same kernel (``--reps`` per window, candidates alternating over ``--rounds`` rounds,
median of the rounds): for the merge kernels, which run a few microseconds, that is the dispatch interval -- an upper bound of the kernel.

Target: local + merge <= 2 x the single-rank finalize, per direction (two latency-bound launches replace one).
``--sequence`` runs both forms in product order (streaming passes on, ops.* entries) for a separate ``rocprofv3 --kernel-trace --stats``
run; ``--stats DIR`` then adds each kernel's in-sequence average from that run's kernel_stats.csv (there the partials were written by a
1.7 GB streaming pass just before, so the finalize-shaped kernels wait on colder loads than in the back-to-back windows).
NOT measured here: the collectives between local and merge (all_gather_into_tensor of (2C + 1) / 2C doubles per rank) -- one GPU has
no second device to gather from, and gloo stages through the host.

    python -m pointtinybenchmark_amd.build --bench-hooks
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bn -- python tools/bn_sync_bench.py --sequence
    python tools/bn_sync_bench.py --stats DIR --out profiles/bn_sync_bench.json"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('CPR_BENCH_HOOKS', '1')   # measurement build (libcprhip_bench.so: python -m pointtinybenchmark_amd.build --bench-hooks)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shape', type=int, nargs=4, default=(64, 160, 160, 256))
    ap.add_argument('--ranks', type=int, default=8, help='records the merge kernels read (the map itself is one rank\'s)')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--sequence', action='store_true', help='no timing: both forms in product order, for a rocprofv3 run')
    ap.add_argument('--stats', default=None, help='directory of that rocprofv3 run: adds in_sequence_us per kernel')
    args = ap.parse_args()
    t0 = time.time()
    if args.sequence:
        return sequence(args)
    import torch
    from pointtinybenchmark_amd import _lib
    from pointtinybenchmark_amd.ops import _ptr, _stream
    if not torch.cuda.is_available():
        raise SystemExit('bn_sync_bench needs the GPU: a CPU run says nothing about these kernels')
    N, H, W, C = args.shape
    M, R = N * H * W, args.ranks
    dev = 'cuda'
    torch.manual_seed(0)
    y = torch.randn((N, H, W, C), device=dev)
    dout = torch.randn_like(y)
    z = torch.relu(torch.randn_like(y))
    dy = torch.empty_like(y)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros((), device=dev, dtype=torch.int64)
    st = torch.empty((7, C), device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws_f = torch.empty((_lib.call('cpr_bn_train_ws', M, C, positive=True),), device=dev)     # statistics partials
    ws_b = torch.empty_like(ws_f)                                                             # backward partials + coef
    rec_f = torch.empty((2 * C + 1,), device=dev, dtype=torch.float64)
    rec_b = torch.empty((2 * C,), device=dev, dtype=torch.float64)
    count = torch.empty((1,), device=dev, dtype=torch.float64)
    stp = [_ptr(st[i]) for i in range(7)]

    def stats_finalize():
        _lib.call('cpr_bn_batch_stats', _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(nbt), 0.1, 1e-5, *stp, _ptr(ws_f), M, C,
                  _stream())

    def stats_local():
        _lib.call('cpr_bn_sync_stats_local', _ptr(y), _ptr(rec_f), _ptr(ws_f), M, C, _stream())

    def bwd_finalize():
        _lib.call('cpr_bn_train_bwd', _ptr(dout), _ptr(z), _ptr(y), stp[4], stp[5], stp[1], _ptr(gamma), _ptr(dy), _ptr(dg), _ptr(db),
                  _ptr(ws_b), M, C, _stream())

    def bwd_local():
        _lib.call('cpr_bn_sync_bwd_local', _ptr(dout), _ptr(z), _ptr(y), stp[4], stp[5], stp[1], _ptr(dg), _ptr(db), _ptr(rec_b), _ptr(ws_b),
                  M, C, _stream())

    # one full pass with the streaming kernels on: partials in both workspaces, statistics, records
    stats_finalize()
    stats_local()
    bwd_finalize()
    bwd_local()
    recs_f = rec_f.repeat(R, 1).contiguous()
    recs_b = rec_b.repeat(R, 1).contiguous()

    def stats_merge():
        _lib.call('cpr_bn_sync_stats_merge', _ptr(recs_f), R, _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(nbt), 0.1, 1e-5,
                  *stp, _ptr(count), C, _stream())

    def bwd_merge():
        _lib.call('cpr_bn_sync_bwd_merge', _ptr(recs_b), R, _ptr(count), _ptr(dout), _ptr(z), _ptr(y), stp[4], stp[5], stp[1], _ptr(gamma),
                  _ptr(dy), _ptr(ws_b), M, C, _stream())
    stats_merge()
    torch.cuda.synchronize()
    cands = [('bn_stats_finalize_kernel', stats_finalize), ('bn_stats_local_kernel', stats_local), ('bn_stats_merge_kernel', stats_merge),
             ('bn_bwd_finalize_kernel', bwd_finalize), ('bn_bwd_local_kernel', bwd_local), ('bn_bwd_merge_kernel', bwd_merge)]
    _lib.call('cpr_bn_set_finalize_only', 1)
    try:
        for _, fn in cands:                      # warm-up
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        us = {name: [] for name, _ in cands}
        for _ in range(args.rounds):             # alternate: clock / temperature drift hits every candidate alike
            for name, fn in cands:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    finally:
        _lib.call('cpr_bn_set_finalize_only', 0)
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    rows_per_block = max(64, -(-M // max(1, 2048 // -(-C // 1024))))
    out = dict(shape=list(args.shape), rows=M, row_blocks=-(-M // rows_per_block), ranks_in_merge=R, reps=args.reps, rounds=args.rounds,
               timing='device events around back-to-back launches of one kernel; median of the rounds, microseconds per launch',
               kernels={k: dict(us=med[k], min_us=min(us[k]), max_us=max(us[k])) for k in us},
               stats=dict(finalize_us=med['bn_stats_finalize_kernel'],
                          local_plus_merge_us=med['bn_stats_local_kernel'] + med['bn_stats_merge_kernel']),
               bwd=dict(finalize_us=med['bn_bwd_finalize_kernel'], local_plus_merge_us=med['bn_bwd_local_kernel'] + med['bn_bwd_merge_kernel']),
               target='local + merge <= 2 x finalize, per direction',
               not_measured='the all_gather_into_tensor between local and merge, and any run over RCCL on distinct devices',
               device=torch.cuda.get_device_name(0))
    for d in ('stats', 'bwd'):
        out[d]['ratio'] = out[d]['local_plus_merge_us'] / out[d]['finalize_us']
        out[d]['met'] = out[d]['ratio'] <= 2.0
    if args.stats:
        import csv
        import glob
        paths = glob.glob(os.path.join(args.stats, '**', '*kernel_stats.csv'), recursive=True)
        assert paths, 'no kernel_stats.csv under %s' % args.stats
        rows = list(csv.DictReader(open(paths[0])))
        for k in out['kernels']:
            hit = [r for r in rows if k in r['Name']]
            assert hit, k
            out['kernels'][k].update(in_sequence_us=float(hit[0]['AverageNs']) / 1e3, in_sequence_calls=int(hit[0]['Calls']))
        seq = {k: v['in_sequence_us'] for k, v in out['kernels'].items()}
        for d in ('stats', 'bwd'):
            lm = seq['bn_%s_local_kernel' % d] + seq['bn_%s_merge_kernel' % d]
            out[d].update(in_sequence_finalize_us=seq['bn_%s_finalize_kernel' % d], in_sequence_local_plus_merge_us=lm,
                          in_sequence_ratio=lm / seq['bn_%s_finalize_kernel' % d])
            out[d]['met'] = out[d]['met'] and out[d]['in_sequence_ratio'] <= 2.0
    out['wall_s'] = round(time.time() - t0, 1)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


def sequence(args):
    import torch
    from pointtinybenchmark_amd import ops
    N, H, W, C = args.shape
    R = args.ranks
    torch.manual_seed(0)
    y = torch.randn((N, H, W, C), device='cuda')
    dout = torch.randn_like(y)
    gamma, beta = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    nbt = torch.zeros((), device='cuda', dtype=torch.int64)
    for _ in range(5):
        st = ops.bn_batch_stats(y, gamma, beta, rm, rv, nbt, 0.1, 1e-5)
        z = ops.bn_apply(y, st.scale, st.cshift, center=st.center, relu=True)
        ops.bn_train_bwd(dout, y, st.cmean, st.rstd, gamma, mask=z, center=st.center)
        del z
        rec, _ = ops.bn_sync_local_stats(y)
        rec[2 * C] /= R                          # R records that merge to this map's own statistics
        st = ops.bn_sync_merge_stats(rec.repeat(R, 1), y, gamma, beta, rm, rv, nbt, 0.1, 1e-5)
        z = ops.bn_apply(y, st.scale, st.cshift, center=st.center, relu=True)
        brec, ws, _, _ = ops.bn_sync_local_bwd(dout, y, st.cmean, st.rstd, mask=z, center=st.center)
        ops.bn_sync_merge_bwd((brec / R).repeat(R, 1), ws, st.count, dout, y, st.cmean, st.rstd, gamma, mask=z, center=st.center)
        del z
    torch.cuda.synchronize()
    print(json.dumps(dict(mode='sequence', shape=list(args.shape), ranks_in_merge=R)))


if __name__ == '__main__':
    main()
