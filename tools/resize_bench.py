"""What the job kernel of the image pipeline costs (csrc/preprocess.hip: cpr_preprocess_jobs_u8) next to the stacked kernel it sits
beside (cpr_preprocess_u8, unchanged), on the same output shape in the same run:

  upscale     8 x 480x640 -> 800x1067, padded to 800x1088
  tiles       16 tiles of 1024 x 1024 x 2 flips, crop rectangles of ONE 4000x4000 image
  downscale   8 x 1600x2134 -> 800x1067 (2:1), padded to 800x1088
  ragged      8 images of different sizes at scale 1 in one launch, against one cpr_preprocess_u8 launch per image

Device-event time per launch (median), the two kernels alternating, each over a ring of distinct source / output buffers larger
than 1 GiB so that the 256 MiB Infinity Cache cannot serve a re-read or absorb a write.  Bytes: 16 B per output pixel of the padded
slot plus 3 B per DISTINCT source pixel touched.  ``ratio`` = time / (stacked time x bytes / stacked bytes); the issue's allowance
for the byte gathers is 1.25.  Prints one JSON object (--out FILE also writes it: profiles/resize_bench.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
RING_BYTES = 1.25 * (1 << 30)


def _pad32(v):
    return (v + 31) // 32 * 32


def cases():
    """name -> (sources [(h, w)], jobs [(source index, crop, dw, dh, flip)])"""
    ragged = [(480, 640), (427, 640), (640, 480), (500, 375), (333, 500), (612, 612), (375, 500), (640, 427)]
    tiles = [(x, y, 1024, 1024) for y in (0, 992, 1984, 2976) for x in (0, 992, 1984, 2976)]
    return {
        'upscale': ([(480, 640)] * 8, [(i, (0, 0, 640, 480), 1067, 800, i % 2) for i in range(8)]),
        'tiles': ([(4000, 4000)], [(0, t, 1024, 1024, f) for t in tiles for f in (0, 1)]),
        'downscale': ([(1600, 2134)] * 8, [(i, (0, 0, 2134, 1600), 1067, 800, i % 2) for i in range(8)]),
        'ragged': (ragged, [(i, (0, 0, w, h), w, h, i % 2) for i, (h, w) in enumerate(ragged)]),
    }


def distinct_source_pixels(sources, jobs):
    import numpy as np
    n = 0
    for i, (h, w) in enumerate(sources):
        mask = np.zeros((h, w), dtype=bool)
        for s, (x0, y0, cw, ch), _, _, _ in jobs:
            if s == i:
                mask[y0:y0 + ch, x0:x0 + cw] = True
        n += int(mask.sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--cases', default='upscale,tiles,downscale,ragged')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from pointtinybenchmark_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit('resize_bench.py measures on the GPU; none is visible')
    mean = (ctypes.c_float * 3)(*MEAN)
    stdinv = (ctypes.c_float * 3)(*(1.0 / np.float64(np.array(STD, np.float32))).astype(np.float32).tolist())
    mp, sp = ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(stdinv, ctypes.c_void_p)
    result = dict(iters=args.iters, ring_bytes=RING_BYTES, cases={})
    for name, (sources, jobs) in cases().items():
        if name not in args.cases.split(','):
            continue
        uniform = name != 'ragged'
        Hp, Wp = max(_pad32(j[3]) for j in jobs), max(_pad32(j[2]) for j in jobs)
        n = len(jobs)
        out_px = n * Hp * Wp
        src_bytes = sum(h * w * 3 for h, w in sources)
        sets = int(RING_BYTES // (out_px * 16 + src_bytes)) + 2
        ring = []
        for k in range(sets):
            g = torch.Generator(device='cuda').manual_seed(k)
            srcs = [torch.randint(0, 256, (h, w, 3), device='cuda', dtype=torch.uint8, generator=g) for h, w in sources]
            out = torch.empty((n, Hp, Wp, 4), device='cuda', dtype=torch.float32)
            table = np.zeros((n,), dtype=np.dtype(ops.PREPROCESS_JOB))
            for q, (s, crop, dw, dh, flip) in enumerate(jobs):
                h, w = sources[s]
                table[q] = (srcs[s].data_ptr(), q * Hp * Wp, 0.0, 0.0, w * 3, w, h) + crop + (dw, dh, flip, Hp, Wp)
            table = ops.preprocess_job_table(table, out_px)
            entry = dict(srcs=srcs, out=out, table=torch.from_numpy(table.view(np.uint8).reshape(-1)).cuda(),
                         flips=torch.tensor([j[4] for j in jobs], dtype=torch.int32, device='cuda'))
            if uniform:       # the stacked kernel's input: n images of the OUTPUT's unpadded size
                entry['stack'] = torch.randint(0, 256, (n, jobs[0][3], jobs[0][2], 3), device='cuda', dtype=torch.uint8, generator=g)
            ring.append(entry)

        def run_jobs(e):
            _lib.call('cpr_preprocess_jobs_u8', ops._ptr(e['table']), n, mp, sp, 1, ops._ptr(e['out']), out_px, ops._stream())

        def run_base(e):
            if uniform:
                _lib.call('cpr_preprocess_u8', ops._ptr(e['stack']), ops._ptr(e['flips']), mp, sp, 1, ops._ptr(e['out']), n,
                          jobs[0][3], jobs[0][2], Hp, Wp, ops._stream())
            else:             # the loop the ragged path used to run: one launch per image into its slot
                for q, (s, _, dw, dh, _) in enumerate(jobs):
                    _lib.call('cpr_preprocess_u8', ops._ptr(e['srcs'][s]), ops._ptr(e['flips'][q:q + 1]), mp, sp, 1,
                              ops._ptr(e['out'][q:q + 1]), 1, dh, dw, Hp, Wp, ops._stream())
        times = dict(jobs=[], base=[])
        for it in range(args.warmup + args.iters):
            for which, fn in (('jobs', run_jobs), ('base', run_base)):
                e = ring[(2 * it + (which == 'base')) % len(ring)]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(e)
                b.record()
                b.synchronize()
                if it >= args.warmup:
                    times[which].append(a.elapsed_time(b))
        t_jobs, t_base = statistics.median(times['jobs']), statistics.median(times['base'])
        bytes_jobs = out_px * 16 + 3 * distinct_source_pixels(sources, jobs)
        bytes_base = out_px * 16 + 3 * sum(j[2] * j[3] for j in jobs)
        rec = dict(jobs=n, out_shape=[n, Hp, Wp, 4], ring_sets=sets, jobs_ms=t_jobs, base_ms=t_base,
                   jobs_ms_minmax=[min(times['jobs']), max(times['jobs'])], base_ms_minmax=[min(times['base']), max(times['base'])],
                   jobs_bytes=bytes_jobs, base_bytes=bytes_base, jobs_TBps=bytes_jobs / t_jobs / 1e9, base_TBps=bytes_base / t_base / 1e9,
                   base='cpr_preprocess_u8, one launch' if uniform else 'cpr_preprocess_u8, one launch per image')
        rec['ratio'] = t_jobs / (t_base * bytes_jobs / bytes_base)
        rec['within_1.25'] = rec['ratio'] <= 1.25
        result['cases'][name] = rec
        del ring
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
