#!/usr/bin/env python3
"""Decoding a scan window by window (cgcnn.decode_series) against predict() on host-cut windows, at the two shapes of
tools/saliency_bench.py:

  atlas:    training.py's network -- a 360-vertex kNN graph, K = 10, F = [32]*6, p = [1]*6, channel 15, b1relu, batch 128;
  config1:  BASELINE configs[1] -- the seeded synthetic N = 10000 graph after one coarsening level (M = 10466), K = 5,
            F = [32]*6, b2relu, channel 15, batch 64.

For runs of T = 284 and 1200 time points and strides 1 and 5, windows/s (device-synchronised, the host copy of the result
included) of
  (a) predict() on the windows cut on the host and staged -- what a user had to do before decode_series, THE BASELINE; the time
      to cut and stage them is reported beside it (stage_ms), not inside it;
  (b) decode_series(share=False), the materialised path;
  (c) decode_series(share=True), the shared path;
each as the median of --reps repetitions after a warm-up, with the spread (min .. max) and the peak device memory of the call;
what 'auto' picks; and the per-kernel times (ops.KernelTimers, by kernel template) of ONE batch of each of (b) and (c), the
windowed contraction's HBM share from its shapes, 4*B*M*(C*K + Fout/pool) bytes over 8 TB/s (the count contract_fwd is given,
although overlapping windows re-read planes that may still sit in L2 / the Infinity Cache).  Prints one JSON line.  Needs a
GPU; there is no CPU fallback.

    python tools/decode_bench.py [--reps 7] [--shapes atlas,config1] [--T 284,1200] [--strides 1,5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from saliency_bench import build, instrumented   # noqa: E402


def timed(fn, reps):
    """Seconds of fn(): (median, min, max) over ``reps`` synchronised repetitions after one warm-up; peak device bytes."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts), int(torch.cuda.max_memory_allocated())


def rate(n, t):
    med, lo, hi, peak = t
    return {'win_s': n / med, 'win_s_min': n / hi, 'win_s_max': n / lo, 'ms': 1e3 * med, 'peak_MB': peak / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--T', default='284,1200')
    ap.add_argument('--strides', default='1,5')
    ap.add_argument('--out', default=None, help='also write the full result (every kernel) as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('decode_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    res = {'device': torch.cuda.get_device_name(0), 'cus': torch.cuda.get_device_properties(0).multi_processor_count,
           'torch': torch.__version__, 'hip': torch.version.hip, 'reps': args.reps}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        C, M = int(net.channel), int(net._M0)
        r = {'M': M, 'batch': B, 'channel': C, 'runs': {}}
        for T in (int(t) for t in args.T.split(',')):
            series = np.random.RandomState(T).randn(T, M).astype(np.float32)
            for stride in (int(s) for s in args.strides.split(',')):
                starts = np.arange(0, T - C + 1, stride)
                W = len(starts)
                t0 = time.perf_counter()
                x = np.ascontiguousarray(series[starts[:, None] + np.arange(C)[None, :]].transpose(0, 2, 1))
                staged = net.stage(x)
                torch.cuda.synchronize()
                stage_ms = 1e3 * (time.perf_counter() - t0)
                e = {'windows': W, 'stage_ms': stage_ms, 'staged_MB': x.nbytes / 2 ** 20}
                del x
                e['predict'] = rate(W, timed(lambda: net.predict(staged), args.reps))
                del staged
                torch.cuda.empty_cache()
                e['materialised'] = rate(W, timed(lambda: net.decode_series(series, stride=stride, share=False), args.reps))
                e['shared'] = rate(W, timed(lambda: net.decode_series(series, stride=stride, share=True), args.reps))
                net.decode_series(series, stride=stride)
                e['auto'] = net.last_decode_path
                # spread of the repetitions, as a fraction of the median: (c) against (b) is judged against it
                e['shared_over_materialised'] = e['shared']['win_s'] / e['materialised']['win_s']
                e['spread'] = max((v['win_s_max'] - v['win_s_min']) / v['win_s'] for v in (e['materialised'], e['shared']))
                r['runs']['T%d_s%d' % (T, stride)] = e
        # one batch of each path, kernel by kernel
        series = np.random.RandomState(0).randn(B + C - 1, M).astype(np.float32)
        kern = {}
        for share in (False, True):
            net.decode_series(series, share=share, batch_size=B)
            k = instrumented(lambda: net.decode_series(series, share=share, batch_size=B))
            kern['shared' if share else 'materialised'] = {
                'kernels_ms': sum(v['total_ms'] for v in k.values()),
                'by_kernel': {n: {'launches': v['launches'], 'total_ms': v['total_ms'], 'bytes': v['bytes'], 'hbm_share': v['hbm_share']}
                              for n, v in k.items()}}
        first = {n: v for n, v in kern['shared']['by_kernel'].items() if n.startswith('contract_fwd_windows')}
        r['one_batch'] = kern
        r['windowed_contraction'] = first
        res[shape] = r
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
