#!/usr/bin/env python3
"""kNN graph building measured: the device path (graph.knn_device / graph.connectivity_graph, chebgcn_knn) against the host path
(graph.distance_sklearn_metrics: full N x N matrix + argsort) on the same machine.

  cube10k / cube20k   N = 10 000 / 20 000 uniform points in the unit cube, D = 3, euclidean, k = 8 (the direct arm);
  cos20k              N = 20 000, D = 1200, cosine, k = 8 (the Gram arm);
  conn20k             connectivity_graph at M = 20 000 with 4 runs of 1200 time points, k = 8.

Per case: ``kernel_ms`` -- HIP events around the library call alone on resident planes (after --warmup calls, --reps repeats:
median / min / max), for the Gram arm with its share of the 157 TF fp32 matrix peak (2 N^2 D flop); ``device_s`` -- wall time of
the whole Python call, host staging, upload and download included; ``host_s`` -- wall time of the host path (one call; skipped
with --no-host, and for conn20k the host arm is np.corrcoef per run + argsort).  Prints one JSON line.  Needs a GPU.

    python tools/knn_bench.py [--cases cube10k,cube20k,cos20k,conn20k] [--reps 5] [--warmup 2] [--no-host] [--out FILE]
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

from gcn_fmri_decoding_amd import _lib, graph, ops   # noqa: E402

MATRIX_PEAK_F32 = 157e12


def spread(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def planes_of(z, dev):
    p = np.zeros((z.shape[1], ops.plane_stride(len(z))), np.float32)
    p[:, :len(z)] = z.T
    return torch.as_tensor(p).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='cube10k,cube20k,cos20k,conn20k')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('knn_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    res = {'device': torch.cuda.get_device_name(0), 'cus': torch.cuda.get_device_properties(0).multi_processor_count,
           'torch': torch.__version__, 'hip': torch.version.hip, 'reps': args.reps, 'warmup': args.warmup,
           'host_cpus': len(os.sched_getaffinity(0))}
    k = 8
    for case in args.cases.split(','):
        rs = np.random.RandomState(0)
        r = {}
        if case in ('cube10k', 'cube20k', 'cos20k'):
            N = 10000 if case == 'cube10k' else 20000
            D, metric = (1200, 'cosine') if case == 'cos20k' else (3, 'euclidean')
            z = rs.rand(N, D).astype(np.float32) if D == 3 else rs.randn(N, D).astype(np.float32)
            p = planes_of(z, dev)
            m = graph.KNN_METRICS.index(metric)
            ms = event_ms(lambda: ops.knn(p, N, k, m), args.warmup, args.reps)
            r.update(N=N, D=D, metric=metric, k=k, dispatch=_lib.last_dispatch(), kernel_ms=spread(ms))
            if D > 8:
                r['share_of_f32_matrix_peak'] = 2.0 * N * N * D / (np.median(ms) * 1e-3) / MATRIX_PEAK_F32
            r['device_s'], (d, idx) = wall(lambda: graph.knn_device(z, k=k, metric=metric, device=dev))
            if not args.no_host:
                r['host_s'], (dh, ih) = wall(lambda: graph.distance_sklearn_metrics(z, k=k, metric=metric))
                r['rows_with_equal_indices'] = float((idx == ih).all(axis=1).mean())
        elif case == 'conn20k':
            M, T, R = 20000, 1200, 4
            runs = [rs.randn(T, M).astype(np.float32) for _ in range(R)]
            offs = torch.as_tensor(np.arange(R + 1, dtype=np.int64) * T).to(dev)
            p = torch.zeros((R * T, ops.plane_stride(M)), dtype=torch.float32, device=dev)
            for i, run in enumerate(runs):
                p[i * T:(i + 1) * T, :M] = torch.as_tensor(run).to(dev)
            zn = ops.series_normalise(p, offs, M, scale=0.5)
            r.update(M=M, T=T, runs=R, k=k)
            r['normalise_ms'] = spread(event_ms(lambda: ops.series_normalise(p, offs, M, scale=0.5, out=zn), args.warmup, args.reps))
            ms = event_ms(lambda: ops.knn(zn, M, k, _lib.KNN_DOT), args.warmup, args.reps)
            r['dispatch'] = _lib.last_dispatch()
            r['kernel_ms'] = spread(ms)
            r['share_of_f32_matrix_peak'] = 2.0 * M * M * R * T / (np.median(ms) * 1e-3) / MATRIX_PEAK_F32
            del p, zn
            r['device_s'], _ = wall(lambda: graph.connectivity_graph(runs, k=k, device=dev))
            if not args.no_host:
                def host():
                    acc = np.zeros((M, M), np.float32)
                    for run in runs:
                        acc += np.corrcoef(run.T).astype(np.float32)
                    acc /= R
                    np.fill_diagonal(acc, -np.inf)
                    return np.argsort(-acc)[:, :k]
                r['host_s'], _ = wall(host)
        else:
            raise SystemExit('knn_bench: unknown case %r' % case)
        res[case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
