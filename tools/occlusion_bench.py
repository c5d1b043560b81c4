#!/usr/bin/env python3
"""Occlusion maps (base_model.occlusion / occlusion_maps) against predict(), at the two shapes of tools/saliency_bench.py:

  atlas:    training.py's network -- a 360-vertex kNN graph, K = 10, F = [32]*6, channel 15, b1relu, batch 128, head
            M = [512, 256, 22]; groups: one per vertex (G = 360);
  config1:  BASELINE configs[1] -- the N = 10000 synthetic graph after one coarsening level (M = 10466), K = 5, F = [32]*6,
            b2relu, channel 15, batch 64; groups: the clusters of coarsening level --level (np.arange(M) >> level), and one
            per vertex on a few windows.

Prints one JSON line: windows/s of predict, occlusion and occlusion_maps (device-synchronised, the host copy of the result
included), forward rows/s of each (a window costs G + 1 rows), the share of the new kernels (occlusion_rows, occlusion_score,
the class sums and the class seed) in the kernel time of one call (ops.KernelTimers), and each new kernel's HBM share
(bytes from the shapes over 8 TB/s).

    python tools/occlusion_bench.py [--windows 64] [--reps 3] [--level 4] [--shapes atlas,config1] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from saliency_bench import build, kernel_shares, timed     # noqa: E402

NEW = ('occlusion_rows', 'occlusion_score', 'occlusion_class_sums', 'saliency_seed')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--vertex-windows', type=int, default=2, help='windows of the per-vertex run at config1')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--level', type=int, default=4, help='coarsening level of the config1 groups')
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--out', default=None, help='also write the full result (every kernel) as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('occlusion_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    res = {}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        S, M = args.windows, int(net._M0)
        data = net.stage(np.random.RandomState(1).randn(S, M, 15).astype(np.float32))
        labels = np.random.RandomState(2).randint(0, 22, S)
        groups = None if shape == 'atlas' else np.arange(M) >> args.level
        G = M if groups is None else int(groups.max()) + 1
        r = {'M': M, 'batch': B, 'windows': S, 'G': G}
        r['predict_win_s'] = S / timed(lambda: net.predict(data), args.reps)
        r['predict_rows_s'] = r['predict_win_s']
        r['occlusion_win_s'] = S / timed(lambda: net.occlusion(data, groups=groups), args.reps)
        r['occlusion_rows_s'] = r['occlusion_win_s'] * (G + 1)
        r['maps_win_s'] = S / timed(lambda: net.occlusion_maps(data, labels, groups=groups), args.reps)
        r['maps_rows_s'] = r['maps_win_s'] * (G + 1)
        # one call's kernels: a few windows (every pass alike), and the class sums once
        n = max(1, -(-4 * B // (G + 1)))
        r['occlusion_kernels'] = kernel_shares(lambda: net.occlusion(data[:n], groups=groups), NEW)
        r['maps_kernels'] = kernel_shares(lambda: net.occlusion_maps(data[:n], labels[:n], groups=groups), NEW)
        if shape != 'atlas':
            nv = args.vertex_windows
            r['vertex_G'] = M
            r['vertex_win_s'] = nv / timed(lambda: net.occlusion(data[:nv]), 1)
            r['vertex_rows_s'] = r['vertex_win_s'] * (M + 1)
        res[shape] = r
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
