#!/usr/bin/env python3
"""Shapley maps (base_model.shapley / shapley_maps) beside occlusion, at the two shapes of tools/occlusion_bench.py:

  atlas:    training.py's network -- a 360-vertex kNN graph, K = 10, F = [32]*6, channel 15, b1relu, batch 128, head
            M = [512, 256, 22]; groups: 8-vertex parcels (np.arange(M) >> 3, G = 45);
  config1:  BASELINE configs[1] -- the N = 10000 synthetic graph after one coarsening level (M = 10466), K = 5, F = [32]*6,
            b2relu, channel 15, batch 64; groups: the clusters of coarsening level --level (np.arange(M) >> level).

Both methods run on the same groups, so both are forward rows through the same network: a window costs G + 1 rows under
occlusion and P (G + 1) under shapley.  Prints one JSON line: windows/s and forward rows/s of occlusion, shapley and
shapley_maps (device-synchronised, the host copy of the result included), the share of each method's own kernels in the
kernel time of one call (ops.KernelTimers), the row builders' shares of it, and each kernel's HBM share (bytes from the
shapes over 8 TB/s).

    python tools/shapley_bench.py [--windows 16] [--permutations 16] [--reps 3] [--level 6] [--shapes atlas,config1] [--out FILE]
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

OCC = ('occlusion_rows', 'occlusion_score', 'saliency_seed')
NEW = ('shapley_rows', 'shapley_score', 'shapley_reduce', 'occlusion_class_sums', 'saliency_seed')


def _share(shares, name):
    """The share of the launches called ``name`` in the kernel time of an instrumented call."""
    ms = sum(v['avg_ms'] * v['launches'] for k, v in shares['new'].items() if k.split(' | ')[0] == name)
    return ms / shares['kernels_ms'] if shares['kernels_ms'] else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=16)
    ap.add_argument('--permutations', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--level', type=int, default=6, help='coarsening level of the config1 groups')
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--out', default=None, help='also write the full result as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('shapley_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    P = args.permutations
    res = {}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        S, M = args.windows, int(net._M0)
        data = net.stage(np.random.RandomState(1).randn(S, M, 15).astype(np.float32))
        labels = np.random.RandomState(2).randint(0, 22, S)
        groups = np.arange(M) >> (3 if shape == 'atlas' else args.level)
        G = int(groups.max()) + 1
        r = {'M': M, 'batch': B, 'windows': S, 'G': G, 'P': P}
        r['occlusion_win_s'] = S / timed(lambda: net.occlusion(data, groups=groups), args.reps)
        r['occlusion_rows_s'] = r['occlusion_win_s'] * (G + 1)
        r['shapley_win_s'] = S / timed(lambda: net.shapley(data, groups=groups, permutations=P), args.reps)
        r['shapley_rows_s'] = r['shapley_win_s'] * P * (G + 1)
        r['maps_win_s'] = S / timed(lambda: net.shapley_maps(data, labels, groups=groups, permutations=P), args.reps)
        r['maps_rows_s'] = r['maps_win_s'] * P * (G + 1)
        # one call's kernels on a few passes (every pass alike)
        n = max(1, -(-4 * B // (G + 1)))
        r['occlusion_kernels'] = kernel_shares(lambda: net.occlusion(data[:n], groups=groups), OCC)
        r['occlusion_rows_share'] = _share(r['occlusion_kernels'], 'occlusion_rows')
        n = max(1, -(-4 * B // (P * (G + 1))))
        r['shapley_kernels'] = kernel_shares(lambda: net.shapley(data[:n], groups=groups, permutations=P), NEW)
        r['shapley_rows_share'] = _share(r['shapley_kernels'], 'shapley_rows')
        res[shape] = r
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
