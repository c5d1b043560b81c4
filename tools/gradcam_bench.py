#!/usr/bin/env python3
"""Grad-CAM maps (base_model.gradcam / gradcam_maps) against predict() and saliency(method='gradient'), at the two shapes of
tools/saliency_bench.py:

  atlas:    training.py's network -- a 360-vertex kNN graph, K = 10, F = [32]*6, channel 15, b1relu, batch 128, head
            M = [512, 256, 22];
  config1:  BASELINE configs[1] -- the N = 10000 synthetic graph after one coarsening level (M = 10466, relabelled), K = 5,
            F = [32]*6, b2relu, channel 15, batch 64.

Prints one JSON line: windows/s of predict, saliency(method='gradient'), gradcam at conv1 and at the top layer (both methods at
the top) and gradcam_maps (device-synchronised, the host copy of the result included); the share of the new kernels
(gradcam_weights, gradcam_map) in the kernel time of one pass (ops.KernelTimers); and each new kernel's HBM share, its bytes
computed from the shapes (B F N 4 per operand read, B M 4 written) over 8 TB/s.

    python tools/gradcam_bench.py [--windows 512] [--reps 3] [--shapes atlas,config1] [--out FILE]
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

from saliency_bench import build, instrumented, kernel_shares, timed      # noqa: E402

NEW = ('gradcam_weights', 'gradcam_map')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--out', default=None, help='also write the full result (every kernel) as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gradcam_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    res = {}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        S, M = args.windows, int(net._M0)
        data = net.stage(np.random.RandomState(1).randn(S, M, 15).astype(np.float32))
        labels = np.random.RandomState(2).randint(0, 22, S)
        top = 'conv%d' % len(net.p)
        r = {'M': M, 'batch': B, 'windows': S}
        r['predict_win_s'] = S / timed(lambda: net.predict(data), args.reps)
        r['saliency_gradient_win_s'] = S / timed(lambda: net.saliency(data), args.reps)
        r['gradcam_conv1_win_s'] = S / timed(lambda: net.gradcam(data, 'conv1'), args.reps)
        r['gradcam_top_win_s'] = S / timed(lambda: net.gradcam(data, top), args.reps)
        r['gxa_top_win_s'] = S / timed(lambda: net.gradcam(data, top, method='grad_x_activation'), args.reps)
        r['maps_top_win_s'] = S / timed(lambda: net.gradcam_maps(data, labels, layer=top), args.reps)
        r['top_vs_saliency'] = r['gradcam_top_win_s'] / r['saliency_gradient_win_s']
        # one pass (one batch) of each: the kernel time and the new kernels' share of it
        r['kernels_conv1'] = kernel_shares(lambda: net.gradcam(data[:B], 'conv1', batch_size=B), NEW)
        r['kernels_top'] = kernel_shares(lambda: net.gradcam(data[:B], top, batch_size=B), NEW)
        r['kernels_top_gxa'] = kernel_shares(lambda: net.gradcam(data[:B], top, method='grad_x_activation', batch_size=B), NEW)
        r['kernels_saliency'] = sum(v['total_ms'] for v in instrumented(lambda: net.saliency(data[:B], batch_size=B)).values())
        res[shape] = r
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
