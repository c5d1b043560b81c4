#!/usr/bin/env python3
"""Monte-Carlo dropout (cgcnn.predict_mc) against what it replaces, at the two shapes of tools/saliency_bench.py:

  atlas:    training.py's network -- a 360-vertex kNN graph, K = 10, F = [32]*6, p = [1]*6, channel 15, b1relu, batch 128;
  config1:  BASELINE configs[1] -- the seeded synthetic N = 10000 graph after one coarsening level (M = 10466), K = 5,
            F = [32]*6, b2relu, channel 15, batch 64;
both with the head M = [512, 256, 22] and dropout 0.5.

For 256 staged windows and S = 32 samples, device-synchronised, the best of --reps repetitions after a warm-up:
  (a) predict(): one deterministic pass, the floor;
  (b) THE BASELINE: S stochastic passes of the whole network, ``_inference_storage(x, dropout)`` with dropout on torch's
      generator over batches gathered once -- what a user had to do before predict_mc (S trunk passes, and a result that
      depends on the batch size and on every call before it);
  (c) predict_mc(samples=S): one trunk pass, the sampled head, the reduction.
Then the per-kernel times of one predict_mc call (ops.KernelTimers, by kernel template), and the head alone at one batch: the
two fused launches of chebgcn_fc_fwd_dropout (S samples each) against 2 S launches of chebgcn_fc_fwd on inputs masked
beforehand (the masking itself not timed: the floor of a version that stores its masks).  Prints one JSON line.  Needs a GPU.

    python tools/mc_bench.py [--reps 5] [--shapes atlas,config1] [--samples 32] [--windows 256] [--out FILE]
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

from gcn_fmri_decoding_amd import ops, uncertainty   # noqa: E402
from saliency_bench import build, instrumented, timed   # noqa: E402


def event_ms(fn, reps):
    """Best device time of fn() in ms over ``reps`` runs after a warm-up (HIP events around the whole call)."""
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def head_alone(net, B, S, reps):
    """The sampled layers behind fc1 at one batch: fused (2 launches) against plain fc_fwd on stored masked inputs (2 S)."""
    dev = net.device
    M1, M2, C = (int(m) for m in net.M)
    var = lambda n: net._params[n].detach()
    h = torch.relu(torch.randn(B, M1, device=dev))
    win = torch.arange(B, dtype=torch.int32, device=dev)
    T, inv = uncertainty.dropout_threshold(0.5)

    def fused():
        h2 = ops.fc_forward_dropout(h, var('fc2/weights'), var('fc2/bias'), True, win, S, 0, 0, 0, T, inv)
        return ops.fc_forward_dropout(h2, var('logits/weights'), var('logits/bias'), False, win, S, 0, 1, 0, T, inv)
    m1 = (torch.rand(S, B, M1, device=dev) < 0.5).float() * 2.0
    m2 = (torch.rand(S, B, M2, device=dev) < 0.5).float() * 2.0
    hm = h[None] * m1                                                     # stored masked inputs of the first site

    def plain():
        out = []
        for s in range(S):
            h2 = ops.fc_forward(hm[s], var('fc2/weights'), var('fc2/bias'), True)
            out.append(ops.fc_forward(h2 * m2[s], var('logits/weights'), var('logits/bias'), False))
        return out

    def plain_no_mask():                                                  # the 2 S launches alone: no second-site masking
        for s in range(S):
            ops.fc_forward(ops.fc_forward(hm[s], var('fc2/weights'), var('fc2/bias'), True), var('logits/weights'),
                           var('logits/bias'), False)
    return {'fused_ms': event_ms(fused, reps), 'plain_fc_fwd_ms': event_ms(plain_no_mask, reps),
            'plain_fc_fwd_with_second_mask_ms': event_ms(plain, reps), 'launches_fused': 2, 'launches_plain': 2 * S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--samples', type=int, default=32)
    ap.add_argument('--windows', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mc_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    S, n = args.samples, args.windows
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hip': torch.version.hip, 'reps': args.reps,
           'samples': S, 'windows': n}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        M, C = int(net._M0), int(net.channel)
        staged = net.stage(np.random.RandomState(0).randn(n, M, C).astype(np.float32))
        batches = [net._gather(staged, torch.arange(b0, min(b0 + B, n), dtype=torch.int32, device=dev)) for b0 in range(0, n, B)]

        def loop():
            net.training_mode = False
            with torch.no_grad():
                for _ in range(S):
                    for x in batches:
                        net._inference_storage(x, net.dropout)
            torch.cuda.synchronize()
        r = {'M': M, 'batch': B, 'head': [int(m) for m in net.M]}
        r['predict_ms'] = 1e3 * timed(lambda: net.predict(staged), args.reps)
        r['loop_of_%d_passes_ms' % S] = 1e3 * timed(loop, args.reps)
        r['predict_mc_ms'] = 1e3 * timed(lambda: net.predict_mc(staged, samples=S, seed=0), args.reps)
        r['predict_mc_over_predict'] = r['predict_mc_ms'] / r['predict_ms']
        r['loop_over_predict_mc'] = r['loop_of_%d_passes_ms' % S] / r['predict_mc_ms']
        k = instrumented(lambda: net.predict_mc(staged, samples=S, seed=0))
        r['kernels_ms'] = sum(v['total_ms'] for v in k.values())
        r['by_kernel'] = {name: {'launches': v['launches'], 'total_ms': v['total_ms']} for name, v in k.items()}
        r['head_alone_one_batch'] = head_alone(net, B, S, args.reps)
        res[shape] = r
        del net, staged, batches
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
