#!/usr/bin/env python3
"""Saliency maps (cgcnn.saliency) against predict() and the eager training step, at two shapes:

  atlas:    training.py's network -- a 360-vertex kNN graph, K = 10, F = [32]*6, p = [1]*6, channel 15, b1relu, batch 128,
            head M = [512, 256, 22];
  config1:  BASELINE configs[1] -- the seeded synthetic N = 10000 graph after one coarsening level (M = 10466), K = 5,
            F = [32]*6, b2relu, channel 15, batch 64, head M = [512, 256, 22].

Prints one JSON line: windows/s of predict, saliency(method='gradient'), saliency(method='integrated', steps=32) and
saliency_maps on S windows each (device-synchronised; the host copy of the result included) and the wall time of one eager
training step at the same batch; kernel time against kernel time (ops.KernelTimers) of one eager training step and one
gradient pass over a batch; the HBM share (bytes from the shapes over 8 TB/s) of the saliency kernels in a gradient and an
integrated pass; and a host profile of one saliency_maps call (where its wall time goes).

    python tools/saliency_bench.py [--windows 512] [--reps 3] [--shapes atlas,config1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcn_fmri_decoding_amd import graph as graph_mod       # noqa: E402
from gcn_fmri_decoding_amd import models_gcn, ops           # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def knn_laplacian(M, k=8, seed=0):
    pts = np.random.RandomState(seed).rand(M, 3).astype(np.float32)
    d, idx = graph_mod.distance_sklearn_metrics(pts, k=k)
    return sp.csr_matrix(graph_mod.laplacian(graph_mod.adjacency(d, idx).astype(np.float32), normalized=True))


def build(shape, dev):
    if shape == 'atlas':
        L, K, B, brelu = [knn_laplacian(360)], 10, 128, 'b1relu'
    else:
        L, K, B, brelu = graph_mod.synthetic_graph(10000, k=8, levels=1)[0][:1], 5, 64, 'b2relu'
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': dev}, L * 6, [32] * 6, [K] * 6, [1] * 6, [512, 256, 22], brelu=brelu, channel=15,
                           batch_size=B, regularization=5e-4, dropout=0.5, verbose=False)
    return net, B


def timed(fn, reps):
    fn()                                        # warm-up: every shape the timed calls use
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def instrumented(fn):
    """Per-kernel times of one call (ops.KernelTimers, by kernel template), with the HBM share of each."""
    ops.timers = ops.KernelTimers(by_dispatch=True)
    try:
        ops.timers.next_step()
        fn()
        kern = ops.timers.summary()
    finally:
        ops.timers = None
    for v in kern.values():
        v['hbm_share'] = v['bytes'] / (v['total_ms'] * 1e-3) / HBM_BYTES_PER_S if v['total_ms'] > 0 else 0.0
    return kern


def kernel_shares(fn, names):
    """One instrumented call: its kernel time, and the share and per-kernel figures of the launches called ``names``."""
    kern = instrumented(fn)
    total = sum(v['total_ms'] for v in kern.values())
    new = {k: v for k, v in kern.items() if k.split(' | ')[0] in names}
    return {'kernels_ms': total, 'new_kernels_ms': sum(v['total_ms'] for v in new.values()),
            'new_share': sum(v['total_ms'] for v in new.values()) / total if total else 0.0,
            'new': {k: {'launches': v['launches'], 'avg_ms': v['avg_ms'], 'bytes': v['bytes'], 'hbm_share': v['hbm_share']}
                    for k, v in new.items()}}


def host_profile(fn, batches):
    """One call under cProfile: wall ms per batch, ms per batch spent in Tensor.cpu (waiting for the device and copying the
    result), the top host functions by own time, and the allocator's counters over the call."""
    import cProfile
    import pstats
    fn()
    torch.cuda.synchronize()
    keys = ('num_device_alloc', 'num_device_free', 'num_alloc_retries', 'num_sync_all_streams')
    before = torch.cuda.memory_stats()
    prof = cProfile.Profile()
    t0 = time.perf_counter()
    prof.enable()
    fn()
    prof.disable()
    wall = time.perf_counter() - t0
    after = torch.cuda.memory_stats()
    st = pstats.Stats(prof).stats
    own = sorted(((v[2], '%s:%d:%s' % (k[0].split('/')[-1], k[1], k[2])) for k, v in st.items()), reverse=True)[:8]
    cpu_wait = sum(v[3] for k, v in st.items() if k[2] in ("<method 'cpu' of 'torch._C.TensorBase' objects>",
                                                           "<method 'cpu' of 'torch._C._TensorBase' objects>"))
    return {'wall_ms_per_batch': 1e3 * wall / batches, 'cpu_copy_wait_ms_per_batch': 1e3 * cpu_wait / batches,
            'top_own_ms_per_batch': [(round(1e3 * t / batches, 3), name) for t, name in own],
            'allocator': {k: after.get(k, 0) - before.get(k, 0) for k in keys if k in after}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=32, help='steps of the integrated gradients')
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--out', default=None, help='also write the full result (every kernel) as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('saliency_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    res = {}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        S = args.windows
        data = net.stage(np.random.RandomState(1).randn(S, net._M0, 15).astype(np.float32))
        labels = np.random.RandomState(2).randint(0, 22, S)
        r = {'M': int(net._M0), 'batch': B, 'windows': S}
        r['predict_win_s'] = S / timed(lambda: net.predict(data), args.reps)
        r['gradient_win_s'] = S / timed(lambda: net.saliency(data), args.reps)
        r['integrated%d_win_s' % args.steps] = S / timed(lambda: net.saliency(data, method='integrated', steps=args.steps),
                                                        args.reps)
        r['maps_gradient_win_s'] = S / timed(lambda: net.saliency_maps(data, labels), args.reps)
        # one eager training step at the same batch (what a gradient pass is a subset of)
        x = net._gather(data, torch.arange(B, dtype=torch.int32, device=dev))
        lab = torch.as_tensor(labels[:B]).to(dev)
        r['train_step_eager_ms'] = 1e3 * timed(lambda: net.train_step(x, lab), args.reps * 5)
        r['gradient_pass_ms'] = 1e3 * B / r['gradient_win_s']
        r['maps_pass_ms'] = 1e3 * B / r['maps_gradient_win_s']
        # kernel time against kernel time: one instrumented eager training step, one instrumented gradient pass (one batch)
        kern_train = instrumented(lambda: net.train_step(x, lab))
        r['train_step_kernels_ms'] = sum(v['total_ms'] for v in kern_train.values())
        kern = instrumented(lambda: net.saliency(data[:B], batch_size=B))
        r['gradient_pass_kernels_ms'] = sum(v['total_ms'] for v in kern.values())
        r['kernels_gradient_batch'] = kern
        kern_ig = instrumented(lambda: net.saliency(data[:B], method='integrated', steps=args.steps, batch_size=B))
        r['saliency_kernels'] = {k: {'avg_ms': v['avg_ms'], 'hbm_share': v['hbm_share']}
                                 for k, v in list(kern.items()) + list(kern_ig.items()) if k.startswith('saliency_')}
        # where the wall time of a saliency_maps call goes on the host: Python profile of one call (time spent waiting on the
        # device shows up in the device-to-host copies), and the caching allocator's device allocations / frees / retries
        r['maps_host'] = host_profile(lambda: net.saliency_maps(data, labels), S // B)
        res[shape] = r
        del net
        torch.cuda.empty_cache()
    line = {s: {k: v for k, v in r.items() if k != 'kernels_gradient_batch'} for s, r in res.items()}
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
