#!/usr/bin/env python3
"""Eager training step of the reference's Fourier model (training.py:56-62 with model.py:182-225: filter='fourier',
F = [32]*6, p = [1]*6, M = [512, 256, 22], channel 15, batch 128) on a 360-vertex kNN graph (the atlas size).

Prints one JSON line: the step time (device-synchronised wall clock over --steps steps), the per-kernel times of one
instrumented step (ops.KernelTimers, by kernel template), the Fourier transform's share of the 157.3 TF fp32 matrix peak,
and the same step restated in torch on the CPU (fp32, autograd) for comparison.

    python tools/spectral_bench.py [--steps 20] [--warmup 3] [--cpu-steps 2] [--out FILE]

--out also writes the full result (every kernel's entry) as JSON to FILE.
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

PEAK_F32_MATRIX = 157.3e12


def atlas_laplacian(M, k=8, seed=0):
    z = np.random.RandomState(seed).rand(M, 3).astype(np.float32)
    d, idx = graph_mod.distance_sklearn_metrics(z, k=k)
    A = graph_mod.adjacency(d, idx).astype(np.float32)
    return sp.csr_matrix(graph_mod.laplacian(A, normalized=True))


def cpu_step(U, params, x, labels, F, Mfc):
    """The same forward + backward in torch fp32 on the CPU (autograd; no optimizer)."""
    h = x
    for i in range(len(F)):
        W, b = params['conv%d/weights' % (i + 1)], params['conv%d/bias' % (i + 1)]
        xh = torch.einsum('jm,njf->nmf', U, h)
        yh = torch.einsum('mof,nmf->nmo', W, xh)
        h = torch.relu(torch.einsum('jm,nmo->njo', U, yh) + b)
    h = h.mean(dim=2)
    for i in range(len(Mfc)):
        scope = 'logits' if i == len(Mfc) - 1 else 'fc%d' % (i + 1)
        h = h @ params[scope + '/weights'] + params[scope + '/bias']
        if i < len(Mfc) - 1:
            h = torch.relu(h)
    loss = torch.nn.functional.cross_entropy(h, labels)
    loss.backward()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', type=int, default=360)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cpu-steps', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the full result as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spectral_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    M, B, channel = args.M, args.batch, 15
    F, K, p, Mfc = [32] * 6, [5] * 6, [1] * 6, [512, 256, 22]
    L = atlas_laplacian(M)
    t0 = time.time()
    net = models_gcn.cgcnn({'device': dev}, [L], F, K, p, Mfc, filter='fourier', brelu='b1relu', channel=channel,
                           batch_size=B, regularization=5e-4, dropout=0.5, verbose=False)
    t_build = time.time() - t0
    rs = np.random.RandomState(1)
    x = ops.plane_storage(torch.as_tensor(rs.randn(B, M, channel).astype(np.float32)).to(dev))
    labels = torch.as_tensor(rs.randint(0, Mfc[-1], size=B)).to(dev)

    for _ in range(args.warmup):
        net.train_step(x, labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        net.train_step(x, labels)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / args.steps * 1e3

    ops.timers = ops.KernelTimers(by_dispatch=True)
    ops.timers.next_step()
    net.train_step(x, labels)
    kern = ops.timers.summary()
    ops.timers = None
    Mp = ops.plane_stride(M)
    tr = {k: v for k, v in kern.items() if k.startswith('spectral_analysis') or k.startswith('spectral_synthesis')}
    tr_ms = sum(v['total_ms'] for v in tr.values())
    tr_flops = sum(v['flops'] for v in tr.values())
    # useful work: only the M x M part of the padded Mp x Mp basis
    tr_useful = tr_flops * (M / Mp) ** 2
    for v in kern.values():
        v['tflops'] = v['flops'] / (v['total_ms'] * 1e-3) / 1e12 if v['total_ms'] > 0 else 0.0
    all_ms = sum(v['total_ms'] for v in kern.values())

    # the torch-CPU restatement of the same step
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    _, U = graph_mod.fourier(L)
    Uc = torch.as_tensor(U)
    params = {n: torch.tensor(net.get_var(n), requires_grad=True) for n in net.variables()}
    xc = torch.as_tensor(rs.randn(B, M, channel).astype(np.float32))
    lc = labels.cpu()
    cpu_step(Uc, params, xc, lc, F, Mfc)
    t0 = time.perf_counter()
    for _ in range(args.cpu_steps):
        cpu_step(Uc, params, xc, lc, F, Mfc)
    cpu_ms = (time.perf_counter() - t0) / args.cpu_steps * 1e3

    res = dict(shape=dict(M=M, Mp=Mp, batch=B, channel=channel, F=F, M_fc=Mfc), model_build_s=round(t_build, 3),
               step_ms=step_ms, steps=args.steps, kernels_one_step=kern, kernels_sum_ms=all_ms,
               transform_ms=tr_ms, transform_launches=sum(v['launches'] for v in tr.values()),
               transform_tflops_padded=tr_flops / (tr_ms * 1e-3) / 1e12,
               transform_fraction_of_peak=tr_flops / (tr_ms * 1e-3) / PEAK_F32_MATRIX,
               transform_fraction_of_peak_useful=tr_useful / (tr_ms * 1e-3) / PEAK_F32_MATRIX,
               cpu_torch_threads=torch.get_num_threads(), cpu_torch_fwd_bwd_ms=cpu_ms)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'kernels_one_step'}))
    for k, v in sorted(kern.items(), key=lambda kv: -kv[1]['total_ms']):
        print('%-70s %3d x %8.4f ms  %6.2f TF' % (k, v['launches'], v['avg_ms'], v['tflops']))


if __name__ == '__main__':
    main()
