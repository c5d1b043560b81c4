#!/usr/bin/env python3
"""Training step of finetuning_cgcnn against the full cgcnn step, on the reference network of training.py rebuilt as the
trunk: a 360-vertex kNN graph (the atlas size), K = 10, F = [32]*6, p = [1]*6, channel 15, batch 128, head M = [512, 256, 22].

Prints one JSON line: the captured, device-synchronised step time of the fine-tuning model with flag_tuning False (frozen
trunk) and True (conv4 ... conv6 trained) and of the full cgcnn step of the same network in the same process; the per-kernel
times of one instrumented (eager) step of each fine-tuning model (ops.KernelTimers, by kernel template); and the share of
the HBM bandwidth the Nadam pass and the newfc1 kernels reach (bytes from the shapes, over 8 TB/s).

    python tools/finetune_bench.py [--steps 50] [--warmup 5] [--out FILE]

--out also writes the full result (every kernel's entry) as JSON to FILE.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
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


def time_steps(net, x, labels, steps, warmup):
    """Mean captured step time (ms) over ``steps`` steps after ``warmup`` (the third step captures)."""
    net.enable_step_graph(True)
    for _ in range(warmup):
        net.train_step(x, labels)
    torch.cuda.synchronize()
    if net._sg is None:
        raise SystemExit('finetune_bench: the step was not captured')
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(x, labels)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def kernels_of_one_step(net, x, labels):
    ops.timers = ops.KernelTimers(by_dispatch=True)
    try:
        ops.timers.next_step()
        net.train_step(x, labels)           # (eager: timers keep the step out of the graph)
        kern = ops.timers.summary()
    finally:
        ops.timers = None
    for v in kern.values():
        v['hbm_share'] = v['bytes'] / (v['total_ms'] * 1e-3) / HBM_BYTES_PER_S if v['total_ms'] > 0 else 0.0
    return kern


def share(kern, prefix):
    picked = [v for k, v in kern.items() if k.split(' |')[0] == prefix]
    ms = sum(v['total_ms'] for v in picked)
    nbytes = sum(v['bytes'] for v in picked)
    return {'ms': ms, 'bytes': nbytes, 'hbm_share': nbytes / (ms * 1e-3) / HBM_BYTES_PER_S if ms > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', type=int, default=360)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the full result as JSON here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('finetune_bench: no GPU visible (the measurement does not fall back to the CPU)')
    if args.warmup < 3:
        raise SystemExit('finetune_bench: --warmup must be at least 3 (the third step captures)')
    dev = torch.device('cuda', 0)
    M, B, channel = args.M, args.batch, 15
    F, K, p, Mfc = [32] * 6, [10] * 6, [1] * 6, [512, 256, 22]
    L = knn_laplacian(M)
    rs = np.random.RandomState(1)
    x = ops.plane_storage(torch.as_tensor(rs.randn(B, M, channel).astype(np.float32)).to(dev))
    labels = torch.as_tensor(rs.randint(0, Mfc[-1], size=B)).to(dev)

    home = tempfile.mkdtemp(prefix='finetune_bench_')
    os.environ['CHEBGCN_HOME'] = home
    torch.manual_seed(0)
    full = models_gcn.cgcnn({'device': dev}, [L], F, K, p, Mfc, brelu='b1relu', channel=channel, batch_size=B,
                            regularization=5e-4, dropout=0.5, dir_name='pretrained', verbose=False)
    full._save_best(0.0, 1, [])                 # the trunk the fine-tuning models read
    root = home + '/checkpoints/'
    res = {'shape': dict(M=M, Mp=ops.plane_stride(M), batch=B, channel=channel, F=F, K=K, p=p, M_fc=Mfc)}
    res['full_step_ms'] = time_steps(full, x, labels, args.steps, args.warmup)
    full.enable_step_graph(False)
    for tuning in (False, True):
        net = models_gcn.finetuning_cgcnn({'device': dev}, root, [L], F, K, p, Mfc, channel=channel, batch_size=B,
                                          regularization=5e-4, dropout=0.5, dir_name='pretrained', flag_tuning=tuning,
                                          verbose=False)
        key = 'tuning' if tuning else 'frozen'
        res[key + '_step_ms'] = time_steps(net, x, labels, args.steps, args.warmup)
        net.enable_step_graph(False)
        kern = kernels_of_one_step(net, x, labels)
        res[key + '_trained_variables'] = int(net._n_train)
        res[key + '_kernels_one_step'] = kern
        res[key + '_kernels_sum_ms'] = sum(v['total_ms'] for v in kern.values())
        res[key + '_nadam'] = share(kern, 'nadam')
        # (the timed fc_fwd / fc_bwd launches are newfc1's: ops.FlatFC; the small layers behind it are not instrumented)
        res[key + '_newfc1_fwd'] = share(kern, 'fc_fwd')
        res[key + '_newfc1_bwd'] = share(kern, 'fc_bwd')
        del net
    shutil.rmtree(home, ignore_errors=True)
    for key in ('frozen', 'tuning'):
        res[key + '_vs_full'] = res[key + '_step_ms'] / res['full_step_ms']
    line = {k: v for k, v in res.items() if not k.endswith('_kernels_one_step')}
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
