#!/usr/bin/env python3
"""tangent measured: the batched Jacobi eigensolver alone and the whole ``connectome.tangent`` against what a user would
otherwise run -- batched float64 ``torch.linalg.eigh`` plus ``bmm`` on the same device driving the same iteration, and
``tangent_host`` (NumPy ``eigh`` per matrix, thread pools limited to 16).

  hcp284    S x T x R = 256 x 284 x 360     one HCP task run per subject on the MMP atlas
  rest1200  S x T x R =  64 x 1200 x 360    resting-state runs

Per case, HIP events (after --warmup calls, --reps repeats: median / min / max): ``eigh_ms`` chebgcn_sym_eigh on the S shrunk
covariances whitened by their arithmetic mean (what every iteration decomposes), with its sweep counts; ``torch_eigh_ms``
``torch.linalg.eigh`` on the same stack; ``tangent_s`` / ``torch_tangent_s`` the wall time of the whole iteration on resident
float64 Sigma (``tangent`` also stages the scans); ``host_s`` the host path (one pass; skipped with --no-host).  Beside them
``fma_floor_ms``: the float64 FMAs of one solve, sweeps x 4 S R^3 (the Gram entries and the two updates of every block pair), at
the 39.3 T FMA/s vector rate.  Prints one JSON line and writes profiles/tangent_bench.json.  Needs a GPU.

    python tools/tangent_bench.py [--cases hcp284,rest1200] [--reps 20] [--warmup 2] [--tangent-reps 20] [--no-host] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcn_fmri_decoding_amd import _lib, connectome as cn, ops   # noqa: E402
from connectome_bench import CASES, FMA_RATE_F64, HOST_THREADS, event_ms, series, spread, torch_cov   # noqa: E402


def torch_fun(A, f):
    w, V = torch.linalg.eigh(A)
    return torch.matmul(V * f(w)[..., None, :], V.transpose(-1, -2))


def torch_tangent(sigma, max_iter=30, tol=1e-7):
    """nilearn's rule on batched ``torch.linalg.eigh`` and ``matmul`` -> (G, the tangent matrices float32, iterations)."""
    R = sigma.shape[-1]
    G = sigma.mean(dim=0)
    step, norm_old, it = 1.0, np.inf, 0
    for it in range(1, max_iter + 1):
        w, V = torch.linalg.eigh(G)
        W = (V / torch.sqrt(w)) @ V.T
        H = (V * torch.sqrt(w)) @ V.T
        M = torch_fun(W @ sigma @ W, torch.log).mean(dim=0)
        norm = float(torch.linalg.norm(M))
        G = H @ torch_fun(M, lambda x: torch.exp(step * x)) @ H
        G = (G + G.T) / 2
        if norm < norm_old:
            norm_old = norm
        elif norm > norm_old:
            step, norm = step / 2.0, norm_old
        if norm / R ** 2 < tol:
            break
    W = torch_fun(G, lambda x: 1 / torch.sqrt(x))
    return G, torch_fun(W @ sigma @ W, torch.log).float(), it


def wall(fn, warmup, reps):
    out = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='hcp284,rest1200')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--tangent-reps', type=int, default=20)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tangent_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tangent_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    torch.set_num_threads(min(HOST_THREADS, torch.get_num_threads()))
    res = {'device': torch.cuda.get_device_name(0), 'cus': torch.cuda.get_device_properties(0).multi_processor_count,
           'torch': torch.__version__, 'hip': torch.version.hip, 'reps': args.reps, 'warmup': args.warmup,
           'tangent_reps': args.tangent_reps, 'host_cpus': len(os.sched_getaffinity(0)), 'geometry': ops.tangent_geometry()}
    for case in args.cases.split(','):
        if case not in CASES:
            raise SystemExit('tangent_bench: unknown case %r' % case)
        S, T, R = CASES[case]
        x = series(S, T, R)
        xs = torch.as_tensor(x).to(dev)
        sigma = torch_cov(xs)
        sigma = (sigma + sigma.transpose(1, 2)) / 2
        W = torch_fun(sigma.mean(dim=0), lambda v: 1 / torch.sqrt(v))
        B = W @ sigma @ W
        B = ((B + B.transpose(1, 2)) / 2).contiguous()
        r = {'S': S, 'T': T, 'R': R}
        r['eigh_ms'] = spread(event_ms(lambda: ops.sym_eigh(B), args.warmup, args.reps))
        r['eigh_dispatch'] = _lib.last_dispatch()
        w, Vt, sweeps, ok = ops.sym_eigh(B)
        r['sweeps'] = {'min': int(sweeps.min()), 'max': int(sweeps.max())}
        r['eig_converged'] = bool(ok.all())
        r['torch_eigh_ms'] = spread(event_ms(lambda: torch.linalg.eigh(B), args.warmup, args.reps))
        ref = torch.linalg.eigvalsh(B)
        r['max_eigenvalue_diff_to_torch'] = float((torch.sort(w, dim=1).values - ref).abs().max())
        r['fma_floor_ms'] = 1e3 * r['sweeps']['max'] * 4.0 * S * R ** 3 / FMA_RATE_F64
        print(case, json.dumps(r), file=sys.stderr, flush=True)
        runs = list(x)
        got = cn.tangent(runs, device=dev)
        r['iterations'], r['tangent_sweeps'], r['converged'] = got.iterations, got.sweeps, bool(got.converged)
        r['tangent_s'] = spread(wall(lambda: cn.tangent(runs, device=dev), min(args.warmup, 1), args.tangent_reps))
        G, mats, it = torch_tangent(sigma)
        r['torch_iterations'] = it
        r['torch_tangent_s'] = spread(wall(lambda: torch_tangent(sigma), min(args.warmup, 1), args.tangent_reps))
        r['max_abs_diff_to_torch'] = float((mats - got.matrices).abs().max())
        if not args.no_host:
            try:
                from threadpoolctl import threadpool_limits
                limit = threadpool_limits(limits=HOST_THREADS)
            except ImportError:
                limit = None
            t0 = time.perf_counter()
            host = cn.tangent_host(runs)
            r['host_s'] = time.perf_counter() - t0
            r['host_threads_limited'] = limit is not None
            r['max_abs_diff_to_host'] = float(np.abs(got.matrices.cpu().numpy() - host.matrices).max())
        res[case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
        del xs, sigma, B, got
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
