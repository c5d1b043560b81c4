#!/usr/bin/env python3
"""connectome measured: per-run partial correlation matrices (Ledoit-Wolf shrinkage) on the device against what a user would
otherwise run -- torch on the same device (float64 centring, ``bmm``, batched ``torch.linalg.inv``; where the vendor library
refuses that, ``cholesky`` + ``cholesky_inverse``, and the JSON says so) and the host path
(scikit-learn ``LedoitWolf`` + ``numpy.linalg.inv`` per run, thread pools limited to 16).

  hcp284    S x T x R = 256 x 284 x 360     one HCP task run per subject on the MMP atlas
  rest1200  S x T x R =  64 x 1200 x 360    resting-state runs

Per case, on resident planes, HIP events around each C entry (after --warmup calls, --reps repeats: median / min / max):
``cov_ms`` (centre + rowsq + cov kernels), ``finish_ms`` (finish<inverse> + invert + gram), ``mean_ms``, ``call_ms`` the three
together; ``torch_cov_ms`` / ``torch_inv_ms`` / ``torch_ms`` the torch path; ``device_s`` the wall time of the whole Python call
(staging and upload included); ``host_s`` the host path (one pass; skipped with --no-host).  Beside them two floors:
``fma_floor_ms`` the float64 FMAs of the covariance pass, S T R (R + 1) / 2, and of the inverse, S R^3 / 2, at the 39.3 T FMA/s
vector rate, and ``read_floor_ms`` the planes read once at the 6.29 TB/s copy rate (both rates: DESIGN 4.22).  The kernels of one
entry are told apart by a profiler run of this tool (``--kernel-trace --stats``); events cannot separate launches of one call.
Prints one JSON line and writes profiles/connectome_bench.json.  Needs a GPU.

    python tools/connectome_bench.py [--cases hcp284,rest1200] [--reps 20] [--warmup 2] [--no-host] [--out FILE]
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

from gcn_fmri_decoding_amd import _lib, connectome as cn, ops   # noqa: E402

FMA_RATE_F64 = 39.3e12
COPY_RATE = 6.29e12
CASES = {'hcp284': (256, 284, 360), 'rest1200': (64, 1200, 360)}
HOST_THREADS = 16


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


def series(S, T, R, seed=0):
    """Latent-factor AR(1) runs [S, T, R] float32."""
    rng = np.random.RandomState(seed)
    e = rng.randn(S, T, 6)
    f = np.empty_like(e)
    f[:, 0] = e[:, 0]
    for t in range(1, T):
        f[:, t] = 0.4 * f[:, t - 1] + e[:, t]
    return (f @ rng.randn(6, R) + rng.randn(S, T, R)).astype(np.float32)


def torch_cov(x):
    """[S, T, R] float32 on the device -> the Ledoit-Wolf shrunk covariance, float64 [S, R, R]."""
    S, T, R = x.shape
    d = x.double()
    d = d - d.mean(dim=1, keepdim=True)
    C = torch.bmm(d.transpose(1, 2), d) / T
    q = (d * d).sum(dim=2)
    beta_ = (q * q).sum(dim=1)
    delta_ = (C * C).sum(dim=(1, 2))
    tr = torch.diagonal(C, dim1=1, dim2=2).sum(dim=1)
    mu = tr / R
    beta = (beta_ / T - delta_) / (R * T)
    delta = (delta_ - 2.0 * mu * tr + R * mu * mu) / R
    s = torch.clamp(torch.minimum(beta, delta), min=0.0) / delta
    return (1.0 - s)[:, None, None] * C + (s * mu)[:, None, None] * torch.eye(R, dtype=torch.float64, device=x.device)


def torch_inverse(sigma, how):
    if how == 'inv':
        return torch.linalg.inv(sigma)
    return torch.cholesky_inverse(torch.linalg.cholesky(sigma))


def torch_partial(sigma, how='inv'):
    P = torch_inverse(sigma, how)
    dd = torch.diagonal(P, dim1=1, dim2=2)
    out = -P / torch.sqrt(dd[:, :, None] * dd[:, None, :])
    out.diagonal(dim1=1, dim2=2).fill_(1.0)
    return out.float()


def host_partial(x):
    from sklearn.covariance import LedoitWolf
    out = np.empty((x.shape[0], x.shape[2], x.shape[2]), np.float32)
    for s, run in enumerate(x):
        P = np.linalg.inv(LedoitWolf(store_precision=False).fit(run.astype(np.float64)).covariance_)
        dd = np.diag(P)
        m = -P / np.sqrt(np.outer(dd, dd))
        np.fill_diagonal(m, 1.0)
        out[s] = m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='hcp284,rest1200')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'connectome_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('connectome_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    torch.set_num_threads(min(HOST_THREADS, torch.get_num_threads()))
    res = {'device': torch.cuda.get_device_name(0), 'cus': torch.cuda.get_device_properties(0).multi_processor_count,
           'torch': torch.__version__, 'hip': torch.version.hip, 'reps': args.reps, 'warmup': args.warmup,
           'host_cpus': len(os.sched_getaffinity(0)), 'kind': 'partial correlation', 'shrinkage': 'auto',
           'geometry': ops.connectome_geometry()}
    kind = cn.KINDS.index('partial correlation')
    for case in args.cases.split(','):
        if case not in CASES:
            raise SystemExit('connectome_bench: unknown case %r' % case)
        S, T, R = CASES[case]
        x = series(S, T, R)
        Rp = ops.plane_stride(R)
        planes = torch.zeros((S * T, Rp), dtype=torch.float32, device=dev)
        planes[:, :R] = torch.as_tensor(x.reshape(S * T, R)).to(dev)
        offs = torch.as_tensor(np.arange(S + 1, dtype=np.int64) * T).to(dev)
        mats = torch.empty((S, R, R), dtype=torch.float32, device=dev)
        shr = torch.empty((S,), dtype=torch.float64, device=dev)
        flags = torch.empty((S,), dtype=torch.int32, device=dev)
        r = {'S': S, 'T': T, 'R': R}

        def cov():
            return ops.connectome_cov(planes, offs, R)

        def finish():
            ops.connectome_finish(ops.connectome_cov(planes, offs, R), offs, S * T, R, kind, -1.0, mats, shr, flags)

        def call():
            finish()
            return ops.connectome_mean(mats, flags)

        r['cov_ms'] = spread(event_ms(cov, args.warmup, args.reps))
        r['cov_dispatch'] = _lib.last_dispatch()
        both = event_ms(finish, args.warmup, args.reps)             # (finish overwrites what cov left: timed together, cov taken off)
        r['finish_dispatch'] = _lib.last_dispatch()
        r['finish_ms'] = spread(np.asarray(both) - r['cov_ms']['median'])
        r['mean_ms'] = spread(event_ms(lambda: ops.connectome_mean(mats, flags), args.warmup, args.reps))
        r['call_ms'] = spread(event_ms(call, args.warmup, args.reps))
        r['degenerate_runs'] = int(flags.sum().item())
        xs = planes[:, :R].reshape(S, T, R)
        r['torch_cov_ms'] = spread(event_ms(lambda: torch_cov(xs), args.warmup, args.reps))
        sigma = torch_cov(xs)
        print(case, json.dumps(r), file=sys.stderr, flush=True)
        for how in ('inv', 'cholesky_inverse'):                  # (batched float64 inv may be refused by the vendor library)
            try:
                r['torch_inv_ms'] = spread(event_ms(lambda: torch_partial(sigma, how), args.warmup, args.reps))
                r['torch_ms'] = spread(event_ms(lambda: torch_partial(torch_cov(xs), how).mean(dim=0), args.warmup, args.reps))
                r['max_abs_diff_to_torch'] = float((torch_partial(sigma, how) - mats).abs().max().item())
                r['torch_inverse'] = how
                break
            except RuntimeError as e:
                r['torch_%s_error' % how] = str(e).splitlines()[0][:200]
        r['fma_floor_ms'] = {'cov': 1e3 * S * T * R * (R + 1) / 2 / FMA_RATE_F64, 'inverse': 1e3 * S * R ** 3 / 2 / FMA_RATE_F64}
        r['read_floor_ms'] = 1e3 * 4.0 * S * T * Rp / COPY_RATE
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = cn.connectome(list(x), 'partial correlation', device=dev)
        torch.cuda.synchronize()
        r['device_s'] = time.perf_counter() - t0
        if not args.no_host:
            try:
                from threadpoolctl import threadpool_limits
                limit = threadpool_limits(limits=HOST_THREADS)
            except ImportError:
                limit = None
            t0 = time.perf_counter()
            ref = host_partial(x)
            r['host_s'] = time.perf_counter() - t0
            r['host_threads_limited'] = limit is not None
            r['max_abs_diff_to_host'] = float(np.abs(got.matrices.cpu().numpy() - ref).max())
        res[case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
        del planes, mats, sigma, xs
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
