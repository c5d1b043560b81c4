#!/usr/bin/env python3
"""Per-kernel micro-benchmark of libchebgcn.so on the benchmark graph (M = 10466).

    python tools/kbench.py [--B 64 256] [--fin 32] [--fout 32] [--K 5] [--iters 20]
                           [--kernels recurrence_fwd ...]
    python tools/kbench.py --parcellate [--iters 20] [--json out.json]      # the parcellation leg alone
    python tools/kbench.py glm [--iters 20] [--json out.json]               # the first-level GLM kernels alone
    python tools/kbench.py glm_ar1 [--iters 20] [--json out.json]           # ... and the AR(1) pair beside them and beside torch
    python tools/kbench.py searchlight [--iters 20] [--json out.json]       # the searchlight kernels alone
    python tools/kbench.py searchlight_lda [--iters 10] [--json out.json]   # the LDA searchlight kernel alone
    python tools/kbench.py searchlight_rdm [--iters 10] [--json out.json]   # the RSA searchlight kernel alone
    python tools/kbench.py searchlight_svc [--iters 3] [--json out.json]    # the SVM searchlight kernel alone

Times each C-ABI entry point with HIP events on the launch stream and prints achieved
algorithmic GB/s (SURVEY.md 8d byte counts) and the fraction of the 8 TB/s HBM roofline.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_atlas(V=91282, R=360, cortex=59412, seed=0, scattered=False):
    """Labels shaped like a cortical atlas on grayordinates: the first ``cortex`` vertices belong to R parcels in runs of 1..32
    consecutive indices drawn from a pool of 12 parcels that drifts along V (a parcel is local but not contiguous), the rest
    (subcortex) is background.  ``scattered``: every cortical vertex an independent uniform draw instead."""
    rs = np.random.RandomState(seed)
    lab = np.zeros(V, np.int64)
    if scattered:
        lab[:cortex] = rs.randint(1, R + 1, size=cortex)
    else:
        v = 0
        while v < cortex:
            n = int(rs.randint(1, 33))
            centre = v * R // cortex
            lab[v:min(v + n, cortex)] = 1 + (centre + int(rs.randint(-6, 6))) % R
            v += n
    lab[:R] = np.arange(1, R + 1)           # every parcel exists
    return lab


def _timeit(fn, iters, warm):
    """``(median, min, max)`` ms of ``iters`` event-timed calls of ``fn`` after ``warm`` untimed ones."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in evs:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in evs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def parcellate_leg(args):
    """ops.parcellate on device-resident runs of HCP size against what the parent commit could do -- torch's index_add_ on the
    device, np.add.reduceat on label-sorted columns on the host -- and Parcellation.reduce end to end from host memory."""
    import time
    import torch
    from gcn_fmri_decoding_amd import Parcellation, _lib, ops
    dev = torch.device('cuda:0')
    results = []

    timeit = lambda fn, iters: _timeit(fn, iters, 3)

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    def note(name, T, atlas, t, nbytes):
        med, lo, hi = t
        r = {'leg': name, 'T': T, 'atlas': atlas, 'median_ms': med, 'min_ms': lo, 'max_ms': hi, 'GBps': nbytes / med / 1e6,
             'frac_hbm': nbytes / med / 1e6 / 8000.0}
        results.append(r)
        print('%-28s T=%-5d %-9s %9.3f ms (min %8.3f, max %8.3f)  %7.0f GB/s  %5.1f%% of 8 TB/s'
              % (name, T, atlas, med, lo, hi, r['GBps'], 100 * r['frac_hbm']), flush=True)

    V, R = 91282, 360
    for atlas in ('local', 'scattered'):
        P = Parcellation(synthetic_atlas(V, R, scattered=atlas == 'scattered'))
        ptr, idx, region_of, _ = P._tables(dev)
        kept = torch.as_tensor(P.idx.astype(np.int64)).to(dev)
        reg_kept = region_of[kept].long()
        counts = torch.as_tensor(P.counts.astype(np.float32)).to(dev)
        wts = torch.rand(V, device=dev) + 0.5
        for T in (1200, 284):
            torch.manual_seed(T)
            x = torch.randn(T, V, device=dev) + 100.0 * (2 * torch.rand(V, device=dev) - 1)
            out = torch.empty(T, R, device=dev)
            nbytes = 4.0 * T * V + 4.0 * T * R
            note('parcellate', T, atlas, timeit(lambda: ops.parcellate(x, ptr, idx, R, out=out), args.iters), nbytes)
            print('   ', _lib.last_dispatch())
            if atlas == 'local':
                note('parcellate weighted', T, atlas, timeit(lambda: ops.parcellate(x, ptr, idx, R, w=wts, out=out), args.iters),
                     nbytes)

                def torch_way():
                    return torch.zeros(T, R, device=dev).index_add_(1, reg_kept, x[:, kept]) / counts
                note('torch index_add_', T, atlas, timeit(torch_way, args.iters), nbytes)
                ref = torch_way()
                got = ops.parcellate(x, ptr, idx, R)
                print('    max |kernel - torch| = %.3e' % float((got - ref).abs().max()))
    # the host baseline and the end-to-end call from host memory, T = 1200
    P = Parcellation(synthetic_atlas(V, R))
    T = 1200
    xh = (np.random.RandomState(1).randn(T, V) + 100.0).astype(np.float32)
    nbytes = 4.0 * T * V + 4.0 * T * R
    order = P.idx.astype(np.int64)
    starts = P.ptr[:-1].astype(np.int64)

    def host_way():
        return np.add.reduceat(xh[:, order], starts, axis=1) / P.counts.astype(np.float32)
    note('host np.add.reduceat', T, 'local', wall(host_way, 3), nbytes)
    note('reduce, pageable host array', T, 'local', wall(lambda: P.reduce(xh), 5), nbytes)
    xp = torch.as_tensor(xh).pin_memory()
    note('reduce, pinned host tensor', T, 'local', wall(lambda: P.reduce(xp), 5), nbytes)
    xd = torch.as_tensor(xh).to(dev)
    note('reduce, device tensor', T, 'local', wall(lambda: P.reduce(xd), 5), nbytes)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def glm_leg(args):
    """chebgcn_glm_project and chebgcn_glm_finish at two shapes -- one HCP dtseries run (1200 x 91282, k = 40) and 256 atlas runs
    (284 x 360, k = 22) -- each against the bytes-once HBM floor (6.29 TB/s measured copy rate, 8 TB/s spec), the float64 FMA
    count at the vector rate (78.6 TFLOP/s: half the fp32 vector rate) and what a user would write in torch on the same device:
    ``Q.T @ series.double()`` per run plus the residual algebra."""
    import torch
    from gcn_fmri_decoding_amd import _lib, ops
    dev = torch.device('cuda:0')
    HBM, HBM_SPEC, FMA64 = 6.29e12, 8.0e12, 78.6e12 / 2
    results = []

    timeit = lambda fn, iters: _timeit(fn, iters, 3)

    def note(name, shape, t, nbytes, fmas, dispatch=''):
        med, lo, hi = t
        r = {'leg': name, 'shape': shape, 'median_ms': med, 'min_ms': lo, 'max_ms': hi, 'bytes': nbytes, 'fma64': fmas,
             'hbm_floor_ms': 1e3 * nbytes / HBM, 'hbm_spec_floor_ms': 1e3 * nbytes / HBM_SPEC, 'fma_floor_ms': 1e3 * fmas / FMA64,
             'dispatch': dispatch}
        results.append(r)
        print('%-22s %-22s %9.3f ms (min %8.3f, max %8.3f)  HBM floor %7.3f ms (%4.1fx)  fp64 FMA floor %7.3f ms (%4.1fx)  %s'
              % (name, shape, med, lo, hi, r['hbm_floor_ms'], med / r['hbm_floor_ms'], r['fma_floor_ms'],
                 med / max(r['fma_floor_ms'], 1e-9), dispatch), flush=True)

    for R, T, M, k, C in ((1, 1200, 91282, 40, 4), (256, 284, 360, 22, 4)):
        shape = '%dx%dx%d k=%d' % (R, T, M, k)
        Mp = _lib.plane_stride(M)
        g = torch.Generator(device=dev).manual_seed(R)
        planes = torch.zeros(R * T, Mp, device=dev)
        planes[:, :M] = 1e4 + 50.0 * torch.randn(R * T, M, device=dev, generator=g)
        offs = torch.arange(R + 1, device=dev, dtype=torch.int64) * T
        Q = torch.linalg.qr(torch.randn(R, T, k, device=dev, dtype=torch.float64, generator=g))[0].reshape(R * T, k).contiguous()
        U = torch.randn(R, C, k, device=dev, dtype=torch.float64, generator=g)
        un2 = (U * U).sum(dim=2)
        rank = torch.full((R,), k, device=dev, dtype=torch.int32)
        e64 = torch.empty(R, C, Mp, device=dev, dtype=torch.float64)
        v64 = torch.empty_like(e64)
        panels = -(-k // ops.glm_geometry()['panel'])
        a, yy = ops.glm_project(planes, offs, M, Q)
        note('glm_project', shape, timeit(lambda: ops.glm_project(planes, offs, M, Q), args.iters),
             4.0 * R * T * Mp + 8.0 * R * (k + 1) * Mp + 8.0 * R * T * k, float(R) * T * Mp * (k + 1), _lib.last_dispatch())
        if panels > 1:
            print('    (%d panels: the scan is read %d times, %.3f ms at the copy rate)' % (panels, panels,
                                                                                          1e3 * 4.0 * R * T * Mp * panels / HBM))
        note('glm_finish', shape, timeit(lambda: ops.glm_finish(a, yy, offs, R * T, rank, U, un2, M, out64=(e64, v64)), args.iters),
             8.0 * R * (k + 1) * Mp + 16.0 * R * C * Mp, float(R) * Mp * k * (1 + C), _lib.last_dispatch())
        y3 = planes.view(R, T, Mp)
        Q3 = Q.view(R, T, k)

        def torch_project():
            yd = y3.double()
            return torch.bmm(Q3.transpose(1, 2), yd), (yd * yd).sum(dim=1)

        def torch_finish(at, yt):
            s2 = (yt - (at * at).sum(dim=1)).clamp_min(0.0) / float(T - k)
            e = torch.bmm(U, at)
            v = s2[:, None, :] * un2[:, :, None]
            return e, v, e / v.sqrt()
        at, yt = torch_project()
        print('    max |a - torch| / max |a| = %.3e' % float((a - at).abs().max() / at.abs().max()))
        note('torch Q.T @ y.double()', shape, timeit(torch_project, args.iters), 4.0 * R * T * Mp + 8.0 * R * (k + 1) * Mp + 8.0 * R * T * k,
             float(R) * T * Mp * (k + 1))
        note('torch residual algebra', shape, timeit(lambda: torch_finish(at, yt), args.iters), 8.0 * R * (k + 1) * Mp + 16.0 * R * C * Mp,
             float(R) * Mp * k * (1 + C))
        del planes, Q, y3, Q3, at, yt, a, yy
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def glm_ar1_leg(args):
    """chebgcn_glm_project_ar1 + chebgcn_glm_finish_ar1 at the two shapes of the glm leg, beside the OLS pair on the same data and
    the same algebra written in torch on the device (float64 bmm for the sums, batched ``torch.linalg.cholesky`` and
    ``solve_triangular`` for the k x k systems).  Floors: the scan read once per panel at the measured copy rate, and the float64
    FMA count at the vector rate -- 2k + 2 per scan element for the pass, k^3 / 6 + (1 + C) k^2 / 2 per vertex for the finish."""
    import numpy as np
    import torch
    from gcn_fmri_decoding_amd import _lib, glm, ops
    dev = torch.device('cuda:0')
    HBM, FMA64 = 6.29e12, 78.6e12 / 2
    results = []
    timeit = lambda fn, iters: _timeit(fn, iters, 3)

    def note(name, shape, t, nbytes, fmas, dispatch=''):
        med, lo, hi = t
        r = {'leg': name, 'shape': shape, 'median_ms': med, 'min_ms': lo, 'max_ms': hi, 'hbm_floor_ms': 1e3 * nbytes / HBM,
             'fma_floor_ms': 1e3 * fmas / FMA64, 'dispatch': dispatch}
        results.append(r)
        print('%-26s %-22s %9.3f ms (min %8.3f, max %8.3f)  HBM floor %7.3f ms  fp64 FMA floor %7.3f ms  %s'
              % (name, shape, med, lo, hi, r['hbm_floor_ms'], r['fma_floor_ms'], dispatch), flush=True)

    for R, T, M, k, C in ((1, 1200, 91282, 40, 4), (256, 284, 360, 22, 4)):
        shape = '%dx%dx%d k=%d' % (R, T, M, k)
        Mp = _lib.plane_stride(M)
        g = torch.Generator(device=dev).manual_seed(R)
        planes = torch.zeros(R * T, Mp, device=dev)
        planes[:, :M] = 1e4 + 50.0 * torch.randn(R * T, M, device=dev, generator=g)
        offs = torch.arange(R + 1, device=dev, dtype=torch.int64) * T
        X = torch.randn(R, T, k, device=dev, dtype=torch.float64, generator=g)
        X[:, :, 0] = 1.0                                        # the intercept: the series' mean is in the span
        Q3 = torch.linalg.qr(X)[0].contiguous()
        Qs3 = torch.zeros_like(Q3)
        Qs3[:, 1:] += Q3[:, :-1]
        Qs3[:, :-1] += Q3[:, 1:]
        W = torch.cat([Q3, Qs3], dim=2).reshape(R * T, 2 * k).contiguous()
        Q = Q3.reshape(R * T, k).contiguous()
        D = torch.bmm(Q3.transpose(1, 2), Qs3)
        D = (0.5 * (D + D.transpose(1, 2))).contiguous()
        E = (Q3[:, 0, :, None] * Q3[:, 0, None, :] + Q3[:, -1, :, None] * Q3[:, -1, None, :]).contiguous()
        U = torch.randn(R, C, k, device=dev, dtype=torch.float64, generator=g)
        un2 = (U * U).sum(dim=2)
        rank = torch.full((R,), k, device=dev, dtype=torch.int32)
        e64 = torch.empty(R, C, Mp, device=dev, dtype=torch.float64)
        v64 = torch.empty_like(e64)
        panel = ops.glm_geometry()['panel']
        scan = 4.0 * R * T * Mp

        a, yy = ops.glm_project(planes, offs, M, Q)
        t_p = timeit(lambda: ops.glm_project(planes, offs, M, Q), args.iters)
        note('glm_project', shape, t_p, scan * -(-k // panel), float(R) * T * Mp * (k + 1), _lib.last_dispatch())
        t_f = timeit(lambda: ops.glm_finish(a, yy, offs, R * T, rank, U, un2, M, out64=(e64, v64)), args.iters)
        note('glm_finish', shape, t_f, 8.0 * R * (k + 1) * Mp + 16.0 * R * C * Mp, float(R) * Mp * k * (1 + C), _lib.last_dispatch())

        ah, s0, s1 = ops.glm_project_ar1(planes, offs, M, W)
        t_pa = timeit(lambda: ops.glm_project_ar1(planes, offs, M, W), args.iters)
        note('glm_project_ar1', shape, t_pa, scan * -(-2 * k // panel), float(R) * T * Mp * (2 * k + 2), _lib.last_dispatch())
        fin = lambda rho: ops.glm_finish_ar1(ah, s0, s1, planes, W, offs, rank, D, E, U, M, rho=rho, out64=(e64, v64))
        fmas = float(R) * Mp * (k ** 3 / 6.0 + (1 + C) * k * k / 2.0)
        rho_dev, ev_dev = fin(None)[4].double(), e64.clone()
        t_fa = timeit(lambda: fin(None), args.iters)
        note('glm_finish_ar1 (estimated)', shape, t_fa, 8.0 * R * (2 * k + 2) * Mp + 16.0 * R * C * Mp, fmas, _lib.last_dispatch())
        note('glm_finish_ar1 (given)', shape, timeit(lambda: fin(0.3), args.iters), 8.0 * R * (2 * k + 2) * Mp + 16.0 * R * C * Mp, fmas,
             _lib.last_dispatch())
        print('    AR(1) pair %.3f ms, OLS pair %.3f ms' % (t_pa[0] + t_fa[0], t_p[0] + t_f[0]))

        y3 = planes.view(R, T, Mp)
        eye = torch.eye(k, device=dev, dtype=torch.float64)

        def torch_sums():
            yd = y3.double()
            return (torch.bmm(Q3.transpose(1, 2), yd), torch.bmm(Qs3.transpose(1, 2), yd), (yd * yd).sum(dim=1),
                    (yd[:, 1:] * yd[:, :-1]).sum(dim=1), yd[:, 0], yd[:, -1])

        def torch_fit(at, ht, S0, S1, y0, yL):
            rss = (S0 - (at * at).sum(dim=1)).clamp_min(0.0)
            num = S1 - (at * ht).sum(dim=1) + 0.5 * (at * torch.bmm(D, at)).sum(dim=1)
            rho = torch.where(rss > 0, num / rss.clamp_min(1e-300), torch.zeros_like(rss)).clamp(-glm.RHO_MAX, glm.RHO_MAX)      # [R, Mp]
            c1, r2 = 1.0 + rho * rho, rho * rho
            Mm = c1[:, :, None, None] * eye - rho[:, :, None, None] * D[:, None] - r2[:, :, None, None] * E[:, None]              # [R, Mp, k, k]
            gq = Q3[:, 0, :, None] * y0[:, None, :] + Q3[:, -1, :, None] * yL[:, None, :]
            gv = (c1[:, None, :] * at - rho[:, None, :] * ht - r2[:, None, :] * gq).transpose(1, 2)                               # [R, Mp, k]
            L = torch.linalg.cholesky(Mm)
            rhs = torch.cat([gv[..., None], U.transpose(1, 2)[:, None].expand(R, Mp, k, C)], dim=3)
            sol = torch.linalg.solve_triangular(L, rhs, upper=False)
            z, w = sol[..., 0], sol[..., 1:]
            rs = (c1 * S0 - 2.0 * rho * S1 - r2 * (y0 * y0 + yL * yL) - (z * z).sum(dim=2)).clamp_min(0.0)
            e = (w * z[..., None]).sum(dim=2).transpose(1, 2)
            v = (rs / float(T - k))[:, None, :] * (w * w).sum(dim=2).transpose(1, 2)
            return e, v, e / v.sqrt(), rho

        sums = torch_sums()
        e_t, v_t, _, rho_t = torch_fit(*sums)
        print('    max |rho - torch| = %.3e, max |effect - torch| / max |effect| = %.3e'
              % (float((rho_dev[:, :M] - rho_t[:, :M]).abs().max()), float((ev_dev[..., :M] - e_t[..., :M]).abs().max() / e_t[..., :M].abs().max())))
        t_ts = timeit(torch_sums, args.iters)
        note('torch sums (bmm, float64)', shape, t_ts, scan, float(R) * T * Mp * (2 * k + 2))
        t_tf = timeit(lambda: torch_fit(*sums), args.iters)
        note('torch cholesky + solves', shape, t_tf, 8.0 * R * (2 * k + 2) * Mp, fmas)
        print('    torch pair %.3f ms' % (t_ts[0] + t_tf[0]))
        del planes, W, Q, Q3, Qs3, y3, sums, ah, s0, s1, a, yy, e_t, v_t, rho_t
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def _searchlight_problem(offset=1e4, noise=50.0, signal=25.0):
    """The problem of the searchlight legs: the synthetic 10k-vertex kNN graph (M = 10466) and its 2-hop balls, ``S = 2048`` patterns
    of ``C = 8`` classes, ``offset + noise * N(0, 1)`` plus a class pattern of ``signal * N(0, 1)`` ->
    ``(L, balls, M, S, C, y, X float32 [S, M], the random state after X)``."""
    from gcn_fmri_decoding_amd import graph
    S, C = 2048, 8
    L = graph.synthetic_graph(10000, k=8, levels=1)[0][0]
    M = int(L.shape[0])
    rs = np.random.RandomState(0)
    y = np.arange(S) % C
    X = (offset + noise * rs.randn(S, M) + signal * rs.randn(C, M)[y]).astype(np.float32)
    return L, graph.hop_balls(L, 2), M, S, C, y, X, rs


def _bucket_launches(of_row, b, up):
    """``(buckets, [(bucket, its rows int32 on the device)])`` of bucket ``b``; ``b = 0``: the whole pass, every bucket's launch."""
    ks = [b] if b else sorted(set(of_row.tolist()))
    return ks, [(k, up(np.flatnonzero(of_row == k).astype(np.int32))) for k in ks]


def searchlight_leg(args):
    """chebgcn_searchlight_spread / _fit / _score on the synthetic 10k-vertex kNN graph (M = 10466) with 2-hop balls: 2048
    samples, 8 classes, 2 folds.  The score kernel issues three float64 vector instructions per (sample, class, neighbour) term
    -- subtract, multiply, fma: 4 floating-point operations -- so its floor is the float64 vector issue rate (39.3e12 lane
    instructions a second: the 78.6 TFLOP/s of FMAs, half the fp32 vector rate), and the bytes-once HBM floor is far below."""
    import torch
    from gcn_fmri_decoding_amd import _lib, ops, searchlight as sl
    dev = torch.device('cuda:0')
    HBM, ISSUE64 = 6.29e12, 78.6e12 / 2
    results = []

    def note(name, shape, t, nbytes, instr, flops, dispatch=''):
        med, lo, hi = t
        r = {'leg': name, 'shape': shape, 'median_ms': med, 'min_ms': lo, 'max_ms': hi, 'bytes': nbytes, 'fp64_instructions': instr,
             'flops': flops, 'hbm_floor_ms': 1e3 * nbytes / HBM, 'issue_floor_ms': 1e3 * instr / ISSUE64,
             'tflops': flops / med / 1e9, 'dispatch': dispatch}
        results.append(r)
        print('%-20s %-30s %9.3f ms (min %8.3f, max %8.3f)  HBM floor %7.3f ms  fp64 issue floor %7.3f ms (%4.1fx)  %6.2f TFLOP/s '
              'of 78.6  %s' % (name, shape, med, lo, hi, r['hbm_floor_ms'], r['issue_floor_ms'], med / max(r['issue_floor_ms'], 1e-9),
                               r['tflops'], dispatch), flush=True)

    _, balls, M, S, C, y, X, _ = _searchlight_problem()
    F, nnz = 2, int(balls.nnz)
    fold = np.arange(S) // C % F
    a = sl._check(X, y, balls, fold, None, True, None, False, False, None, 'kbench')
    plan = sl._device_plan(a, ops.searchlight_geometry()['buckets'][C])
    up = lambda v: torch.as_tensor(v).to(dev)
    Xt = sl._transposed(up(X), plan.order, dev)
    shape = 'S=%d M=%d C=%d folds=%d nnz=%d' % (S, M, C, F, nnz)
    lptr, lidx, cptr, cidx = up(plan.list_ptr), up(plan.list_idx), up(plan.class_ptr), up(plan.class_idx)
    ntrain = float(plan.list_idx.size)
    note('searchlight_spread', shape, _timeit(lambda: ops.searchlight_spread(Xt, S, lptr, lidx), args.iters, 3),
         4.0 * M * S + 8.0 * plan.NM * M, 3.0 * ntrain * M, 3.0 * ntrain * M, '')
    print('   ', _lib.last_dispatch())
    eps = 1e-9 * ops.searchlight_spread(Xt, S, lptr, lidx).max(dim=1).values
    note('searchlight_fit', shape, _timeit(lambda: ops.searchlight_fit(Xt, S, cptr, cidx, C, eps), args.iters, 3),
         4.0 * M * S + 24.0 * plan.NM * M * plan.NC, 3.0 * ntrain * M, 3.0 * ntrain * M, _lib.last_dispatch())
    par, lg = ops.searchlight_fit(Xt, S, cptr, cidx, C, eps)
    correct = torch.zeros((1, C, a.U), dtype=torch.int32, device=dev)
    rowptr, colidx = up(a.indptr.astype(np.int32)), up(a.indices.astype(np.int32))
    tabs = [up(v) for v in (plan.test_ptr, plan.logprior, plan.sgroup, plan.slabel, plan.order.astype(np.int32))]

    def score():
        ops.searchlight_score(Xt, S, rowptr, colidx, 0, a.U, tabs[0], plan.tmax, C, par, lg, tabs[1], tabs[2], tabs[3], tabs[4], correct)
    t = _timeit(score, args.iters, 3)
    terms = float(S) * nnz * plan.NC                            # (sample, neighbour, class) terms the kernel works through
    note('searchlight_score', shape, t, 4.0 * M * S + 24.0 * plan.NM * M * plan.NC + 4.0 * nnz, 3.0 * terms, 4.0 * terms,
         _lib.last_dispatch())
    print('    balls of %.1f vertices on average (largest %d); %.3g terms; accuracy of the last pass %.3f'
          % (nnz / float(a.U), int(np.diff(a.indptr).max()), terms, float(correct.sum()) / (args.iters + 3.0) / S / a.U))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def searchlight_lda_leg(args):
    """chebgcn_searchlight_lda at the shape of the searchlight leg (the synthetic 10k-vertex kNN graph, M = 10466, 2-hop balls,
    2048 samples, 8 classes, 2 folds): one workgroup per (centre, model).  The covariance costs n P (P + 1) / 2 float64 FMAs per
    (model, centre), n the model's training samples, so the floor is (sum over balls of P (P + 1) / 2) x (sum over models of n)
    lane-FMAs at the float64 vector issue rate (39.3e12 lane instructions a second); factorisation, solves and scoring come on
    top, and the HBM floor (Xt once) is far below."""
    import torch
    from gcn_fmri_decoding_amd import _lib, ops, searchlight as sl
    dev = torch.device('cuda:0')
    HBM, ISSUE64 = 6.29e12, 78.6e12 / 2
    results = []
    _, balls, M, S, C, y, X, _ = _searchlight_problem()
    F, nnz = 2, int(balls.nnz)
    fold = np.arange(S) // C % F
    a = sl._check(X, y, balls, fold, None, True, None, False, False, None, 'kbench', classifier='lda')
    plan = sl._device_plan(a, ops.searchlight_geometry()['buckets'][C])
    up = lambda v: torch.as_tensor(v).to(dev)
    Xt = sl._transposed(up(X), plan.order, dev)
    cptr, cidx = up(plan.class_ptr), up(plan.class_idx)
    par, _ = ops.searchlight_fit(Xt, S, cptr, cidx, C, torch.zeros(plan.NM, dtype=torch.float64, device=dev))
    correct = torch.zeros((1, C, a.U), dtype=torch.int32, device=dev)
    rowptr, colidx = up(a.indptr.astype(np.int32)), up(a.indices.astype(np.int32))
    tabs = [up(v) for v in (plan.test_ptr, plan.logprior, plan.sgroup, plan.slabel, plan.order.astype(np.int32))]
    P = np.diff(a.indptr)
    buckets = ops.searchlight_lda_geometry()['buckets']
    of_row = np.array([buckets[int(n)] for n in P])
    ntrain = float(plan.class_idx.size)                         # summed over the models
    tri = (P * (P + 1) // 2).astype(np.float64)
    print('balls of %.1f vertices on average (largest %d); sum P (P + 1) / 2 = %d; %d training samples over %d models: floor %.3f ms'
          % (P.mean(), P.max(), tri.sum(), ntrain, plan.NM, 1e3 * tri.sum() * ntrain / ISSUE64), flush=True)
    for shrink, tag in ((0.1, 'g=0.1'), (-1.0, "g='auto'")):
        total = [0.0, 0.0]
        for b in sorted(set(of_row.tolist())) + [0]:
            ks, launches = _bucket_launches(of_row, b, up)
            fmas = float(sum(tri[of_row == k].sum() for k in ks)) * ntrain

            def run():
                for k, rows in launches:
                    ops.searchlight_lda(Xt, S, rowptr, colidx, rows, k, cptr, cidx, tabs[0], plan.tmax, C, par, tabs[1], shrink, tabs[2],
                                        tabs[3], tabs[4], correct)
            med, lo, hi = _timeit(run, args.iters, 2)
            n_rows = int(sum(r.numel() for _, r in launches))
            nbytes = 4.0 * M * S + 4.0 * nnz
            name = 'searchlight_lda ' + ('all' if not b else '<%d>' % b)
            results.append({'leg': name, 'shape': 'S=%d M=%d C=%d folds=%d nnz=%d %s' % (S, M, C, F, nnz, tag), 'centres': n_rows,
                            'median_ms': med, 'min_ms': lo, 'max_ms': hi, 'covariance_fma64': fmas, 'issue_floor_ms': 1e3 * fmas / ISSUE64,
                            'hbm_floor_ms': 1e3 * nbytes / HBM, 'dispatch': _lib.last_dispatch() if b else 'every bucket'})
            print('%-22s %-10s %6d centres %9.3f ms (min %8.3f, max %8.3f)  covariance floor %7.3f ms (%5.1fx)  %6.2f TFLOP/s of 78.6'
                  % (name, tag, n_rows, med, lo, hi, 1e3 * fmas / ISSUE64, med / max(1e3 * fmas / ISSUE64, 1e-9), 2.0 * fmas / med / 1e9),
                  flush=True)
    print('    accuracy of the last pass %.3f' % (float(correct.sum()) / S / a.U / (2 * (2 + args.iters)) / 2), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def searchlight_rdm_leg(args):
    """chebgcn_searchlight_rdm at the shape of the searchlight legs (the synthetic 10k-vertex kNN graph, M = 10466, 2-hop balls,
    2048 samples, 8 classes), with 2 and with 8 partitions: one workgroup per (centre, group).  One covariance per group serves all
    its cells, so it costs S P (P + 1) / 2 float64 FMAs per centre whatever the number of partitions -- the floor is
    (sum over balls of P (P + 1) / 2) x S lane-FMAs at the float64 vector issue rate (39.3e12 lane instructions a second);
    factorisation and one forward solve per cell come on top, and the HBM floor (Xt once) is far below."""
    import torch
    from gcn_fmri_decoding_amd import _lib, ops, searchlight as sl
    dev = torch.device('cuda:0')
    HBM, ISSUE64 = 6.29e12, 78.6e12 / 2
    results = []
    _, balls, M, S, C, y, X, _ = _searchlight_problem()
    nnz = int(balls.nnz)
    up = lambda v: torch.as_tensor(v).to(dev)
    for F in (2, 8):
        part = np.arange(S) // C % F
        a = sl._check_rdm(X, y, balls, part, None, None, 0.1, None, 'kbench')
        plan = sl._rdm_plan(a)
        Xt = sl._transposed(up(X), plan.order, dev)
        cell_ptr, cptr, cidx = up(plan.cell_ptr), up(plan.class_ptr), up(plan.class_idx)
        par, _ = ops.searchlight_fit(Xt, S, cptr, cidx, C, torch.zeros(plan.NM, dtype=torch.float64, device=dev))
        rdm = torch.zeros((1, C * (C - 1) // 2, a.U), dtype=torch.float64, device=dev)
        gam = torch.zeros((1, a.U), dtype=torch.float64, device=dev)
        rowptr, colidx = up(a.indptr.astype(np.int32)), up(a.indices.astype(np.int32))
        P = np.diff(a.indptr)
        buckets = ops.searchlight_rdm_geometry()['buckets']
        of_row = np.array([buckets[int(n)] for n in P])
        tri = (P * (P + 1) // 2).astype(np.float64)
        if F == 2:
            print('balls of %.1f vertices on average (largest %d); sum P (P + 1) / 2 = %d; %d samples: floor %.3f ms'
                  % (P.mean(), P.max(), tri.sum(), S, 1e3 * tri.sum() * S / ISSUE64), flush=True)
        for shrink, tag in ((0.1, 'g=0.1'), (-1.0, "g='auto'")):
            for b in sorted(set(of_row.tolist())) + [0]:
                ks, launches = _bucket_launches(of_row, b, up)
                fmas = float(sum(tri[of_row == k].sum() for k in ks)) * S

                def run():
                    for k, rows in launches:
                        ops.searchlight_rdm(Xt, S, rowptr, colidx, rows, k, cell_ptr, cptr, cidx, C, par, shrink, rdm, gamma_out=gam)
                med, lo, hi = _timeit(run, args.iters, 2)
                n_rows = int(sum(r.numel() for _, r in launches))
                nbytes = 4.0 * M * S + 4.0 * nnz
                name = 'searchlight_rdm ' + ('all' if not b else '<%d>' % b)
                results.append({'leg': name, 'shape': 'S=%d M=%d C=%d partitions=%d nnz=%d %s' % (S, M, C, F, nnz, tag), 'centres': n_rows,
                                'median_ms': med, 'min_ms': lo, 'max_ms': hi, 'covariance_fma64': fmas, 'issue_floor_ms': 1e3 * fmas / ISSUE64,
                                'hbm_floor_ms': 1e3 * nbytes / HBM, 'dispatch': _lib.last_dispatch() if b else 'every bucket'})
                print('%-22s F=%d %-10s %6d centres %9.3f ms (min %8.3f, max %8.3f)  covariance floor %7.3f ms (%5.1fx)  %6.2f TFLOP/s of 78.6'
                      % (name, F, tag, n_rows, med, lo, hi, 1e3 * fmas / ISSUE64, med / max(1e3 * fmas / ISSUE64, 1e-9),
                         2.0 * fmas / med / 1e9), flush=True)
        print('    F=%d: mean distance of the last pass %.4f, degenerate balls %d' % (F, float(rdm.mean()), int((gam < 0).sum())), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def searchlight_svc_leg(args):
    """chebgcn_searchlight_svm at the shape of the other searchlight legs (the synthetic 10k-vertex kNN graph, M = 10466, 2-hop
    balls, 2048 samples, 8 classes) but WITHIN 16 subjects of 128 samples and 2 folds each, so that a training set holds 64
    samples: 32 models, one workgroup per (centre, model); and one parcel-sized leg: 360 rows of 300 vertices.  z-scored
    patterns, C = 1, squared hinge, tol = 1e-3, at most 100 sweeps.  Two floors per leg.  The Gram matrix costs P n (n + 1) / 2
    multiplies and as many adds per (model, centre) -- nothing is fused -- at the float64 vector issue rate (39.3e12 lane
    instructions a second).  The solve is a chain: a coordinate step cannot begin before the last one's g is known, and costs at
    least a float64 division (about ten dependent instructions), two multiplies, an add, two readlanes and an LDS read, about
    120 cycles = 50 ns at 2.4 GHz; a (model, centre) runs ceil(C / 4) rounds of classes of (sweeps x n) steps each, and a CU
    overlaps as many workgroups as the kernel's occupancy admits."""
    import scipy.sparse as sp
    import torch
    from gcn_fmri_decoding_amd import _lib, ops, searchlight as sl
    dev = torch.device('cuda:0')
    ISSUE64, STEP_S, CUS = 78.6e12 / 2, 50e-9, 256
    OCC = {32: 4, 64: 2, 128: 1}                                # workgroups per CU: the compiler's report
    results = []
    _, balls, M, S, C, y, X, rs = _searchlight_problem(offset=0.0, noise=1.0, signal=0.5)
    G, F, CAP = 16, 2, 100
    fold = np.arange(S) // C % F
    groups = (np.arange(S) // (C * F) % G).tolist()
    parcels = np.zeros((360, M), np.int8)
    for r in range(360):
        parcels[r, rs.choice(M, 300, replace=False)] = 1
    up = lambda v: torch.as_tensor(v).to(dev)
    for tag, rows in (('balls', balls), ('parcels', sp.csr_matrix(parcels))):
        a = sl._check(X, y, rows, fold, groups, True, None, False, False, None, 'kbench', classifier='svc', max_iter=CAP)
        plan = sl._device_plan(a, ops.searchlight_geometry()['buckets'][C])
        Xt = sl._transposed(up(X), plan.order, dev)
        n = np.diff(plan.list_ptr)
        bucket = int(ops.searchlight_svm_geometry()['buckets'][int(n.max())])
        assert len(set(n.tolist())) == 1
        correct = torch.zeros((G, C, a.U), dtype=torch.int32, device=dev)
        sweeps = torch.zeros((plan.NM, a.U), dtype=torch.int32, device=dev)
        resid = torch.zeros((plan.NM, a.U), dtype=torch.float64, device=dev)
        rowptr, colidx = up(a.indptr.astype(np.int32)), up(a.indices.astype(np.int32))
        tabs = [up(v) for v in (plan.list_ptr, plan.list_idx, plan.test_ptr, plan.sgroup, plan.slabel, plan.order.astype(np.int32))]
        centres, models = up(np.arange(a.U, dtype=np.int32)), up(np.arange(plan.NM, dtype=np.int32))

        def run():
            ops.searchlight_svm(Xt, S, rowptr, colidx, centres, models, bucket, tabs[0], tabs[1], tabs[2], plan.tmax, C, 1.0, 'squared_hinge',
                                1e-3, CAP, tabs[3], tabs[4], tabs[5], correct, sweeps=sweeps, residual=resid)
        med, lo, hi = _timeit(run, args.iters, 1)
        P = np.diff(a.indptr).astype(np.float64)
        nn = float(n[0])
        gram_ops = 2.0 * P.sum() * plan.NM * (nn * (nn + 1) / 2 + 64.0 * nn)     # the triangle and the test samples' rows (64 a model)
        sw = sweeps.cpu().numpy().astype(np.float64)
        steps = float((-(-C // 4)) * sw.sum() * nn)
        chain_ms = 1e3 * steps * STEP_S / (CUS * OCC[bucket])
        gram_ms = 1e3 * gram_ops / ISSUE64
        conv = float((resid.cpu().numpy() <= 1e-3).mean())
        acc = float(correct.sum()) / S / a.U / (1 + args.iters)
        results.append({'leg': 'searchlight_svc ' + tag, 'shape': 'S=%d M=%d C=%d groups=%d folds=%d n=%d nnz=%d cap=%d' % (
            S, M, C, G, F, int(nn), int(rows.nnz), CAP), 'centres': int(a.U), 'models': int(plan.NM), 'median_ms': med, 'min_ms': lo,
            'max_ms': hi, 'mean_vertices': float(P.mean()), 'mean_sweeps': float(sw.mean()), 'max_sweeps': float(sw.max()),
            'converged': conv, 'gram_floor_ms': gram_ms, 'chain_floor_ms': chain_ms, 'accuracy': acc, 'dispatch': _lib.last_dispatch()})
        print('searchlight_svc %-8s %6d rows of %.1f vertices x %d models of n = %d: %10.3f ms (min %9.3f, max %9.3f); sweeps mean %.1f max %d, '
              '%.4f converged; Gram floor %.3f ms, chain floor %.3f ms (%.1fx their sum); accuracy %.3f; %s'
              % (tag, a.U, P.mean(), plan.NM, int(nn), med, lo, hi, sw.mean(), int(sw.max()), conv, gram_ms, chain_ms,
                 med / (gram_ms + chain_ms), acc, _lib.last_dispatch()), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('leg', nargs='?', choices=['glm', 'glm_ar1', 'searchlight', 'searchlight_lda', 'searchlight_rdm', 'searchlight_svc'],
                    help='glm: the first-level GLM kernels alone (ops.glm_project / glm_finish); searchlight: the searchlight kernels alone; '
                         'searchlight_lda: the LDA searchlight kernel alone; searchlight_rdm: the RSA searchlight kernel alone; '
                         'searchlight_svc: the SVM searchlight kernel alone')
    ap.add_argument('--parcellate', action='store_true', help='the parcellation leg alone (ops.parcellate at HCP size)')
    ap.add_argument('--B', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--fin', type=int, default=32)
    ap.add_argument('--fout', type=int, default=32)
    ap.add_argument('--K', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--kernels', nargs='+', default=['recurrence_fwd', 'recurrence_fwd_inplace', 'recurrence_bwd', 'contract_fwd',
                                                     'contract_bwd_w_relu', 'contract_bwd_x_relu', 'bias_grad_relu', 'contract_bwd_w', 'contract_bwd_x',
                                                     'brelu_pool_bwd', 'recurrence_fwd_t', 'contract_fwd_dx', 'brelu_pool_bwd_mask', 'contract_fwd_dx_gated',
                                                     'bias_grad_sum'])
    ap.add_argument('--nodes', type=int, default=10000, help='points of the synthetic kNN graph (10000 -> M = 10466)')
    ap.add_argument('--levels', type=int, default=1, help='coarsening levels of the synthetic graph (1 -> fake vertices behind the real ones)')
    ap.add_argument('--json', default=None)
    ap.add_argument('--planes', type=int, default=0, help='planes per workgroup of the recurrence kernel (0 = automatic, 2, 4)')
    ap.add_argument('--order', default='length', choices=['bank', 'length', 'reference'],
                    help="vertex order of the graph: 'length' = relabelled by descending row length as cgcnn does for a network "
                         "without pooling (ordered recurrence kernels); 'reference' = the caller's numbering")
    ap.add_argument('--stamps', action='store_true', help='print the in-kernel phase stamps of a CG_X&64 build (tools/xbuild.sh 64)')
    ap.add_argument('--stagger', type=int, default=0, help='chebgcn_tune(4, x): start stagger override (x-1 eighths), 0 = automatic')
    ap.add_argument('--wide', type=int, default=0, help='chebgcn_tune(3, x): 1 = 1024-thread recurrence shape')
    args = ap.parse_args()
    if args.parcellate:
        return parcellate_leg(args)
    if args.leg == 'glm':
        return glm_leg(args)
    if args.leg == 'glm_ar1':
        return glm_ar1_leg(args)
    if args.leg == 'searchlight':
        return searchlight_leg(args)
    if args.leg == 'searchlight_lda':
        return searchlight_lda_leg(args)
    if args.leg == 'searchlight_rdm':
        return searchlight_rdm_leg(args)
    if args.leg == 'searchlight_svc':
        return searchlight_svc_leg(args)

    import torch
    import bench
    from gcn_fmri_decoding_amd import _lib, ops
    dev = torch.device('cuda:0')
    Ls, perm = bench.load_graph(args.nodes, args.levels, 0, 1, None)
    lib = _lib.lib()
    import ctypes
    handle = ctypes.CDLL(_lib.LIB_PATH)
    tune = getattr(handle, 'chebgcn_tune', None)          # experiment builds only (tools/xbuild.sh, CHEBGCN_LIB=...)
    if tune is None and (args.wide or args.stagger or (args.stamps and not hasattr(handle, 'chebgcn_debug_stampsb'))):
        raise SystemExit('--wide / --stagger / --stamps need an experiment build (tools/xbuild.sh)')
    if tune is not None:
        tune(3, args.wide)
        tune(4, args.stagger)
    from gcn_fmri_decoding_amd import graph as G
    # 'bank': the length order refined inside its equal-length classes against LDS bank conflicts (graph.bank_order; experiment)
    order = None if (args.order == 'reference' or args.planes) else G.length_order(Ls[0]) if args.order == 'length' else G.bank_order(Ls[0])
    g = ops.Graph(Ls[0], dev, planes=args.planes, order=order)
    print('ordered recurrence kernels:', bool(g.query(12)), ' planes of the ordered image:', g.query(16), flush=True)
    print('planes per workgroup:', g.query(6), ' gather LDS cost (before, after placement, ideal):', g.query(9), g.query(10),
          g.query(11), ' ordered image:', g.query(13), g.query(14), g.query(15), flush=True)
    M, Mp = g.M, g.Mp
    print('M = %d, Mp = %d (plane stride %d bytes)' % (M, Mp, 4 * Mp), flush=True)
    results = []

    def timeit(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for s, e in evs:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        ms = sorted(s.elapsed_time(e) for s, e in evs)
        return ms[len(ms) // 2], ms[0]

    for B in args.B:
        Fin, Fout, K = args.fin, args.fout, args.K
        if Fin != Fout:
            args.kernels = [k for k in args.kernels if k not in ('recurrence_fwd_t', 'contract_fwd_dx', 'contract_fwd_dx_gated')]
        torch.manual_seed(0)
        x = torch.randn(B, Fin, Mp, device=dev)
        stack = torch.randn(K, B, Fin, Mp, device=dev)
        gstack = torch.randn(K, B, Fin, Mp, device=dev)
        dx = torch.empty(B, Fin, Mp, device=dev)
        W = torch.randn(Fin * K, Fout, device=dev) * 0.1
        Wt = torch.randn(Fout * K, Fin, device=dev) * 0.1       # (gstack below is [K, B, Fin, Mp]: the dx entries assume Fin == Fout)
        bias = torch.randn(Fout, Mp, device=dev)
        out = torch.empty(B, Fout, Mp, device=dev)
        dy = torch.randn(B, Fout, Mp, device=dev)
        dy16 = dy.to(torch.bfloat16)
        dbias = torch.empty(Fout, Mp, device=dev)
        dW = torch.empty(Fin * K, Fout, device=dev)
        ws = torch.empty(lib.chebgcn_contract_bwd_w_workspace(B, M, Fin, K, Fout), dtype=torch.uint8, device=dev)
        ws16 = torch.empty(lib.chebgcn_contract_fwd_bf16_workspace(Fin, K, Fout), dtype=torch.uint8, device=dev)
        wsx16 = torch.empty(lib.chebgcn_contract_bwd_x_bf16_workspace(Fin, K, Fout), dtype=torch.uint8, device=dev)
        wsw16 = torch.empty(lib.chebgcn_contract_bwd_w_bf16_workspace(B, M, Fin, K, Fout), dtype=torch.uint8, device=dev)
        mask = torch.randint(0, 16, (B, Fout, Mp // 4), dtype=torch.uint8, device=dev)     # ReLU bit mask, half the bits set
        st = ops._stream()
        P = ops._p
        calls = {
            'recurrence_fwd': (lambda: lib.chebgcn_recurrence_fwd(g.handle, P(x), P(stack), B, Fin, K, st),
                               4.0 * M * Fin * K * B, 0.0),
            # T_0 already in slab 0 of the stack (what the model does): no copy of the input
            'recurrence_fwd_inplace': (lambda: lib.chebgcn_recurrence_fwd(g.handle, P(stack), P(stack), B, Fin, K, st),
                                       4.0 * M * Fin * K * B, 0.0),
            'recurrence_bwd': (lambda: lib.chebgcn_recurrence_bwd(g.handle, P(gstack), P(dx), B, Fin, K, st),
                               4.0 * M * Fin * (K + 1) * B, 0.0),
            # the input gradient as the training step forms it (ops.dx_by_forward): the FORWARD kernel on the planes of dy with the
            # transposed operator, in place in slab 0 of the gradient stack, then the forward contraction on the re-indexed weights
            # (no bias, no ReLU, no mask)
            'recurrence_fwd_t': (lambda: lib.chebgcn_recurrence_fwd_t(g.handle, P(gstack), P(gstack), B, Fout, K, st),
                                 4.0 * M * Fout * K * B, 0.0),
            'contract_fwd_dx': (lambda: lib.chebgcn_contract_fwd(P(gstack), P(Wt), None, 0, P(dx), None, B, M, Fout, K, Fin,
                                                                 1, 0, 0, st),
                                4.0 * B * M * (Fout * K + Fin), 2.0 * B * M * Fin * K * Fout),
            # ... with the ReluGrad of the layer below in its epilogue (ops.GateLink: layers 3-6 of the bench network), and what is
            # left of that layer's own ReluGrad pass: the plain sum of the gated dy for the bias gradient
            'contract_fwd_dx_gated': (lambda: lib.chebgcn_contract_fwd_gated(P(gstack), P(Wt), P(mask), P(dx), B, M, Fout, K, Fin, st),
                                      B * M * (4.0 * (Fout * K + Fin) + Fin / 4.0), 2.0 * B * M * Fin * K * Fout),
            'bias_grad_sum': (lambda: lib.chebgcn_brelu_pool_bwd(P(dy), None, None, None, P(dbias), 2, B, M, Fout, 1, 0, 0, None, 0, st),
                              B * Fout * M * 4.0, 0.0),
            'contract_fwd': (lambda: lib.chebgcn_contract_fwd(P(stack), P(W), P(bias), 2, P(out), None, B, M, Fin, K, Fout,
                                                              1, 0, 1, st),
                             4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_fwd_bf16': (lambda: lib.chebgcn_contract_fwd_bf16(P(stack), P(W), P(bias), 2, P(out), None, B, M, Fin, K,
                                                                        Fout, 1, 0, 1, 1, P(ws16), ws16.numel(), st),
                                  4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_fwd_bf16x3': (lambda: lib.chebgcn_contract_fwd_bf16(P(stack), P(W), P(bias), 2, P(out), None, B, M, Fin,
                                                                          K, Fout, 1, 0, 1, 3, P(ws16), ws16.numel(), st),
                                    4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_w': (lambda: lib.chebgcn_contract_bwd_w(P(stack), P(dy), P(dW), P(ws), ws.numel(), B, M, Fin, K,
                                                                  Fout, st),
                               4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_x': (lambda: lib.chebgcn_contract_bwd_x(P(dy), P(W), P(gstack), B, M, Fin, K, Fout, st),
                               4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            # the gradients of a pool == 1 ReLU layer as the model runs them: ReluGrad folded in (bit mask)
            'contract_bwd_w_relu': (lambda: lib.chebgcn_contract_bwd_w_relu(P(stack), P(dy), P(mask), P(dW), P(ws), ws.numel(), B, M,
                                                                            Fin, K, Fout, st),
                                    B * M * (4.0 * (Fin * K + Fout) + Fout / 4.0), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_x_relu': (lambda: lib.chebgcn_contract_bwd_x_relu(P(dy), P(mask), P(W), P(gstack), B, M, Fin, K, Fout, st),
                                    B * M * (4.0 * (Fin * K + Fout) + Fout / 4.0), 2.0 * B * M * Fin * K * Fout),
            'bias_grad_relu': (lambda: lib.chebgcn_brelu_pool_bwd(P(dy), None, P(mask), None, P(dbias), 2, B, M, Fout, 1, 0, 1, None, 0, st),
                               B * Fout * M * 4.25, 0.0),
            'contract_bwd_w_bf16': (lambda: lib.chebgcn_contract_bwd_w_bf16(P(stack), P(dy), P(dW), P(wsw16), wsw16.numel(), B, M, Fin,
                                                                            K, Fout, 1, st),
                                    4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_w_bf16x3': (lambda: lib.chebgcn_contract_bwd_w_bf16(P(stack), P(dy), P(dW), P(wsw16), wsw16.numel(), B, M,
                                                                              Fin, K, Fout, 3, st),
                                      4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_x_bf16': (lambda: lib.chebgcn_contract_bwd_x_bf16(P(dy), P(W), P(gstack), B, M, Fin, K, Fout, 1, P(wsx16),
                                                                            wsx16.numel(), st),
                                    4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_x_bf16x3': (lambda: lib.chebgcn_contract_bwd_x_bf16(P(dy), P(W), P(gstack), B, M, Fin, K, Fout, 3, P(wsx16),
                                                                              wsx16.numel(), st),
                                      4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            # wide bf16 layers: ReluGrad writes dy as bf16, the two gradients read it (same results as the fp32-dy entries above)
            'relu_grad_bf16': (lambda: lib.chebgcn_relu_grad_bf16(P(dy), P(mask), P(dy16), P(dbias), 2, B, M, Fout, None, 0, st),
                               B * Fout * M * 6.25, 0.0),
            'brelu_pool_bwd_mask': (lambda: lib.chebgcn_brelu_pool_bwd(P(dy), None, P(mask), P(out), P(dbias), 2, B, M, Fout, 1, 0, 1,
                                                                       None, 0, st), B * Fout * M * 8.25, 0.0),
            'contract_bwd_w_bf16_dy16': (lambda: lib.chebgcn_contract_bwd_w_bf16_dy16(P(stack), P(dy16), P(dW), P(wsw16), wsw16.numel(),
                                                                                      B, M, Fin, K, Fout, st),
                                         4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'contract_bwd_x_bf16_dy16': (lambda: lib.chebgcn_contract_bwd_x_bf16_dy16(P(dy16), P(W), P(gstack), B, M, Fin, K, Fout,
                                                                                      P(wsx16), wsx16.numel(), st),
                                         4.0 * B * M * (Fin * K + Fout), 2.0 * B * M * Fin * K * Fout),
            'brelu_pool_bwd': (lambda: lib.chebgcn_brelu_pool_bwd(P(dy), P(out), None, P(dx) if Fin == Fout else P(out),
                                                                  P(dbias), 2, B, M, Fout, 1, 0, 1, None, 0, st),
                               4.0 * B * Fout * 3 * M, 0.0),
        }
        for name in args.kernels:
            fn, nbytes, flops = calls[name]
            for abl in [0]:
                med, best = timeit(lambda: _lib.check(fn(), name), args.iters)
                r = {'kernel': name, 'B': B, 'Fin': Fin, 'Fout': Fout, 'K': K, 'ablate': abl, 'median_ms': med,
                     'min_ms': best, 'GBps': nbytes / med / 1e6, 'frac_hbm': nbytes / med / 1e6 / 8000.0,
                     'TFLOPs': flops / med / 1e9}
                results.append(r)
                if args.stamps and (name.startswith('recurrence') or (hasattr(handle, 'chebgcn_debug_stampsb') and 'bf16' in name)):
                    buf = (ctypes.c_longlong * (16 * 64))()
                    if not name.startswith('recurrence'):
                        assert handle.chebgcn_debug_stampsb(buf) == 0       # tools/bbuild.sh x64 "-DCG_EXPERIMENT=1 -DCG_X=64"
                    else:
                        assert (handle.chebgcn_debug_stampso if g.query(12) else handle.chebgcn_debug_stamps4 if g.query(6) == 4 and g.query(7) > 2048 else handle.chebgcn_debug_stamps)(buf) == 0
                    t = np.array(buf, dtype=np.int64).reshape(16, 64)
                    t0 = t[t > 0].min()
                    print('   stamps (cycle counter ticks since the first wave entered the group), one row per wave:')
                    ids = [i for i in range(64) if (t[:, i] > 0).any()]
                    print('   id   ' + ' '.join('%7d' % i for i in ids))
                    for w in range(16):
                        if (t[w] > 0).any():
                            print('   w%-3d ' % w + ' '.join('%7d' % (t[w, i] - t0 if t[w, i] > 0 else -1) for i in ids))
                print('%-16s B=%-4d abl=%-2d  %8.3f ms (min %7.3f)  %7.0f GB/s  %5.1f%% of 8 TB/s  %6.1f TFLOP/s   %s'
                      % (name, B, abl, med, best, r['GBps'], 100 * r['frac_hbm'], r['TFLOPs'], _lib.last_dispatch()), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
