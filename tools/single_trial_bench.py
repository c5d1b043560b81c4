"""Timings of ``glm.single_trial`` and of the three other routes to the same maps (EXPERIMENTS 30).

    python tools/single_trial_bench.py [--out FILE] [--runs 8] [--rows 284] [--vertices 20484] [--confounds 8] [--trials 32 96]
                                       [--fused-only]

R runs of T rows and M vertices, q = confounds + 1 nuisance columns, n evenly spaced trials per run in two conditions
(``others='condition'``: G = 2), BOLD-scaled series (mean 1e4, sd 50) staged on the device once.  Per n:

* ``fused``: what ``single_trial`` launches -- ``chebgcn_glm_project`` over ``[Qn | Z_S]`` and ``chebgcn_glm_trials`` -- with
  the tables already on the device; beta and t.  ``trials_ms`` is the ``glm_trials`` call alone, with its bytes and flops as
  ``ops.glm_trials_model`` (the ``_launch`` model) counts them, the achieved share of the 8 TB/s HBM roofline (and of the
  6.29 TB/s a copy reaches) and of the float64 FMA peak.
* ``unfused``: ``chebgcn_glm_project`` over ``Z`` in chunks of 64 columns, every chunk's planes copied out of the workspace
  into one float64 ``[R, n, Mp]`` tensor, and the epilogue in torch float64 on it (the same algebra, vectorised).  Its beta
  must agree with the fused route's to float32 rounding.
* ``matmul``: ``torch.bmm`` in float64 of ``[Qn | Z_S | Z]^T`` with the series converted to float64 beforehand (the conversion
  is timed beside it): the projections alone, no epilogue.
* ``first_level``: ``first_level(betas=True)`` once per trial index on that trial's explicit design ``[x_j | others | N]`` of
  every run, series as device tensors -- the only route before ``single_trial``.  Timed end to end (host clock around a call
  that ends synchronised) on 4 trial indices and SCALED to n.
* ``end_to_end_s``: ``single_trial`` itself on device tensors, host clock, the per-trial host tables included.

A variant of the kernel is a library built with other macros of ``csrc/glm_trials.hip`` (``CG_GLM_TRIALS_Z=1``: the full panels of
a call in grid.z of one launch), named by ``CHEBGCN_LIB``; ``--fused-only`` times its fused route alone.

Device events around LAUNCHES repeats, ROUNDS rounds, median and minimum per repeat, after a warm-up.  No GPU: the script
fails, it never falls back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_fmri_decoding_amd import _lib, glm, ops  # noqa: E402

LAUNCHES, ROUNDS, TR = 10, 5, 0.72
HBM_SPEC, HBM_COPY, FMA64 = 8.0e12, 6.29e12, 78.6e12 / 2


def timed(fn):
    """Median and minimum ms of ``fn`` over ROUNDS rounds of LAUNCHES calls between device events, after a warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / LAUNCHES)
    return float(np.median(ts)), float(min(ts))


def designs_of(rng, R, T, n, confounds):
    step = (T - 14.0) / n
    out = []
    for _ in range(R):
        ev = [((1.0 + i * step + 0.3 * rng.rand()) * TR, min(3.0, 0.7 * step) * TR, 'ab'[i % 2]) for i in range(n)]
        out.append(glm.trial_design(events=ev, T=T, tr=TR, high_pass=None, confounds=rng.randn(T, confounds)))
    return out


def torch_epilogue(p, a, yy, T, q, G, own, rank, w, F, toffs):
    """The epilogue of chebgcn_glm_trials in torch float64 on stored projections ``p`` [R, n, Mp]: ``(beta, t)`` float32."""
    R, n, Mp = p.shape
    c = a[:, q:q + G]                                                                   # [R, G, Mp]
    onehot = torch.nn.functional.one_hot(own.long().view(R, n), G).to(torch.float64)     # [R, n, G]
    d = torch.cat([p.unsqueeze(2), c.unsqueeze(1) - onehot.unsqueeze(3) * p.unsqueeze(2)], dim=2)       # [R, n, G1, Mp]
    w, F = w.view(R, n, G + 1), F.view(R, n, G + 1, G + 1)
    beta = (w.unsqueeze(3) * d).sum(dim=2)
    Fd = torch.einsum('rnab,rnbm->rnam', F, d)
    ssq = (a[:, :q] * a[:, :q]).sum(dim=1).unsqueeze(1) + (Fd * Fd).sum(dim=2)
    y2 = yy.unsqueeze(1)
    rk = rank.view(R, n, 1).to(torch.float64)
    rss = y2 - ssq
    rss = torch.where(rss < 4.0 * (T + q + rk) * 2.0 ** -53 * y2, torch.zeros_like(rss), rss)
    var = rss / (T - q - rk) * w[:, :, :1]
    t = torch.where(var > 0, beta / torch.sqrt(torch.where(var > 0, var, torch.ones_like(var))), torch.zeros_like(var))
    return beta.to(torch.float32), t.to(torch.float32)


def bench(R, T, M, confounds, n, dev, fused_only=False):
    rng = np.random.RandomState(n)
    designs = designs_of(rng, R, T, n, confounds)
    Mp = _lib.plane_stride(M)
    planes = torch.zeros((R * T, Mp), dtype=torch.float32, device=dev)
    planes[:, :M] = 1e4 + 50.0 * torch.randn((R * T, M), device=dev, generator=torch.Generator(dev).manual_seed(n))
    runs = [planes[r * T:(r + 1) * T, :M] for r in range(R)]
    pl = glm._trial_plan(runs, designs, 'condition', ('beta', 't'), None, 'bench')
    G, q = pl.G, pl.tables[0].q
    assert all(tb.q == q for tb in pl.tables)
    Q, Z, toffs, qrank, own, rank, w, F = (torch.as_tensor(a).to(dev) for a in glm._trial_tables(pl.tables, G))
    offs = torch.as_tensor(np.arange(R + 1, dtype=np.int64) * T).to(dev)
    k, N = int(Q.shape[1]), R * n
    out = {'n': n, 'q': q, 'G': G}

    def fused():
        a, yy = ops.glm_project(planes, offs, M, Q)
        return ops.glm_trials(planes, offs, M, Z, toffs, a, yy, qrank, own, rank, w, F, outputs=('beta', 't'))

    a, yy = ops.glm_project(planes, offs, M, Q)
    a, yy = a.clone(), yy.clone()
    beta_f, _, t_f = fused()
    med, lo = timed(fused)
    tmed, tlo = timed(lambda: ops.glm_trials(planes, offs, M, Z, toffs, a, yy, qrank, own, rank, w, F, outputs=('beta', 't')))
    nbytes, flops = ops.glm_trials_model(R * T, Mp, R, k, n, N, G + 1, 2)
    out['fused'] = {'median_ms': med, 'min_ms': lo, 'trials_ms': tmed, 'trials_min_ms': tlo, 'dispatch': _lib.last_dispatch(),
                    'model_bytes': nbytes, 'model_flops': flops, 'hbm_spec_share': nbytes / (tmed * 1e-3) / HBM_SPEC,
                    'hbm_copy_share': nbytes / (tmed * 1e-3) / HBM_COPY, 'fma64_share': flops / 2.0 / (tmed * 1e-3) / FMA64}

    if fused_only:
        return out

    p = torch.empty((R, n, Mp), dtype=torch.float64, device=dev)

    def unfused():
        for j0 in range(0, n, 64):
            pj = ops.glm_project(planes, offs, M, Z[:, j0:j0 + 64].contiguous())[0]
            p[:, j0:j0 + 64] = pj
        a2, yy2 = ops.glm_project(planes, offs, M, Q)
        return torch_epilogue(p, a2, yy2, T, q, G, own, rank, w, F, toffs)

    beta_u, t_u = unfused()
    out['unfused_vs_fused_beta_rel'] = float((beta_u - beta_f.view(R, n, Mp)).abs().max() / beta_f.abs().max())
    med, lo = timed(unfused)
    out['unfused'] = {'median_ms': med, 'min_ms': lo, 'workspace_bytes': 8.0 * R * (n + k + 1) * Mp}
    del p, beta_u, t_u

    t0 = time.perf_counter()
    y64 = planes.view(R, T, Mp).to(torch.float64)
    torch.cuda.synchronize()
    convert = time.perf_counter() - t0
    W = torch.cat([Q, Z], dim=1).view(R, T, k + n).transpose(1, 2).contiguous()
    med, lo = timed(lambda: torch.bmm(W, y64))
    out['matmul'] = {'median_ms': med, 'min_ms': lo, 'convert_ms': 1e3 * convert}
    del y64, W

    picks = sorted({0, n // 3, 2 * n // 3, n - 1})

    def explicit(j):
        ds = []
        for tb in pl.tables:
            D = np.concatenate([tb.X[:, j:j + 1], glm._others(tb, j, G)[:, tb.keep[j, 1:]], tb.N], axis=1)
            ds.append(glm.Design(D, ['c%d' % i for i in range(D.shape[1])], ['c0']))
        return ds

    glm.first_level(runs, explicit(0), np.eye(1, 1 + G + confounds + 1), betas=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in picks:
        res = glm.first_level(runs, explicit(j), np.eye(1, int(pl.tables[0].keep[j].sum()) + confounds + 1), betas=True)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / len(picks)
    out['first_level'] = {'per_trial_index_ms': 1e3 * per, 'scaled_to_n_ms': 1e3 * per * n, 'timed_trial_indices': picks}
    out['first_level_vs_fused_beta_rel'] = float((res.betas[0][0] - beta_f[n - 1, :M]).abs().max() / beta_f[n - 1, :M].abs().max())

    glm.single_trial(runs, designs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    glm.single_trial(runs, designs)
    torch.cuda.synchronize()
    out['end_to_end_s'] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--runs', type=int, default=8)
    ap.add_argument('--rows', type=int, default=284)
    ap.add_argument('--vertices', type=int, default=20484)
    ap.add_argument('--confounds', type=int, default=8)
    ap.add_argument('--trials', type=int, nargs='+', default=[32, 96])
    ap.add_argument('--fused-only', action='store_true', help='time the fused route alone (for a variant library)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('single_trial_bench needs an MI355X')
    dev = torch.device('cuda')
    res = {'device': torch.cuda.get_device_name(0), 'R': a.runs, 'T': a.rows, 'M': a.vertices,
           'cases': [bench(a.runs, a.rows, a.vertices, a.confounds, n, dev, a.fused_only) for n in a.trials]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
