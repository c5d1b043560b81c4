"""Timings of ``chebgcn_perm_glm_t`` and of ``stats.design_test`` end to end (EXPERIMENTS 28).

    python tools/design_test_bench.py [--out FILE] [--subjects 100] [--vertices 10242] [--perms 256]

Kernel: S subjects, M vertices, Pb permutations with flips, a random orthonormal Uf of rank r for r in 1, 2, 4, 8, 12, 16, 33, 64;
device events around 20 launches, five rounds, median and minimum in ms per launch, after a warm-up launch whose first 4
permutations must equal ``stats.perm_t_host`` bit for bit.  ``pairs_per_s`` counts the float64 multiply-add pairs
``Pb M S r`` of the projections.  End to end: two groups and two nuisance columns on a random graph of degree 6, 1000
permutations, ``'max'`` and ``'tfce'``, a host clock around a call that ends synchronised, after a warm-up call; ``map_test``
on the same maps beside it.  The tile constants are build macros of ``csrc/cluster.hip`` (``CG_PERM_NW``, ``CG_PERM_PTL1``,
``CG_PERM_PTL4``, ``CG_PERM_PTL``, ``CG_PERM_U``, ``CG_PERM_UWIDE``): a variant is a library built with others, named by
``CHEBGCN_LIB``.  No GPU: the script fails, it never falls back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_fmri_decoding_amd import _lib, ops, stats  # noqa: E402

RANKS, LAUNCHES, ROUNDS = (1, 2, 4, 8, 12, 16, 33, 64), 20, 5


def kernel(S, M, Pb, r, dev):
    rs = np.random.RandomState(r)
    Uf = np.ascontiguousarray(np.linalg.qr(rs.randn(S, r))[0])
    u = rs.randn(r)
    e = rs.randn(S, M).astype(np.float32)
    ed = e.astype(np.float64)
    q = np.zeros(M)
    for j in range(S):
        q = q + ed[j] * ed[j]
    rows = stats.permutations(S, Pb, 1, flips=True)
    te, tq, tU, tu = (torch.as_tensor(a).to(dev) for a in (e, q, Uf, u))
    trows = torch.as_tensor(rows.view(np.int32)).to(dev)
    out = torch.empty((Pb, M), dtype=torch.float32, device=dev)
    ops.perm_glm_t(te, tq, tU, tu, 0.5, S - r, trows, out=out)
    if not np.array_equal(out[:4].cpu().numpy(), stats.perm_t_host(e, q, Uf, u, 0.5, S - r, rows[:4])):
        raise SystemExit('perm_glm_t differs from perm_t_host at r = %d' % r)
    ts = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            ops.perm_glm_t(te, tq, tU, tu, 0.5, S - r, trows, out=out)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / LAUNCHES)
    med = float(np.median(ts))
    return {'median_ms': med, 'min_ms': float(min(ts)), 'dispatch': _lib.last_dispatch(),
            'perms_per_workgroup': ops.perm_glm_geometry(r)['perms'], 'pairs_per_s': float(Pb) * M * S * r / (med * 1e-3)}


def end_to_end(S, M, perms):
    rs = np.random.RandomState(0)
    n = 3 * M
    pairs = np.stack([rs.randint(0, M, n), rs.randint(0, M, n)], 1)
    A = sp.csr_matrix((np.ones(n, np.float32), (pairs[:, 0], pairs[:, 1])), shape=(M, M))
    W = ((A + A.T) > 0).astype(np.float64) + sp.identity(M)
    x = rs.randn(S, M)
    x[::2, :M // 10] += 1.0
    x = np.ascontiguousarray((W @ x.T).T / np.asarray(W.sum(1)).ravel()[None, :], dtype=np.float32)
    g = (np.arange(S) % 2).astype(np.float64)
    D = np.column_stack([g, 1 - g, rs.randn(S, 2)])
    out = {}
    for stat in ('max', 'tfce'):
        kw = dict(stat=stat, tail=1, seed=1)
        stats.design_test(x, A, D, [1, -1, 0, 0], n_perm=20, **kw)
        stats.map_test(x, A, n_perm=20, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats.design_test(x, A, D, [1, -1, 0, 0], n_perm=perms, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stats.map_test(x, A, n_perm=perms, **kw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out[stat] = {'design_test_s': t1 - t0, 'map_test_s': t2 - t1}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--subjects', type=int, default=100)
    ap.add_argument('--vertices', type=int, default=10242)
    ap.add_argument('--perms', type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('design_test_bench needs an MI355X')
    dev = torch.device('cuda')
    res = {'device': torch.cuda.get_device_name(0), 'S': a.subjects, 'M': a.vertices, 'Pb': a.perms,
           'kernel': {str(r): kernel(a.subjects, a.vertices, a.perms, r, dev) for r in RANKS if r < a.subjects},
           'end_to_end_1000_perms': end_to_end(a.subjects, a.vertices, 1000)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
