"""Graph-filter timings (EXPERIMENTS): chebgcn_cheb_filter against what the library could do before it for the same
result -- chebgcn_recurrence_fwd into a K-slab stack, then a torch.einsum over k.

    python tools/filter_bench.py [--out FILE]

Shapes: a sphere-like kNN graph (k = 6, graph.knn_device) of M = 32 492 vertices, which has no on-chip image (rolling arm against
the launch-per-step fallback + einsum), and one of M = 10 000 in length order (stack arm and rolling arm against the ordered
recurrence + einsum); 256 planes, heat(8) at K = 30, J = 1 and 4.  HIP events after warm-up, medians of 20 repeats, the variants
interleaved in both orders.  Prints one JSON line per (shape, J)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_fmri_decoding_amd import _lib, filters, graph, ops  # noqa: E402

DEV = torch.device('cuda', 0)
PLANES, K, REPS, WARM = 256, 30, 20, 3


def sphere_graph(M, relabel):
    z = np.random.RandomState(0).standard_normal((M, 3))
    z = (z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float32)
    L = graph.laplacian(graph.adjacency(*graph.knn_device(z, k=6, device=DEV)), normalized=True)
    return ops.Graph(L, DEV, order=graph.length_order(L) if relabel else None)


def medians(variants):
    """name -> fn; interleaved in both orders; name -> [median ms in order 1, in order 2]."""
    names = list(variants)
    out = {n: [] for n in names}
    for order in (names, names[::-1]):
        for n in order:
            for _ in range(WARM):
                variants[n]()
        ev = {n: [] for n in names}
        for _ in range(REPS):
            for n in order:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                variants[n]()
                b.record()
                ev[n].append((a, b))
        torch.cuda.synchronize()
        for n in names:
            out[n].append(float(np.median([a.elapsed_time(b) for a, b in ev[n]])))
    return out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def bench(M, relabel, J):
    g = sphere_graph(M, relabel)
    x = torch.randn((PLANES, g.Mp), device=DEV)
    hs = [filters.heat(8.0), filters.heat(2.0), filters.mexican_hat(4.0), filters.mexican_hat(1.0)][:J]
    coeff = torch.as_tensor(np.atleast_2d(filters.cheb_coefficients(hs, K)).astype(np.float32)).to(DEV)
    lib = _lib.lib()
    y = torch.empty((J, PLANES, g.Mp), device=DEV)
    names = {}

    def arm(a):
        def run():
            ops.cheb_filter(g, x, coeff, arm=a, out=y)
            names[a] = _lib.last_dispatch()
        return run

    def parent():
        stack = torch.empty((K, PLANES, g.Mp), device=DEV)
        _lib.check(lib.chebgcn_recurrence_fwd(g.handle, ops._p(x), ops._p(stack), 1, PLANES, K, ops._stream()), 'recurrence_fwd')
        names['parent'] = _lib.last_dispatch() + ' + einsum'
        return torch.einsum('jk,kpm->jpm', coeff, stack)

    image = g.on_chip or g.ordered
    variants = {'rolling': arm(1), 'parent': parent}
    if image:
        variants['stack'] = arm(2)
    ref = parent()[:, :, :g.M]
    scale = float(ref.abs().max())
    err = {}
    for n, fn in variants.items():
        if n != 'parent':
            fn()
            err[n] = float((y[:, :, :g.M] - ref).abs().max()) / scale
    del ref
    ops._workspaces.clear()
    mem = {n: peak(fn) for n, fn in variants.items()}
    ms = medians(variants)
    slab = 4.0 * PLANES * g.Mp
    return {'M': M, 'Mp': g.Mp, 'nnz': g.nnz, 'planes': PLANES, 'K': K, 'J': J, 'image': bool(image), 'slab_MiB': slab / 2 ** 20,
            'median_ms_both_orders': ms, 'peak_MiB': mem, 'max_diff_vs_parent_over_scale': err,
            'dispatch': {str(k): v for k, v in names.items()}}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for M, relabel in ((32492, False), (10000, True)):
        for J in (1, 4):
            rows.append(bench(M, relabel, J))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
