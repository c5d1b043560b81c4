"""Permutation-inference timings (EXPERIMENTS): ``stats.map_test(stat='tfce')`` on the device, in both arms of
chebgcn_cluster_enhance, against its host restatement ``stats.map_test_host`` (SciPy connected components per height and
permutation) on the same inputs.

    python tools/map_test_bench.py [--out FILE] [--perms 1000] [--device-seconds 0.5] [--host-seconds 60]

Shapes: an atlas-sized kNN graph of N = 360 vertices (on chip by itself; the streamed arm forced beside it) and the N = 10 000
benchmark graph whose checksums tests/golden/bench_graph_n10000.npz holds (streamed; above the on-chip limit), S = 20 maps of
neighbour-averaged unit noise with an effect on a tenth of the vertices, tail = 1, the default step (100 heights on the observed
map).  The device is timed end to end -- uploads, kernels, the download of the null, p-values -- with a host clock around a call that
ends synchronised, after a warm-up call, three repeats per arm with the arms alternating.  A call runs as many permutations as
a calibration call predicts for ``--device-seconds`` (at least ``--perms``); all times are reported per ``--perms`` permutations.
The host is timed on as many permutations as a calibration on 4 predicts for ``--host-seconds`` and scaled likewise; its null
must equal the device's on those permutations bit for bit, or the script fails.  No GPU: the script fails, it never falls
back.  Prints one JSON line per shape."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_fmri_decoding_amd import _lib, graph, ops, stats  # noqa: E402

S, REPS = 20, 3


def inputs(N):
    _, _, graphs = graph.synthetic_graph(N, k=8, levels=0)
    A = sp.csr_matrix(graphs[0])
    if N == 10000:
        z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                 'bench_graph_n10000.npz'))
        assert A.nnz == int(z['A_nnz']) and hashlib.sha256(np.ascontiguousarray(A.indices.astype(np.int64)).tobytes()).hexdigest() \
            == str(z['A_indices_sha256']), 'not the benchmark graph of tests/golden'
    rs = np.random.RandomState(1)
    x = rs.randn(S, N)
    x[:, :N // 10] += 0.8
    W = (A > 0).astype(np.float64) + sp.identity(N)
    x = (W @ x.T).T / np.asarray(W.sum(1)).ravel()[None, :]
    return A, x.astype(np.float32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench(N, perms, device_seconds, host_seconds):
    A, x = inputs(N)
    kw = dict(stat='tfce', tail=1, seed=0)
    arms = {'streamed': 2}
    if N <= ops.cluster_geometry()['onchip_M']:
        arms = {'on_chip': 0, 'streamed': 2}
    res, secs, names = {}, {a: [] for a in arms}, {}
    run = perms
    for a, code in arms.items():                        # warm-up (code objects, workspaces) and calibration
        stats.ARM = code
        stats.map_test(x, A, n_perm=64, **kw)
        dt, _ = timed(lambda: stats.map_test(x, A, n_perm=perms, **kw))
        run = max(run, min(int(perms * device_seconds / dt), 400000))
    for _ in range(REPS):
        for a, code in arms.items():
            stats.ARM = code
            dt, res[a] = timed(lambda: stats.map_test(x, A, n_perm=run, **kw))
            names[a] = _lib.last_dispatch()
            secs[a].append(dt * perms / run)
    stats.ARM = 0
    first = res[next(iter(arms))]
    for a in arms:
        assert np.array_equal(res[a].null, first.null) and np.array_equal(res[a].p, first.p), 'the arms disagree'
    t0 = time.perf_counter()
    stats.map_test_host(x, A, n_perm=4, **kw)
    per = (time.perf_counter() - t0) / 4
    ph = int(min(run, max(8, host_seconds / per)))
    t0 = time.perf_counter()
    host = stats.map_test_host(x, A, n_perm=ph, **kw)
    host_s = time.perf_counter() - t0
    assert np.array_equal(host.null, first.null[:ph]) and np.array_equal(host.stat, first.stat), 'device and host disagree'
    host_scaled = host_s * perms / ph
    med = {a: float(np.median(v)) for a, v in secs.items()}
    return {'N': N, 'S': S, 'perms': perms, 'device_perms_per_call': run, 'heights_observed': int(np.floor(first.t.max() / first.step)),
            'significant_vertices': int((first.p < 0.05).sum()), 'device_s_per_perms': secs, 'device_median_s_per_perms': med, 'dispatch': names,
            'host_perms': ph, 'host_s': host_s, 'host_s_per_perms': host_scaled,
            'host_over_device': {a: host_scaled / m for a, m in med.items()}}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--perms', type=int, default=1000)
    ap.add_argument('--device-seconds', type=float, default=0.5)
    ap.add_argument('--host-seconds', type=float, default=60.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('map_test_bench: needs an MI355X')
    rows = []
    for N in (360, 10000):
        rows.append(bench(N, args.perms, args.device_seconds, args.host_seconds))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
