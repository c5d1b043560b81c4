#!/usr/bin/env python3
"""Generate tests/golden/knn_ref.npz by RUNNING THE REFERENCE's graph construction.

The reference's ``distance_sklearn_metrics`` followed by ``adjacency`` (lib_new/graph.py:9-45) run verbatim on seeded inputs,
with the three metrics the function is called with or that this project serves ('euclidean', 'cosine', 'correlation'; all are
metrics of sklearn's ``pairwise_distances``, which is what the reference function takes).  Two inputs: coordinates in the unit
cube (300 x 3) and latent-factor features (257 x 12).  The file holds data only: the inputs, the ``[N, k]`` distance and index
tables and the adjacency matrices in CSR form.

    python tools/gen_knn_golden.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8


def inputs():
    rs = np.random.RandomState(20)
    cube = rs.rand(300, 3).astype(np.float32)
    load = rs.randn(257, 4) * (rs.rand(257, 4) < 0.5)
    feat = (load @ rs.randn(4, 12) + 0.7 * rs.randn(257, 12) + 0.5).astype(np.float32)
    return {'cube': cube, 'feat': feat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference project (holds lib_new/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import lib_new.graph as rgraph

    fields = {'k': np.int64(K), 'numpy_version': np.array(np.__version__)}
    for name, z in inputs().items():
        fields['z_' + name] = z
        for metric in ('euclidean', 'cosine', 'correlation'):
            d, idx = rgraph.distance_sklearn_metrics(z, k=K, metric=metric)
            A = sp.csr_matrix(rgraph.adjacency(d, idx))
            A.sort_indices()
            key = '%s_%s' % (name, metric)
            fields['d_' + key], fields['idx_' + key] = d, idx.astype(np.int64)
            fields['A_%s_data' % key], fields['A_%s_indices' % key] = A.data, A.indices.astype(np.int32)
            fields['A_%s_indptr' % key], fields['A_%s_shape' % key] = A.indptr.astype(np.int32), np.array(A.shape)
    path = os.path.join(args.out, 'knn_ref.npz')
    np.savez_compressed(path, **fields)
    print('wrote %s %.1f KB' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
