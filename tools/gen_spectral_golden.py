#!/usr/bin/env python3
"""Generate tests/golden/inference_{fourier,spline}_n*.npz by RUNNING THE REFERENCE's spectral filters.

The reference's ``fourier`` / ``spline`` / ``filter_in_fourier`` / ``_inference`` (lib_new/models_gcn.py:512-556, :658-682)
run verbatim under the NumPy stand-in for TensorFlow of ``oracle.gen_golden`` (plus ``tf.constant``), with the same
preset-variable harness as ``gen_golden.run_inference``, on uncoarsened kNN graphs.  Each file holds the Laplacians, their
eigenvalues / eigenvectors (``graph.fourier``), the spline bases, the variables, the input and the logits.

    python tools/gen_spectral_golden.py [--ref <reference checkout>] [--out tests/golden]

The output depends on the basis only up to the sign of each eigenvector, and only while no eigenvalue repeats: every graph
used here is checked for a minimum gap between consecutive eigenvalues.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as G      # noqa: E402

MIN_EIGEN_GAP = 5e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference project (holds lib_new/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()

    tf = G._make_tf_stub([])
    tf.constant = lambda value, dtype=None: G._t(np.asarray(value, dtype))
    sys.modules['tensorflow'] = tf
    sys.path.insert(0, args.ref)
    import lib_new.graph as rgraph
    import lib_new.models_gcn as rmodels

    class Harness(rmodels.cgcnn):
        """cgcnn without __init__: variables come from a preset list."""

        def __init__(self, variables, **attrs):      # noqa: super not called on purpose
            self._vars = list(variables)
            self.__dict__.update(attrs)

        def _weight_variable(self, shape, regularization=True):
            v = self._vars.pop(0)
            assert list(v.shape) == [int(s) for s in shape], (v.shape, shape)
            return G._t(v)

        _bias_variable = _weight_variable

    def knn_laplacian(N, k, seed):
        z = np.random.RandomState(seed).rand(N, 3).astype(np.float32)
        d, idx = rgraph.distance_sklearn_metrics(z, k=k, metric='euclidean')
        A = rgraph.adjacency(d, idx).astype(np.float32)
        L = sp.csr_matrix(rgraph.laplacian(A, normalized=True))
        lamb, U = rgraph.fourier(L)
        gap = float(np.diff(lamb.astype(np.float64)).min())
        assert gap >= MIN_EIGEN_GAP, 'graph N=%d seed=%d: eigen-gap %.2e' % (N, seed, gap)
        return L, lamb, U, gap

    rs = np.random.RandomState(11)

    def run(name, Ls_all, filt, F, K, p, Mfc, channel, brelu, N):
        Lk, j = [], 0
        for pp in p:
            Lk.append(Ls_all[j])
            j += int(np.log2(pp)) if pp > 1 else 0
        variables, names = [], []
        Fin = channel
        for i, (Fo, Kk, pp) in enumerate(zip(F, K, p)):
            Mi = Lk[i].shape[0]
            shape = (Mi, Fo, Fin) if filt == 'fourier' else (Kk, Fo * Fin)
            variables.append((rs.randn(*shape) * np.sqrt(1.0 / Fin)).astype(np.float32))
            names.append('conv%d/weights' % (i + 1))
            bshape = (1, 1, Fo) if brelu == 'b1relu' else (1, Mi, Fo)
            variables.append((0.1 * rs.randn(*bshape)).astype(np.float32))
            names.append('conv%d/bias' % (i + 1))
            Fin = Fo
        Min = Lk[-1].shape[0] // p[-1]
        for i, Mo in enumerate(Mfc):
            scope = 'logits' if i == len(Mfc) - 1 else 'fc%d' % (i + 1)
            variables.append((rs.randn(Min, Mo) * np.sqrt(2.0 / Min)).astype(np.float32))
            names.append(scope + '/weights')
            variables.append((0.2 + 0.1 * rs.randn(Mo)).astype(np.float32))
            names.append(scope + '/bias')
            Min = Mo
        x = rs.randn(N, Lk[0].shape[0], channel).astype(np.float32)
        h = Harness([v.copy() for v in variables], L=Lk, F=F, K=K, p=p, M=Mfc)
        h.filter, h.brelu, h.pool = getattr(h, filt), getattr(h, brelu), h.mpool1
        with contextlib.redirect_stdout(io.StringIO()):      # spline() prints its shapes
            logits = h._inference(G._t(x), 1)
        assert not h._vars
        fields = dict(x=x, logits=np.asarray(logits), F=np.array(F), K=np.array(K), p=np.array(p), M=np.array(Mfc),
                      channel=np.int64(channel), brelu=np.array(brelu), filter=np.array(filt),
                      nlevels=np.int64(len(Ls_all)), numpy_version=np.array(np.__version__))
        for i, L in enumerate(Ls_all):
            fields.update(G._csr_fields('L%d' % i, L))
            lamb, U = rgraph.fourier(L)
            fields['lamb%d' % i], fields['U%d' % i] = lamb, U
        if filt == 'spline':
            for i, Kk in enumerate(K):
                lamb, _ = rgraph.fourier(Lk[i])
                fields['B%d' % i] = np.asarray(rmodels.bspline_basis(Kk, lamb, degree=3))
        for n, v in zip(names, variables):
            fields['param:' + n] = v
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **fields)
        print('wrote %-34s %7.1f KB' % (name + '.npz', os.path.getsize(path) / 1024))

    L100, _, _, gap100 = knn_laplacian(100, 8, 7)
    L50, _, _, gap50 = knn_laplacian(50, 6, 3)
    print('eigen-gaps: N=100 %.2e, N=50 %.2e' % (gap100, gap50))
    run('inference_fourier_n100', [L100], 'fourier', F=[8, 6], K=[5, 5], p=[1, 1], Mfc=[16, 5], channel=3,
        brelu='b1relu', N=3)
    run('inference_fourier_n100_p21', [L100, L50], 'fourier', F=[6, 8], K=[3, 3], p=[2, 1], Mfc=[5], channel=2,
        brelu='b2relu', N=2)
    run('inference_spline_n100', [L100], 'spline', F=[8, 6], K=[10, 6], p=[1, 1], Mfc=[16, 5], channel=3,
        brelu='b1relu', N=3)
    run('inference_spline_n100_p21', [L100, L50], 'spline', F=[6, 8], K=[7, 5], p=[2, 1], Mfc=[5], channel=2,
        brelu='b2relu', N=2)


if __name__ == '__main__':
    main()
