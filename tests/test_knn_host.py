"""kNN graphs, the parts that need no device: the ABI, the argument checks of ``graph.knn_device`` /
``graph.connectivity_graph`` (refused before the device is touched), the float64 brute-force kNN the GPU tests compare against
(checked here against ``distance_sklearn_metrics``), and the host path against tests/golden/knn_ref.npz, which holds what the
reference's own ``distance_sklearn_metrics`` + ``adjacency`` gave (tools/gen_knn_golden.py)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import assert_csr_equal, load_golden
from gcn_fmri_decoding_amd import _lib, graph

METRICS = ('euclidean', 'cosine', 'correlation')


def similarity64(z, metric):
    """float64 similarity (cosine / correlation; zero-norm and constant rows: 0 to everything) or, for 'euclidean', the
    squared-free distance matrix by differences.  Dense: test sizes only."""
    z = np.asarray(z, np.float64)
    if metric == 'euclidean':
        d = np.zeros((len(z), len(z)))
        for c in range(z.shape[1]):                   # by differences, never the Gram form
            d += (z[:, None, c] - z[None, :, c]) ** 2
        return np.sqrt(d)
    if metric == 'correlation':
        z = z - z.mean(axis=1, keepdims=True)
    n = np.sqrt((z * z).sum(axis=1))
    zn = z * np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)[:, None]
    return zn @ zn.T


def knn64(z, k, metric):
    """Brute-force float64 kNN: (d [N, k + 1] ascending, idx [N, k + 1], full distance matrix); self excluded by index, ties
    by lower index.  One more neighbour than asked for, for the gap rule."""
    s = similarity64(z, metric)
    d = s if metric == 'euclidean' else 1.0 - s
    d = d.copy()
    np.fill_diagonal(d, np.inf)
    kk = min(k + 1, len(d) - 1)
    idx = np.argsort(d, axis=1, kind='stable')[:, :kk]
    return np.take_along_axis(d, idx, 1), idx, d


def test_abi_symbols_exist():
    lib = _lib.lib()
    for name in ('chebgcn_knn', 'chebgcn_knn_workspace', 'chebgcn_series_normalise'):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert (_lib.KNN_EUCLIDEAN, _lib.KNN_COSINE, _lib.KNN_CORRELATION) == (0, 1, 2)
    assert lib.chebgcn_knn_workspace(1000, 3, 8) > 0
    assert lib.chebgcn_knn_workspace(20000, 1200, 32) > 0


@pytest.mark.parametrize('N,D,k,code', [(100, 3, 33, -4), (100, 3, 0, -1), (8, 3, 8, -1), (8, 3, 9, -1), (1, 3, 1, -1),
                                        (100, 0, 4, -1)])
def test_abi_refuses_shapes_before_any_launch(N, D, k, code):
    """k outside [1, 32] or k >= N: a status from status.h, with every pointer NULL (nothing can have been launched)."""
    lib = _lib.lib()
    rc = lib.chebgcn_knn(None, N, D, k, 0, None, None, None, 0, None)
    assert rc == code, (rc, lib.chebgcn_last_error())
    assert lib.chebgcn_knn_workspace(N, D, k) == 0


def test_value_errors_without_a_device(monkeypatch):
    import torch
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(torch.cuda, 'current_device', boom)
    monkeypatch.setattr(torch.Tensor, 'to', boom)
    z = np.random.RandomState(0).rand(50, 3).astype(np.float32)
    with pytest.raises(ValueError):
        graph.knn_device(z, k=4, metric='manhattan')
    for k in (0, 33, 50, 51):
        with pytest.raises(ValueError):
            graph.knn_device(z, k=k)
    with pytest.raises(ValueError):
        graph.knn_device(z[0], k=4)
    with pytest.raises(ValueError):
        graph.knn_device(z[None], k=4)
    bad = z.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        graph.knn_device(bad, k=4)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        graph.knn_device(bad, k=4, metric='cosine')
    runs = [np.random.RandomState(1).randn(20, 12).astype(np.float32) for _ in range(2)]
    with pytest.raises(ValueError):
        graph.connectivity_graph(runs, k=12)
    with pytest.raises(ValueError):
        graph.connectivity_graph([runs[0], runs[1][:, :5]], k=3)
    with pytest.raises(ValueError):
        graph.connectivity_graph([runs[0], runs[1][:1]], k=3)
    with pytest.raises(ValueError):
        graph.connectivity_graph([], k=3)
    with pytest.raises(ValueError):
        graph.synthetic_graph(64, knn='gpu')


@pytest.mark.parametrize('metric', METRICS)
def test_float64_helper_agrees_with_host_path(metric):
    rs = np.random.RandomState(5)
    z = (rs.randn(120, 6) + 0.4).astype(np.float32)       # continuous: no ties
    k = 7
    d, idx = graph.distance_sklearn_metrics(z, k=k, metric=metric)
    d64, i64, _ = knn64(z, k, metric)
    assert np.array_equal(idx, i64[:, :k])
    np.testing.assert_allclose(d, d64[:, :k], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('name', ['cube', 'feat'])
@pytest.mark.parametrize('metric', METRICS)
def test_host_path_reproduces_reference_fixture(name, metric):
    g = load_golden('knn_ref')
    z, k = g['z_' + name], int(g['k'])
    key = '%s_%s' % (name, metric)
    d, idx = graph.distance_sklearn_metrics(z, k=k, metric=metric)
    assert np.array_equal(idx, g['idx_' + key])
    np.testing.assert_allclose(d, g['d_' + key], rtol=1e-6, atol=1e-7)
    A_ref = sp.csr_matrix((g['A_%s_data' % key], g['A_%s_indices' % key], g['A_%s_indptr' % key]),
                          shape=tuple(g['A_%s_shape' % key]))
    assert_csr_equal(graph.adjacency(d, idx), A_ref, exact=False, rtol=1e-5, atol=1e-7)
    # the fixture's tables are what the float64 helper finds as well
    d64, i64, _ = knn64(z, k, metric)
    assert np.array_equal(i64[:, :k], g['idx_' + key])
