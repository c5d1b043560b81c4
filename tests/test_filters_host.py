"""Graph filters, the parts that need no device: Chebyshev coefficients against closed forms, ``cheb_order``, the float64
restatement ``GraphFilter.apply_host`` against the exact ``U h(Lambda) U^T x`` of a dense eigendecomposition, every refusal, and
the C entry point's argument checks.  ``knn_laplacian`` is what tests/test_gpu_filters.py builds its graphs with.

The bound against ``eigh`` is derived, not measured: on the spectrum ``|h(lambda) - sum_{k<K} c_k T_k| <= tail(K) = sum_{k>=K}
|c_k|`` (``|T_k| <= 1``), so a row x of the input is filtered within ``tail(K) * ||x||_2`` in the 2-norm, hence in every entry.
The tail is taken over 256 coefficients; what lies beyond is below float64 round-off for the filters used here.  A float32
normalised Laplacian is its own float32-rounded operand (``L - I`` is exact), so with ``lmax = 2`` nothing else enters.  With
``lmax != 2`` the entries of ``L * (2 / lmax)`` are rounded to float32 (``apply_host`` restates the device's operands): a
perturbation dL of the operator moves T_k by at most ``k^2 ||dL||_2`` and ``||dL||_2 <= 2^-24 || |L~| ||_2 <= 2 * 2^-24``, the
coefficients of a filter with ``0 <= h <= 1`` are at most 2 in magnitude and decay, so that test allows ``2 K^2 2^-24 ||x||_2``
on top of the tail."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.special import ive

from gcn_fmri_decoding_amd import GraphFilter, _lib, filters, graph

U32 = 2.0 ** -24


def knn_laplacian(M, k=8, seed=0, normalized=True, dim=3):
    """The Laplacian of a kNN graph on M random points (graph.distance_sklearn_metrics -> adjacency -> laplacian), float32."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((M, dim)).astype(np.float32)
    dist, idx = graph.distance_sklearn_metrics(z, k=min(k, M - 1))
    return graph.laplacian(graph.adjacency(dist, idx), normalized=normalized)


def exact(L, h, x):
    """U h(Lambda) U^T x in float64; x [R, M]."""
    lam, Uu = np.linalg.eigh(L.toarray().astype(np.float64))
    return (Uu @ (h(lam)[:, None] * (Uu.T @ x.astype(np.float64).T))).T


def tail(h, K, lmax=2.0):
    return np.abs(filters.cheb_coefficients(h, 256, lmax))[K:].sum()


@pytest.fixture(scope='module')
def L100():
    return knn_laplacian(100)


@pytest.mark.parametrize('t', [0.5, 2.0, 8.0, 30.0])
def test_heat_coefficients_match_the_bessel_closed_form(t):
    K = 60
    k = np.arange(K)
    ref = 2.0 * (-1.0) ** k * ive(k, t)              # ive = exp(-t) I_k(t)
    ref[0] *= 0.5
    c = filters.cheb_coefficients(filters.heat(t), K)
    assert c.shape == (K,) and c.dtype == np.float64
    assert np.abs(c - ref).max() <= 1e-13


def test_polynomial_coefficients_are_exact():
    # h(lambda) = T_3(t) - 0.5 T_2(t) + 0.25 T_1(t) + 2 with t = lambda - 1
    def h(lam):
        t = lam - 1.0
        return (4 * t ** 3 - 3 * t) - 0.5 * (2 * t ** 2 - 1) + 0.25 * t + 2.0
    c = filters.cheb_coefficients(h, 12)
    assert np.abs(c[:4] - [2.0, 0.25, -0.5, 1.0]).max() <= 1e-14
    assert np.abs(c[4:]).max() <= 1e-14


def test_list_of_callables_gives_a_table():
    hs = [filters.heat(1.0), filters.mexican_hat(2.0), filters.heat(3.0)]
    c = filters.cheb_coefficients(hs, 9)
    assert c.shape == (3, 9)
    for j, h in enumerate(hs):
        assert np.array_equal(c[j], filters.cheb_coefficients(h, 9))


def test_cheb_order():
    h = filters.heat(8.0)
    ks = [filters.cheb_order(h, tol) for tol in (1e-2, 1e-4, 1e-6, 1e-9)]
    assert ks == sorted(ks) and ks[0] < ks[-1]
    for tol, K in zip((1e-2, 1e-4, 1e-6, 1e-9), ks):
        assert tail(h, K) <= tol and (K == 1 or tail(h, K - 1) > tol)
    assert filters.cheb_order(lambda lam: 3.0 + 0 * lam, 1e-6) == 1
    assert filters.cheb_order([filters.heat(2.0), h], 1e-6) == max(filters.cheb_order(filters.heat(2.0), 1e-6), ks[2])
    with pytest.raises(ValueError, match='kmax'):
        filters.cheb_order(filters.heat(30.0), 1e-9, kmax=16)


@pytest.mark.parametrize('name', ['heat', 'mexican_hat'])
def test_apply_host_against_eigh(L100, name):
    if name == 'heat':
        h, K = filters.heat(2.0), 10
        f = GraphFilter(L100, h, K=K)
    else:
        h = filters.mexican_hat(4.0)
        f = GraphFilter(L100, h)
        K = f.K
        assert K == filters.cheb_order(h, 1e-6) and tail(h, K) <= 1e-6
    x = np.random.RandomState(1).standard_normal((7, 100)).astype(np.float32)
    got = f.apply_host(x)
    assert got.shape == (7, 100) and got.dtype == np.float64
    err = np.abs(got - exact(L100, h, x)).max(axis=1)
    norm = np.linalg.norm(x.astype(np.float64), axis=1)
    assert (err <= tail(h, K) * norm).all(), (err / norm, tail(h, K))


def test_lmax_of_a_combinatorial_laplacian():
    L = knn_laplacian(80, k=6, seed=3, normalized=False)
    lm = float(graph.lmax(L, normalized=False))
    h = filters.heat(0.7)
    f = GraphFilter(L, h, tol=1e-8, lmax=lm)
    assert f.K == filters.cheb_order(h, 1e-8, lmax=lm)
    x = np.random.RandomState(2).standard_normal((5, 80)).astype(np.float32)
    err = np.abs(f.apply_host(x) - exact(L, h, x)).max(axis=1)
    norm = np.linalg.norm(x.astype(np.float64), axis=1)
    assert (err <= (tail(h, f.K, lm) + 2 * f.K ** 2 * U32) * norm).all(), err / norm


def test_coeffs_given_directly(L100):
    c = filters.cheb_coefficients(filters.heat(2.0), 10)
    x = np.random.RandomState(4).standard_normal((3, 100)).astype(np.float32)
    a = GraphFilter(L100, coeffs=c).apply_host(x)
    b = GraphFilter(L100, filters.heat(2.0), K=10).apply_host(x)
    assert np.array_equal(a, b)
    assert GraphFilter(L100, coeffs=c[None]).apply_host(x).shape == (1, 3, 100)


def test_runs_and_filter_axes(L100):
    hs = [filters.heat(0.5 * (j + 1)) for j in range(9)]                 # more than one group of 8
    f = GraphFilter(L100, hs, K=12)
    assert (f.J, f.K, f.single) == (9, 12, False)
    rs = np.random.RandomState(5)
    runs = [rs.standard_normal((4, 100)).astype(np.float32), rs.standard_normal((2, 100)).astype(np.float32)]
    out = f.apply_host(runs)
    assert isinstance(out, list) and [o.shape for o in out] == [(9, 4, 100), (9, 2, 100)]
    for j, h in enumerate(hs):                                          # every filter in its own place
        assert np.array_equal(out[0][j], GraphFilter(L100, h, K=12).apply_host(runs[0]))
    assert np.array_equal(f.apply_host(runs[1]), out[1])
    one = GraphFilter(L100, hs[0], K=12).apply_host(runs)
    assert isinstance(one, list) and one[0].shape == (4, 100)


def test_refusals(L100):
    import torch
    h = filters.heat(1.0)
    with pytest.raises(ValueError, match='L must be square'):
        GraphFilter(sp.csr_matrix(np.ones((3, 4))), h)
    A = L100.tolil(copy=True)
    A[0, 1] = A[0, 1] + 0.5
    with pytest.raises(ValueError, match='L must be symmetric'):
        GraphFilter(A.tocsr(), h)
    with pytest.raises(ValueError, match='K = 257'):
        GraphFilter(L100, h, K=257)
    with pytest.raises(ValueError, match='K = 300'):
        GraphFilter(L100, coeffs=np.ones(300))
    with pytest.raises(ValueError, match='coeffs hold non-finite'):
        GraphFilter(L100, coeffs=[1.0, np.nan])
    with pytest.raises(ValueError, match='coefficients of h hold non-finite'):
        GraphFilter(L100, lambda lam: np.full_like(lam, np.nan), K=4)
    with pytest.raises(ValueError, match='either h or coeffs'):
        GraphFilter(L100)
    with pytest.raises(ValueError, match='relabel'):
        GraphFilter(L100, h, relabel='yes')
    f = GraphFilter(L100, h, K=4)
    for bad in (np.zeros((3, 99), np.float32), np.zeros(100, np.float32), [np.zeros((3, 100)), np.zeros((3, 101))]):
        with pytest.raises(ValueError, match='series'):
            f.apply_host(bad)
        with pytest.raises(ValueError, match='series'):
            f.apply(bad)
    with pytest.raises(ValueError, match='series is a float64 tensor'):
        f.apply(torch.zeros((3, 100), dtype=torch.float64))
    with pytest.raises(ValueError, match='chunk_rows'):
        f.apply(np.zeros((3, 100), np.float32), chunk_rows=0)
    with pytest.raises(ValueError, match='arm'):
        f.apply(np.zeros((3, 100), np.float32), arm=3)


def test_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.lib()
    assert _lib.FILTER_JMAX == filters.JMAX and _lib.FILTER_KMAX == filters.KMAX
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(g=None, x=p, c=p, y=p, ws=p, nplanes=1, K=4, J=2, arm=0):
        rc = lib.chebgcn_cheb_filter(g, x, c, y, ws, nplanes, K, J, arm, None)
        return rc, lib.chebgcn_last_error().decode()

    assert call() == (-1, 'cheb_filter: NULL argument')
    for kw, word in (({'J': 0}, 'J = 0'), ({'J': 9}, 'J = 9'), ({'K': 0}, 'K = 0'), ({'K': 257}, 'K = 257'),
                     ({'arm': 3}, 'arm = 3'), ({'arm': -1}, 'arm = -1'), ({'nplanes': 0}, 'nplanes = 0'),
                     ({'nplanes': 1 << 30}, 'nplanes = ')):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    assert lib.chebgcn_cheb_filter_workspace(None, 4, 4, 2, 1) == 0
