"""connectome on the host: the NumPy yardstick against scikit-learn's LedoitWolf and against the definition of a partial
correlation, the clamp of the shrinkage, the mean, ``graph.knn_from_similarity``, and every refusal of ``connectome``,
``connectivity_graph(kind=)`` and the C entries -- none of it needs a GPU.

``connectome_host`` returns float32 matrices; its float64 values before the one rounding come from ``connectome.host_run``, which
is what the 1e-12 and 1e-10 bounds below are taken on (a float32 matrix cannot show them).
"""
import ctypes

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, connectome as cn, graph


def latent(T, R, seed, factors=4, rho=0.4, mix=1.0):
    """Latent-factor AR(1) series [T, R] float32: ``factors`` shared AR(1) sources mixed into R regions with weights of
    standard deviation ``mix``, plus white noise."""
    rng = np.random.RandomState(seed)
    e = rng.randn(T, factors)
    f = np.empty_like(e)
    f[0] = e[0]
    for t in range(1, T):
        f[t] = rho * f[t - 1] + e[t]
    return (f @ (mix * rng.randn(factors, R)) + rng.randn(T, R)).astype(np.float32)


@pytest.mark.parametrize('T,R', [(3, 5), (3, 33), (64, 129), (100, 360), (284, 360), (1200, 64)])
def test_covariance_and_shrinkage_are_scikit_learns(T, R):
    cov = pytest.importorskip('sklearn.covariance')
    x = latent(T, R, seed=T + R)
    lw = cov.LedoitWolf(store_precision=False).fit(x.astype(np.float64))
    h = cn.connectome_host(x, 'covariance')
    assert h.shrinkage.dtype == np.float64 and h.matrices.dtype == np.float32 and h.matrices.shape == (1, R, R)
    assert abs(h.shrinkage[0] - lw.shrinkage_) <= 1e-12 * abs(lw.shrinkage_)
    m64, s, flag = cn.host_run(x, 'covariance', -1.0)
    assert s == h.shrinkage[0] and not flag
    assert np.abs(m64 - lw.covariance_).max() <= 1e-12 * np.abs(lw.covariance_).max()
    assert np.array_equal(h.matrices[0], m64.astype(np.float32))


def test_partial_correlation_is_the_correlation_of_residuals():
    T, R = 200, 5
    x = latent(T, R, seed=7, factors=2)
    pc, _, flag = cn.host_run(x, 'partial correlation', 0.0)
    assert not flag
    d = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    for i in range(R):
        for j in range(i):
            others = [k for k in range(R) if k not in (i, j)]
            Z = d[:, others]
            ri = d[:, i] - Z @ np.linalg.lstsq(Z, d[:, i], rcond=None)[0]
            rj = d[:, j] - Z @ np.linalg.lstsq(Z, d[:, j], rcond=None)[0]
            ref = (ri @ rj) / np.sqrt((ri @ ri) * (rj @ rj))
            assert abs(pc[i, j] - ref) <= 1e-10, (i, j, pc[i, j], ref)
    prec, _, _ = cn.host_run(x, 'precision', 0.0)
    sigma, _, _ = cn.host_run(x, 'covariance', 0.0)
    assert np.abs(prec @ sigma - np.eye(R)).max() <= 1e-10
    for kind in cn.KINDS:
        m = cn.connectome_host(x, kind, 0.3).matrices[0]
        assert np.array_equal(m, m.T), kind
    for kind in ('correlation', 'partial correlation'):
        assert (np.diag(cn.connectome_host(x, kind).matrices[0]) == 1.0).all()


def test_two_time_points_shrinkage_is_a_positive_zero_and_precision_is_flagged():
    x = latent(2, 6, seed=3)
    for kind in cn.KINDS:
        h = cn.connectome_host(x, kind)
        assert h.shrinkage[0] == 0.0 and not np.signbit(h.shrinkage[0]), kind
        if kind in ('precision', 'partial correlation'):
            assert h.degenerate[0] and np.array_equal(h.matrices[0], np.eye(6, dtype=np.float32))
            assert not h.mean.any()
        else:
            assert not h.degenerate[0] and np.isfinite(h.matrices).all()


def test_degenerate_runs_by_kind():
    flat = np.full((30, 4), 3.5, np.float32)
    wide = latent(8, 12, seed=1)                        # T <= R: singular without shrinkage
    dead = latent(40, 6, seed=2)
    dead[:, 2] = 7.0                                    # a region constant in time
    for x, shrink, flagged in [(flat, 'auto', True), (wide, 0.0, True), (wide, 'auto', False), (dead, 0.0, True),
                               (dead, 'auto', False)]:
        for kind in ('precision', 'partial correlation'):
            h = cn.connectome_host(x, kind, shrink)
            assert bool(h.degenerate[0]) == flagged, (kind, shrink)
            assert np.isfinite(h.matrices).all()
            if flagged:
                assert np.array_equal(h.matrices[0], np.eye(x.shape[1], dtype=np.float32))
    c = cn.connectome_host(dead, 'correlation', 0.0).matrices[0]
    assert c[2, 2] == 1.0 and not np.delete(c[2], 2).any() and not np.delete(c[:, 2], 2).any() and not cn.connectome_host(
        dead, 'correlation', 0.0).degenerate[0]
    assert not cn.connectome_host(flat, 'covariance').matrices.any()


def test_mean_is_restated_bit_for_bit_and_leaves_degenerate_runs_out():
    runs = [latent(50, 7, seed=1), latent(2, 7, seed=2), latent(64, 7, seed=3), latent(33, 7, seed=4)]
    h = cn.connectome_host(runs, 'partial correlation')
    assert h.degenerate.tolist() == [False, True, False, False]
    acc, n = np.zeros((7, 7), np.float64), 0
    for m, flag in zip(h.matrices, h.degenerate):
        if not flag:
            acc += m.astype(np.float64)
            n += 1
    assert n == 3 and np.array_equal(h.mean, (acc / n).astype(np.float32)) and h.mean.dtype == np.float32
    assert np.array_equal(h.mean, cn.mean_of(h.matrices, h.degenerate))
    none = cn.connectome_host([runs[1], latent(2, 7, seed=5)], 'precision')
    assert none.degenerate.all() and none.mean.shape == (7, 7) and not none.mean.any()
    cov = cn.connectome_host(runs, 'covariance')
    assert not cov.degenerate.any() and np.array_equal(cov.mean, cn.mean_of(cov.matrices, [False] * 4))


def test_knn_from_similarity():
    m = np.array([[9, 1, 1, 0], [1, 9, 2, 2], [0, 3, 9, 3], [5, 4, 3, -9.]], np.float32)
    v, idx = graph.knn_from_similarity(m, 2)
    assert idx.dtype == np.int64 and idx.tolist() == [[1, 2], [2, 3], [1, 3], [0, 1]]       # ties: the lower index first
    assert v.tolist() == [[1, 1], [2, 2], [3, 3], [5, 4]] and v.dtype == np.float32
    flat = np.ones((4, 4))
    assert graph.knn_from_similarity(flat, 3)[1].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]      # self: by index
    rng = np.random.RandomState(0)
    a = rng.randn(40, 40)
    a = a + a.T
    v, idx = graph.knn_from_similarity(a, 5)
    b = a.copy()
    np.fill_diagonal(b, -np.inf)
    assert np.array_equal(idx, np.argsort(-b, axis=1)[:, :5])
    assert np.array_equal(v, np.take_along_axis(a, idx, axis=1)) and (np.diff(v, axis=1) <= 0).all()
    for bad in [dict(matrix=np.ones((3, 4)), k=1), dict(matrix=np.ones(3), k=1), dict(matrix=flat, k=4), dict(matrix=flat, k=0),
                dict(matrix=flat, k=1.5), dict(matrix=np.full((3, 3), np.nan), k=1)]:
        with pytest.raises(ValueError, match='knn_from_similarity'):
            graph.knn_from_similarity(**bad)


def test_refusals_come_before_the_device():
    x = latent(20, 6, seed=0)
    limit = _lib.lib().chebgcn_connectome_query(0)
    nan = x.copy()
    nan[3, 2] = np.nan
    for call in (cn.connectome, cn.connectome_host):
        for kw, match in [(dict(kind='tangent'), 'unknown kind'), (dict(kind=None), 'unknown kind'),
                          (dict(shrinkage=1.5), 'outside'), (dict(shrinkage=-0.1), 'outside'), (dict(shrinkage=float('nan')), 'outside'),
                          (dict(shrinkage='lw'), 'shrinkage'), (dict(shrinkage=None), 'shrinkage'), (dict(shrinkage=True), 'shrinkage')]:
            with pytest.raises(ValueError, match=match):
                call(x, **kw)
        for runs, match in [(x[:1], 'two time points'), ([x, x[:, :5]], 'differ'), (nan, 'non-finite'), ([], 'no runs'),
                            (np.zeros(5, np.float32), r'\[T, M\]')]:
            with pytest.raises(ValueError, match=match):
                call(runs)
    with pytest.raises(ValueError, match='at most %d' % limit):
        cn.connectome(np.zeros((4, limit + 1), np.float32))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='batch_runs'):
            cn.connectome(x, batch_runs=bad)
    for kw, match in [(dict(kind='tangent'), 'kind must be'), (dict(kind='precision'), 'kind must be'),
                      (dict(kind='partial correlation', shrinkage=2), 'outside'),
                      (dict(kind='partial correlation', shrinkage='x'), 'shrinkage'),
                      (dict(kind='partial correlation', k=6), 'need more than'), (dict(kind='partial correlation', k=0), 'k = 0')]:
        with pytest.raises(ValueError, match=match):
            graph.connectivity_graph(x, **kw)
    for runs, match in [(x[:1], 'two time points'), ([x, x[:, :5]], 'differ'), (nan, 'non-finite'),
                        (np.zeros((4, limit + 1), np.float32), 'at most')]:
        with pytest.raises(ValueError, match=match):
            graph.connectivity_graph(runs, k=2, kind='partial correlation')


def test_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_connectome_query(i) for i in range(8)]
    assert all(v > 0 for v in q) and L.chebgcn_connectome_query(8) == -1 and L.chebgcn_connectome_query(-1) == -1
    RMAX, SMAX, TILE, ROWS, PANEL, STAGE, THREADS, CLASSES = q
    assert RMAX >= 512 and THREADS >= RMAX and TILE % 4 == 0 and STAGE % PANEL == 0 and 64 % PANEL == 0
    assert (TILE, ROWS, PANEL, STAGE, CLASSES) == (64, 16, 16, 64, 8)      # the edges the ids of tests/test_gpu_connectome.py name
    assert _lib.CONNECTOME_KINDS == cn.KINDS
    assert L.chebgcn_connectome_workspace(3, 33) == 3 * (64 * 64 + 4 * 64) * 8
    for bad in [(0, 33), (3, 0), (-1, 33), (3, RMAX + 1), (SMAX + 1, 33)]:
        assert L.chebgcn_connectome_workspace(*bad) == 0
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)
    odd4, odd8 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 8)
    EINVAL, EUNSUP = -1, -4
    big = 1 << 40

    def cov(series=p, Ttot=4, offs=p, S=1, R=1, ws=p, nbytes=big):
        return L.chebgcn_connectome_cov(series, Ttot, offs, S, R, ws, nbytes, None)

    for kw in [dict(series=None), dict(offs=None), dict(ws=None), dict(Ttot=0), dict(S=0), dict(S=-3), dict(R=0), dict(nbytes=8),
               dict(series=odd8), dict(series=odd4), dict(ws=odd8), dict(offs=odd4)]:
        assert cov(**kw) == EINVAL, kw
        assert b'connectome_cov' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=SMAX + 1), dict(Ttot=1 << 40)]:
        assert cov(**kw) == EUNSUP, kw

    def finish(ws=p, nbytes=big, offs=p, Ttot=4, S=1, R=1, kind=0, shrinkage=-1.0, out=p, so=p, dg=p):
        return L.chebgcn_connectome_finish(ws, nbytes, offs, Ttot, S, R, kind, shrinkage, out, so, dg, None)

    for kw in [dict(ws=None), dict(offs=None), dict(out=None), dict(so=None), dict(dg=None), dict(Ttot=0), dict(S=0), dict(R=0),
               dict(kind=-1), dict(kind=4), dict(shrinkage=1.5), dict(shrinkage=float('nan')), dict(nbytes=8), dict(ws=odd8),
               dict(so=odd4), dict(offs=odd4)]:
        assert finish(**kw) == EINVAL, kw
        assert b'connectome_finish' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=SMAX + 1)]:
        assert finish(**kw) == EUNSUP, kw

    def mean(m=p, dg=p, S=1, R=1, out=p):
        return L.chebgcn_connectome_mean(m, dg, S, R, out, None)

    for kw in [dict(m=None), dict(dg=None), dict(out=None), dict(S=0), dict(R=0), dict(R=-1)]:
        assert mean(**kw) == EINVAL, kw
        assert b'connectome_mean' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=(1 << 24) + 1)]:
        assert mean(**kw) == EUNSUP, kw
