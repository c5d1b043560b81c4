"""The host side of ``searchlight(classifier='lda')``: the float64 restatement against scikit-learn's
``LinearDiscriminantAnalysis(solver='lsqr', shrinkage=g)``, the Ledoit-Wolf helper against ``sklearn.covariance.ledoit_wolf``,
what LDA sees and naive Bayes does not, the degenerate rule, every new refusal, and the C ABI's argument checks.  No GPU.

Measured here (``record_measured`` keeps the figures): class differences of the scores against scikit-learn's at most 1.3e-10 of
the plain scale ``|log prior| + |d . w| / 2 + sum |w| |x - m|`` (at mean 1e4 / sd 50, where scikit-learn's uncentred form
carries the loss; 3.5e-11 at mean 100, 3.5e-14 at mean 0), against a tolerance of 1e-8."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, lda_shrinkage_host, searchlight as sl


def data(rng, S, M, C, mean=100.0, sd=1.0, folds=4):
    """Balanced classes whose means differ by 0.5 sd per vertex; every (fold, class) cell holds S / (folds C) samples."""
    y = np.arange(S) % C
    fold = np.arange(S) // C % folds
    X = (mean + sd * rng.randn(S, M) + 0.5 * sd * rng.randn(C, M)[y]).astype(np.float32)
    return X, y, fold


def rows_of(M, lengths, step=7):
    """Row i: ``lengths[i]`` consecutive vertices from ``step * i``."""
    r = sp.lil_matrix((len(lengths), M))
    for i, P in enumerate(lengths):
        assert step * i + P <= M
        r[i, step * i:step * i + P] = 1
    return r.tocsr()


def kappa_of(A, ytr, C, g):
    """The condition number of Sigma of one (training set, ball), restated."""
    mu = np.stack([A[ytr == c].mean(axis=0) for c in range(C)])
    R = A - mu[ytr]
    S = R.T @ R / len(A)
    ev = np.linalg.eigvalsh((1.0 - g) * S + g * np.trace(S) / A.shape[1] * np.eye(A.shape[1]))
    return ev[-1] / ev[0]


# ---- 1. against scikit-learn ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mean,sd', [(100.0, 1.0), (1e4, 50.0), (0.0, 1.0)])
def test_host_lda_against_sklearn(mean, sd):
    pytest.importorskip('sklearn')
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    rng = np.random.RandomState(int(mean) + 1)
    S, M, C, F = 96, 200, 3, 4
    X, y, fold = data(rng, S, M, C, mean, sd, F)
    lengths = [5, 31, 81, 127]
    nb = rows_of(M, lengths)
    X64 = X.astype(np.float64)
    worst = 0.0
    for g in (0.01, 0.1, 1):
        res, scale = sl.searchlight_host(X, y, nb, fold, classifier='lda', shrinkage=g, scores=True, predictions=True, return_scale=True)
        assert res.scores.shape == scale.shape == (S, C, 4) and np.isfinite(res.scores).all() and (scale > 0).all()
        for u, P in enumerate(lengths):
            cols = np.arange(7 * u, 7 * u + P)
            for f in range(F):
                tr, te = fold != f, fold == f
                clf = LinearDiscriminantAnalysis(solver='lsqr', shrinkage=g).fit(X64[tr][:, cols], y[tr])
                want = clf.decision_function(X64[te][:, cols])
                got = res.scores[te, :, u]
                plain = scale[te, :, u] / kappa_of(X64[tr][:, cols], y[tr], C, g)
                err = np.abs((got[:, 1:] - got[:, :1]) - (want[:, 1:] - want[:, :1])) / np.maximum(plain[:, 1:], plain[:, :1])
                worst = max(worst, float(err.max()))
                assert np.array_equal(res.predictions[te, u], clf.predict(X64[te][:, cols]))
    record_measured('searchlight_lda_host_sklearn_mean%g' % mean, rel=worst)
    print('class differences against scikit-learn: %.3g of the plain scale' % worst)
    assert worst <= 1e-8, worst


def test_shrinkage_helper_against_sklearn():
    pytest.importorskip('sklearn')
    from sklearn.covariance import ledoit_wolf
    rng = np.random.RandomState(3)
    worst = 0.0
    for n, P, mix in [(72, 5, 0.5), (72, 31, 1.0), (72, 127, 2.0), (500, 20, 3.0), (10, 64, 0.2)]:
        R = rng.randn(n, P) + mix * rng.randn(n, 1) * rng.randn(1, P)          # one strong common factor
        g, want = lda_shrinkage_host(R), float(ledoit_wolf(R, assume_centered=True)[1])
        assert sl.SHRINK_MIN < want < 1.0, want                 # (the clip is not what is compared)
        worst = max(worst, abs(g - want) / want)
    record_measured('searchlight_lda_shrinkage_helper', rel=worst)
    assert worst <= 1e-12, worst
    assert lda_shrinkage_host(np.zeros((6, 3))) == sl.SHRINK_MIN               # beta == 0: g = 0, clipped to the floor
    assert lda_shrinkage_host(rng.randn(1, 4)) == sl.SHRINK_MIN                # one sample: beta_ / n == delta_
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((3, 0))):
        with pytest.raises(ValueError, match='lda_shrinkage_host'):
            lda_shrinkage_host(bad)


# ---- 2. what LDA is for ---------------------------------------------------------------------------------------------------------

def test_signal_in_a_difference_of_correlated_vertices():
    """Both vertices of a ball carry one large common noise (sd 20); the class moves only their difference (by 4, at an
    independent noise of sd 0.5 per vertex: d' = 5.7 for a classifier that sees the difference; a single vertex has d' = 0.2).
    Measured: LDA at least 0.979, naive Bayes within 0.06 of chance.  The shrinkage is estimated: at 180 training samples for 2 vertices it is small, and a fixed 0.1 would drown the
    small eigenvalue (0.25) in 0.1 nu = 40."""
    rng = np.random.RandomState(5)
    S, M = 240, 8
    y = np.arange(S) % 2
    fold = np.arange(S) // 2 % 4
    common = 20.0 * rng.randn(S, M // 2)
    X = 100.0 + np.repeat(common, 2, axis=1) + 0.5 * rng.randn(S, M)
    X[:, 0::2] += 4.0 * y[:, None]
    nb = sp.csr_matrix(np.kron(np.eye(M // 2), np.ones((1, 2))))
    lda = sl.searchlight_host(X.astype(np.float32), y, nb, fold, classifier='lda', shrinkage='auto')
    gnb = sl.searchlight_host(X.astype(np.float32), y, nb, fold)
    record_measured('searchlight_lda_difference_signal', lda=float(lda.accuracy.min()), gnb=float(np.abs(gnb.accuracy - 0.5).max()))
    assert lda.accuracy.min() >= 0.9, lda.accuracy
    assert np.abs(gnb.accuracy - 0.5).max() <= 0.15, gnb.accuracy


# ---- 3. the degenerate rule -----------------------------------------------------------------------------------------------------

def test_full_shrinkage_zero_balls_and_partly_zero_balls():
    rng = np.random.RandomState(6)
    S, M, C = 60, 12, 3
    X, y, fold = data(rng, S, M, C, folds=3)
    y = np.where(np.arange(S) % 7 == 0, 2, y)                   # class 2 is the most frequent one in every training set
    X[:, 6:] = 0.0
    nb = sp.csr_matrix(np.array([[1] * 6 + [0] * 6, [0] * 6 + [1] * 6, [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]]))
    res = sl.searchlight_host(X, y, nb, fold, classifier='lda', shrinkage=1, scores=True, predictions=True)
    X64 = X.astype(np.float64)
    for f in range(3):
        tr, te = fold != f, fold == f
        n = np.bincount(y[tr], minlength=C).astype(np.float64)
        A = X64[tr][:, :6]
        mu = np.stack([A[y[tr] == c].mean(axis=0) for c in range(C)])
        m = (n[:, None] * mu).sum(axis=0) / n.sum()
        nu = ((A - mu[y[tr]]) ** 2).sum() / n.sum() / 6
        w = (mu - m) / nu                                       # g = 1: Sigma = nu I
        want = np.log(n / n.sum()) - 0.5 * ((mu - m) * w).sum(axis=1) + (X64[te][:, :6] - m) @ w.T
        assert np.allclose(res.scores[te, :, 0], want, rtol=1e-12, atol=1e-12)
        assert np.array_equal(res.scores[te, :, 1], np.broadcast_to(np.log(n / n.sum()), (te.sum(), C)))     # exactly log prior
    assert (res.predictions[:, 1] == 2).all() and np.isfinite(res.scores).all()
    for g in (1e-6, 0.1, 'auto'):
        part = sl.searchlight_host(X, y, nb, fold, classifier='lda', shrinkage=g, scores=True)
        assert np.isfinite(part.scores).all()
        assert not np.array_equal(part.scores[:, :, 2], part.scores[:, :, 1])      # the two live vertices of row 2 speak


def test_priors_change_the_intercept_only():
    rng = np.random.RandomState(7)
    X, y, fold = data(rng, 72, 10, 3, folds=3)
    y = np.where(np.arange(72) % 5 == 0, 0, y)
    nb = rows_of(10, [4, 6], step=2)
    emp = sl.searchlight_host(X, y, nb, fold, classifier='lda', scores=True)
    uni = sl.searchlight_host(X, y, nb, fold, classifier='lda', priors='uniform', scores=True)
    shift = uni.scores - emp.scores                             # log(1 / C) - log(n_c / n) per (fold, class): the same at every centre
    assert np.allclose(shift[:, :, 0], shift[:, :, 1], rtol=0, atol=1e-12) and np.abs(shift).max() > 0.1
    for f in range(3):
        assert np.allclose(shift[fold == f], shift[fold == f][:1], rtol=0, atol=1e-12)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------

def test_every_new_refusal_before_the_device():
    rng = np.random.RandomState(8)
    S, M = 24, 130
    X, y, fold = data(rng, S, M, 2, folds=2)
    balls = rows_of(M, [3, 128], step=1)
    long_row = rows_of(M, [3, 129], step=1)
    for fn in (sl.searchlight_host, sl.searchlight):
        for nb, kw, what in [
                (long_row, dict(classifier='lda'), r"neighbourhood 1 holds 129 vertices.*classifier='gnb'"),
                (balls, dict(classifier='lda', shrinkage=0.0), 'shrinkage'), (balls, dict(classifier='lda', shrinkage=1e-7), 'shrinkage'),
                (balls, dict(classifier='lda', shrinkage=1.5), 'shrinkage'), (balls, dict(classifier='lda', shrinkage=-0.1), 'shrinkage'),
                (balls, dict(classifier='lda', shrinkage=np.nan), 'shrinkage'), (balls, dict(classifier='lda', shrinkage='lw'), 'shrinkage'),
                (balls, dict(classifier='lda', shrinkage=None), 'shrinkage'), (balls, dict(classifier='lda', shrinkage=True), 'shrinkage'),
                (balls, dict(classifier='lda', variance='pooled'), 'variance and var_smoothing'),
                (balls, dict(classifier='lda', var_smoothing=1e-3), 'variance and var_smoothing'),
                (balls, dict(classifier='lda', var_smoothing=0.0), 'variance and var_smoothing'),
                (balls, dict(classifier='svm'), 'classifier'), (balls, dict(classifier=None), 'classifier'),
                (balls, dict(shrinkage=0.5), "classifier='gnb'"), (balls, dict(shrinkage='auto'), "classifier='gnb'"),
                (balls, dict(classifier='gnb', shrinkage=1), "classifier='gnb'")]:
            with pytest.raises(ValueError, match=what):
                fn(X, y, nb, fold, **kw)
    sl.searchlight_host(X, y, long_row, fold)                   # naive Bayes takes the long row
    sl.searchlight_host(X, y, balls, fold, classifier='lda', shrinkage='auto')
    sl.searchlight_host(X, y, balls, fold, classifier='gnb', shrinkage=0.1)
    run = np.zeros((20, M), np.float32)
    names = ['rest'] * 3 + ['a'] * 7 + ['b'] * 7 + ['rest'] * 3
    for nb, kw, what in [(long_row, dict(classifier='lda'), 'holds 129 vertices'), (balls, dict(classifier='lda', shrinkage=2), 'shrinkage'),
                         (balls, dict(classifier='lda', shrinkage='none'), 'shrinkage'),
                         (balls, dict(classifier='lda', variance='pooled'), 'variance and var_smoothing'),
                         (balls, dict(classifier='lda', var_smoothing=0.5), 'variance and var_smoothing'),
                         (balls, dict(classifier='qda'), 'classifier'), (balls, dict(shrinkage='auto'), "classifier='gnb'")]:
        with pytest.raises(ValueError, match=what):
            sl.searchlight_events(run, names, ['a', 'b'], 3, nb, **kw)


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------

def test_entry_point_checks_its_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_searchlight_lda_query(i) for i in range(9)]
    assert all(v > 0 for v in q) and L.chebgcn_searchlight_lda_query(9) == -1 and L.chebgcn_searchlight_lda_query(-1) == -1
    THREADS, PMAX, TILE, CMAX, BLOCKS, NMAX, TILES, GMAX, NARROW = q
    assert (PMAX, CMAX, NMAX, GMAX) == (sl.LDA_PMAX, sl.CMAX, sl.NMAX, sl.GMAX) and THREADS % 64 == 0 and NARROW < CMAX
    buckets = [L.chebgcn_searchlight_lda_query(100 + P) for P in range(1, PMAX + 1)]
    assert sorted(set(buckets)) == [32, 64, 128] and all(b >= P for P, b in zip(range(1, PMAX + 1), buckets)) and buckets == sorted(buckets)
    assert [buckets[P - 1] for P in (1, 32, 33, 64, 65, 128)] == [32, 32, 64, 64, 128, 128]
    assert L.chebgcn_searchlight_lda_query(100) == -1 and L.chebgcn_searchlight_lda_query(101 + PMAX) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    EINVAL, EUNSUP = -1, -4

    def lda(Xt=p, S=4, M=1, rowptr=p, colidx=p, nnz=1, U=2, centres=p, Ub=2, bucket=32, cptr=p, cidx=p, nidx=1, tptr=p, tmax=1, NM=1, C=2,
            par=p, lp=p, g=0.1, sg=p, sy=p, so=p, G=1, correct=p, scores=None, pred=None, gamma=None):
        return L.chebgcn_searchlight_lda(Xt, S, M, rowptr, colidx, nnz, U, centres, Ub, bucket, cptr, cidx, nidx, tptr, tmax, NM, C, par, lp,
                                         g, sg, sy, so, G, correct, scores, pred, gamma, None)

    for kw in [dict(Xt=None), dict(rowptr=None), dict(colidx=None), dict(centres=None), dict(cptr=None), dict(cidx=None), dict(tptr=None),
               dict(par=None), dict(lp=None), dict(sg=None), dict(sy=None), dict(so=None), dict(correct=None), dict(S=0), dict(M=0),
               dict(S=2 ** 31 - 1, tmax=1), dict(nnz=0), dict(U=0), dict(Ub=0), dict(Ub=-1), dict(bucket=0), dict(bucket=-32), dict(nidx=0),
               dict(tmax=0), dict(tmax=5), dict(NM=0), dict(C=1), dict(C=0), dict(G=0), dict(g=0.0), dict(g=1e-7), dict(g=1.0000001),
               dict(g=float('nan')), dict(g=float('inf')), dict(Xt=odd2), dict(centres=odd2), dict(cidx=odd2), dict(correct=odd2),
               dict(par=odd4), dict(lp=odd4), dict(scores=odd4), dict(gamma=odd4)]:
        assert lda(**kw) == EINVAL, kw
        assert b'searchlight_lda' in L.chebgcn_last_error()
    for kw in [dict(NM=NMAX + 1), dict(C=CMAX + 1), dict(G=GMAX + 1), dict(S=TILES * 64 + 64, tmax=TILES * 64 + 1), dict(bucket=16),
               dict(bucket=33), dict(bucket=256)]:
        assert lda(**kw) == EUNSUP, kw
        assert b'searchlight_lda' in L.chebgcn_last_error()
