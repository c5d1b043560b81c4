"""The host side of ``searchlight(classifier='svc')``: the float64 restatement against scikit-learn's ``LinearSVC(dual=True,
fit_intercept=True, intercept_scaling=1, multi_class='ovr')`` on the training-mean-centred row, what the SVM sees and naive Bayes
does not, the properties of the stated model, every new refusal, and the C ABI's argument checks.  No GPU.

Measured here: class differences of the host's decision values (``tol = 1e-8``, ``max_iter = 100000``; every problem converges,
asserted) against scikit-learn's (``tol = 1e-10``) differ by at most 2.0e-8 of the largest decision value of the case, over
rows of 5, 40, 129 and 300 vertices, 2, 3 and 8 classes, ``C`` = 0.01 and 1 and both losses.  ``BOUND`` is 10 x that: the margin
covers liblinear's own stopping rule and its shuffled coordinate order."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from gcn_fmri_decoding_amd import _lib, searchlight as sl

BOUND = 2e-7
LENGTHS = [5, 40, 129, 300]


def rows_of(M, lengths, step=7):
    """Row i: ``lengths[i]`` consecutive vertices from ``step * i``."""
    r = sp.lil_matrix((len(lengths), M))
    for i, P in enumerate(lengths):
        assert step * i + P <= M
        r[i, step * i:step * i + P] = 1
    return r.tocsr()


def data(rng, y, M, shift=1.0):
    """Unit noise, class means ``shift`` apart per vertex."""
    C = int(np.max(y)) + 1
    return (rng.randn(len(y), M) + shift * rng.randn(C, M)[y]).astype(np.float32)


def one_class(K, t, D, Ub, sweeps):
    """``sweeps`` sweeps of the dual coordinate descent of one class, scalar by scalar as the docstring states it."""
    n = len(t)
    alpha, g = [0.0] * n, [-1.0] * n
    for _ in range(sweeps):
        for i in range(n):
            G = g[i]
            PG = min(G, 0.0) if alpha[i] == 0.0 else max(G, 0.0) if alpha[i] == Ub else G
            if PG != 0.0:
                a = min(max(alpha[i] - G / ((K[i, i] + 1.0) + D), 0.0), Ub)
                delta = a - alpha[i]
                alpha[i] = a
                for j in range(n):
                    g[j] = g[j] + (t[i] * t[j]) * (delta * (K[j, i] + 1.0))
                g[i] = g[i] + delta * D
    return np.array(alpha)


# ---- 1. against scikit-learn ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C,S,F', [(2, 48, 3), (3, 48, 4), (8, 64, 2)])
def test_host_svc_against_sklearn(C, S, F):
    pytest.importorskip('sklearn')
    from sklearn.svm import LinearSVC
    rng = np.random.RandomState(C)
    M = 330
    y = np.arange(S) % C
    fold = np.arange(S) // C % F
    X = data(rng, y, M)
    X64 = X.astype(np.float64)
    nb = rows_of(M, LENGTHS)
    worst = 0.0
    for loss in sl.SVC_LOSSES:
        for Creg in (0.01, 1.0):
            res, info = sl.searchlight_host(X, y, nb, fold, classifier='svc', C=Creg, loss=loss, tol=1e-8, max_iter=100000, scores=True,
                                            predictions=True, return_solver=True)
            assert (info.residual <= 1e-8).all() and info.sweeps.max() < 100000           # no case is silently left out
            for u, P in enumerate(LENGTHS):
                cols = np.arange(7 * u, 7 * u + P)
                for f in range(F):
                    tr, te = fold != f, fold == f
                    A = X64[tr][:, cols]
                    m = A.mean(axis=0)
                    clf = LinearSVC(loss=loss, C=Creg, dual=True, fit_intercept=True, intercept_scaling=1, multi_class='ovr', tol=1e-10,
                                    max_iter=2000000).fit(A - m, y[tr])
                    want = clf.decision_function(X64[te][:, cols] - m)
                    if C == 2:
                        want = np.stack([-want, want], axis=1)
                    got = res.scores[te, :, u]
                    top = np.abs(want).max()
                    worst = max(worst, float(np.abs((got[:, 1:] - got[:, :1]) - (want[:, 1:] - want[:, :1])).max() / top))
                    two = np.sort(want, axis=1)
                    decided = two[:, -1] - two[:, -2] > 2.0 * BOUND * top
                    assert np.array_equal(res.predictions[te, u][decided], np.argmax(want, axis=1)[decided])
    print('class differences against scikit-learn: %.3g of the largest decision value (bound %.3g)' % (worst, BOUND))
    assert worst <= BOUND, worst


# ---- 2. what the SVM is for -----------------------------------------------------------------------------------------------------

def test_signal_in_differences_of_vertices_that_share_noise():
    """One row of 300 vertices; all of them carry ONE common noise of sd 20, each an own noise of sd 0.5, and the class adds 1 to
    the even ones: (sum of the even) - (sum of the odd) has d' = 17, a single vertex 0.05, and naive Bayes's sum over the even
    vertices still 0.05.  Measured on the host: 'svc' recall 1.0 in both classes (fixed here at 0.95; its 100 sweeps do not
    reach ``tol`` on this ill-conditioned row, which ``SolverInfo`` says), 'gnb' accuracy 0.5; 'lda' refuses the row."""
    rng = np.random.RandomState(5)
    S, M = 120, 300
    y = np.arange(S) % 2
    fold = np.arange(S) // 2 % 4
    X = 100.0 + 20.0 * rng.randn(S, 1) + 0.5 * rng.randn(S, M)
    X[:, 0::2] += 1.0 * y[:, None]
    X = X.astype(np.float32)
    nb = sp.csr_matrix(np.ones((1, M)))
    svc, info = sl.searchlight_host(X, y, nb, fold, classifier='svc', max_iter=100, return_solver=True)
    gnb = sl.searchlight_host(X, y, nb, fold)
    print('svc recall', svc.recall.ravel(), 'gnb accuracy', gnb.accuracy.ravel(), 'sweeps', info.sweeps.ravel(), 'residual', info.residual.ravel())
    assert svc.recall.min() >= 0.95, svc.recall
    assert abs(float(gnb.accuracy[0, 0]) - 0.5) <= 0.1, gnb.accuracy
    assert info.sweeps.shape == (4, 1) and (info.sweeps == 100).all() and (info.residual > 1e-3).all()
    with pytest.raises(ValueError, match=r"holds 300 vertices.*classifier='gnb'.*classifier='svc'"):
        sl.searchlight_host(X, y, nb, fold, classifier='lda')


# ---- 3. properties of the stated model ------------------------------------------------------------------------------------------

def gram(X64, tr, te, cols):
    A = X64[tr][:, cols]
    m = A.sum(axis=0) / len(A)
    return (A - m) @ (A - m).T, (X64[te][:, cols] - m) @ (A - m).T


@pytest.mark.parametrize('loss', sl.SVC_LOSSES)
def test_one_sweep_equals_one_hand_written_sweep(loss):
    rng = np.random.RandomState(20)
    S, M, C = 18, 6, 3
    y = np.arange(S) % C
    fold = np.arange(S) // C % 3
    X = data(rng, y, M)
    X64 = X.astype(np.float64)
    Creg = 0.7
    D, Ub = (1.0 / (2.0 * Creg), np.inf) if loss == 'squared_hinge' else (0.0, Creg)
    for sweeps in (1, 2):
        res, info = sl.searchlight_host(X, y, sp.csr_matrix(np.ones((1, M))), fold, classifier='svc', C=Creg, loss=loss, tol=0.0,
                                        max_iter=sweeps, scores=True, return_solver=True)
        assert (info.sweeps == sweeps).all()
        for f in range(3):
            tr, te = fold != f, fold == f
            K, Kt = gram(X64, tr, te, np.arange(M))
            for c in range(C):
                t = np.where(y[tr] == c, 1.0, -1.0)
                want = (Kt + 1.0) @ (one_class(K, t, D, Ub, sweeps) * t)
                assert np.allclose(res.scores[te, c, 0], want, rtol=1e-11, atol=1e-12)      # (the Gram matrix here is BLAS's)


def test_two_classes_are_mirror_images_exactly():
    rng = np.random.RandomState(21)
    y = np.arange(40) % 2
    fold = np.arange(40) // 2 % 4
    X = data(rng, y, 30, 0.5)
    for loss in sl.SVC_LOSSES:
        res = sl.searchlight_host(X, y, rows_of(30, [3, 30], step=0), fold, classifier='svc', loss=loss, scores=True, predictions=True)
        assert np.array_equal(res.scores[:, 1], -res.scores[:, 0]) and np.abs(res.scores).min() > 0
        assert np.array_equal(res.predictions, (res.scores[:, 1] > res.scores[:, 0]).astype(np.uint8))


def test_all_zero_rows_and_duplicated_training_samples():
    rng = np.random.RandomState(22)
    S, M = 36, 12
    y = np.arange(S) % 3
    fold = np.arange(S) // 3 % 3
    X = data(rng, y, M)
    X[:, 6:] = 0.0
    nb = sp.csr_matrix(np.array([[0] * 6 + [1] * 6, [0] * 4 + [1] * 8]))
    res, info = sl.searchlight_host(X, y, nb, fold, classifier='svc', scores=True, predictions=True, return_solver=True)
    assert np.isfinite(res.scores).all() and np.isfinite(info.residual).all()
    assert np.array_equal(res.predictions, np.argmax(res.scores, axis=1).astype(np.uint8))           # the first maximal class
    for f in range(3):                                          # K = 0: the bias alone, the same for every test sample
        assert (res.scores[fold == f][:, :, 0] == res.scores[fold == f][:1, :, 0]).all()
    assert not np.array_equal(res.scores[:, :, 1], res.scores[:, :, 0])
    twice = np.concatenate([X, X])                              # every training sample twice: a singular Gram matrix
    dup, dinfo = sl.searchlight_host(twice, np.concatenate([y, y]), rows_of(M, [6], step=0), np.concatenate([fold, fold]), classifier='svc',
                                     scores=True, return_solver=True)
    assert np.isfinite(dup.scores).all() and (dinfo.residual <= 1e-3).all()
    assert np.array_equal(dup.scores[:S], dup.scores[S:])


def test_hinge_with_a_tiny_C_leaves_alpha_at_the_bound():
    rng = np.random.RandomState(23)
    S, M, Creg = 30, 8, 1e-3
    y = np.arange(S) % 3
    fold = np.arange(S) // 3 % 2
    X = data(rng, y, M)
    X64 = X.astype(np.float64)
    res, info = sl.searchlight_host(X, y, sp.csr_matrix(np.ones((1, M))), fold, classifier='svc', C=Creg, loss='hinge', scores=True,
                                    return_solver=True)
    assert (info.sweeps == 2).all() and (info.residual == 0).all()              # the second sweep finds every PG = max(G, 0) = 0
    for f in range(2):
        tr, te = fold != f, fold == f
        _, Kt = gram(X64, tr, te, np.arange(M))
        for c in range(3):
            want = (Kt + 1.0) @ (Creg * np.where(y[tr] == c, 1.0, -1.0))        # alpha = C everywhere
            assert np.allclose(res.scores[te, c, 0], want, rtol=1e-11, atol=1e-15)


def test_a_case_that_does_not_converge_says_so():
    rng = np.random.RandomState(24)
    y = np.arange(64) % 2
    fold = np.arange(64) // 2 % 2
    X = data(rng, y, 5, 0.2)                                    # 32 training samples for 5 vertices, C = 10: thousands of sweeps
    _, info = sl.searchlight_host(X, y, sp.csr_matrix(np.ones((1, 5))), fold, classifier='svc', C=10.0, max_iter=3, return_solver=True)
    assert info.sweeps.dtype == np.int32 and info.residual.dtype == np.float64 and info.models == [(0, 0), (0, 1)]
    assert (info.sweeps == 3).all() and (info.residual > 1e-3).all()
    res = sl.searchlight_host(X, y, sp.csr_matrix(np.ones((1, 5))), fold, classifier='svc', C=10.0, max_iter=3)
    assert isinstance(res, sl.SearchlightResult) and res._fields == ('correct', 'support', 'recall', 'accuracy', 'groups', 'classes',
                                                                     'scores', 'predictions')


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------

BAD = [(dict(C=0.0), 'C must'), (dict(C=-1.0), 'C must'), (dict(C=np.inf), 'C must'), (dict(C=np.nan), 'C must'), (dict(C='1'), 'C must'),
       (dict(C=True), 'C must'), (dict(C=None), 'C must'), (dict(loss='l2'), 'loss'), (dict(loss=None), 'loss'), (dict(loss=0), 'loss'),
       (dict(tol=-1e-9), 'tol'), (dict(tol=np.inf), 'tol'), (dict(tol=np.nan), 'tol'), (dict(tol=None), 'tol'),
       (dict(max_iter=0), 'max_iter'), (dict(max_iter=100001), 'max_iter'), (dict(max_iter=10.0), 'max_iter'), (dict(max_iter=True), 'max_iter'),
       (dict(priors='uniform'), "priors.*classifier='svc'"), (dict(variance='pooled'), "variance.*classifier='svc'"),
       (dict(var_smoothing=1e-3), "var_smoothing.*classifier='svc'"), (dict(shrinkage=0.5), "shrinkage.*classifier='svc'"),
       (dict(shrinkage='auto'), "shrinkage.*classifier='svc'"), (dict(return_solver=1), 'return_solver')]


def test_every_new_refusal_before_the_device():
    rng = np.random.RandomState(30)
    S, M = 24, 10
    y = np.arange(S) % 2
    fold = np.arange(S) // 2 % 2
    X = data(rng, y, M)
    nb = rows_of(M, [3, 10], step=0)
    big = 133                                                   # folds of 129 and 4: the model tested on fold 1 trains on 129
    for fn in (sl.searchlight_host, sl.searchlight):
        for kw, what in BAD:
            with pytest.raises(ValueError, match=what):
                fn(X, y, nb, fold, classifier='svc', **kw)
        for clf in ('svm', 'qda', None):
            with pytest.raises(ValueError, match="classifier must be 'gnb', 'lda' or 'svc'"):
                fn(X, y, nb, fold, classifier=clf)
        for kw in (dict(C=2.0), dict(loss='hinge'), dict(tol=0.0), dict(max_iter=5), dict(return_solver=True)):
            for clf in ('gnb', 'lda'):
                with pytest.raises(ValueError, match="classifier='svc'"):
                    fn(X, y, nb, fold, classifier=clf, **kw)
        Xb, yb, fb = np.zeros((big, M), np.float32), np.arange(big) % 2, (np.arange(big) >= 129).astype(int) + 3
        with pytest.raises(ValueError, match=r"group 's7', fold 4 holds 129 samples.*up to 128.*within=False"):
            fn(Xb, yb, nb, fb, groups=['s7'] * big, classifier='svc')
        with pytest.raises(ValueError, match=r'the training set of fold 4 holds 129 samples'):
            fn(Xb, yb, nb, fb, within=False, classifier='svc')
    sl.searchlight_host(X, y, nb, fold, classifier='svc', tol=0, max_iter=1, C=1)           # ints are numbers
    names = ['rest'] * 3 + ['a'] * 7 + ['b'] * 7 + ['rest'] * 3
    run = np.zeros((len(names), M), np.float32)
    for kw, what in BAD:
        with pytest.raises(ValueError, match=what):
            sl.searchlight_events([run, run], [names, names], ['a', 'b'], 3, nb, classifier='svc', **kw)
    for kw, what in [(dict(classifier='svm'), 'classifier must'), (dict(C=2.0), "classifier='svc'"), (dict(return_solver=True), "classifier='svc'"),
                     (dict(classifier='svc', gamma=1.0), 'unknown keyword')]:
        with pytest.raises(ValueError, match=what):
            sl.searchlight_events([run, run], [names, names], ['a', 'b'], 3, nb, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                         # (trials of one row: match_events warns)
        with pytest.raises(ValueError, match=r"group 's', fold 1 holds 129 samples"):
            sl.searchlight_events([np.zeros((130, M), np.float32), np.zeros((4, M), np.float32)], [['a', 'b'] * 65, ['a', 'b'] * 2],
                                  ['a', 'b'], 1, nb, groups=['s', 's'], classifier='svc')


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------

def test_entry_point_checks_its_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_searchlight_svm_query(i) for i in range(10)]
    assert all(v > 0 for v in q) and L.chebgcn_searchlight_svm_query(10) == -1 and L.chebgcn_searchlight_svm_query(-1) == -1
    THREADS, NMAXS, TILE, CMAX, CHUNK, MODELS, TILES, GMAX, ITMAX, SUPER = q
    assert (NMAXS, CMAX, MODELS, GMAX, ITMAX) == (sl.SVC_NMAX, sl.CMAX, sl.NMAX, sl.GMAX, sl.SVC_ITMAX)
    assert THREADS == 256 and SUPER % TILE == 0 and CHUNK == 32 and TILE == 16
    buckets = [L.chebgcn_searchlight_svm_query(100 + n) for n in range(1, NMAXS + 1)]
    assert sorted(set(buckets)) == [32, 64, 128] and all(b >= n for n, b in zip(range(1, NMAXS + 1), buckets)) and buckets == sorted(buckets)
    assert [buckets[n - 1] for n in (1, 32, 33, 64, 65, 128)] == [32, 32, 64, 64, 128, 128]
    assert L.chebgcn_searchlight_svm_query(100) == -1 and L.chebgcn_searchlight_svm_query(101 + NMAXS) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    EINVAL, EUNSUP = -1, -4

    def svm(Xt=p, S=4, M=1, rowptr=p, colidx=p, nnz=1, U=2, centres=p, Ub=2, models=p, NMb=1, bucket=32, lptr=p, lidx=p, nidx=1, tptr=p,
            tmax=1, NM=1, C=2, Creg=1.0, loss=0, tol=1e-3, it=10, sg=p, sy=p, so=p, G=1, correct=p, scores=None, pred=None, sweeps=None,
            resid=None):
        return L.chebgcn_searchlight_svm(Xt, S, M, rowptr, colidx, nnz, U, centres, Ub, models, NMb, bucket, lptr, lidx, nidx, tptr, tmax, NM,
                                         C, Creg, loss, tol, it, sg, sy, so, G, correct, scores, pred, sweeps, resid, None)

    for kw in [dict(Xt=None), dict(rowptr=None), dict(colidx=None), dict(centres=None), dict(models=None), dict(lptr=None), dict(lidx=None),
               dict(tptr=None), dict(sg=None), dict(sy=None), dict(so=None), dict(correct=None), dict(S=0), dict(M=0),
               dict(S=2 ** 31 - 1, tmax=1), dict(nnz=0), dict(U=0), dict(Ub=0), dict(Ub=-1), dict(NMb=0), dict(bucket=0), dict(bucket=-32),
               dict(nidx=0), dict(tmax=0), dict(tmax=5), dict(NM=0), dict(C=1), dict(C=0), dict(G=0), dict(Creg=0.0), dict(Creg=-1.0),
               dict(Creg=float('nan')), dict(Creg=float('inf')), dict(tol=-1e-9), dict(tol=float('nan')), dict(tol=float('inf')),
               dict(loss=2), dict(loss=-1), dict(it=0), dict(it=ITMAX + 1), dict(Xt=odd2), dict(centres=odd2), dict(models=odd2),
               dict(lidx=odd2), dict(correct=odd2), dict(sweeps=odd2), dict(scores=odd4), dict(resid=odd4)]:
        assert svm(**kw) == EINVAL, kw
        assert b'searchlight_svm' in L.chebgcn_last_error()
    for kw in [dict(NM=MODELS + 1), dict(NMb=MODELS + 1), dict(C=CMAX + 1), dict(G=GMAX + 1), dict(S=TILES * 64 + 64, tmax=TILES * 64 + 1),
               dict(bucket=16), dict(bucket=33), dict(bucket=256)]:
        assert svm(**kw) == EUNSUP, kw
        assert b'searchlight_svm' in L.chebgcn_last_error()
