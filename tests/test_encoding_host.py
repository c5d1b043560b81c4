"""encoding on the host: ``ridge_cv_host`` -- the statistics route, with the restated chains of the kernels -- against a yardstick
that uses none of its algebra (encoding_cases.yardstick: fit on the stacked training rows, predict the held-out rows, form the
residuals) and against scikit-learn's ``Ridge``; the selection, ``alpha='shared'``, ``score='r'``, explicit folds, the refit,
``predict``, ``delay_features`` and every refusal.  None of it needs a GPU.

The bound (encoding_cases): ``|got - ref| <= c s`` with ``s = (yy_te + |p| + q) / tss_te``.  Measured between the two routes on
the data below, in float64 before the one rounding: c = 1.5e-15 for R^2 (full rank; 1.4e-15 on the rank-deficient data) and
6.7e-16 for Pearson's r; asserted with a margin of 100: c = 1.5e-13, which at s ~ 1e4 (mean 100, unit variance) is 1.5e-9 in
R^2.  The float32 results are allowed one rounding more.  The yardstick excuses 1 of the 300 vertices from the selection, the
one that is constant in time.
"""
import numpy as np
import pytest

import encoding_cases as ec
from gcn_fmri_decoding_amd import EncodingResult, delay_features, encoding as en, ridge_cv_host


MAPS = ('score', 'alpha_index', 'weights', 'scores')


def host(duplicate=False, **kw):
    runs, feats = ec.data(duplicate)
    kw.setdefault('groups', ec.GROUPS)
    kw.setdefault('scores', True)
    return ridge_cv_host(list(runs), list(feats), ec.case_alphas(duplicate), **kw)


@pytest.mark.parametrize('duplicate', [False, True])
@pytest.mark.parametrize('kind', ['r2', 'r'])
def test_chains_agree_with_the_explicit_route_in_float64(duplicate, kind):
    """The float64 value of every (fold, penalty, vertex) before any rounding, against the bound itself."""
    runs, feats = ec.data(duplicate)
    alphas = ec.case_alphas(duplicate)
    worst = 0.0
    for mem, ref in zip(ec.members(), ec.reference(duplicate)):
        Xc = [feats[r] - feats[r].sum(axis=0) / feats[r].shape[0] for r in mem]
        Y = [np.asarray(runs[r], np.float64) for r in mem]
        c = np.stack([x.T @ y for x, y in zip(Xc, Y)])
        tss = np.stack([en.tss_of((y * y).sum(axis=0), y.sum(axis=0), float(y.shape[0])) for y in Y])
        models = en.subject_models(len(mem), [[i] for i in range(len(mem))])
        V, H, d = en.model_tables(Xc, models, alphas)
        assert np.array_equal(H, H.transpose(0, 2, 1))
        for e, (train, test) in enumerate(models[:-1]):
            z, g = en.model_chains(c, train, test, V[e])
            got = en.score_chains(z, g, en._list_sum(tss, test), H[e], d[e], kind)
            live = np.isfinite(ref['scale'][e])
            assert np.isfinite(got).all() and (got[~live] == 0).all()
            ratio = (np.abs(got - ref[kind][e])[live] / ref['scale'][e][live]).max()
            worst = max(worst, ratio)
    print('%s, duplicate = %s: c = %.3e (asserted: %.3e)' % (kind, duplicate, worst, ec.C_BOUND))
    assert worst <= ec.C_BOUND


@pytest.mark.parametrize('duplicate', [False, True])
@pytest.mark.parametrize('kind', ['r2', 'r'])
def test_ridge_cv_host_against_the_yardstick(duplicate, kind):
    res = host(duplicate, score=kind)
    assert isinstance(res, EncodingResult)
    assert res.score.dtype == np.float32 and res.score.shape == (2, ec.M)
    assert res.alpha_index.dtype == np.int32 and res.alpha_index.shape == (2, ec.M)
    assert res.weights.dtype == np.float32 and res.weights.shape == (2, ec.F, ec.M)
    assert res.scores.dtype == np.float32 and res.scores.shape == (2, len(ec.case_alphas(duplicate)), ec.M)
    assert res.groups == ['a', 'b'] and res.folds == [[[0], [1], [2]], [[0], [1], [2], [3]]]
    assert np.array_equal(res.alphas, ec.case_alphas(duplicate))
    ec.check_result(res, duplicate, kind)
    half = res.score[:, ::2].mean(), res.score[:, 1::2].mean()
    assert half[0] > 0.5 > 0.1 > half[1]                       # (the planted half is explained, the other half is not)


@pytest.mark.parametrize('duplicate', [False, True])
def test_yardstick_agrees_with_scikit_learn(duplicate):
    """Where alpha > 0: ``Ridge(alpha, fit_intercept=False)`` on the same centred rows in place of ``numpy.linalg.solve``."""
    lm = pytest.importorskip('sklearn.linear_model')
    runs, feats = ec.data(duplicate)
    alphas = ec.ALPHAS[[0, 5, 11]]
    res = ridge_cv_host(list(runs), list(feats), alphas, groups=ec.GROUPS, scores=True)

    def fit(X, Y, alpha):
        return lm.Ridge(alpha=alpha, fit_intercept=False, solver='cholesky').fit(X, Y).coef_.T

    for s, mem in enumerate(ec.members()):
        ref = ec.yardstick(runs, feats, alphas, mem, fit=fit)
        scale = ref['scale'].mean(axis=0)
        live = np.isfinite(scale)
        mean = ref['r2'].mean(axis=0)
        err = np.abs(res.scores[s].astype(np.float64) - mean)[live]
        assert (err <= ec.C_BOUND * scale[live] + 2.0 ** -23 * np.abs(mean[live])).all()
        for a, alpha in enumerate(alphas):
            cols = res.alpha_index[s] == a
            err = np.abs(res.weights[s].astype(np.float64) - ref['weights'][a])
            assert (err <= ec.weights_bound(feats, mem, alpha, ref['weights'][a]))[:, cols].all()


def test_shared_alpha():
    res = host(alpha='shared')
    ec.check_result(res, False, 'r2', shared=True)
    per = host()
    assert np.array_equal(res.scores, per.scores)               # (the table does not depend on the selection)
    for s in range(2):
        assert len(np.unique(res.alpha_index[s])) == 1
        assert res.score[s].astype(np.float64).mean() <= per.score[s].astype(np.float64).mean()


def test_explicit_folds():
    folds = [[[0, 1], [2]], [[3, 0], [1, 2]]]
    res = host(folds=folds)
    assert res.folds == [[[0, 1], [2]], [[0, 3], [1, 2]]]
    ec.check_result(res, False, 'r2', folds=res.folds)
    loro = host(folds=[[[0], [1], [2]], [[0], [1], [2], [3]]])
    ref = host()
    for name in MAPS:
        assert np.array_equal(getattr(loro, name), getattr(ref, name))


def test_flags_and_subject_order():
    runs, feats = ec.data()
    res = ridge_cv_host(list(runs), list(feats), ec.ALPHAS, groups=ec.GROUPS, weights=False)
    assert res.weights is None and res.scores is None
    full = host()
    assert np.array_equal(res.score, full.score) and np.array_equal(res.alpha_index, full.alpha_index)
    order = [3, 4, 0, 5, 1, 6, 2]                               # (subject 'b' first; the runs of a subject keep their order)
    perm = ridge_cv_host([runs[r] for r in order], [feats[r] for r in order], ec.ALPHAS, groups=[ec.GROUPS[r] for r in order],
                         scores=True)
    assert perm.groups == ['b', 'a']
    for name in MAPS:
        assert np.array_equal(getattr(perm, name)[::-1], getattr(full, name))
    one = ridge_cv_host(list(runs[:3]), list(feats[:3]), ec.ALPHAS, scores=True)      # (groups=None: one subject)
    for name in MAPS:
        assert np.array_equal(getattr(one, name)[0], getattr(full, name)[0])


def test_a_null_feature_changes_no_bit():
    """A feature that is constant in every run is its own eigenvector: appended (the 65th column of F = 64 is the chunk edge of
    the statistics on the device), every other number is the same bits."""
    runs, feats = ec.data()
    wide = [np.concatenate([x, np.full((x.shape[0], 1), 3.0)], axis=1) for x in feats]
    a = host()
    b = ridge_cv_host(list(runs), wide, ec.ALPHAS, groups=ec.GROUPS, scores=True)
    assert np.array_equal(a.score, b.score) and np.array_equal(a.alpha_index, b.alpha_index) and np.array_equal(a.scores, b.scores)
    assert np.array_equal(a.weights, b.weights[:, :-1]) and (b.weights[:, -1] == 0).all()


def test_pseudo_inverse_and_zero_reciprocals():
    runs, feats = ec.data(True)
    mem = ec.members()[0]
    Xc = [feats[r] - feats[r].mean(axis=0) for r in mem]
    V, H, d = en.model_tables(Xc, en.subject_models(3, [[0], [1], [2]]), [0.0, 1.0])
    assert ((d[:, 0] == 0).sum(axis=1) == 1).all() and (d[:, 1] > 0).all()     # one null direction: the duplicated column
    G = sum(x.T @ x for x in Xc)
    assert np.abs((V[-1] * d[-1][0]) @ V[-1].T - np.linalg.pinv(G)).max() <= 1e-12 * np.abs(np.linalg.pinv(G)).max()
    flat = [np.zeros_like(x) for x in Xc]                        # (no feature varies: every weight is 0, every R^2 is 0)
    res = ridge_cv_host([runs[r] for r in mem], flat, [0.0, 1.0], scores=True)
    assert (res.scores == 0).all() and (res.weights == 0).all() and (res.alpha_index == 0).all()


def test_predict():
    runs, feats = ec.data()
    res = host()
    X = feats[4]
    got = res.predict(X, 'b')
    assert got.dtype == np.float32 and got.shape == (X.shape[0], ec.M)
    ref = (X - X.mean(axis=0)) @ res.weights[1].astype(np.float64)
    assert np.abs(got - ref).max() <= 2.0 ** -23 * np.abs(ref).max()
    assert np.array_equal(res.predict(X), res.predict(X, 'a'))
    yc = runs[4].astype(np.float64) - runs[4].astype(np.float64).mean(axis=0)
    planted = np.arange(0, ec.M, 2) != ec.CONSTANT_VERTEX - 1
    r = [np.corrcoef(got[:, m], yc[:, m])[0, 1] for m in np.arange(0, ec.M, 2)[planted][:20]]
    assert min(r) > 0.6
    for bad, kw in ((X[:, :-1], {}), (X, dict(group='c')), (np.where(X > 9, X, np.nan), {})):
        with pytest.raises(ValueError, match='predict'):
            res.predict(bad, **kw)
    with pytest.raises(ValueError, match='no weights'):
        host(weights=False).predict(X)


def test_delay_features():
    X = np.arange(12.0).reshape(4, 3) + 1
    out = delay_features(X, [0, 2, 5])
    assert out.dtype == np.float64 and out.shape == (4, 9)
    assert np.array_equal(out[:, :3], X)
    assert np.array_equal(out[:2, 3:6], np.zeros((2, 3))) and np.array_equal(out[2:, 3:6], X[:2])
    assert (out[:, 6:] == 0).all()
    out[0, 0] = -1
    assert X[0, 0] == 1                                          # (a copy)
    for bad in ([], [1.5], [-1], [True]):
        with pytest.raises(ValueError, match='delay_features'):
            delay_features(X, bad)
    with pytest.raises(ValueError, match='delay_features'):
        delay_features(X[0], [0])


def refusals():
    runs, feats = (list(a) for a in ec.data())
    g = list(ec.GROUPS)
    short = [x[:-1] for x in feats]
    nan = [x.copy() for x in feats]
    nan[2][3, 4] = np.nan
    narrow = feats[:3] + [x[:, :-1] for x in feats[3:]]
    bad_runs = runs[:6] + [runs[6][:, :-1]]
    inf_runs = [r.copy() for r in runs]
    inf_runs[1][0, 0] = np.inf
    return [
        ('no runs', dict(runs=[])),
        ('must be \\[T, M\\]', dict(runs=[r[0] for r in runs])),
        ('differ in the number of vertices', dict(runs=bad_runs)),
        ('at least two time points', dict(runs=[r[:1] for r in runs], features=[x[:1] for x in feats])),
        ('non-finite', dict(runs=inf_runs)),
        ('one \\[T, F\\] matrix per run', dict(features=feats[:-1])),
        ('real \\[T, F\\] matrix', dict(features=[x[0] for x in feats])),
        ('real \\[T, F\\] matrix', dict(features=[x.astype(str) for x in feats])),
        ('real \\[T, F\\] matrix', dict(features=[x[:, :0] for x in feats])),
        ('rows, the run', dict(features=short)),
        ('non-finite', dict(features=nan)),
        ('features, run 0 has', dict(features=narrow)),
        ('alphas must be a vector', dict(alphas=[])),
        ('alphas must be a vector', dict(alphas=[[1.0]])),
        ('alphas must be a vector', dict(alphas=['a'])),
        ('finite and >= 0', dict(alphas=[1.0, -1.0])),
        ('finite and >= 0', dict(alphas=[np.inf])),
        ('finite and >= 0', dict(alphas=[np.nan])),
        ("score must be 'r2' or 'r'", dict(score='rho')),
        ("alpha must be 'per_vertex' or 'shared'", dict(alpha='global')),
        ('one key per run', dict(groups=g[:-1])),
        ('not hashable', dict(groups=[[k] for k in g])),
        ('has 1 run', dict(groups=g[:-1] + ['c'])),
        ('one list per subject', dict(folds=[[[0]]])),
        ('held-out sets of run positions', dict(folds=[3, 4])),
        ('has no folds', dict(folds=[[], [[0]]])),
        ('run positions in', dict(folds=[[[3]], [[0]]])),
        ('run positions in', dict(folds=[[[0.5]], [[0]]])),
        ('run positions in', dict(folds=[[[-1]], [[0]]])),
        ('at least one run, each once', dict(folds=[[[]], [[0]]])),
        ('at least one run, each once', dict(folds=[[[1, 1]], [[0]]])),
        ('training set is empty', dict(folds=[[[0, 1, 2]], [[0]]])),
        ('weights must be True or False', dict(weights=1)),
        ('scores must be True or False', dict(scores=None)),
    ]


@pytest.mark.parametrize('case', range(len(refusals())))
def test_refusals_of_the_host_path(case):
    match, change = refusals()[case]
    runs, feats = (list(a) for a in ec.data())
    kw = dict(runs=runs, features=feats, alphas=ec.ALPHAS, groups=list(ec.GROUPS))
    kw.update(change)
    with pytest.raises(ValueError, match='ridge_cv_host: .*' + match):
        ridge_cv_host(**kw)


def device_refusals():
    runs, feats = (list(a) for a in ec.data())
    wide = [np.zeros((x.shape[0], 257)) for x in feats]
    many = 33
    return refusals() + [
        ('F = 257 features', dict(features=wide)),
        ('33 penalties', dict(alphas=np.arange(1.0, many + 1))),
        ('has 65 runs', dict(runs=[runs[0][:2]] * 65, features=[feats[0][:2]] * 65, groups=None)),
        ('batch_runs must be an int >= 1', dict(batch_runs=0)),
        ('batch_runs must be an int >= 1', dict(batch_runs=1.5)),
    ]


@pytest.mark.parametrize('case', range(len(device_refusals())))
def test_refusals_of_the_device_path_come_before_any_launch(case, monkeypatch):
    """``ridge_cv`` refuses the same arguments, and the limits of the kernels, before it touches the device: the staging and the
    launches are made to fail the test if they are reached."""
    from gcn_fmri_decoding_amd import runs as _runs

    def reached(*a, **k):
        raise AssertionError('the device was reached')

    monkeypatch.setattr(_runs, 'stage', reached)
    monkeypatch.setattr(_runs, 'cuda_device', reached)
    match, change = device_refusals()[case]
    runs, feats = (list(a) for a in ec.data())
    kw = dict(runs=runs, features=feats, alphas=ec.ALPHAS, groups=list(ec.GROUPS))
    kw.update(change)
    with pytest.raises(ValueError, match='ridge_cv: .*' + match):
        en.ridge_cv(**kw)


def test_abi_refuses_before_any_launch():
    """The C entries' own checks need no device: every refusal comes before the first launch."""
    import ctypes
    from gcn_fmri_decoding_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    EINVAL, EUNSUPPORTED = -1, -4                              # (CHEBGCN_EINVAL, CHEBGCN_EUNSUPPORTED)
    q = lib.chebgcn_ridge_query
    assert [q(i) for i in range(7)] == [64, 16, 256, 32, 64, 65535, 256] and q(7) == -1 and q(100) == -1 and q(357) == -1
    assert [q(100 + F) for F in (1, 64, 65, 128, 129, 256)] == [64, 64, 128, 128, 256, 256]
    ws = lib.chebgcn_ridge_workspace
    assert ws(3, 5, 33) == 3 * 2 * 5 * 64 * 8 and ws(65535, 256, 1) > 0
    assert ws(0, 5, 33) == 0 and ws(65536, 5, 33) == 0 and ws(1, 257, 33) == 0 and ws(1, 0, 33) == 0 and ws(1, 5, 0) == 0

    def rotate(c=p, R=1, ptr=p, runs=p, nlist=1, V=p, E=1, F=1, M=1, w=p, nb=1 << 40):
        return lib.chebgcn_ridge_rotate(c, R, ptr, runs, nlist, V, E, F, M, w, nb, None)

    def score(w=p, nb=1 << 40, tss=p, R=1, ptr=p, runs=p, nlist=1, H=p, d=p, fp=p, E=1, Ef=1, S=1, F=1, A=1, M=1, kind=0, fold=p, sc=p,
              idx=p, table=None):
        return lib.chebgcn_ridge_score(w, nb, tss, R, ptr, runs, nlist, H, d, fp, E, Ef, S, F, A, M, kind, fold, sc, idx, table, None)

    def weights(w=p, nb=1 << 40, Vt=p, d=p, model=p, idx=p, E=1, S=1, F=1, A=1, M=1, out=p):
        return lib.chebgcn_ridge_weights(w, nb, Vt, d, model, idx, E, S, F, A, M, out, None)

    for call, names in ((rotate, ('c', 'ptr', 'runs', 'V', 'w')), (score, ('w', 'tss', 'ptr', 'runs', 'H', 'd', 'fp', 'fold', 'sc', 'idx')),
                        (weights, ('w', 'Vt', 'd', 'model', 'idx', 'out'))):
        for name in names:
            assert call(**{name: None}) == EINVAL, name
            assert b'NULL' in lib.chebgcn_last_error()
        for name in ('E', 'F', 'M'):
            assert call(**{name: 0}) == EINVAL, name
        assert call(nb=7) == EINVAL and b'workspace' in lib.chebgcn_last_error()
        assert call(F=257) == EUNSUPPORTED and call(E=65536) == EUNSUPPORTED
        assert call(w=odd) == EINVAL and b'unaligned' in lib.chebgcn_last_error()
    assert rotate(R=0) == EINVAL and rotate(nlist=0) == EINVAL and rotate(V=odd) == EINVAL
    assert score(A=33) == EUNSUPPORTED and score(S=65536, E=65535, Ef=1) == EUNSUPPORTED and weights(A=33) == EUNSUPPORTED
    assert weights(S=65536) == EUNSUPPORTED
    assert score(A=0) == EINVAL and score(S=0) == EINVAL and score(Ef=0) == EINVAL and score(Ef=2) == EINVAL and score(kind=2) == EINVAL
    assert score(kind=-1) == EINVAL and score(R=0) == EINVAL and weights(A=0) == EINVAL and weights(S=0) == EINVAL
    assert score(H=odd) == EINVAL and weights(Vt=odd) == EINVAL
    assert _lib.RIDGE_SCORES == ('r2', 'r')
