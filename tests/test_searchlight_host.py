"""The host side of ``searchlight``: the float64 restatement against scikit-learn's GaussianNB, a planted signal, ``hop_balls``
against a breadth-first search, the default folds of ``searchlight_events``, every refusal, and the C ABI's argument checks.
No GPU."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, graph, searchlight as sl


def ring(M, hops=1):
    i = np.arange(M)
    A = sp.csr_matrix((np.ones(2 * M), (np.concatenate([i, i]), np.concatenate([(i + 1) % M, (i - 1) % M]))), shape=(M, M))
    return graph.hop_balls(A, hops)


def data(rng, S, M, C, mean=100.0, sd=1.0, gain=0.5, folds=3):
    y = rng.permutation(np.arange(S) % C)
    X = (mean + sd * rng.randn(S, M) + gain * sd * rng.randn(C, M)[y]).astype(np.float32)
    return X, y, rng.permutation(np.arange(S) % folds)


def sklearn_fold(X, y, f, fold, cols):
    from sklearn.naive_bayes import GaussianNB
    X = X.astype(np.float64)
    tr, te = fold != f, fold == f
    clf = GaussianNB(var_smoothing=1e-9).fit(X[tr][:, cols], y[tr])
    return te, clf._joint_log_likelihood(X[te][:, cols]), clf.predict(X[te][:, cols])


def test_whole_brain_row_against_sklearn():
    pytest.importorskip('sklearn')
    rng = np.random.RandomState(0)
    S, M, C = 90, 40, 3
    X, y, fold = data(rng, S, M, C)
    row = sp.csr_matrix(np.ones((1, M)))
    res = sl.searchlight_host(X, y, row, fold, scores=True, predictions=True)
    assert res.scores.shape == (S, C, 1) and res.predictions.shape == (S, 1) and res.predictions.dtype == np.uint8
    worst = 0.0
    for f in range(3):
        te, jll, pred = sklearn_fold(X, y, f, fold, np.arange(M))
        assert np.array_equal(res.predictions[te, 0], pred)
        worst = max(worst, float((np.abs(res.scores[te, :, 0] - jll) / np.abs(jll)).max()))
    record_measured('searchlight_host_sklearn', rel=worst)
    assert worst <= 1e-9, worst
    assert res.correct.sum() == (res.predictions[:, 0] == y).sum() and res.support.tolist() == [[30, 30, 30]]


def test_two_hop_balls_against_sklearn():
    pytest.importorskip('sklearn')
    rng = np.random.RandomState(1)
    S, M, C = 60, 24, 3
    X, y, fold = data(rng, S, M, C, gain=1.0)
    balls = ring(M, 2)
    res = sl.searchlight_host(X, y, balls, fold, predictions=True)
    for u in range(M):
        cols = balls.indices[balls.indptr[u]:balls.indptr[u + 1]]
        assert cols.tolist() == sorted((u + d) % M for d in range(-2, 3))
        for f in range(3):
            te, _, pred = sklearn_fold(X, y, f, fold, cols)
            assert np.array_equal(res.predictions[te, u], pred), (u, f)
    want = np.zeros((1, C, M), np.int32)
    np.add.at(want, (0, y[:, None], np.arange(M)[None, :]), res.predictions == y[:, None])
    assert np.array_equal(res.correct, want) and res.correct.dtype == np.int32 and res.support.dtype == np.int64
    assert np.array_equal(res.recall, (want / 20.0).astype(np.float32)) and res.recall.dtype == np.float32
    assert np.array_equal(res.accuracy, (want.sum(axis=1) / 60.0).astype(np.float32)) and res.accuracy.shape == (1, M)


def test_planted_signal_is_found_where_the_ball_covers_it():
    rng = np.random.RandomState(2)
    S, M = 200, 120
    y = np.arange(S) % 2
    X = 100.0 + rng.randn(S, M)
    X[:, 50:61] += 2.0 * y[:, None]                             # the class means differ on vertices 50 .. 60 only
    res = sl.searchlight_host(X.astype(np.float32), y, ring(M, 2), np.arange(S) // 2 % 4)
    acc = res.accuracy[0]
    inside = np.arange(52, 59)                                  # all five vertices of the ball carry the signal
    outside = np.concatenate([np.arange(0, 48), np.arange(63, M)])      # none does
    record_measured('searchlight_host_planted', inside_min=float(acc[inside].min()), outside_dev=float(np.abs(acc[outside] - 0.5).max()))
    assert (acc[inside] >= 0.9).all(), acc[inside]
    assert (np.abs(acc[outside] - 0.5) <= 4.5 * np.sqrt(0.25 / S)).all(), acc[outside]     # 4.5 binomial sd over 105 centres


def test_groups_within_and_across():
    rng = np.random.RandomState(3)
    S, M = 48, 6
    X, y, _ = data(rng, S, M, 2)
    groups = ['b', 'a', 'c'] * 16
    fold = np.arange(S) // 3 % 2
    balls = ring(M, 1)
    res = sl.searchlight_host(X, y, balls, fold, groups=groups, scores=True)
    assert res.groups == ['b', 'a', 'c'] and res.correct.shape == (3, 2, M) and res.support.sum(axis=1).tolist() == [16, 16, 16]
    for g, key in enumerate(res.groups):
        own = np.array([k == key for k in groups])
        alone = sl.searchlight_host(X[own], y[own], balls, fold[own], scores=True)
        assert np.array_equal(alone.scores, res.scores[own]) and np.array_equal(alone.correct[0], res.correct[g])
    across = sl.searchlight_host(X, y, balls, fold, groups=groups, within=False, scores=True)
    pooled = sl.searchlight_host(X, y, balls, fold, scores=True)
    assert np.array_equal(across.scores, pooled.scores) and np.array_equal(across.correct.sum(axis=0), pooled.correct[0])


def test_an_integer_table_gets_its_centre_added_and_a_pattern_does_not():
    rng = np.random.RandomState(4)
    S, M = 40, 7
    X, y, fold = data(rng, S, M, 2, folds=2)
    table = np.stack([(np.arange(M) + 1) % M, (np.arange(M) + 2) % M, (np.arange(M) + 1) % M], axis=1)      # a duplicate column
    as_table = sl.searchlight_host(X, y, table, fold, scores=True)
    rows = np.repeat(np.arange(M), 3)
    with_centre = sp.csr_matrix((np.ones(3 * M), (np.concatenate([rows[::3], rows[::3], rows[::3]]),
                                                  np.concatenate([np.arange(M), table[:, 0], table[:, 1]]))), shape=(M, M))
    assert np.array_equal(as_table.scores, sl.searchlight_host(X, y, with_centre, fold, scores=True).scores)
    without = sp.csr_matrix((np.zeros(2 * M), (np.concatenate([np.arange(M)] * 2), table[:, :2].T.ravel())), shape=(M, M))
    bare = sl.searchlight_host(X, y, without, fold, scores=True, var_smoothing=0)      # stored zeros are members: values are ignored
    assert not np.array_equal(bare.scores, sl.searchlight_host(X, y, table, fold, scores=True, var_smoothing=0).scores)
    one = sl.searchlight_host(X[:, [1, 2]], y, sp.csr_matrix(np.ones((1, 2))), fold, scores=True, var_smoothing=0)
    assert np.array_equal(bare.scores[:, :, 0], one.scores[:, :, 0])
    indptr, indices = sl._neighbourhoods(sp.csr_matrix((np.ones(3), ([0, 0, 0], [4, 1, 4])), shape=(1, M)), M, 't')
    assert indptr.tolist() == [0, 2] and indices.tolist() == [1, 4]        # sorted, duplicates merged


def test_hop_balls_against_a_breadth_first_search():
    rng = np.random.RandomState(5)
    M = 60
    A = sp.random(M, M, density=0.04, random_state=rng, format='csr')
    A = sp.lil_matrix(A + A.T)
    A[3, :] = 0                                                 # an isolated vertex
    A[:, 3] = 0
    A = sp.csr_matrix(A)
    A.data[:5] = 0                                              # stored zeros are no edges
    nbrs = [set(np.flatnonzero(A[v].toarray().ravel() != 0).tolist()) for v in range(M)]
    for hops in (0, 1, 2, 3):
        B = graph.hop_balls(A, hops)
        assert B.dtype == np.bool_ and B.shape == (M, M) and B.has_sorted_indices and B.data.all()
        for v in range(M):
            seen, front = {v}, {v}
            for _ in range(hops):
                front = set().union(*[nbrs[w] for w in front]) - seen
                seen |= front
            got = B.indices[B.indptr[v]:B.indptr[v + 1]].tolist()
            assert got == sorted(seen), (hops, v)
    assert graph.hop_balls(A, 2)[3].indices.tolist() == [3]
    for bad in [(A, -1), (A, 1.5), (A, True), (A.toarray(), 1), (sp.csr_matrix(np.ones((2, 3))), 1)]:
        with pytest.raises(ValueError, match='hop_balls'):
            graph.hop_balls(*bad)


def test_default_folds_of_searchlight_events():
    groups = ['s2', 's1', 's2', 's1', 's2', 's3']
    assert sl.default_folds(groups, within=True).tolist() == [0, 0, 1, 1, 2, 0]
    assert sl.default_folds(groups, within=False).tolist() == [0, 1, 0, 1, 0, 2]
    names = ['rest'] * 3 + ['a'] * 8 + ['rest'] * 3 + ['b'] * 8 + ['rest'] * 2
    runs = [names, ['rest'] * len(names), names[::-1], names, names, names]          # run 1 has no trial: it drops out
    T = len(names)
    for within, want in ((True, [0, 1, 1, 2, 0]), (False, [0, 0, 1, 0, 2])):
        idx, labels, tg, tf, classes = sl._events_plan([T] * 6, runs, ['a', 'b'], 4, groups, None, within, {})
        assert classes == ['a', 'b'] and idx.shape == (5 * 4, 4) and idx.dtype == np.int64
        assert tg == [g for g in ['s2', 's2', 's1', 's2', 's3'] for _ in range(4)]
        assert tf.tolist() == [f for f in want for _ in range(4)]
        assert labels.tolist() == (['a', 'a', 'b', 'b'] + ['b', 'b', 'a', 'a'] + ['a', 'a', 'b', 'b'] * 3)
        assert idx[0].tolist() == [3, 4, 5, 6] and idx[4].tolist() == [2 * T + 2, 2 * T + 3, 2 * T + 4, 2 * T + 5]
    given = sl._events_plan([T] * 6, runs, ['a', 'b'], 4, groups, [5, 6, 7, 8, 9, 10], True, {})[3]
    assert given.tolist() == [f for f in [5, 7, 8, 9, 10] for _ in range(4)]
    shifted = sl._events_plan([T] * 6, runs, ['a', 'b'], 4, groups, None, True, {'start_trial': 2})[0]
    assert shifted[0].tolist() == [5, 6, 7, 8]
    for kw, what in [(dict(block_dura=17), 'block_dura'), (dict(block_dura=0), 'block_dura'), (dict(groups=['a']), 'groups'),
                     (dict(folds=[0, 1]), 'folds'), (dict(folds=[0.5] * 6), 'folds'), (dict(within=1), 'within'),
                     (dict(lengths=[T] * 5 + [T + 1]), 'rows'), (dict(label_runs=runs[:5]), 'label_runs'),
                     (dict(label_runs=[['rest'] * T] * 6), 'no run yields')]:
        args = dict(lengths=[T] * 6, label_runs=runs, target_name=['a', 'b'], block_dura=4, groups=groups, folds=None, within=True,
                    match_kw={})
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            sl._events_plan(**args)


def test_both_calls_refuse_before_the_device():
    rng = np.random.RandomState(6)
    S, M = 24, 5
    X, y, fold = data(rng, S, M, 2, folds=2)
    balls = ring(M, 1)
    bad = X.copy()
    bad[3, 1] = np.nan
    empty = sp.csr_matrix((np.ones(2), ([0, 2], [1, 2])), shape=(3, M))
    lonely = y.copy()
    lonely[fold == 1] = 0                                       # class 1 is never trained on by the model that tests fold 0
    big = 1 << 12
    for fn in (sl.searchlight_host, sl.searchlight):
        for args, kw, what in [
                ((X[0], y, balls, fold), {}, r'\[S >= 2, M >= 1\]'), ((X[:1], y[:1], balls, fold[:1]), {}, r'\[S >= 2'),
                ((X.astype(complex), y, balls, fold), {}, 'dtype'), ((X.astype(str), y, balls, fold), {}, 'dtype'),
                ((bad, y, balls, fold), {}, 'non-finite'),
                ((X, y[:-1], balls, fold), {}, 'labels'), ((X, y.astype(float), balls, fold), {}, 'labels of dtype'),
                ((X, np.zeros(S, int), balls, fold), {}, 'two distinct classes'), ((X, lonely, balls, fold), {}, 'no training sample'),
                ((X, y, balls, fold), dict(classes=[0]), 'two distinct classes'), ((X, y, balls, fold), dict(classes=[0, 0, 1]), 'distinct'),
                ((X, y, balls, fold), dict(classes=[0, 2]), 'not in classes'),
                ((X, y, ring(M + 1), fold), {}, 'neighbourhoods'), ((X, y, empty, fold), {}, 'neighbourhood 1 is empty'),
                ((X, y, np.zeros((M, 2)), fold), {}, 'integer table'), ((X, y, np.zeros((M + 1, 2), int), fold), {}, 'integer table'),
                ((X, y, np.full((M, 2), M), fold), {}, 'outside'), ((X, y, np.arange(M), fold), {}, 'integer table'),
                ((X, y, balls, fold[:-1]), {}, 'folds'), ((X, y, balls, fold + 0.5), {}, 'folds must be ints'),
                ((X, y, balls, fold), dict(groups=[0] * (S - 1)), 'groups'), ((X, y, balls, fold), dict(groups=[[0]] * S), 'hashable'),
                ((X, y, balls, fold), dict(within=1), 'within'), ((X, y, balls, fold), dict(variance='full'), 'variance'),
                ((X, y, balls, fold), dict(priors='flat'), 'priors'), ((X, y, balls, fold), dict(var_smoothing=-1e-9), 'var_smoothing'),
                ((X, y, balls, fold), dict(var_smoothing=np.nan), 'var_smoothing'), ((X, y, balls, fold), dict(var_smoothing='1'), 'var_smoothing'),
                ((X, y, balls, fold), dict(scores=1), 'scores'), ((X, y, balls, fold), dict(predictions='yes'), 'predictions'),
                ((X, y, balls, fold), dict(batch_centres=0), 'batch_centres'), ((X, y, balls, fold), dict(batch_centres=2.0), 'batch_centres'),
                ((np.zeros((big, M), np.float32), np.arange(big) % 2, sp.csr_matrix(np.ones((big * 16, 1))) @ sp.csr_matrix(np.ones((1, M))),
                  np.arange(big) // 2 % 2), dict(scores=True), 'refused beyond')]:
            with pytest.raises(ValueError, match=what):
                fn(*args, **kw)
        with pytest.raises(ValueError, match=r"group 'b', fold 1"):
            fn(X, np.where((np.arange(S) % 2 == 1) & (fold == 0), 0, y), balls, fold, groups=['a', 'b'] * (S // 2))
        with pytest.raises(ValueError, match='for the test samples of fold 0'):
            fn(X, lonely, balls, fold, groups=['a', 'b'] * (S // 2), within=False)
    many = np.arange(2 * (sl.CMAX + 1)) % (sl.CMAX + 1)
    with pytest.raises(ValueError, match='served'):
        sl.searchlight(np.zeros((many.size, M), np.float32), many, balls, np.arange(many.size) // (sl.CMAX + 1))
    for kw, what in [(dict(TRstep=2), 'TRstep'), (dict(classes=['a']), 'classes'), (dict(smoothing=1), 'unknown keyword'),
                     (dict(variance='full'), 'variance')]:
        with pytest.raises(ValueError, match=what):
            sl.searchlight_events(np.zeros((20, M), np.float32), ['rest'] * 3 + ['a'] * 7 + ['b'] * 7 + ['rest'] * 3, ['a', 'b'], 3, balls, **kw)
    with pytest.raises(ValueError, match='vertices'):
        sl.searchlight_events([np.zeros((20, M)), np.zeros((20, M + 1))], [['a'] * 20] * 2, ['a', 'b'], 3, balls)


def test_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_searchlight_query(i) for i in range(11)]
    assert all(v > 0 for v in q) and L.chebgcn_searchlight_query(11) == -1 and L.chebgcn_searchlight_query(-1) == -1
    TILE, CENTRES, UNROLL, CMAX, VERTS, NMAX, TILES, GMAX, NARROW, PER_LANE, UNROLL2 = q
    assert (CMAX, NMAX, GMAX) == (sl.CMAX, sl.NMAX, sl.GMAX) and TILE == 64 and NARROW < CMAX
    buckets = [L.chebgcn_searchlight_query(100 + c) for c in range(1, CMAX + 1)]
    assert all(b >= c for c, b in zip(range(1, CMAX + 1), buckets)) and buckets == sorted(buckets) and buckets[-1] == CMAX
    assert L.chebgcn_searchlight_query(100) == -1 and L.chebgcn_searchlight_query(101 + CMAX) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    EINVAL, EUNSUP = -1, -4

    def spread(Xt=p, S=4, M=1, ptr=p, idx=p, n=1, NM=1, out=p):
        return L.chebgcn_searchlight_spread(Xt, S, M, ptr, idx, n, NM, out, None)

    for kw in [dict(Xt=None), dict(ptr=None), dict(idx=None), dict(out=None), dict(S=0), dict(M=0), dict(n=0), dict(NM=0), dict(NM=-1),
               dict(S=2 ** 31 - 1), dict(Xt=odd2), dict(idx=odd2), dict(out=odd4)]:
        assert spread(**kw) == EINVAL, kw
        assert b'searchlight_spread' in L.chebgcn_last_error()
    assert spread(NM=NMAX + 1) == EUNSUP and b'searchlight_spread' in L.chebgcn_last_error()

    def fit(Xt=p, S=4, M=1, ptr=p, idx=p, n=1, NM=1, C=2, pooled=0, eps=p, par=p, lg=p):
        return L.chebgcn_searchlight_fit(Xt, S, M, ptr, idx, n, NM, C, pooled, eps, par, lg, None)

    for kw in [dict(Xt=None), dict(ptr=None), dict(idx=None), dict(eps=None), dict(par=None), dict(lg=None), dict(S=0), dict(M=0),
               dict(n=0), dict(NM=0), dict(C=1), dict(C=0), dict(pooled=2), dict(ptr=odd2), dict(eps=odd4), dict(par=odd4), dict(lg=odd4)]:
        assert fit(**kw) == EINVAL, kw
        assert b'searchlight_fit' in L.chebgcn_last_error()
    for kw in [dict(NM=NMAX + 1), dict(C=CMAX + 1)]:
        assert fit(**kw) == EUNSUP, kw
        assert b'searchlight_fit' in L.chebgcn_last_error()

    def score(Xt=p, S=4, M=1, rowptr=p, colidx=p, nnz=1, U=2, u0=0, Ub=2, tptr=p, tmax=1, NM=1, C=2, par=p, lg=p, lp=p, sg=p, sy=p, so=p,
              G=1, base=p, correct=p, scores=None, pred=None):
        return L.chebgcn_searchlight_score(Xt, S, M, rowptr, colidx, nnz, U, u0, Ub, tptr, tmax, NM, C, par, lg, lp, sg, sy, so, G, base,
                                           correct, scores, pred, None)

    for kw in [dict(Xt=None), dict(rowptr=None), dict(colidx=None), dict(tptr=None), dict(par=None), dict(lg=None), dict(lp=None),
               dict(sg=None), dict(sy=None), dict(so=None), dict(base=None), dict(correct=None), dict(S=0), dict(M=0), dict(nnz=0),
               dict(U=0), dict(u0=-1), dict(Ub=0), dict(u0=1), dict(Ub=3), dict(tmax=0), dict(tmax=5), dict(NM=0), dict(C=1), dict(G=0),
               dict(Xt=odd2), dict(correct=odd2), dict(par=odd4), dict(base=odd4), dict(scores=odd4)]:
        assert score(**kw) == EINVAL, kw
        assert b'searchlight_score' in L.chebgcn_last_error()
    for kw in [dict(NM=NMAX + 1), dict(C=CMAX + 1), dict(G=GMAX + 1), dict(S=TILES * TILE + 64, tmax=TILES * TILE + 1),
               dict(U=2 ** 31 - 1, Ub=(2 ** 31 - 1) // CMAX + 1)]:
        assert score(**kw) == EUNSUP, kw
        assert b'searchlight_score' in L.chebgcn_last_error()
