"""The host side of ``searchlight.crossnobis``: the float64 restatement ``crossnobis_host`` (explicit double sum over pairs of
different cells) against the ``t - q`` identity the kernel uses, against closed forms (two partitions; full shrinkage), the
``'auto'`` shrinkage against ``sklearn.covariance.ledoit_wolf``, the pair order against ``squareform``, invariances, what the
estimator is for (unbiased; whitening finds what a Euclidean distance drowns in shared noise), ``compare_rdms``, every new
refusal, degenerate balls and the C ABI's argument checks.  No GPU."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial.distance import squareform

from conftest import record_measured
from gcn_fmri_decoding_amd import RDMResult, _lib, compare_rdms, crossnobis, crossnobis_events, crossnobis_host, lda_shrinkage_host
from gcn_fmri_decoding_amd import searchlight as sl


def data(rng, S, M, C, mean=100.0, sd=1.0, parts=4):
    """Balanced classes whose means differ by 0.5 sd per vertex; every (partition, class) cell holds S / (parts C) samples."""
    y = np.arange(S) % C
    part = np.arange(S) // C % parts
    X = (mean + sd * rng.randn(S, M) + 0.5 * sd * rng.randn(C, M)[y]).astype(np.float32)
    return X, y, part


def rows_of(M, lengths, step=7):
    r = sp.lil_matrix((len(lengths), M))
    for i, P in enumerate(lengths):
        assert step * i + P <= M
        r[i, step * i:step * i + P] = 1
    return r.tocsr()


def whitened(A, y, part, g):
    """``(u [F, C, P], nu, R)`` of one ball, restated: cell means, residuals about them, Sigma, the forward solve."""
    parts, C, P = np.unique(part), int(y.max()) + 1, A.shape[1]
    mu = np.stack([np.stack([A[(part == k) & (y == c)].mean(axis=0) for c in range(C)]) for k in parts])
    R = np.concatenate([A[(part == k) & (y == c)] - mu[i, c] for i, k in enumerate(parts) for c in range(C)])
    S = R.T @ R / len(A)
    nu = np.trace(S) / P
    if g == 'auto':
        g = lda_shrinkage_host(R)
    L = np.linalg.cholesky((1.0 - g) * S + g * nu * np.eye(P))
    d = mu - A.mean(axis=0)                                     # (balanced or not: sum n_kc mu_kc / n is the plain mean)
    return np.linalg.solve(L, d.reshape(-1, P).T).T.reshape(len(parts), C, P), nu, R


# ---- 1. the estimator -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('parts', [2, 3, 5])
def test_explicit_sum_against_the_identity(parts):
    rng = np.random.RandomState(parts)
    C = 4
    X, y, part = data(rng, 3 * parts * C, 60, C, parts=parts)
    nb = rows_of(60, [1, 5, 33], step=3)
    res, scale = crossnobis_host(X, y, nb, part, return_scale=True)
    assert isinstance(res, RDMResult) and res.rdm.shape == scale.shape == (1, 6, 3) and res.rdm.dtype == np.float64
    assert res.shrinkage.shape == (1, 3) and (res.shrinkage == 0.1).all() and res.folds.tolist() == [parts] and res.groups == [0]
    assert res.classes == [0, 1, 2, 3] and res.pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    worst = 0.0
    for u in range(3):
        cols = nb[u].indices
        w, _, _ = whitened(X.astype(np.float64)[:, cols], y, part, 0.1)
        T = w.sum(axis=0)
        for i, (a, b) in enumerate(res.pairs):
            q = ((w[:, a] - w[:, b]) ** 2).sum()
            t = ((T[a] - T[b]) ** 2).sum()
            want = (t - q) / (parts * (parts - 1) * cols.size)
            worst = max(worst, abs(res.rdm[0, i, u] - want) / ((t + q) / (parts * (parts - 1) * cols.size)))
            assert scale[0, i, u] >= (t + q) / (parts * (parts - 1) * cols.size) * (1 - 1e-9)       # kappa >= 1
    record_measured('rsa_host_identity_F%d' % parts, rel=worst)
    assert worst <= 1e-9, worst


def test_two_partitions_written_out():
    rng = np.random.RandomState(12)
    X, y, part = data(rng, 24, 20, 3, parts=2)
    nb = rows_of(20, [4, 11], step=5)
    res = crossnobis_host(X, y, nb, part, shrinkage=0.05)
    for u in range(2):
        cols = nb[u].indices
        w, _, _ = whitened(X.astype(np.float64)[:, cols], y, part, 0.05)
        for i, (a, b) in enumerate(res.pairs):
            want = (w[0, a] - w[0, b]) @ (w[1, a] - w[1, b]) / cols.size
            assert abs(res.rdm[0, i, u] - want) <= 1e-12 * max(abs(want), 1.0)


def test_full_shrinkage_is_the_cross_validated_euclidean_distance():
    rng = np.random.RandomState(13)
    parts, C = 3, 3
    X, y, part = data(rng, 54, 12, C, parts=parts)
    nb = rows_of(12, [5, 12], step=0)
    res = crossnobis_host(X, y, nb, part, shrinkage=1)
    X64 = X.astype(np.float64)
    for u in range(2):
        A = X64[:, nb[u].indices]
        P = A.shape[1]
        mu = np.stack([np.stack([A[(part == k) & (y == c)].mean(axis=0) for c in range(C)]) for k in range(parts)])
        nu = sum(((A[(part == k) & (y == c)] - mu[k, c]) ** 2).sum() for k in range(parts) for c in range(C)) / len(A) / P
        for i, (a, b) in enumerate(res.pairs):
            d = mu[:, a] - mu[:, b]
            cv = sum(d[k] @ d[l] for k in range(parts) for l in range(parts) if k != l) / (parts * (parts - 1))
            assert np.isclose(res.rdm[0, i, u], cv / (nu * P), rtol=1e-11, atol=0)


def test_auto_shrinkage_against_sklearn():
    pytest.importorskip('sklearn')
    from sklearn.covariance import ledoit_wolf
    rng = np.random.RandomState(14)
    X, y, part = data(rng, 72, 40, 3, 1e3, 5.0, parts=4)
    X[:, :20] += (20.0 * rng.randn(72, 1)).astype(np.float32)   # a common factor: the coefficient is inside (0, 1)
    nb = rows_of(40, [6, 20, 40], step=0)
    res = crossnobis_host(X, y, nb, part, shrinkage='auto')
    for u in range(3):
        _, _, R = whitened(X.astype(np.float64)[:, nb[u].indices], y, part, 0.5)
        want = float(ledoit_wolf(R, assume_centered=True)[1])
        assert sl.SHRINK_MIN < want < 1 and abs(res.shrinkage[0, u] - want) <= 1e-12 * want
        assert res.shrinkage[0, u] == lda_shrinkage_host(R)


def test_pair_order_is_squareform_and_square():
    rng = np.random.RandomState(15)
    X, y, part = data(rng, 40, 8, 5, parts=2)
    res = crossnobis_host(X, y, rows_of(8, [3, 8], step=0), part)
    sq = res.square(0)
    assert sq.shape == (2, 5, 5) and np.array_equal(sq, sq.transpose(0, 2, 1))
    for u in range(2):
        assert np.array_equal(squareform(sq[u], checks=False), res.rdm[0, :, u])
        assert np.array_equal(squareform(res.rdm[0, :, u]), sq[u])
    assert np.array_equal(res.model_maps(np.ones((1, 10)), 'cosine'), compare_rdms(res.rdm, np.ones((1, 10)), 'cosine'))


def test_relabelling_and_permuting_leave_the_rdm_unchanged():
    rng = np.random.RandomState(16)
    X, y, part = data(rng, 72, 30, 3, parts=3)
    nb = rows_of(30, [2, 9, 30], step=0)
    res, scale = crossnobis_host(X, y, nb, part, return_scale=True)
    perm = rng.permutation(72)
    moved = crossnobis_host(X[perm], y[perm], nb, part[perm])
    assert (np.abs(moved.rdm - res.rdm) <= 1e-12 * scale).all()
    names = np.array(['c', 'a', 'b'])[y]                        # class 0 -> 'c' (sorted last), 1 -> 'a', 2 -> 'b'
    other = crossnobis_host(X, names, nb, part * 7 - 3, groups=['s'] * 72)
    assert other.classes == ['a', 'b', 'c'] and other.groups == ['s']
    back = {('a', 'b'): (1, 2), ('a', 'c'): (0, 1), ('b', 'c'): (0, 2)}
    for i, (a, b) in enumerate(other.pairs):
        j = res.pairs.tolist().index(list(back[(other.classes[a], other.classes[b])]))
        assert (np.abs(other.rdm[0, i] - res.rdm[0, j]) <= 1e-12 * scale[0, j]).all()
    given = crossnobis_host(X, y, nb, part, classes=[2, 0, 1])  # classes in the caller's order
    assert given.classes == [2, 0, 1] and (np.abs(given.rdm[0, 0] - res.rdm[0, 1]) <= 1e-12 * scale[0, 1]).all()


def test_groups_are_independent():
    rng = np.random.RandomState(17)
    X, y, part = data(rng, 120, 10, 2, parts=5)
    groups = np.array(['b', 'a', 'c'])[np.arange(120) // 2 % 3]
    part = np.where(groups == 'a', part % 2, np.where(groups == 'c', part % 3, part))       # 5, 2 and 3 partitions
    nb = rows_of(10, [4, 10], step=0)
    res = crossnobis_host(X, y, nb, part, groups=groups)
    assert res.groups == ['b', 'a', 'c'] and res.folds.tolist() == [5, 2, 3] and res.rdm.shape == (3, 1, 2)
    for g, key in enumerate(res.groups):
        own = groups == key
        alone = crossnobis_host(X[own], y[own], nb, part[own])
        assert np.array_equal(alone.rdm[0], res.rdm[g]) and np.array_equal(alone.shrinkage[0], res.shrinkage[g])


# ---- 2. what it is for ----------------------------------------------------------------------------------------------------------

def test_unbiased_and_what_whitening_is_for():
    """64 two-vertex balls, 3 classes, 4 partitions x 6 samples per cell; a common noise of sd 20 on both vertices plus an
    independent one of sd 1; class 1 is shifted by +2 / -2 on the two vertices, class 2 is class 0.  Whitened (g = 0.01) the
    distances to class 1 stand out and d_02 is zero on average; Euclidean (g = 1) the common noise drowns all three."""
    rng = np.random.RandomState(18)
    balls, C, parts, per = 64, 3, 4, 6
    S = C * parts * per
    y = np.arange(S) % C
    part = np.arange(S) // C % parts
    X = 100.0 + np.repeat(20.0 * rng.randn(S, balls), 2, axis=1) + rng.randn(S, 2 * balls)
    X[:, 0::2] += 2.0 * (y == 1)[:, None]
    X[:, 1::2] -= 2.0 * (y == 1)[:, None]
    nb = sp.csr_matrix(np.kron(np.eye(balls), np.ones((1, 2))))
    white = crossnobis_host(X.astype(np.float32), y, nb, part, shrinkage=0.01).rdm[0].mean(axis=1)
    plain = crossnobis_host(X.astype(np.float32), y, nb, part, shrinkage=1).rdm[0].mean(axis=1)
    record_measured('rsa_host_unbiased', d01=white[0], d02=white[1], d12=white[2], e01=plain[0], e02=plain[1], e12=plain[2])
    print('whitened', white, 'euclidean', plain)
    assert white[0] > 0.7 and white[2] > 0.7 and abs(white[1]) < 0.15, white
    assert np.abs(plain).max() < 0.15, plain


# ---- 3. compare_rdms ------------------------------------------------------------------------------------------------------------

def test_compare_rdms_against_numpy_and_its_zero_rules():
    rng = np.random.RandomState(19)
    G, n, U, Q = 2, 6, 5, 3
    rdm = rng.randn(G, n, U)
    rdm[0, :, 1] = 0.37                                         # a constant RDM
    rdm[1, :, 2] = 0.0                                          # an all-zero one
    models = rng.rand(Q, n)
    models[2] = 1.0                                             # a constant model
    r = compare_rdms(rdm, models)
    c = compare_rdms(rdm, models, method='cosine')
    assert r.shape == c.shape == (G, Q, U) and r.dtype == c.dtype == np.float64
    for g in range(G):
        for q in range(Q):
            for u in range(U):
                x, m = rdm[g, :, u], models[q]
                dead = x.max() == x.min() or m.max() == m.min()
                assert np.isclose(r[g, q, u], 0.0 if dead else np.corrcoef(x, m)[0, 1], rtol=1e-12, atol=1e-15)
                zero = not x.any() or not m.any()
                assert np.isclose(c[g, q, u], 0.0 if zero else x @ m / np.sqrt((x @ x) * (m @ m)), rtol=1e-12, atol=1e-15)
    assert (r[0, :, 1] == 0).all() and (r[1, :, 2] == 0).all() and (r[:, 2] == 0).all() and (c[1, :, 2] == 0).all()
    assert (c[0, :, 1] != 0).all()                              # a constant RDM has a cosine
    assert (compare_rdms(rng.randn(1, 1, 4), [[1.0]]) == 0).all()          # two classes: one pair, no correlation
    import torch
    t = compare_rdms(torch.as_tensor(rdm), models)
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.allclose(t.numpy(), r, rtol=1e-13, atol=1e-15)
    for bad, kw in [(rdm[0], {}), (rdm, dict(method='spearman')), (rdm, dict(models=models[:, :5])), (rdm, dict(models=models[0]))]:
        with pytest.raises(ValueError, match='compare_rdms'):
            compare_rdms(bad, kw.pop('models', models), **kw)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------

def test_every_new_refusal_before_the_device():
    rng = np.random.RandomState(20)
    S, M = 24, 130
    X, y, part = data(rng, S, M, 2, parts=2)
    balls = rows_of(M, [3, 128], step=1)
    groups = ['s1'] * 12 + ['s2'] * 12
    lacking = y.copy()
    lacking[(part == 1) & (np.arange(S) >= 12)] = 0             # group s2, partition 1 holds no sample of class 1
    many = np.arange(S * 2) % 33
    for fn in (crossnobis_host, crossnobis):
        for args, kw, what in [
                ((X, lacking, balls, part), dict(groups=groups), r"group 's2', partition 1 holds no sample of class 1"),
                ((X, y, balls, np.where(np.arange(S) < 12, part, 5)), dict(groups=groups), r"group 's2' has only one partition \(5\)"),
                ((X, y, balls, np.zeros(S, int)), {}, 'has only one partition'),
                ((X, y, rows_of(M, [3, 129], step=1), part), {}, 'neighbourhood 1 holds 129 vertices'),
                ((X, np.zeros(S, int), balls, part), {}, 'at least two distinct classes'),
                ((X, y, balls, part), dict(classes=[1]), 'at least two distinct classes'),
                ((X, y, balls, part), dict(shrinkage=0.0), 'shrinkage'), ((X, y, balls, part), dict(shrinkage=1e-7), 'shrinkage'),
                ((X, y, balls, part), dict(shrinkage=1.5), 'shrinkage'), ((X, y, balls, part), dict(shrinkage='lw'), 'shrinkage'),
                ((X, y, balls, part), dict(shrinkage=None), 'shrinkage'), ((X, y, balls, part), dict(shrinkage=True), 'shrinkage'),
                ((X, y, balls, part.astype(float)), {}, 'partitions must be ints'), ((X, y, balls, part[:-1]), {}, 'partitions'),
                ((X, y, balls, part), dict(batch_centres=0), 'batch_centres'), ((X, y[:-1], balls, part), {}, 'labels'),
                ((X, y, balls, part), dict(groups=groups[:-1]), 'groups'), ((X[0], y, balls, part), {}, 'samples')]:
            with pytest.raises(ValueError, match=what):
                fn(*args, **kw)
    with pytest.raises(ValueError, match='33 classes; served: up to 32'):
        crossnobis(np.zeros((S * 2, 4), np.float32), many, rows_of(4, [2], step=0), np.arange(S * 2) // 33 % 2)
    bad = X.copy()
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        crossnobis(bad, y, balls, part)
    run = np.zeros((20, M), np.float32)
    names = ['rest'] * 3 + ['a'] * 7 + ['b'] * 7 + ['rest'] * 3
    for runs, labels, nb, kw, what in [
            ([run, run], [names, names], rows_of(M, [3, 129], step=1), {}, 'holds 129 vertices'),
            ([run, run], [names, names], balls, dict(shrinkage=2), 'shrinkage'),
            ([run, run], [names, names], balls, dict(classifier='lda'), 'unknown keyword'),
            ([run, run], [names, names], balls, dict(partitions=[0, 1]), 'partitions are not taken'),
            ([run, run], [names, names], balls, dict(groups=['s1', 's2']), 'has only one partition'),
            (run, names, balls, {}, 'has only one partition'),
            ([run, run], [names, ['rest'] * 3 + ['a'] * 14 + ['rest'] * 3], balls, {}, "partition 1 holds no sample of class 'b'")]:
        with pytest.raises(ValueError, match=what):
            crossnobis_events(runs, labels, ['a', 'b'], 3, nb, **kw)


# ---- 5. degenerate balls --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('g', [1e-6, 0.1, 1, 'auto'])
def test_all_zero_and_partly_zero_balls(g):
    rng = np.random.RandomState(21)
    S, M = 48, 40
    X, y, part = data(rng, S, M, 3, parts=2)
    X[:, 20:] = 0.0
    nb = sp.vstack([rows_of(M, [6, 20], step=0), rows_of(M, [20], step=0)[:, ::-1], rows_of(M, [34], step=0)[:, ::-1]]).tocsr()
    res, scale = crossnobis_host(X, y, nb, part, shrinkage=g, return_scale=True)
    assert np.isfinite(res.rdm).all() and np.isfinite(res.shrinkage).all() and np.isfinite(scale).all()
    assert (res.rdm[0, :, 2] == 0).all() and res.shrinkage[0, 2] == -1 and (scale[0, :, 2] == 0).all()     # the all-zero ball
    live = [0, 1, 3]
    assert (res.shrinkage[0, live] > 0).all() and (res.rdm[0][:, live] != 0).all()      # 14 live vertices among 20 zero ones speak
    if g != 'auto':
        assert (res.shrinkage[0, live] == g).all()


# ---- 6. the C ABI ---------------------------------------------------------------------------------------------------------------

def test_entry_point_checks_its_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_searchlight_rdm_query(i) for i in range(7)]
    assert all(v > 0 for v in q) and L.chebgcn_searchlight_rdm_query(7) == -1 and L.chebgcn_searchlight_rdm_query(-1) == -1
    THREADS, PMAX, TILE, CMAX, PAIRS, CELLS, NARROW = q
    lda = [L.chebgcn_searchlight_lda_query(i) for i in (0, 1, 2, 3, 5, 8)]
    assert [THREADS, PMAX, TILE, CMAX, CELLS, NARROW] == lda and (PMAX, CMAX, CELLS) == (sl.LDA_PMAX, sl.CMAX, sl.NMAX)
    assert PAIRS == CMAX * (CMAX - 1) // 2 <= 2 * THREADS
    assert [L.chebgcn_searchlight_rdm_query(100 + P) for P in range(PMAX + 2)] == \
        [L.chebgcn_searchlight_lda_query(100 + P) for P in range(PMAX + 2)]
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    EINVAL, EUNSUP = -1, -4

    def rdm(Xt=p, S=4, M=1, rowptr=p, colidx=p, nnz=1, U=2, centres=p, Ub=2, bucket=32, cell=p, cptr=p, cidx=p, nidx=1, NM=2, C=2, par=p,
            g=0.1, G=1, out=p, gamma=None):
        return L.chebgcn_searchlight_rdm(Xt, S, M, rowptr, colidx, nnz, U, centres, Ub, bucket, cell, cptr, cidx, nidx, NM, C, par, g, G, out,
                                         gamma, None)

    for kw in [dict(Xt=None), dict(rowptr=None), dict(colidx=None), dict(centres=None), dict(cell=None), dict(cptr=None), dict(cidx=None),
               dict(par=None), dict(out=None), dict(S=0), dict(M=0), dict(S=2 ** 31 - 1), dict(nnz=0), dict(U=0), dict(Ub=0), dict(Ub=-1),
               dict(bucket=0), dict(bucket=-32), dict(nidx=0), dict(NM=0), dict(C=1), dict(C=0), dict(G=0), dict(g=0.0), dict(g=1e-7),
               dict(g=1.0000001), dict(g=float('nan')), dict(g=float('inf')), dict(NM=1), dict(NM=3, G=2), dict(NM=2, G=2),
               dict(Xt=odd2), dict(centres=odd2), dict(cell=odd2), dict(cidx=odd2), dict(par=odd4), dict(out=odd4), dict(gamma=odd4)]:
        assert rdm(**kw) == EINVAL, kw
        assert b'searchlight_rdm' in L.chebgcn_last_error()
    for kw in [dict(NM=CELLS + 1), dict(C=CMAX + 1), dict(bucket=16), dict(bucket=33), dict(bucket=256)]:
        assert rdm(**kw) == EUNSUP, kw
        assert b'searchlight_rdm' in L.chebgcn_last_error()
