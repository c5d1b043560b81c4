"""The data, the yardstick and the bound that tests/test_encoding_host.py and tests/test_gpu_encoding.py share (plain helpers, no
fixtures).

The yardstick uses none of the statistics algebra of ``encoding``: per fold it centres every run, stacks the training rows, solves
``(X^T X + alpha I) w = X^T Y`` with ``numpy.linalg.solve`` (``numpy.linalg.lstsq`` at alpha = 0, where a duplicated column makes
the system singular and the minimum-norm solution is meant), predicts the held-out rows explicitly, forms the residuals, and takes
R^2 and Pearson's r from them.

The bound.  ``rss = tss - 2 p + q`` is a difference of numbers that are themselves differences of sums of squares of size
``yy_te`` (the uncentred sum of squares of the held-out signal: BOLD-like data has mean 100 and a standard deviation near 1), so
an error of a few ulps of ``yy_te + |p| + q`` shows in ``rss / tss`` at the scale ``s = (yy_te + |p| + q) / tss_te``; the bound
is ``|got - ref| <= C_BOUND * s``.  ``C_MEASURED`` is the largest ``|got - ref| / s`` between ``ridge_cv_host`` and the yardstick
over every case of test_encoding_host.py, measured on the CPU; ``C_BOUND`` is 100 times that (the GLM tests give their measured
constants 500 times; this route has fewer sources of error).
"""
import functools

import numpy as np

C_MEASURED = 1.5e-15        # R^2, full rank, subject 'a'; rank-deficient 1.4e-15; Pearson's r 6.7e-16 at most
C_BOUND = 100 * C_MEASURED
ALPHAS = np.logspace(-2, 4, 12)
CONSTANT_VERTEX = 7
LENGTHS = (57, 80, 64, 71, 60, 77, 66)
GROUPS = ('a', 'a', 'a', 'b', 'b', 'b', 'b')
F, M = 40, 300


@functools.lru_cache(maxsize=None)
def data(duplicate=False, seed=0):
    """2 subjects of 3 and 4 runs, T 57 .. 80, F = 40, M = 300: ``(runs float32, features float64)``.  Planted weights at half
    the vertices, unit noise, mean 100, vertex CONSTANT_VERTEX constant in time.  ``duplicate``: column 5 is a copy of column
    2 (rank-deficient)."""
    rng = np.random.RandomState(seed)
    W = np.zeros((F, M))
    W[:, ::2] = 0.25 * rng.randn(F, M // 2)
    runs, feats = [], []
    for T in LENGTHS:
        X = rng.randn(T, F) + rng.randn(F)                      # (the columns have means of their own: centring matters)
        if duplicate:
            X[:, 5] = X[:, 2]
        Y = 100.0 + X @ W + rng.randn(T, M)
        Y[:, CONSTANT_VERTEX] = 100.0
        runs.append(Y.astype(np.float32))
        feats.append(X)
    for a in runs + feats:
        a.setflags(write=False)
    return tuple(runs), tuple(feats)


def members():
    keys = sorted(set(GROUPS), key=GROUPS.index)
    return [[r for r, g in enumerate(GROUPS) if g == k] for k in keys]


def _centre(a):
    a = np.asarray(a, np.float64)
    return a - a.mean(axis=0)


def _solve(X, Y, alpha):
    if alpha == 0:
        return np.linalg.lstsq(X, Y, rcond=None)[0]
    return np.linalg.solve(X.T @ X + alpha * np.eye(X.shape[1]), X.T @ Y)


def yardstick(runs, feats, alphas, mem, folds=None, fit=_solve):
    """One subject (the runs ``mem``) by the explicit route -> a dict: ``r2`` / ``r`` / ``scale`` float64 [folds, A, M] per
    fold, ``weights`` float64 [A, F, M] the refit on all the runs at every penalty.  ``folds``: held-out sets of positions
    (default: leave one run out).  ``fit(X, Y, alpha)`` solves one training set."""
    Xc = [_centre(feats[r]) for r in mem]
    Yc = [_centre(runs[r]) for r in mem]
    yy = [(np.asarray(runs[r], np.float64) ** 2).sum(axis=0) for r in mem]
    folds = [[i] for i in range(len(mem))] if folds is None else folds
    A = len(alphas)
    shape = (len(folds), A, Yc[0].shape[1])
    out = dict(r2=np.zeros(shape), r=np.zeros(shape), scale=np.zeros(shape))
    for f, test in enumerate(folds):
        train = [i for i in range(len(mem)) if i not in test]
        Xtr, Ytr = np.concatenate([Xc[i] for i in train]), np.concatenate([Yc[i] for i in train])
        Xte, Yte = np.concatenate([Xc[i] for i in test]), np.concatenate([Yc[i] for i in test])
        tss = (Yte * Yte).sum(axis=0)
        live = tss > 0
        den = np.where(live, tss, 1.0)
        for a, alpha in enumerate(alphas):
            pred = Xte @ fit(Xtr, Ytr, alpha)
            res = Yte - pred
            q = (pred * pred).sum(axis=0)
            p = (pred * Yte).sum(axis=0)
            out['r2'][f, a] = np.where(live, 1.0 - (res * res).sum(axis=0) / den, 0.0)
            ok = live & (q > 0)
            out['r'][f, a] = np.where(ok, p / np.sqrt(np.where(ok, tss * q, 1.0)), 0.0)
            out['scale'][f, a] = np.where(live, (sum(yy[i] for i in test) + np.abs(p) + q) / den, np.inf)
    Xall, Yall = np.concatenate(Xc), np.concatenate(Yc)
    out['weights'] = np.stack([fit(Xall, Yall, alpha) for alpha in alphas])
    return out


@functools.lru_cache(maxsize=None)
def reference(duplicate=False):
    """The yardstick of both subjects of ``data(duplicate)`` under leave-one-run-out, computed once: a list of dicts."""
    runs, feats = data(duplicate)
    alphas = np.concatenate([[0.0], ALPHAS]) if duplicate else ALPHAS
    return [yardstick(runs, feats, alphas, mem) for mem in members()]


def case_alphas(duplicate):
    return np.concatenate([[0.0], ALPHAS]) if duplicate else ALPHAS


def mean_and_choice(values):
    """The mean over the folds and, per vertex, the best penalty and whether the choice is DECIDED: the best and the second-best
    mean differ by more than 1e-9."""
    mean = values.mean(axis=0)
    order = np.sort(mean, axis=0)
    decided = (order[-1] - order[-2] > 1e-9) if mean.shape[0] > 1 else np.ones(mean.shape[1], bool)
    return mean, mean.argmax(axis=0), decided


def weights_bound(feats, mem, alpha, ref):
    """The forward error of a backward-stable solve of the refit: ``64 F 2^-53 cond max|w|``, ``cond`` the condition number of
    ``X^T X + alpha I`` on its range (both routes solve that system; neither can do better than its condition allows), plus the
    one float32 rounding."""
    lam = np.linalg.eigvalsh(sum(_centre(feats[r]).T @ _centre(feats[r]) for r in mem))
    lam = lam[lam > lam.max() * len(lam) * 2.0 ** -52] + alpha
    return 64 * len(lam) * 2.0 ** -53 * (lam.max() / lam.min()) * np.abs(ref).max() + 2.0 ** -23 * np.abs(ref)


def check_result(res, duplicate, kind, folds=None, shared=False):
    """An ``EncodingResult`` with ``scores`` and ``weights`` (NumPy) of ``data(duplicate)`` against the yardstick: every mean
    score within ``C_BOUND`` times the mean of the folds' scales plus one float32 rounding, the selection wherever the yardstick's
    is decided (at most 1 % of the vertices excused), the refit.  Returns the largest fraction of the score bound used."""
    runs, feats = data(duplicate)
    alphas = case_alphas(duplicate)
    refs = reference(duplicate) if folds is None else [yardstick(runs, feats, alphas, mem, f) for mem, f in zip(members(), folds)]
    used = 0.0
    for s, (mem, ref) in enumerate(zip(members(), refs)):
        mean, best, decided = mean_and_choice(ref[kind])
        scale = ref['scale'].mean(axis=0)
        live = np.isfinite(scale)
        assert not live[:, CONSTANT_VERTEX].any() and live.sum() == live.size - live.shape[0]
        got = np.asarray(res.scores[s], np.float64)
        assert np.isfinite(got).all() and (got[:, CONSTANT_VERTEX] == 0).all()
        bound = C_BOUND * scale[live] + 2.0 ** -23 * np.abs(mean[live])
        err = np.abs(got - mean)[live]
        print('subject %d %s: worst error %.3e, %.3g of its bound' % (s, kind, err.max(), (err / bound).max()))
        assert (err <= bound).all()
        used = max(used, float((err / bound).max()))
        index = np.asarray(res.alpha_index[s])
        if shared:
            a = int(np.argmax(np.asarray(res.scores[s], np.float32).astype(np.float64).mean(axis=1)))
            assert (index == a).all()
            full = mean.mean(axis=1)
            if np.sort(full)[-1] - np.sort(full)[-2] > 1e-9:
                assert a == int(full.argmax())
        else:
            assert (~decided).mean() <= 0.01                    # (a condition of the test, not a measurement)
            assert np.array_equal(index[decided], best[decided])
        assert np.array_equal(np.asarray(res.score[s]), np.asarray(res.scores[s])[index, np.arange(len(index))])
        for a in np.unique(index):
            cols = index == a
            err = np.abs(np.asarray(res.weights[s], np.float64) - ref['weights'][a])
            assert (err <= weights_bound(feats, mem, alphas[a], ref['weights'][a]))[:, cols].all()
    return used
