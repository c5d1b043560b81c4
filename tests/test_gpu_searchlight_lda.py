"""``searchlight.searchlight(classifier='lda')`` on the device (chebgcn_searchlight_fit, then chebgcn_searchlight_lda per bucket
of row length and batch of centres) against its float64 host restatement ``searchlight.searchlight_host``, which slices every
ball out, forms the residuals with NumPy and solves with SciPy's Cholesky.  Shapes come from ``ops.searchlight_lda_geometry()``.

The bound, for EVERY score:  ``|got - ref| <= B scale``,  ``scale = kappa (|log prior| + |d . w| / 2 + sum_v |w_v| |x_v - m_v|)``
from the reference, ``kappa`` the 2-norm condition number of that (model, centre)'s ``Sigma``: the magnitude a float64 solve may
be off by.  ``B = BOUND`` is set near 10x the worst ratio measured on an MI355X against the host restatement -- float64
round-off and nothing else (the two sides sum the covariance in different orders and factorise with different kernels).  A
covariance accumulated in float32 misses the bound by more than 100x on the P = 127, g = 0.01 rows at mean 1e4 / sd 50
(asserted on the CPU in the parity test).  Predictions, and with them ``correct``, must agree wherever the reference's top-two
margin exceeds twice the bound; at most 1e-3 of the (sample, centre) pairs may be left out that way.  ``recall`` and
``accuracy`` are float64 quotients of the counts rounded once, exactly.

``B = 3e-13``.  Measured on an MI355X (``record_measured`` keeps every case's figures), as fractions of ``scale``: worst 2.66e-14
(the uneven folds: training sets of up to 578 samples at mean / sd = 100, where the class means -- a plain chain on the device,
pairwise sums in NumPy -- carry the difference), at most 8.5e-16 in every other case (3.6e-16 on the edge rows at mean 1e4 /
sd 50, kappa up to 555); no (sample, centre) pair is left out in any case; the reference's least top-two margin is 4.5e-10 of
``scale`` (g = 1e-6 on a partly-zero ball), 4.6e-8 on the parity data.  The float32 covariance misses the bound by 3.1e4.  The
shrinkage the kernel reports agrees with ``lda_shrinkage_host`` to 1.0e-15 relative, and exactly where the rule clips.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, events, lda_shrinkage_host, searchlight as sl

pytestmark = pytest.mark.gpu

BOUND = 3e-13
LEFT_OUT = 1e-3
EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128]                   # every bucket at its edges


@pytest.fixture(scope='module')
def geo():
    from gcn_fmri_decoding_amd import ops
    g = ops.searchlight_lda_geometry()
    assert [g['buckets'][P] for P in EDGES] == [32, 32, 32, 64, 64, 64, 128, 128, 128] and g['max_P'] == sl.LDA_PMAX
    return g


def data(rng, S, M, C, mean=100.0, sd=1.0, folds=4, stride=1, common=0.0):
    """Balanced classes whose means differ by 0.5 sd per vertex; every (fold, class) cell holds S / (folds C) samples, spread
    evenly over ``stride`` interleaved groups.  ``common``: the sd (in units of sd) of one noise all vertices share."""
    y = np.arange(S) // stride % C
    fold = np.arange(S) // (stride * C) % folds
    X = (mean + sd * rng.randn(S, M) + common * sd * rng.randn(S, 1) + 0.5 * sd * rng.randn(C, M)[y]).astype(np.float32)
    return X, y, fold


def rows_of(M, lengths, step=7):
    """Row i: ``lengths[i]`` consecutive vertices from ``step * i``."""
    r = sp.lil_matrix((len(lengths), M))
    for i, P in enumerate(lengths):
        assert step * i + P <= M
        r[i, step * i:step * i + P] = 1
    return r.tocsr()


def ring(M, hops=1):
    from gcn_fmri_decoding_amd import graph
    i = np.arange(M)
    A = sp.csr_matrix((np.ones(2 * M), (np.concatenate([i, i]), np.concatenate([(i + 1) % M, (i - 1) % M]))), shape=(M, M))
    return graph.hop_balls(A, hops)


def launches_of(nb, geo, batch=None):
    """The buckets of the launches one call makes, in order: the buckets ascending, each cut into batches of centres."""
    of_row = [geo['buckets'][int(n)] for n in np.diff(nb.indptr)]
    out = []
    for b in sorted(set(of_row)):
        n = of_row.count(b)
        out += [b] * (1 if batch is None else -(-n // min(batch, n)))
    return out


def run_device(args, kw, launches, head=()):
    """``searchlight`` (or ``searchlight_events``) with ``classifier='lda'`` and the dispatch log checked: exactly the fit, then
    one ``searchlight_lda`` per (bucket, batch) on the bucket's arm."""
    kw = dict(kw)
    fn = kw.pop('fn', sl.searchlight)
    _lib.dispatch_log = log = []
    try:
        res = fn(*args, classifier='lda', **kw)
    finally:
        _lib.dispatch_log = None
    assert [w for w, _ in log] == list(head) + ['searchlight_fit'] + ['searchlight_lda'] * len(launches), log
    assert [d for w, d in log if w.startswith('searchlight')] == ['searchlight_fit_kernel'] + ['searchlight_lda_kernel<%d>' % b for b in launches]
    return res


def against_host(name, args, kw, geo, batch=None):
    """Device against host the way the module's docstring states it; returns ``(device result, host result, scale)``."""
    kw = dict(kw)
    ref, scale = sl.searchlight_host(*args, scores=True, predictions=True, return_scale=True, classifier='lda', **kw)
    C = len(ref.classes)
    nb = sp.csr_matrix(args[2])
    res = run_device(args, dict(kw, scores=True, predictions=True, batch_centres=batch), launches_of(nb, geo, batch))
    S, U = ref.predictions.shape
    assert res.scores.shape == ref.scores.shape == (S, C, U) and res.scores.dtype == np.float64 and np.isfinite(res.scores).all()
    assert res.predictions.dtype == np.uint8 and res.correct.dtype == np.int32 and res.support.dtype == np.int64
    assert res.recall.dtype == res.accuracy.dtype == np.float32 and res.groups == ref.groups and res.classes == ref.classes
    bound = BOUND * scale
    frac = float((np.abs(res.scores - ref.scores) / (bound + 1e-300)).max())
    top = np.sort(ref.scores, axis=1)
    decided = top[:, -1, :] - top[:, -2, :] > 2.0 * bound.max(axis=1)
    left = float((~decided).mean())
    margin = float(((top[:, -1, :] - top[:, -2, :]) / scale.max(axis=1)).min())
    record_measured(name, bound_used=frac, left_out=left, least_margin=margin)
    print(name, 'scores at %.3g of the bound (%.3g of scale), %.3g left out, least margin %.3g of scale' % (frac, frac * BOUND, left, margin))
    assert frac <= 1.0, '%s: a score is off by %.3f of its bound' % (name, frac)
    assert left <= LEFT_OUT, left
    assert np.array_equal(res.predictions[decided], ref.predictions[decided])
    G = len(ref.groups)
    gidx = np.array([ref.groups.index(g) for g in kw.get('groups', [0] * S)])
    y = np.array([ref.classes.index(v) for v in np.asarray(args[1]).tolist()])
    counts = np.zeros((G, C, U), np.int32)
    np.add.at(counts, (gidx[:, None], y[:, None], np.arange(U)[None, :]), (res.predictions == y[:, None]).astype(np.int32))
    assert np.array_equal(res.correct, counts)                  # the atomics count what the predictions say
    if decided.all():
        assert np.array_equal(res.correct, ref.correct)
    assert np.array_equal(res.support, ref.support)
    s = res.support.astype(np.float64)
    assert np.array_equal(res.recall, (res.correct / np.where(s > 0, s, 1.0)[:, :, None]).astype(np.float32))
    assert np.array_equal(res.accuracy, (res.correct.sum(axis=1) / s.sum(axis=1)[:, None]).astype(np.float32))
    return res, ref, scale


def ball_scores(A, ytr, T, g, acc):
    """Scores of one (training set, ball) with the covariance accumulated in ``acc`` precision; everything else float64."""
    import scipy.linalg
    C = int(ytr.max()) + 1
    n = np.bincount(ytr, minlength=C).astype(np.float64)
    mu = np.stack([A[ytr == c].mean(axis=0) for c in range(C)])
    m = (n[:, None] * mu).sum(axis=0) / n.sum()
    R = (A - mu[ytr]).astype(acc)
    S = (R.T @ R).astype(np.float64) / n.sum()
    Sigma = (1.0 - g) * S + g * np.trace(S) / A.shape[1] * np.eye(A.shape[1])
    w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Sigma, lower=True), (mu - m).T).T
    return np.log(n / n.sum()) - 0.5 * ((mu - m) * w).sum(axis=1) + (T - m) @ w.T


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mean,sd', [(100.0, 1.0), (1e4, 50.0), (0.0, 1.0)])
@pytest.mark.parametrize('g', [0.01, 0.1])
def test_parity_on_rows_at_the_bucket_edges(mean, sd, g, geo):
    """72 training samples for up to 128 vertices: S is singular from P = 70 on, the normal case."""
    rng = np.random.RandomState(int(mean) + 1)
    X, y, fold = data(rng, 96, 200, 3, mean, sd)
    nb = rows_of(200, EDGES)
    res, ref, scale = against_host('searchlight_lda_parity_mean%g_g%g' % (mean, g), (X, y, nb, fold), dict(shrinkage=g), geo)
    assert res.correct.shape == (1, 3, 9) and res.support.tolist() == [[32, 32, 32]]
    if mean == 1e4 and g == 0.01:                               # the same covariance summed in float32 misses the bound by > 100x
        u = EDGES.index(127)
        cols = np.arange(7 * u, 7 * u + 127)
        X64 = X.astype(np.float64)
        tr, te = fold != 0, fold == 0
        s64 = ball_scores(X64[tr][:, cols], y[tr], X64[te][:, cols], g, np.float64)
        s32 = ball_scores(X64[tr][:, cols], y[tr], X64[te][:, cols], g, np.float32)
        assert (np.abs(s64 - ref.scores[te, :, u]) <= BOUND * scale[te, :, u]).all()
        miss = float((np.abs(s32 - s64) / (BOUND * scale[te, :, u])).max())
        record_measured('searchlight_lda_float32_covariance', misses_by=miss)
        assert miss >= 100.0, miss


def test_one_call_equals_one_call_per_row_and_any_batching(geo):
    rng = np.random.RandomState(2)
    X, y, fold = data(rng, 96, 200, 3, 1e4, 50.0)
    lengths = [128, 1, 64, 33, 31, 2, 3, 127, 32, 4, 5, 65, 63, 6, 7, 8, 9]        # eleven rows in bucket 32, three in the others
    nb = rows_of(200, lengths, step=4)
    kw = dict(shrinkage=0.01, scores=True, predictions=True)
    whole = run_device((X, y, nb, fold), kw, [32, 64, 128])
    for b, launches in ((1, [32] * 11 + [64] * 3 + [128] * 3), (7, [32, 32, 64, 128])):
        assert launches == launches_of(nb, geo, b)
        part = run_device((X, y, nb, fold), dict(kw, batch_centres=b), launches)
        for name in ('scores', 'predictions', 'correct', 'recall', 'accuracy'):
            assert np.array_equal(getattr(part, name), getattr(whole, name)), (b, name)
    for u, P in enumerate(lengths):
        if P in EDGES:
            alone = run_device((X, y, nb[u], fold), kw, [geo['buckets'][P]])
            assert np.array_equal(alone.scores[:, :, 0], whole.scores[:, :, u]), P
            assert np.array_equal(alone.correct[:, :, 0], whole.correct[:, :, u]), P
    back = run_device((X, y, nb[::-1], fold), kw, [32, 64, 128])                # the centres in another order
    assert np.array_equal(back.scores[:, :, ::-1], whole.scores) and np.array_equal(back.correct[:, :, ::-1], whole.correct)


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------

def test_one_vertex(geo):
    X, y, fold = data(np.random.RandomState(10), 64, 1, 2)
    against_host('searchlight_lda_M1', (X, y, sp.csr_matrix(np.ones((1, 1))), fold), {}, geo)


def test_models_of_1_63_64_65_129_and_257_test_samples(geo):
    """Uneven folds around the wave (64) and the scoring pass (``threads`` = 256 test samples)."""
    sizes = [1, 63, 64, 65, 129, geo['threads'] + 1]
    S, M = sum(sizes), 33
    X, y, _ = data(np.random.RandomState(11), S, M, 2)
    fold = np.repeat(np.roll(np.arange(len(sizes)), 1), sizes)      # (the models are numbered by fold: their columns are reordered)
    assert S % 32 and geo['threads'] == 256
    res, _, _ = against_host('searchlight_lda_uneven_folds', (X, y, ring(M, 1)[::4], fold), {}, geo)
    assert res.support.sum() == S


@pytest.mark.parametrize('C', ['2', '9', 'Cmax'])
def test_class_counts_in_every_bucket(C, geo):
    """2 classes: the narrow class tables; 9 and 32: the wide ones, in each ball bucket."""
    C = geo['max_C'] if C == 'Cmax' else int(C)
    assert (C <= geo['narrow']) == (C == 2) and geo['max_C'] == 32
    X, y, fold = data(np.random.RandomState(C), 4 * C, 70, C, folds=2)
    res, _, _ = against_host('searchlight_lda_C%d' % C, (X, y, rows_of(70, [3, 40, 70], step=0), fold), {}, geo)
    assert res.correct.shape == (1, C, 3) and res.support.tolist() == [[4] * C]


def test_nan_in_the_pad_of_the_patterns_stays_there(geo):
    import torch
    X, y, fold = data(np.random.RandomState(14), 45, 33, 3, folds=3)
    balls = ring(33, 2)
    res = run_device((X, y, balls, fold), dict(scores=True), [32])
    a = sl._check(X, y, balls, fold, None, True, None, True, False, None, 't', classifier='lda')
    from gcn_fmri_decoding_amd import ops
    plan = sl._device_plan(a, ops.searchlight_geometry()['buckets'][3])
    dev = torch.device('cuda')
    Xt = sl._transposed(torch.as_tensor(X).to(dev), plan.order, dev)
    assert Xt.shape == (33, 64)
    Xt[:, 45:] = float('nan')
    correct, sc, _ = sl._run_lda(a, plan, Xt, True, False, None)
    assert np.array_equal(sc.cpu().numpy(), res.scores) and np.array_equal(correct.cpu().numpy(), res.correct)


# ---- 3. groups ------------------------------------------------------------------------------------------------------------------

def test_three_groups_of_two_folds(geo):
    import torch
    rng = np.random.RandomState(20)
    S, M = 108, 40
    X, y, fold = data(rng, S, M, 3, mean=1000.0, sd=5.0, folds=2, stride=3)
    groups = ['s2', 's1', 's3'] * (S // 3)                      # every (group, fold, class) cell holds 6 samples
    fold = fold + 4
    balls = sp.vstack([ring(M, 2)[::5], rows_of(M, [40], step=0)]).tocsr()
    res, ref, _ = against_host('searchlight_lda_groups_within', (X, y, balls, fold), dict(groups=groups), geo)
    assert res.groups == ['s2', 's1', 's3'] and res.correct.shape == (3, 3, 9) and res.support.tolist() == [[12] * 3] * 3
    for g, key in enumerate(res.groups):                        # a group alone: the same bits
        own = np.array([k == key for k in groups])
        alone = run_device((X[own], y[own], balls, fold[own]), dict(scores=True), [32, 64])
        assert np.array_equal(alone.scores, res.scores[own]) and np.array_equal(alone.correct[0], res.correct[g])
    across, _, _ = against_host('searchlight_lda_groups_across', (X, y, balls, fold), dict(groups=groups, within=False), geo)
    assert across.correct.shape == (3, 3, 9) and not np.array_equal(across.scores, res.scores)
    tens = run_device((torch.as_tensor(X).cuda(), y, balls, fold), dict(groups=groups, scores=True, predictions=True), [32, 64])
    assert all(torch.is_tensor(v) and v.is_cuda for v in (tens.correct, tens.recall, tens.accuracy, tens.scores, tens.predictions))
    assert isinstance(tens.support, np.ndarray) and tens.recall.dtype == torch.float32 and tens.correct.dtype == torch.int32
    for name in ('correct', 'recall', 'accuracy', 'scores', 'predictions'):
        assert np.array_equal(getattr(tens, name).cpu().numpy(), getattr(res, name)), name


# ---- 4. ties and degenerate balls -----------------------------------------------------------------------------------------------

def test_duplicate_classes_tie_to_the_lower_class(geo):
    rng = np.random.RandomState(30)
    half, _, fold = data(rng, 48, 30, 1, folds=3)
    X = np.concatenate([half, half])                            # classes 1 and 2 hold the same samples in every fold
    y = np.repeat([2, 1], 48)
    res = run_device((X, y, ring(30, 2), np.concatenate([fold, fold])), dict(scores=True, predictions=True), [32])
    assert res.classes == [1, 2] and np.array_equal(res.scores[:, 0], res.scores[:, 1]) and np.isfinite(res.scores).all()
    assert (res.predictions == 0).all() and (res.recall[0, 0] == 1).all() and (res.recall[0, 1] == 0).all()
    assert (res.accuracy == 0.5).all() and np.array_equal(res.correct[0, 0], np.full(30, 48, np.int32))


@pytest.mark.parametrize('g', [1e-6, 0.1, 1, 'auto'])
def test_all_zero_and_partly_zero_balls(g, geo):
    rng = np.random.RandomState(41)
    S, M = 60, 40
    X, y, fold = data(rng, S, M, 2, folds=3)
    y = np.where(np.arange(S) % 5 == 0, 1, y)                   # class 1 is the more frequent one in every training set
    X[:, 20:] = 0.0
    nb = sp.vstack([rows_of(M, [6, 20], step=0), rows_of(M, [20], step=0)[:, ::-1], rows_of(M, [34], step=0)[:, ::-1]]).tocsr()
    res, ref, _ = against_host('searchlight_lda_zero_balls_g%s' % g, (X, y, nb, fold), dict(shrinkage=g), geo)
    assert np.isfinite(res.scores).all() and (res.predictions[:, 2] == 1).all()     # an all-zero ball: the prior decides
    assert np.array_equal(res.scores[:, :, 2], ref.scores[:, :, 2])                 # exactly log prior
    assert (res.recall[0, 1, 2] == 1) and (res.recall[0, 0, 2] == 0)
    assert not np.array_equal(res.scores[:, :, 3], res.scores[:, :, 2])             # 14 live vertices among 20 zero ones speak


# ---- 5. arms --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw', [dict(priors='uniform'), dict(shrinkage=1), dict(shrinkage=1, priors='uniform')],
                         ids=['uniform', 'full_shrinkage', 'full_shrinkage_uniform'])
def test_uniform_priors_and_full_shrinkage(kw, geo):
    rng = np.random.RandomState(40)
    S, M = 90, 70
    X, y, fold = data(rng, S, M, 3, folds=3, common=2.0)
    y = np.where(np.arange(S) % 7 == 0, 0, y)                   # unbalanced: the empirical prior matters
    nb = rows_of(M, [5, 40, 70], step=0)
    res, ref, _ = against_host('searchlight_lda_' + '_'.join('%s' % v for v in kw.values()), (X, y, nb, fold), kw, geo)
    plain = sl.searchlight_host(X, y, nb, fold, scores=True, classifier='lda')
    assert not np.allclose(ref.scores, plain.scores, rtol=1e-6, atol=0)


def test_ledoit_wolf_shrinkage(geo):
    """``shrinkage='auto'``: the scores against the host, and the shrinkage the kernel used (``gamma_out``) against
    ``lda_shrinkage_host`` on the residuals of every (model, centre) to 1e-10 relative: rows with a common factor (g inside
    (0, 1)), a row of 5 vertices on which one sample is a 1000-sd outlier (the models trained on it: beta / delta is about
    (1 - 1 / n) / (1 - 1 / P) > 1, so beta is cut to delta and g = 1) and an all-zero row (beta = 0: g = 0, clipped to
    ``SHRINK_MIN``).  Where the rule clips, the device gives the limit exactly."""
    import torch
    from gcn_fmri_decoding_amd import ops
    rng = np.random.RandomState(42)
    S, M, C = 96, 230, 3
    X, y, fold = data(rng, S, M, C, 1e4, 50.0)
    y = np.where(np.arange(S) % 7 == 0, 0, y)                   # unbalanced: on the all-zero row the prior decides, without a tie
    X[:, :110] += (100.0 * rng.randn(S, 1)).astype(np.float32)                    # vertices 0 .. 109 share one strong noise
    X[0, 115:120] += 5e4                                        # sample 0 (fold 0): an outlier on vertices 115 .. 119
    X[:, 225:] = 0.0
    spans = [(0, 5), (0, 40), (0, 100), (115, 120), (225, 230)]
    nb = sp.csr_matrix(np.array([[float(lo <= v < hi) for v in range(M)] for lo, hi in spans]))
    against_host('searchlight_lda_auto', (X, y, nb, fold), dict(shrinkage='auto'), geo)
    a = sl._check(X, y, nb, fold, None, True, None, False, False, None, 't', classifier='lda', shrinkage='auto')
    assert a.shrink < 0
    plan = sl._device_plan(a, ops.searchlight_geometry()['buckets'][C])
    dev = torch.device('cuda')
    _, _, _, gam = sl._run_lda(a, plan, sl._transposed(torch.as_tensor(X).to(dev), plan.order, dev), False, False, None, gamma=True)
    gam = gam.cpu().numpy()
    assert gam.shape == (4, 5)
    X64 = X.astype(np.float64)
    worst, clipped = 0.0, set()
    for f in range(4):                                          # model f tests fold f
        tr = fold != f
        for u in range(5):
            A = X64[tr][:, nb[u].indices]
            mu = np.stack([A[y[tr] == c].mean(axis=0) for c in range(C)])
            want = lda_shrinkage_host(A - mu[y[tr]])
            worst = max(worst, abs(gam[f, u] - want) / want)
            if want in (sl.SHRINK_MIN, 1.0):
                assert gam[f, u] == want, (f, u, want, gam[f, u])
                clipped.add((u, want))
            else:
                assert u < 4, (u, want)
    record_measured('searchlight_lda_gamma', rel=worst)
    assert worst <= 1e-10, worst
    assert clipped == {(3, 1.0), (4, sl.SHRINK_MIN)}, clipped


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------

def test_searchlight_events_end_to_end(geo):
    import torch
    rng = np.random.RandomState(60)
    M, dura = 40, 4
    names = ['rest'] * 3 + ['a'] * 8 + ['rest'] * 2 + ['b'] * 9 + ['rest'] * 3 + ['a'] * 5 + ['rest'] + ['b'] * 8 + ['rest'] * 2
    T = len(names)
    subjects = ['s1', 's1', 's2', 's2']
    labels = [names, names[::-1], names, names[::-1]]
    # vertices 10 .. 19 share a large noise; b moves the even ones against the odd ones: nothing for a classifier without covariance
    sign = np.where(np.arange(M) % 2 == 0, 1.0, -1.0) * ((np.arange(M) >= 10) & (np.arange(M) < 20))
    runs = [(1000.0 + 0.5 * rng.randn(T, M) + 30.0 * rng.randn(T, 1) * (sign != 0) + 1.0 * sign * np.array([float(n == 'b') for n in run])[:, None]
             ).astype(np.float32) for run in labels]
    balls = ring(M, 2)
    ev = events.match_events(labels, ['a', 'b'], dura)
    want = np.concatenate([events.host_windows(runs[r], i, fold=dura)[:, :, 0] for r, i in zip(ev.kept, ev.index)])
    idx, lab, tg, tf, classes = sl._events_plan([T] * 4, labels, ['a', 'b'], dura, subjects, None, True, {})
    kw = dict(groups=subjects, shrinkage=0.01)
    res = run_device((runs, labels, ['a', 'b'], dura, balls), dict(kw, fn=sl.searchlight_events, scores=True), [32],
                     head=['gather_windows_indexed'])
    direct = run_device((want, lab, balls, tf), dict(groups=tg, classes=classes, shrinkage=0.01, scores=True), [32])
    assert res.groups == ['s1', 's2'] and res.classes == ['a', 'b'] and isinstance(res.correct, np.ndarray)
    for name in ('scores', 'correct', 'recall', 'accuracy', 'support'):
        assert np.array_equal(getattr(res, name), getattr(direct, name)), name
    host = sl.searchlight_host(want, lab, balls, tf, groups=tg, classes=classes, classifier='lda', shrinkage=0.01)
    assert np.abs(res.correct - host.correct).max() <= 1
    gnb = sl.searchlight_host(want, lab, balls, tf, groups=tg, classes=classes)
    print('accuracy inside the patch: lda %.3f, naive Bayes %.3f; outside: lda %.3f' % (
        res.accuracy[:, 12:18].mean(), gnb.accuracy[:, 12:18].mean(), res.accuracy[:, 24:].mean()))
    assert res.accuracy[:, 12:18].mean() > 0.8 > 0.7 > max(res.accuracy[:, 24:].mean(), gnb.accuracy[:, 12:18].mean())
    tens = run_device(([torch.as_tensor(r).cuda() for r in runs], labels, ['a', 'b'], dura, balls), dict(kw, fn=sl.searchlight_events), [32],
                      head=['gather_windows_indexed'])
    assert torch.is_tensor(tens.recall) and np.array_equal(tens.recall.cpu().numpy(), res.recall) and tens.scores is None


# ---- 7. naive Bayes is what it was ----------------------------------------------------------------------------------------------

def test_gnb_logs_the_dispatches_it_logged(geo):
    X, y, fold = data(np.random.RandomState(70), 48, 10, 3, folds=2)
    for kw in ({}, dict(classifier='gnb'), dict(classifier='gnb', shrinkage=0.1)):
        _lib.dispatch_log = log = []
        try:
            sl.searchlight(X, y, ring(10, 1), fold, batch_centres=4, **kw)
        finally:
            _lib.dispatch_log = None
        score = 'searchlight_base_kernel + searchlight_score_kernel<4>'
        assert log == [('searchlight_spread', 'searchlight_spread_kernel'), ('searchlight_fit', 'searchlight_fit_kernel'),
                       ('searchlight_score', score), ('searchlight_score', score), ('searchlight_score', score)]
