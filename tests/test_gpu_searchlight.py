"""``searchlight.searchlight`` on the device (chebgcn_searchlight_spread / _fit / _score) against its float64 host restatement
``searchlight.searchlight_host``, which slices every ball out and fits it on its own.  Shapes come from
``ops.searchlight_geometry()``.

The bound, for EVERY score:  ``|got - ref| <= 1e-10 scale``,  ``scale = |log prior| + sum_v [(x - mu)^2 / (2 var) + |log(2 pi var) / 2|]``
from the reference -- the worst-case float64 propagation at these inputs with about 10x margin: a mean is off by at most
``n 2^-53 max|x|`` and enters a term as ``2 |t| delta / (2 var)``; at mean 1e4, sd 50, n = 72 that is 1.6e-11 of a term of size 1.
An expanded quadratic ``a x^2 + b x + d`` or any float32 accumulation misses it by orders of magnitude on the second data set.
Predictions, and with them ``correct``, must agree wherever the reference's top-two margin exceeds twice the bound; at most
1e-3 of the (sample, centre) pairs may be left out that way.  ``recall`` and ``accuracy`` are float64 quotients of the counts
rounded once, exactly.

Measured on an MI355X (``record_measured`` keeps every case's figures), as fractions of the bound: scores at most 3.7e-5 (on the
row of 1000 vertices; 6.5e-6 everywhere else) -- float64 round-off and nothing else; no (sample, centre) pair is left out in any
case; the reference's least top-two margin is 1.2e-8 of ``scale`` (32 classes), 1.6e-6 on the second parity data set.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, events, graph, searchlight as sl
from gcn_fmri_decoding_amd.runs import stage

pytestmark = pytest.mark.gpu

BOUND = 1e-10
LEFT_OUT = 1e-3


@pytest.fixture(scope='module')
def geo():
    from gcn_fmri_decoding_amd import ops
    return ops.searchlight_geometry()


def ring(M, hops=1):
    i = np.arange(M)
    A = sp.csr_matrix((np.ones(2 * M), (np.concatenate([i, i]), np.concatenate([(i + 1) % M, (i - 1) % M]))), shape=(M, M))
    return graph.hop_balls(A, hops)


def data(rng, S, M, C, mean=100.0, sd=1.0, folds=4, stride=1):
    """Balanced classes whose means differ by 0.5 sd per vertex; every (fold, class) cell holds S / (folds C) samples, spread
    evenly over ``stride`` interleaved groups."""
    y = np.arange(S) // stride % C
    fold = np.arange(S) // (stride * C) % folds
    X = (mean + sd * rng.randn(S, M) + 0.5 * sd * rng.randn(C, M)[y]).astype(np.float32)
    return X, y, fold


def arm(C, geo):
    return 'searchlight_base_kernel + searchlight_score_kernel<%d>' % geo['buckets'][C]


def run_device(args, kw, geo, batches=1, head=()):
    """``searchlight`` (or ``searchlight_events``) with the dispatch log checked: exactly spread, fit and one score per batch of
    centres, on the arm of the class count."""
    fn = kw.pop('fn', sl.searchlight)
    C = kw.pop('C')
    _lib.dispatch_log = log = []
    try:
        res = fn(*args, **kw)
    finally:
        _lib.dispatch_log = None
    assert [w for w, _ in log] == list(head) + ['searchlight_spread', 'searchlight_fit'] + ['searchlight_score'] * batches, log
    assert [d for w, d in log if w.startswith('searchlight')] == ['searchlight_spread_kernel', 'searchlight_fit_kernel'] + [arm(C, geo)] * batches
    return res


def against_host(name, args, kw, geo, batches=1):
    """Device against host the way the module's docstring states it; returns ``(device result, host result)``."""
    kw = dict(kw)
    ref, scale = sl.searchlight_host(*args, scores=True, predictions=True, return_scale=True, **kw)
    C = len(ref.classes)
    res = run_device(args, dict(kw, scores=True, predictions=True, C=C), geo, batches)
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
    print(name, 'scores at %.3g of the bound, %.3g left out, least margin %.3g of scale' % (frac, left, margin))
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
    return res, ref


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mean,sd', [(100.0, 1.0), (1e4, 50.0), (0.0, 1.0)])
def test_parity_on_two_hop_balls(mean, sd, geo):
    rng = np.random.RandomState(int(mean) + 1)
    X, y, fold = data(rng, 96, 200, 3, mean, sd)
    res, ref = against_host('searchlight_parity_mean%g' % mean, (X, y, ring(200, 2), fold), {}, geo)
    assert res.correct.shape == (1, 3, 200) and res.support.tolist() == [[32, 32, 32]]
    if mean == 1e4:                                             # the same sums in float32 miss the bound by orders of magnitude
        x32 = X[fold != 0][y[fold != 0] == 0]
        mu32 = x32.mean(axis=0, dtype=np.float32)
        mu64 = x32.astype(np.float64).mean(axis=0)
        t = X[0].astype(np.float64) - mu64
        assert (np.abs(mu32 - mu64) * 2 * np.abs(t) / (2 * 50.0 ** 2)).max() > 100 * BOUND


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------

def test_one_vertex(geo):
    X, y, fold = data(np.random.RandomState(10), 64, 1, 2)
    against_host('searchlight_M1', (X, y, sp.csr_matrix(np.ones((1, 1))), fold), {}, geo)


@pytest.mark.parametrize('C', [2, 9])
def test_models_of_1_63_64_and_65_test_samples(C, geo):
    """Uneven folds around the tile, in a narrow class bucket (a lane owns ``per_lane`` samples) and in a wide one (one)."""
    T = geo['tile']
    per_lane = geo['per_lane'][geo['buckets'][C]]
    assert per_lane == (2 if C == 2 else 1)
    sizes = sorted({n for k in range(1, per_lane + 1) for n in (k * T - 1, k * T, k * T + 1)} | {1})
    S, M = sum(sizes), 33
    rng = np.random.RandomState(11)
    X, y, _ = data(rng, S, M, C)
    fold = np.repeat(np.roll(np.arange(len(sizes)), 1), sizes)      # (the models are numbered by fold: their columns are reordered)
    assert S % 32 and M % geo['vertices'] and M % geo['centres']
    res, _ = against_host('searchlight_uneven_folds_C%d' % C, (X, y, ring(M, 1), fold), {}, geo)
    assert res.support.sum() == S


@pytest.mark.parametrize('C', ['2', '5', '9', 'Cmax'])
def test_class_counts_on_every_arm(C, geo):
    C = geo['max_C'] if C == 'Cmax' else int(C)
    X, y, fold = data(np.random.RandomState(C), 4 * C, 21, C, folds=2)
    res, _ = against_host('searchlight_C%d' % C, (X, y, ring(21, 1), fold), {}, geo)
    assert res.correct.shape == (1, C, 21) and res.support.tolist() == [[4] * C]


def test_rows_of_length_one(geo):
    X, y, fold = data(np.random.RandomState(12), 40, 37, 2, folds=2)
    res, ref = against_host('searchlight_single_vertex_rows', (X, y, sp.identity(37, format='csr'), fold), {}, geo)
    assert res.correct.shape == (1, 2, 37)


def test_a_row_of_all_1000_vertices_among_short_ones(geo):
    M = 1000
    X, y, fold = data(np.random.RandomState(13), 70, M, 3, mean=1e4, sd=50.0, folds=2)
    rows = sp.vstack([sp.csr_matrix(np.ones((1, M))), ring(M, 2)[[0, 499]], sp.csr_matrix(np.ones((1, M)))[:, ::-1]]).tocsr()
    assert rows.shape == (4, M) and M % geo['unroll'][4] == 0 and 5 % geo['unroll'][4]
    res, _ = against_host('searchlight_whole_brain_row', (X, y, rows, fold), {}, geo)
    assert np.array_equal(res.scores[:, :, 0], res.scores[:, :, 3]) and res.correct.shape == (1, 3, 4)


def test_nan_in_the_pad_of_the_patterns_stays_there(geo):
    import torch
    X, y, fold = data(np.random.RandomState(14), 45, 33, 3, folds=3)
    balls = ring(33, 2)
    res = run_device((X, y, balls, fold), dict(scores=True, C=3), geo)
    a = sl._check(X, y, balls, fold, None, True, None, True, False, None, 't')
    plan = sl._device_plan(a, geo['buckets'][3])
    dev = torch.device('cuda')
    Xt = sl._transposed(torch.as_tensor(X).to(dev), plan.order, dev)
    assert Xt.shape == (33, 64)
    Xt[:, 45:] = float('nan')
    correct, sc, _ = sl._run(a, plan, Xt, True, False, None)
    assert np.array_equal(sc.cpu().numpy(), res.scores) and np.array_equal(correct.cpu().numpy(), res.correct)


# ---- 3. groups ------------------------------------------------------------------------------------------------------------------

def test_three_groups_of_two_folds(geo):
    import torch
    rng = np.random.RandomState(20)
    S, M = 108, 40
    X, y, fold = data(rng, S, M, 3, mean=1000.0, sd=5.0, folds=2, stride=3)
    groups = ['s2', 's1', 's3'] * (S // 3)                      # every (group, fold, class) cell holds 6 samples
    fold = fold + 4
    balls = ring(M, 2)
    res, ref = against_host('searchlight_groups_within', (X, y, balls, fold), dict(groups=groups), geo)
    assert res.groups == ['s2', 's1', 's3'] and res.correct.shape == (3, 3, M) and res.support.tolist() == [[12] * 3] * 3
    for g, key in enumerate(res.groups):                        # a group alone: the same bits
        own = np.array([k == key for k in groups])
        alone = run_device((X[own], y[own], balls, fold[own]), dict(scores=True, C=3), geo)
        assert np.array_equal(alone.scores, res.scores[own]) and np.array_equal(alone.correct[0], res.correct[g])
    across, _ = against_host('searchlight_groups_across', (X, y, balls, fold), dict(groups=groups, within=False), geo)
    assert across.correct.shape == (3, 3, M) and not np.array_equal(across.scores, res.scores)
    tens = run_device((torch.as_tensor(X).cuda(), y, balls, fold), dict(groups=groups, scores=True, predictions=True, C=3), geo)
    assert all(torch.is_tensor(v) and v.is_cuda for v in (tens.correct, tens.recall, tens.accuracy, tens.scores, tens.predictions))
    assert isinstance(tens.support, np.ndarray) and tens.recall.dtype == torch.float32 and tens.correct.dtype == torch.int32
    for name in ('correct', 'recall', 'accuracy', 'scores', 'predictions'):
        assert np.array_equal(getattr(tens, name).cpu().numpy(), getattr(res, name)), name


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------

def test_duplicate_classes_tie_to_the_lower_class(geo):
    rng = np.random.RandomState(30)
    half, _, fold = data(rng, 48, 30, 1, folds=3)
    X = np.concatenate([half, half])                            # classes 1 and 2 hold the same samples in every fold
    y = np.repeat([2, 1], 48)
    res = run_device((X, y, ring(30, 2), np.concatenate([fold, fold])), dict(scores=True, predictions=True, C=2), geo)
    assert res.classes == [1, 2] and np.array_equal(res.scores[:, 0], res.scores[:, 1])
    assert (res.predictions == 0).all() and (res.recall[0, 0] == 1).all() and (res.recall[0, 1] == 0).all()
    assert (res.accuracy == 0.5).all() and np.array_equal(res.correct[0, 0], np.full(30, 48, np.int32))


# ---- 5. arms --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw', [dict(variance='pooled'), dict(priors='uniform'), dict(variance='pooled', priors='uniform', var_smoothing=0.0),
                                dict(var_smoothing=1e-2)], ids=['pooled', 'uniform', 'pooled_uniform_unsmoothed', 'smoothed'])
def test_pooled_variance_uniform_priors_and_smoothing(kw, geo):
    rng = np.random.RandomState(40)
    S, M = 90, 35
    X, y, fold = data(rng, S, M, 3, folds=3)
    y = np.where(np.arange(S) % 7 == 0, 0, y)                   # unbalanced: the empirical prior matters
    res, ref = against_host('searchlight_' + '_'.join('%s' % v for v in kw.values()), (X, y, ring(M, 2), fold), kw, geo)
    plain = sl.searchlight_host(X, y, ring(M, 2), fold, scores=True)
    assert not np.allclose(ref.scores, plain.scores, rtol=1e-6, atol=0)


def test_a_constant_vertex_and_an_all_constant_input(geo):
    rng = np.random.RandomState(41)
    S, M = 60, 33
    X, y, fold = data(rng, S, M, 2, folds=3)
    y = np.where(np.arange(S) % 5 == 0, 1, y)                   # class 1 is the more frequent one in every training set
    X[:, 5] = 100.0
    res, _ = against_host('searchlight_constant_vertex', (X, y, ring(M, 1), fold), {}, geo)
    alone = run_device((X, y, sp.csr_matrix((np.ones(1), ([0], [5])), shape=(1, M)), fold), dict(scores=True, predictions=True, C=2), geo)
    assert np.isfinite(alone.scores).all() and (alone.predictions == 1).all()       # the smoothed variance decides nothing: the prior does
    flat = np.full((S, M), 7.5, np.float32)
    res, ref = against_host('searchlight_all_constant', (flat, y, ring(M, 1), fold), {}, geo)
    assert np.isfinite(res.scores).all() and (res.predictions == 1).all()
    assert np.array_equal(res.scores, ref.scores)               # log prior alone: no vertex contributes
    assert (res.recall[0, 1] == 1).all() and (res.recall[0, 0] == 0).all()


# ---- 6. batching ----------------------------------------------------------------------------------------------------------------

def test_batches_of_centres_give_the_same_bits(geo):
    X, y, fold = data(np.random.RandomState(50), 66, 23, 3, mean=1e4, sd=50.0, folds=2)
    balls = ring(23, 2)
    whole = run_device((X, y, balls, fold), dict(scores=True, predictions=True, batch_centres=23, C=3), geo)
    same = run_device((X, y, balls, fold), dict(scores=True, predictions=True, C=3), geo)
    for b, n in ((1, 23), (7, 4)):
        part = run_device((X, y, balls, fold), dict(scores=True, predictions=True, batch_centres=b, C=3), geo, batches=n)
        for name in ('scores', 'predictions', 'correct', 'recall', 'accuracy'):
            assert np.array_equal(getattr(part, name), getattr(whole, name)), (b, name)
    assert np.array_equal(same.scores, whole.scores) and np.array_equal(same.correct, whole.correct)


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------

def test_searchlight_events_end_to_end(geo):
    import torch
    rng = np.random.RandomState(60)
    M, dura = 40, 4
    names = ['rest'] * 3 + ['a'] * 8 + ['rest'] * 2 + ['b'] * 9 + ['rest'] * 3 + ['a'] * 5 + ['rest'] + ['b'] * 8 + ['rest'] * 2
    T = len(names)
    subjects = ['s1', 's1', 's2', 's2']
    gain = np.zeros((2, M))
    gain[1, 10:20] = 3.0
    labels = [names, names[::-1], names, names[::-1]]
    runs = [(1000.0 + 2.0 * rng.randn(T, M) + gain[[int(n == 'b') for n in run]]).astype(np.float32) for run in labels]
    balls = ring(M, 2)
    ev = events.match_events(labels, ['a', 'b'], dura)
    want = np.concatenate([events.host_windows(runs[r], i, fold=dura)[:, :, 0] for r, i in zip(ev.kept, ev.index)])
    idx, lab, tg, tf, classes = sl._events_plan([T] * 4, labels, ['a', 'b'], dura, subjects, None, True, {})
    dev = torch.device('cuda')
    planes = stage(runs, M, dev, 't')[1]
    assert planes.shape == (4 * T, _lib.plane_stride(M)) and not planes[:, M:].any()
    planes[:, M:] = float('nan')                                # the pad of the staged planes never reaches a pattern
    got = sl._event_patterns(planes, torch.as_tensor(idx).to(dev), M)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    res = run_device((runs, labels, ['a', 'b'], dura, balls), dict(fn=sl.searchlight_events, groups=subjects, scores=True, C=2), geo,
                     head=['gather_windows_indexed'])
    direct = run_device((want, lab, balls, tf), dict(groups=tg, classes=classes, scores=True, C=2), geo)
    assert res.groups == ['s1', 's2'] and res.classes == ['a', 'b'] and isinstance(res.correct, np.ndarray)
    for name in ('scores', 'correct', 'recall', 'accuracy', 'support'):
        assert np.array_equal(getattr(res, name), getattr(direct, name)), name
    assert res.accuracy[:, 12:18].mean() > 0.8 > 0.6 > res.accuracy[:, 24:].mean()      # the planted patch (vertices 10 .. 19 respond to b)
    tens = run_device(([torch.as_tensor(r).cuda() for r in runs], labels, ['a', 'b'], dura, balls),
                      dict(fn=sl.searchlight_events, groups=subjects, C=2), geo, head=['gather_windows_indexed'])
    assert torch.is_tensor(tens.recall) and np.array_equal(tens.recall.cpu().numpy(), res.recall) and tens.scores is None
    loso = run_device((runs, labels, ['a', 'b'], dura, balls), dict(fn=sl.searchlight_events, groups=subjects, within=False, C=2), geo,
                      head=['gather_windows_indexed'])
    by_subject = run_device((want, lab, balls, sl.default_folds(tg, within=False)), dict(groups=tg, classes=classes, within=False, C=2), geo)
    assert np.array_equal(loso.correct, by_subject.correct) and loso.support.tolist() == [[6, 8], [6, 8]]


# ---- 8. the dispatch log --------------------------------------------------------------------------------------------------------

def test_dispatch_log_of_one_call(geo):
    X, y, fold = data(np.random.RandomState(70), 48, 10, 3, folds=2)
    _lib.dispatch_log = log = []
    try:
        sl.searchlight(X, y, ring(10, 1), fold, batch_centres=4)
    finally:
        _lib.dispatch_log = None
    score = 'searchlight_base_kernel + searchlight_score_kernel<4>'
    assert log == [('searchlight_spread', 'searchlight_spread_kernel'), ('searchlight_fit', 'searchlight_fit_kernel'),
                   ('searchlight_score', score), ('searchlight_score', score), ('searchlight_score', score)]
    assert geo['buckets'][3] == 4 and sorted(set(geo['buckets'].values())) == [2, 4, 8, 16, 32]
