"""``searchlight.searchlight(classifier='svc')`` on the device (chebgcn_searchlight_svm per bucket of training-set size and batch
of centres) against its float64 host restatement ``searchlight.searchlight_host``.

There is no tolerance anywhere in this file.  The model is stated operation by operation -- float64, every multiply, add and
divide rounded on its own, every chain in a fixed order -- and the kernel is compiled with contraction off, so ``scores``,
``predictions``, ``correct``, ``sweeps`` and ``residual`` from the device are ``array_equal`` to the host's.  Shapes come from
``ops.searchlight_svm_geometry()``: a tile of 16 vertices, a super-tile of 256 (the means of so many vertices are formed at
once), sample buckets of 32 / 64 / 128, scoring chunks of 32 test samples, classes round-robin over four waves.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from gcn_fmri_decoding_amd import _lib, events, searchlight as sl

pytestmark = pytest.mark.gpu

NAMES = ('scores', 'predictions', 'correct', 'recall', 'accuracy')


@pytest.fixture(scope='module')
def geo():
    from gcn_fmri_decoding_amd import ops
    g = ops.searchlight_svm_geometry()
    assert (g['tile'], g['super_tile'], g['chunk'], g['max_n'], g['max_C'], g['threads']) == (16, 256, 32, sl.SVC_NMAX, sl.CMAX, 256)
    assert [g['buckets'][n] for n in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)] == [32, 32, 32, 32, 64, 64, 64, 128, 128, 128]
    return g


def data(rng, y, M, shift=1.0):
    """Unit noise, class means ``shift`` apart per vertex."""
    C = int(np.max(y)) + 1
    return (rng.randn(len(y), M) + shift * rng.randn(C, M)[y]).astype(np.float32)


def rows_of(M, lengths, step=7):
    """Row i: ``lengths[i]`` consecutive vertices from ``step * i``."""
    r = sp.lil_matrix((len(lengths), M))
    for i, P in enumerate(lengths):
        assert step * i + P <= M
        r[i, step * i:step * i + P] = 1
    return r.tocsr()


def train_sizes(fold, groups=None, within=True):
    """The training-set size of every model, models in the plan's order (group by group in order of first appearance, folds
    ascending; across groups: folds ascending)."""
    fold = np.asarray(fold)
    groups = np.zeros(len(fold), int) if groups is None or not within else np.unique(np.asarray(groups), return_inverse=True)[1]
    first = {}
    for g in groups:
        first.setdefault(int(g), len(first))
    out = []
    for g in sorted(first, key=first.get):
        for f in np.unique(fold[groups == g]):
            out.append(int(((groups == g) & (fold != f)).sum()))
    return out


def launches_of(sizes, U, geo, batch=None):
    """The buckets of the launches one call makes, in order: the sample buckets ascending, each cut into batches of centres."""
    out = []
    for b in sorted(set(geo['buckets'][n] for n in sizes)):
        out += [b] * (1 if batch is None else -(-U // min(batch, U)))
    return out


def run_device(args, kw, launches, head=()):
    """``searchlight`` (or ``searchlight_events``) with ``classifier='svc'`` and the dispatch log checked by name: exactly one
    ``searchlight_svm`` per (bucket, batch) on the bucket's arm."""
    kw = dict(kw)
    fn = kw.pop('fn', sl.searchlight)
    _lib.dispatch_log = log = []
    try:
        res = fn(*args, classifier='svc', **kw)
    finally:
        _lib.dispatch_log = None
    assert log == [(h, d) for h, d in head] + [('searchlight_svm', 'searchlight_svm_kernel<%d>' % b) for b in launches], log
    return res


def both(args, kw, geo, batch=None):
    """Device against host, bit for bit: ``(device result, device SolverInfo, host result, host SolverInfo)``."""
    full = dict(kw, scores=True, predictions=True, return_solver=True)
    ref, rinfo = sl.searchlight_host(*args, classifier='svc', **full)
    sizes = train_sizes(args[3], kw.get('groups'), kw.get('within', True))
    U = sp.csr_matrix(args[2]).shape[0]
    res, info = run_device(args, dict(full, batch_centres=batch), launches_of(sizes, U, geo, batch))
    assert res.scores.dtype == np.float64 and res.predictions.dtype == np.uint8 and res.correct.dtype == np.int32
    assert info.sweeps.dtype == np.int32 and info.residual.dtype == np.float64 and info.sweeps.shape == info.residual.shape == (len(sizes), U)
    assert np.isfinite(res.scores).all() and np.isfinite(info.residual).all()
    assert info.models == rinfo.models and res.groups == ref.groups and res.classes == ref.classes
    for name in NAMES + ('support',):
        assert np.array_equal(getattr(res, name), getattr(ref, name)), name
    assert np.array_equal(info.sweeps, rinfo.sweeps) and np.array_equal(info.residual, rinfo.residual)
    return res, info, ref, rinfo


# ---- 1. rows of every length ----------------------------------------------------------------------------------------------------

def test_rows_at_the_tile_and_super_tile_edges_and_one_full_row(geo):
    """1, 15, 16, 17 vertices around the tile; 128, 129, 300; 255, 256, 257 around the super-tile; all M = 400 vertices."""
    rng = np.random.RandomState(1)
    S, M = 48, 400
    y = np.arange(S) % 3
    fold = np.arange(S) // 3 % 2
    X = data(rng, y, M)
    lengths = [1, 15, 16, 17, 128, 129, 300, 255, 256, 257, M]
    nb = rows_of(M, lengths, step=0)
    res, info, _, _ = both((X, y, nb, fold), dict(max_iter=100), geo)
    assert res.scores.shape == (S, 3, len(lengths)) and (info.sweeps >= 1).all()
    assert (info.residual[:, 4:] <= 1e-3).all() and info.sweeps[:, 4:].max() < 100                # the long rows converge under the cap
    assert res.accuracy[0, -1] > 0.9                            # the whole-brain row decodes


# ---- 2. training sets at the bucket edges ---------------------------------------------------------------------------------------

def test_training_sets_of_2_to_65_samples_hit_three_buckets_in_one_call(geo):
    """Unequal folds inside three groups: training sets of 63, 64, 65 (folds of 33, 32, 31), of 31 and 2 (folds of 2 and 31)
    and of 33 and 32 (folds of 32 and 33)."""
    rng = np.random.RandomState(2)
    groups = ['a'] * 96 + ['b'] * 33 + ['c'] * 65
    fold = np.concatenate([np.repeat([0, 1, 2], [33, 32, 31]), np.repeat([0, 1], [2, 31]), np.repeat([0, 1], [32, 33])])
    S, M = len(groups), 60
    y = np.arange(S) % 2
    y[96:98] = [0, 1]                                           # the training set of two samples holds both classes
    X = data(rng, y, M, 0.5)
    assert train_sizes(fold, groups) == [63, 64, 65, 31, 2, 33, 32]
    res, info, _, _ = both((X, y, rows_of(M, [5, 40, 60], step=0), fold), dict(groups=groups, max_iter=40), geo)
    assert info.models == [('a', 0), ('a', 1), ('a', 2), ('b', 0), ('b', 1), ('c', 0), ('c', 1)]
    assert np.array_equal(res.scores[:, 1], -res.scores[:, 0])  # two classes: mirror images, exactly


def test_training_sets_of_127_and_128_samples(geo):
    rng = np.random.RandomState(3)
    fold = np.repeat([0, 1, 2], [64, 64, 63])
    S, M = len(fold), 50
    y = np.arange(S) % 3
    X = data(rng, y, M, 0.5)
    assert train_sizes(fold) == [127, 127, 128] and S <= 200
    both((X, y, rows_of(M, [7, 50], step=0), fold), dict(max_iter=12), geo)


# ---- 3. classes, test samples, losses, C, caps ----------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [2, 3, 4, 5, 8, 9, 32])
def test_class_counts_around_the_four_waves(C, geo):
    rng = np.random.RandomState(C)
    S = 4 * C
    y = np.arange(S) % C
    fold = np.arange(S) // C % 2
    X = data(rng, y, 50)
    res, _, _, _ = both((X, y, rows_of(50, [3, 50], step=0), fold), dict(max_iter=25), geo)
    assert res.correct.shape == (1, C, 2) and res.support.tolist() == [[4] * C]


def test_models_of_1_32_33_and_65_test_samples(geo):
    """The scoring chunk holds 32 test samples.  Group 'a': folds of 1, 32, 33; group 'b': folds of 65 and 30."""
    rng = np.random.RandomState(5)
    groups = ['a'] * 66 + ['b'] * 95
    fold = np.concatenate([np.repeat([0, 1, 2], [1, 32, 33]), np.repeat([0, 1], [65, 30])])
    S = len(groups)
    y = (np.arange(S) + 1) % 3
    X = data(rng, y, 40)
    assert train_sizes(fold, groups) == [65, 34, 33, 30, 65]
    res, _, _, _ = both((X, y, rows_of(40, [9, 40], step=0), fold), dict(groups=groups, max_iter=30), geo)
    assert res.support.sum() == S


@pytest.mark.parametrize('loss', ['squared_hinge', 'hinge'])
@pytest.mark.parametrize('Creg', [1e-3, 1.0, 1e3])
def test_both_losses_three_C_and_the_sweep_caps(loss, Creg, geo):
    """``tol = 0`` runs to the cap (1 and 3 sweeps); the default ``tol`` under a cap of 1000."""
    rng = np.random.RandomState(6)
    S, M = 24, 70
    y = np.arange(S) % 3
    fold = np.arange(S) // 3 % 3
    X = data(rng, y, M, 0.3)
    nb = rows_of(M, [4, 70], step=0)                            # 4 vertices for 16 samples: the slow case; 70: the fast one
    for cap in (1, 3):
        _, info, _, _ = both((X, y, nb, fold), dict(C=Creg, loss=loss, tol=0.0, max_iter=cap), geo)
        assert ((info.sweeps == cap) | (info.residual == 0)).all() and (info.sweeps <= cap).all()    # (hinge at the bound: PG = 0)
    _, info, _, _ = both((X, y, nb, fold), dict(C=Creg, loss=loss, max_iter=1000), geo)
    assert (info.sweeps[info.residual > 1e-3] == 1000).all() and (info.residual[info.sweeps < 1000] <= 1e-3).all()
    if Creg <= 1.0:
        assert (info.sweeps[:, 1] < 1000).all()                 # the long row converges


def test_all_zero_and_partly_zero_rows(geo):
    rng = np.random.RandomState(7)
    S, M = 36, 40
    y = np.arange(S) % 3
    fold = np.arange(S) // 3 % 3
    X = data(rng, y, M)
    X[:, 20:] = 0.0
    nb = sp.csr_matrix(np.array([[float(lo <= v) for v in range(M)] for lo in (20, 6, 25)]))       # all zero, 14 live vertices, all zero
    for loss in ('squared_hinge', 'hinge'):
        res, info, _, _ = both((X, y, nb, fold), dict(loss=loss), geo)
        assert np.array_equal(res.scores[:, :, 0], res.scores[:, :, 2])         # all-zero rows: K = 0, the bias alone
        for f in range(3):                                      # ... the same for every test sample of a model
            assert (res.scores[fold == f][:, :, 0] == res.scores[fold == f][:1, :, 0]).all()
        assert np.array_equal(res.predictions[:, 0], np.argmax(res.scores[:, :, 0], axis=1))       # the first maximal class
        assert not np.array_equal(res.scores[:, :, 1], res.scores[:, :, 0])     # 14 live vertices among 20 zero ones speak


# ---- 4. batching, order, groups, input kind -------------------------------------------------------------------------------------

def test_any_batching_any_order_three_groups_and_tensors(geo):
    import torch
    rng = np.random.RandomState(8)
    S, M = 108, 60
    y = np.arange(S) // 3 % 3
    fold = np.arange(S) // 9 % 2 + 4
    groups = ['s2', 's1', 's3'] * (S // 3)                      # every (group, fold, class) cell holds 6 samples
    X = data(rng, y, M, 0.5)
    lengths = [60, 1, 17, 33, 16, 2, 3, 40, 5]
    nb = rows_of(M, lengths, step=0)
    kw = dict(groups=groups, C=0.5, max_iter=30)
    whole, winfo, _, _ = both((X, y, nb, fold), kw, geo)
    assert whole.groups == ['s2', 's1', 's3'] and whole.correct.shape == (3, 3, 9) and winfo.sweeps.shape == (6, 9)
    full = dict(kw, scores=True, predictions=True, return_solver=True)
    for b in (1, 7):
        part, pinfo = run_device((X, y, nb, fold), dict(full, batch_centres=b), [32] * (-(-9 // b)))
        for name in NAMES:
            assert np.array_equal(getattr(part, name), getattr(whole, name)), (b, name)
        assert np.array_equal(pinfo.sweeps, winfo.sweeps) and np.array_equal(pinfo.residual, winfo.residual)
    back, binfo = run_device((X, y, nb[::-1], fold), full, [32])                # the centres in another order
    assert np.array_equal(back.scores[:, :, ::-1], whole.scores) and np.array_equal(back.correct[:, :, ::-1], whole.correct)
    assert np.array_equal(binfo.sweeps[:, ::-1], winfo.sweeps) and np.array_equal(binfo.residual[:, ::-1], winfo.residual)
    for g, key in enumerate(whole.groups):                      # a group alone: the same bits
        own = np.array([k == key for k in groups])
        alone, ainfo = run_device((X[own], y[own], nb, fold[own]), dict(full, groups=None), [32])
        assert np.array_equal(alone.scores, whole.scores[own]) and np.array_equal(alone.correct[0], whole.correct[g])
        assert np.array_equal(ainfo.sweeps, winfo.sweeps[2 * g:2 * g + 2])
    tens, tinfo = run_device((torch.as_tensor(X).cuda(), y, nb, fold), full, [32])
    assert all(torch.is_tensor(v) and v.is_cuda for v in (tens.correct, tens.recall, tens.scores, tens.predictions, tinfo.sweeps, tinfo.residual))
    for name in NAMES:
        assert np.array_equal(getattr(tens, name).cpu().numpy(), getattr(whole, name)), name
    assert np.array_equal(tinfo.sweeps.cpu().numpy(), winfo.sweeps) and np.array_equal(tinfo.residual.cpu().numpy(), winfo.residual)
    plain = run_device((X, y, nb, fold), kw, [32])              # without return_solver: the result alone
    assert isinstance(plain, sl.SearchlightResult) and plain.scores is None and np.array_equal(plain.correct, whole.correct)


def test_across_groups_while_the_training_set_fits(geo):
    rng = np.random.RandomState(9)
    S, M = 120, 40
    y = np.arange(S) % 3
    groups = np.arange(S) // 3 % 4                              # 4 subjects of 30 samples; a fold a subject: 90 training samples
    X = data(rng, y, M, 0.5)
    res, info, _, _ = both((X, y, rows_of(M, [6, 40], step=0), groups), dict(groups=groups.tolist(), within=False, max_iter=20), geo)
    assert info.models == [(None, f) for f in range(4)] and res.correct.shape == (4, 3, 2)
    with pytest.raises(ValueError, match=r'fold 0 holds 129 samples.*within=False'):
        sl.searchlight(np.zeros((172, 5), np.float32), np.arange(172) % 2, rows_of(5, [5], step=0), np.arange(172) // 43,
                       within=False, classifier='svc')


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------

def test_searchlight_events_against_the_host_on_the_patterns_it_cuts(geo):
    import torch
    rng = np.random.RandomState(10)
    M, dura = 40, 4
    names = ['rest'] * 3 + ['a'] * 8 + ['rest'] * 2 + ['b'] * 9 + ['rest'] * 3 + ['a'] * 5 + ['rest'] + ['b'] * 8 + ['rest'] * 2
    T = len(names)
    subjects = ['s1', 's1', 's2', 's2']
    labels = [names, names[::-1], names, names[::-1]]
    sign = np.where(np.arange(M) % 2 == 0, 1.0, -1.0) * ((np.arange(M) >= 10) & (np.arange(M) < 20))
    runs = [(1000.0 + 0.5 * rng.randn(T, M) + 30.0 * rng.randn(T, 1) * (sign != 0)
             + 1.0 * sign * np.array([float(n == 'b') for n in run])[:, None]).astype(np.float32) for run in labels]
    spans = [(0, 10), (10, 40), (20, 30)]                       # outside the patch, the patch and more, outside
    nb = sp.csr_matrix(np.array([[float(lo <= v < hi) for v in range(M)] for lo, hi in spans]))
    ev = events.match_events(labels, ['a', 'b'], dura)
    want = np.concatenate([events.host_windows(runs[r], i, fold=dura)[:, :, 0] for r, i in zip(ev.kept, ev.index)])
    idx, lab, tg, tf, classes = sl._events_plan([T] * 4, labels, ['a', 'b'], dura, subjects, None, True, {})
    kw = dict(groups=subjects, C=10.0, max_iter=200, scores=True, return_solver=True)
    _lib.dispatch_log = log = []
    try:
        res, info = sl.searchlight_events(runs, labels, ['a', 'b'], dura, nb, classifier='svc', **kw)
    finally:
        _lib.dispatch_log = None
    assert [w for w, _ in log] == ['gather_windows_indexed', 'searchlight_svm'] and log[1][1] == 'searchlight_svm_kernel<32>'
    host, hinfo = sl.searchlight_host(want, lab, nb, tf, groups=tg, classes=classes, classifier='svc', C=10.0, max_iter=200, scores=True,
                                      return_solver=True)
    assert res.groups == ['s1', 's2'] and res.classes == ['a', 'b'] and isinstance(res.correct, np.ndarray)
    for name in ('scores', 'correct', 'recall', 'accuracy', 'support'):
        assert np.array_equal(getattr(res, name), getattr(host, name)), name
    assert np.array_equal(info.sweeps, hinfo.sweeps) and np.array_equal(info.residual, hinfo.residual) and info.models == hinfo.models
    assert res.accuracy[:, 1].mean() > 0.8 > 0.7 > max(res.accuracy[:, 0].mean(), res.accuracy[:, 2].mean())
    tens = sl.searchlight_events([torch.as_tensor(r).cuda() for r in runs], labels, ['a', 'b'], dura, nb, classifier='svc',
                                 groups=subjects, C=10.0, max_iter=200)
    assert torch.is_tensor(tens.recall) and np.array_equal(tens.recall.cpu().numpy(), res.recall) and tens.scores is None


# ---- 6. the other classifiers are what they were --------------------------------------------------------------------------------

def test_gnb_and_lda_log_and_give_what_they_did(geo):
    rng = np.random.RandomState(11)
    y = np.arange(48) % 3
    fold = np.arange(48) // 3 % 2
    X = data(rng, y, 10)
    i = np.arange(10)
    nb = sp.csr_matrix((np.ones(30), (np.tile(i, 3), np.concatenate([i, (i + 1) % 10, (i - 1) % 10]))), shape=(10, 10))
    score = 'searchlight_base_kernel + searchlight_score_kernel<4>'
    want = {'gnb': [('searchlight_spread', 'searchlight_spread_kernel'), ('searchlight_fit', 'searchlight_fit_kernel')]
            + [('searchlight_score', score)] * 3,
            'lda': [('searchlight_fit', 'searchlight_fit_kernel')] + [('searchlight_lda', 'searchlight_lda_kernel<32>')] * 3}
    seen = {}
    for turn in range(2):
        for clf in ('gnb', 'lda'):
            _lib.dispatch_log = log = []
            try:
                res = sl.searchlight(X, y, nb, fold, batch_centres=4, classifier=clf, scores=True, predictions=True)
            finally:
                _lib.dispatch_log = None
            assert log == want[clf], (clf, log)
            assert res._fields == ('correct', 'support', 'recall', 'accuracy', 'groups', 'classes', 'scores', 'predictions')
            if turn:
                for name in NAMES:
                    assert np.array_equal(getattr(res, name), getattr(seen[clf], name)), (clf, name)
            seen[clf] = res
            host = sl.searchlight_host(X, y, nb, fold, classifier=clf, scores=True, predictions=True)
            assert np.allclose(res.scores, host.scores, rtol=1e-9, atol=1e-9) and np.array_equal(res.predictions, host.predictions)
        run_device((X, y, nb, fold), {}, [32])                  # an SVM pass in between changes nothing
    for kw in (dict(C=2.0), dict(loss='hinge'), dict(tol=0.0), dict(max_iter=5), dict(return_solver=True)):
        for clf in ('gnb', 'lda'):
            with pytest.raises(ValueError, match="classifier='svc'"):
                sl.searchlight(X, y, nb, fold, classifier=clf, **kw)
