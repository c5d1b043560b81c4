"""Cross-validation on one staged copy of the scans, on the MI355X.  (1)-(5) a view (``WindowSet.select``) against the set staged
from the same runs alone, bit for bit: what ``gather`` forms (plain, balanced, augmented, displaced), the scaler and its
float64 statistics, the jitter bounds -- with the parent and a sibling view untouched.  (6) ``cross_validate_events`` against
the hand-run, fold by fold: ``fit_events`` on the fold's runs in the split's order -- sampled indices, the loss stream and
every variable of the best checkpoint equal, not close.  (7) what a ``CVResult`` holds against ``evaluate`` /
``model_perf.predict`` by hand, one staging per run, ``dir_name`` restored.  (8) the folds as an ensemble against float64.

The model: a synthetic graph of 48 vertices coarsened once (fake vertices), one conv layer, 3 classes, channel 4, batch 8, two
epochs.  The data: 6 subjects with 1-2 runs each, 9 runs of 9 different lengths (offset mistakes hide behind equal ones)."""
import os

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import graph, models_gcn, series, splits, uncertainty

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CHANNEL, TRSTEP = 4, 2
BD = CHANNEL * TRSTEP
TARGETS = ['tool', 'face', 'body']
LENGTHS = [23, 26, 29, 31, 34, 37, 40, 43, 47]
SUBJECTS = ['s0', 's1', 's2', 's1', 's3', 's4', 's3', 's5', 's4']          # of the 9 runs that yield windows
PICK = [4, 0, 3]
_L = []


def _model(**kw):
    if not _L:
        _L.append(graph.synthetic_graph(48, k=4, levels=1, seed=3)[0][0])
    torch.manual_seed(0)
    kw.setdefault('num_epochs', 2)
    net = models_gcn.cgcnn({'device': DEV}, [_L[0]], [4], [3], [1], [3], channel=CHANNEL, batch_size=8, verbose=False,
                           dropout=1, **kw)
    net.contraction = 'f32'
    net.record_fit = True
    assert net._M0 >= 48
    return net


def _runs(M, seed=5):
    rs = np.random.RandomState(seed)
    return [(rs.randn(T, M) * (1 + rs.rand(M)) + rs.randn(M)).astype(np.float32) for T in LENGTHS]


def _starts():
    """Stride 3, a repeated start, and the first and the last possible start of every run."""
    return [np.concatenate([np.arange(0, T - CHANNEL + 1, 3), [3, T - CHANNEL, 0]]).astype(np.int64) for T in LENGTHS]


def _design(rs, T):
    names = ['rest'] * int(rs.randint(0, 3))
    while len(names) < T:
        cond = TARGETS[int(rs.choice([0, 1, 1, 1, 1, 2]))]
        names += [cond] * int(rs.randint(BD, BD + 3)) + ['rest'] * int(rs.randint(1, 3))
    return names[:T]


def _event_data(M, seed=6):
    """``(runs, designs, groups)`` as GIVEN: 10 runs, the sixth all rest (it yields no window and drops out; its subject keeps
    another run); then ``kept`` names the 9 others."""
    rs = np.random.RandomState(seed)
    runs, designs, groups = _runs(M, seed), [_design(rs, T) for T in LENGTHS], list(SUBJECTS)
    runs.insert(5, rs.randn(28, M).astype(np.float32))
    designs.insert(5, ['rest'] * 28)
    groups.insert(5, 's2')
    return runs, designs, groups, [0, 1, 2, 3, 4, 6, 7, 8, 9]


EV_KW = dict(TRstep=TRSTEP, flag_event=1)


def _gathered(net, ws):
    """What ``gather`` forms for every window of the set, pads included (a device tensor)."""
    return ws.gather(net, None).planes.clone()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _gather_is_materialise(net, ws):
    M = net._M0
    got = _gathered(net, ws)[..., :M].permute(0, 2, 1).contiguous().cpu().numpy()
    x = ws.materialise()
    xi = x if net._order is None else x[:, np.asarray(net._order), :]
    return np.array_equal(got.view(np.uint32), np.ascontiguousarray(xi).view(np.uint32))


def _start_sets(net):
    runs, starts = _runs(net._M0), _starts()
    parent = net.stage_windows(runs, starts)
    alone = net.stage_windows([runs[r] for r in PICK], [starts[r] for r in PICK])
    return parent, alone


def _event_sets(net):
    runs, designs, _, kept = _event_data(net._M0)
    parent, labels = net.stage_events(runs, designs, TARGETS, BD, **EV_KW)
    assert len(parent.run_lengths) == 9 and parent.fold == TRSTEP               # the all-rest run dropped out
    alone, alabels = net.stage_events([runs[kept[r]] for r in PICK], [designs[kept[r]] for r in PICK], TARGETS, BD, **EV_KW)
    assert np.array_equal(labels[parent.windows_of(PICK)], alabels)
    return parent, alone, labels


def _sets(net, kind):
    if kind == 'start':
        parent, alone = _start_sets(net)
        labels = (np.arange(len(parent)) % 7 == 0).astype(np.int64) + (np.arange(len(parent)) % 11 == 0)   # unbalanced
    else:
        parent, alone, labels = _event_sets(net)
    return parent, alone, labels


# ------------------------------------------------------------------------------------------------ (1), (2), (5) views

@pytest.mark.parametrize('kind', ['start', 'event'])
def test_a_view_gathers_the_parents_windows_and_leaves_parent_and_sibling_alone(kind):
    net = _model()
    parent, alone, labels = _sets(net, kind)
    w = parent.windows_of(PICK)
    whole = _gathered(net, parent)
    view, sib = parent.select(PICK), parent.select([1, 2, 8])
    assert type(view) is type(parent) and view.planes.data_ptr() == parent.planes.data_ptr() and view.planes is parent.planes
    assert view.run_lengths == [LENGTHS[r] for r in PICK] and len(view) == len(w) == len(alone)
    assert np.array_equal(view.starts, alone.starts)
    assert np.array_equal(view.materialise().view(np.uint32), parent.materialise()[w].view(np.uint32))
    got = _gathered(net, view)
    assert _same(got, whole[torch.as_tensor(w).to(DEV)]) and _same(got, _gathered(net, alone)) and _gather_is_materialise(net, view)
    sib_before = _gathered(net, sib)
    # balance, augment, and (start-cut windows) a displaced refill: as on the set staged alone, and nobody else moves
    vl = labels[w]
    groups = [2, 0, 2]
    la, lb = view.balance(vl, 2, 5, groups), alone.balance(vl, 2, 5, groups)
    assert np.array_equal(la, lb) and len(view) == len(alone) >= len(w)
    if kind == 'start':
        assert len(view) > len(w)                                               # (unbalanced labels: extra windows are drawn)
    assert _same(_gathered(net, view), _gathered(net, alone))
    la, lb = view.augment(la, 2, drop_rate=0.1, seed=3), alone.augment(lb, 2, drop_rate=0.1, seed=3)
    assert np.array_equal(la, lb) and view.aug['D'] >= 4
    if kind == 'start':
        for s in (view, alone):
            s.jitter, s.jitter_rng = 2, np.random.RandomState(4)
    assert np.array_equal(view.refill(), alone.refill())
    assert _same(_gathered(net, view), _gathered(net, alone)) and _gather_is_materialise(net, view)
    assert _same(_gathered(net, parent), whole) and _same(_gathered(net, sib), sib_before)
    assert parent.plan is None and parent.aug is None and len(parent) == whole.shape[0] and len(sib) == sib_before.shape[0]
    for s in (view, alone):
        s.augment(None, 0)
        if kind == 'start':
            s.reset_rows()
        s.balance(None, 0)
    assert _same(_gathered(net, view), got)
    # time shifts (no plan)
    la, lb = view.augment(vl, 2, time_shift=True, seed=9), alone.augment(vl, 2, time_shift=True, seed=9)
    assert np.array_equal(la, lb) and len(view) == 2 * len(w)
    assert _same(_gathered(net, view), _gathered(net, alone)) and _gather_is_materialise(net, view)
    assert np.array_equal(view.refill(), alone.refill()) and _same(_gathered(net, view), _gathered(net, alone))
    view.augment(None, 0)
    # a view of a view
    vv = view.select([2, 0])
    assert vv.planes is parent.planes and _same(_gathered(net, vv), whole[torch.as_tensor(parent.windows_of([3, 4])).to(DEV)])
    assert _same(_gathered(net, parent), whole) and _same(_gathered(net, sib), sib_before)


# ------------------------------------------------------------------------------------------------ (3) the scaler

@pytest.mark.parametrize('kind', ['start', 'event'])
def test_the_scaler_of_a_view_is_that_of_the_set_staged_alone(kind):
    """Bit for bit, the float64 statistics included.  The statistics kernels sum relative to the first row of the buffer they
    are handed and in the order of its rows (chunks of rows, or of windows), so a view hands them its own runs one behind the
    other: a slice of the shared planes where they lie so already ([1, 2]), else a compact copy for the call ([4, 0, 3])."""
    net = _model()
    parent, alone, _ = _sets(net, kind)
    view = parent.select(PICK)
    a, b = view.fit_scaler(), alone.fit_scaler()
    for x, y in zip(a + view.stats, b + alone.stats):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert view.stats[0].dtype == np.float64 and (view.stats[1] > 0).all()
    assert parent.tables is None and parent.scaler is None and parent.stats is None        # installed on the view only
    assert _same(_gathered(net, view), _gathered(net, alone))
    # consecutive runs: no copy; and the whole set is its own view
    runs, starts = _runs(net._M0), _starts()
    if kind == 'start':
        two = net.stage_windows(runs[1:3], starts[1:3])
    else:
        ev = _event_data(net._M0)
        two = net.stage_events([ev[0][ev[3][r]] for r in (1, 2)], [ev[1][ev[3][r]] for r in (1, 2)], TARGETS, BD, **EV_KW)[0]
    v2 = parent.select([1, 2])
    assert v2._stat_planes()[0].data_ptr() == parent.planes[LENGTHS[0]:].data_ptr()
    v2.fit_scaler(), two.fit_scaler()
    for x, y in zip(v2.scaler + v2.stats, two.scaler + two.stats):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    everything = parent.select(list(range(9)))
    everything.fit_scaler(), parent.fit_scaler()
    for x, y in zip(everything.scaler + everything.stats, parent.scaler + parent.stats):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert view.scaler is not parent.scaler and not np.array_equal(view.scaler[0], parent.scaler[0])


# ------------------------------------------------------------------------------------------------ (4) jitter

def test_jitter_on_a_view_stays_inside_the_selected_runs():
    net = _model()
    parent, alone = _start_sets(net)
    view = parent.select(PICK)
    T = np.repeat([LENGTHS[r] for r in PICK], view.run_windows)
    assert ((view.starts == 0).sum() >= 3) and ((view.starts == T - CHANNEL).sum() >= 3)     # windows at both ends of every run
    view.jitter, view.jitter_rng = CHANNEL, np.random.RandomState(12)
    seen = set()
    rng = np.random.RandomState(12)
    for _ in range(4):
        starts = view.refill()
        # the host rule with the runs' OWN bounds, in rows of the set staged alone
        want = series.jitter_rows(alone.base_rows, alone.lo, alone.hi, CHANNEL, rng) - alone.offsets
        assert np.array_equal(starts, want)
        assert (starts >= 0).all() and (starts + CHANNEL <= T).all()
        alone.set_rows(want + alone.offsets)
        assert _same(_gathered(net, view), _gathered(net, alone))
        seen.update((starts - (view.base_rows - view.offsets)).tolist())
    assert min(seen) == -CHANNEL and max(seen) == CHANNEL


# ------------------------------------------------------------------------------------------------ (6) - (8) cross-validation

def _best_variables(ckp_dir):
    path = models_gcn.get_best_checkpoint(os.path.join(ckp_dir, 'model'))
    sd = torch.load(path + '.pt', weights_only=True)
    return {k: np.asarray(sd[k]) for k in sd['names'] + ['window_scaler'] if k in sd}


def _instrument(net, monkeypatch, break_fold=None):
    """``fit`` seeded per fold (torch draws the variables) and recorded; ``_stage_series`` counted."""
    fits, staged, real_fit, real_stage = [], [], net.fit, net._stage_series

    def fit(train_data, train_labels, *a, **k):
        f = int(os.path.basename(net.dir_name)[len('fold'):])
        torch.manual_seed(1000 + f)
        if f == break_fold:
            train_labels = np.array(train_labels)
            train_labels[0] = 3                                                 # outside [0, classes): fit raises a ValueError
            fits.append(dict(train=train_data))
        n = len(train_data)
        out = real_fit(train_data, train_labels, *a, **k)
        fits.append(dict(n=n, refills=len(net.fit_log['starts']), idx=[i.tolist() for i in net.fit_log['idx']],
                         loss=np.asarray(net.fit_log['loss_average'], np.float32), out=out[:2], train=train_data,
                         sources=net.fit_log.get('sources'), augment=net.fit_log.get('augment')))
        return out

    def stage(run, out=None):
        staged.append(int(run.shape[0]))
        return real_stage(run, out=out)

    monkeypatch.setattr(net, 'fit', fit)
    monkeypatch.setattr(net, '_stage_series', stage)
    return fits, staged


CV_KW = dict(n_folds=2, test_size=0.2, val_size=0.1, split_seed=123, standardize=True, scaler='fold', sampling=2, seed=5,
             augment=2, drop_rate=0.1, augment_seed=3, fold_seed=7)


def _hand_run(net, f, split, kruns, kdesigns):
    """Fold ``f`` by hand: ``fit_events`` on the fold's runs in the split's order."""
    tr, va = split.folds[f]
    net.dir_name = os.path.join('hand', 'fold%d' % f)
    np.random.seed(CV_KW['fold_seed'] + f)
    net.fit_events([kruns[r] for r in tr], [kdesigns[r] for r in tr], [kruns[r] for r in va], [kdesigns[r] for r in va], TARGETS,
                   BD, standardize=True, sampling=2, seed=CV_KW['seed'] + f, groups=split.run_subjects[tr], augment=2,
                   drop_rate=0.1, augment_seed=CV_KW['augment_seed'] + f, **EV_KW)
    return net._get_path('checkpoints')


@pytest.mark.parametrize('scheme', ['shuffle', 'kfold'])
def test_cross_validate_events_equals_the_hand_run_and_reports_what_evaluate_gives(scheme, tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    net = _model(dir_name='cv', eval_frequency=200 if scheme == 'shuffle' else 3)
    fits, staged = _instrument(net, monkeypatch)
    runs, designs, groups, kept = _event_data(net._M0)
    res = net.cross_validate_events(runs, designs, TARGETS, BD, groups=groups, scheme=scheme, **dict(CV_KW, **EV_KW))
    assert net.dir_name == 'cv' and sorted(staged) == sorted(len(runs[k]) for k in kept)        # every kept run staged ONCE
    split = res.split
    want = splits.subject_folds([groups[k] for k in kept], 2, 0.2, 0.1, 123, scheme)
    assert split.subjects == ['s0', 's1', 's2', 's3', 's4', 's5'] and len(res.folds) == len(fits) == 2
    assert np.array_equal(split.test_runs, want.test_runs) and len(split.test_subjects) == 2
    kruns, kdesigns = [runs[k] for k in kept], [designs[k] for k in kept]
    whole, labels = net.stage_events(runs, designs, TARGETS, BD, **EV_KW)
    assert np.array_equal(res.labels, labels) and np.array_equal(res.test_labels, labels[whole.windows_of(split.test_runs)])
    cv_fits = list(fits)
    for f, fold in enumerate(res.folds):
        assert np.array_equal(fold.train_runs, want.folds[f][0]) and np.array_equal(fold.val_runs, want.folds[f][1])
        assert fold.checkpoint_dir == os.path.join(str(tmp_path), 'checkpoints', 'cv', 'fold%d' % f)
        assert cv_fits[f]['train'].plan is None and cv_fits[f]['train'].aug is None        # the training view left as selected
        assert cv_fits[f]['train'].planes is cv_fits[0]['train'].planes
        # ---- (6) the hand-run
        hand_dir = _hand_run(net, f, split, kruns, kdesigns)
        a, b = cv_fits[f], fits[-1]
        assert a['idx'] == b['idx'] and len(a['idx']) >= 2
        assert np.array_equal(a['loss'].view(np.uint32), b['loss'].view(np.uint32)), 'loss_average streams differ'
        assert a['out'] == b['out'] and a['out'][0] == fold.fit_accuracies
        assert len(a['sources']) == len(b['sources']) >= 1 and len(a['augment']) >= 1
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(a['sources'], b['sources']))
        va, vb = _best_variables(fold.checkpoint_dir), _best_variables(hand_dir)
        assert set(va) == set(vb) and 'window_scaler' in va and 'conv1/weights' in va
        for k in va:
            assert np.array_equal(va[k].view(np.uint8), vb[k].view(np.uint8)), k
        assert np.array_equal(np.stack(fold.window_scaler), np.stack(net.window_scaler))
        # ---- (7) the results, by hand
        net.dir_name = os.path.join('cv', 'fold%d' % f)
        test_set, test_labels = net.stage_events([kruns[r] for r in split.test_runs], [kdesigns[r] for r in split.test_runs],
                                                 TARGETS, BD, **EV_KW)
        test_set.set_tables(*fold.window_scaler)
        assert tuple(net.evaluate(test_set, test_labels)[1:]) == fold.test
        pred = net.predict(test_set)
        assert fold.test_logits.shape == (len(test_labels), 3) and fold.test_logits.dtype == np.float32
        assert np.array_equal(np.argmax(fold.test_logits, axis=1), pred)
        assert fold.test[0] == 100.0 * np.mean(pred == test_labels)
        train_set, train_labels = net.stage_events([kruns[r] for r in fold.train_runs], [kdesigns[r] for r in fold.train_runs],
                                                   TARGETS, BD, **EV_KW)
        train_set.set_tables(*fold.window_scaler)
        assert tuple(net.evaluate(train_set, train_labels)[1:]) == fold.train
        if scheme == 'shuffle':                     # one checkpoint per fold: the one predict names is the latest
            out = models_gcn.model_perf().predict(fold.checkpoint_dir, test_set, test_labels, batch_size=net.batch_size, model=net)
            assert out[3] == [fold.test[0]] and np.array_equal(out[1], pred)
        net.dir_name = 'cv'
    assert not np.array_equal(cv_fits[0]['idx'], cv_fits[1]['idx'])
    s = res.summary()
    assert s['train_accuracy'] == np.mean([f.train[0] for f in res.folds])
    assert s['val_accuracy'] == np.mean([max(f.fit_accuracies) for f in res.folds]) and s['test_accuracy_std'] >= 0
    # ---- (8) the folds as an ensemble
    ens, acc = res.ensemble()
    z = np.stack([f.test_logits for f in res.folds])
    ref = uncertainty.mc_measures(z)
    assert np.array_equal(ens.labels, ref['labels']) and ens.labels.dtype == np.int64
    assert np.array_equal(ens.votes, ref['votes']) and (ens.votes.sum(axis=1) == 2).all()
    assert np.array_equal(ens.agreement, (ref['votes'][np.arange(len(ref['labels'])), ref['labels']] / np.float32(2)).astype(np.float32))
    tol = 1e-5 * max(1.0, np.log(3))                # the bounds tests/test_gpu_uncertainty_kernels.py holds chebgcn_mc_reduce to
    for k, t in (('probabilities', 1e-5), ('entropy', tol), ('expected_entropy', tol), ('mutual_information', tol)):
        err = float(np.abs(ens[k].astype(np.float64) - ref[k]).max())
        print('ensemble %s: max err %.3e (bound %.1e)' % (k, err, t))
        assert err <= t, (k, err, t)
    assert acc == 100.0 * np.mean(ref['labels'] == res.test_labels)


def test_the_pool_scaler_is_fitted_once_on_all_non_test_subjects(tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    net = _model(dir_name='pool', eval_frequency=200)
    fits, staged = _instrument(net, monkeypatch)
    runs, designs, groups, kept = _event_data(net._M0)
    np.random.seed(3)
    res = net.cross_validate_events(runs, designs, TARGETS, BD, groups=groups, n_folds=2, standardize=True, scaler='pool', **EV_KW)
    tail = np.random.rand()
    assert len(staged) == 9 and net.dir_name == 'pool'
    pool = res.split.pool_runs
    alone = net.stage_events([runs[kept[r]] for r in pool], [designs[kept[r]] for r in pool], TARGETS, BD, **EV_KW)[0]
    scale, shift = alone.fit_scaler()
    for f, fold in enumerate(res.folds):
        assert np.array_equal(fold.window_scaler[0].view(np.uint32), scale.view(np.uint32))
        assert np.array_equal(fold.window_scaler[1].view(np.uint32), shift.view(np.uint32))
        sd = torch.load(models_gcn.get_best_checkpoint(os.path.join(fold.checkpoint_dir, 'model')) + '.pt', weights_only=True)
        assert np.array_equal(sd['window_scaler'].numpy(), np.stack([scale, shift]))
        assert fits[f]['train'].scaler is fits[0]['train'].scaler                          # one scaler, shared by every view
    # fold_seed = None: the global stream saw exactly the draws of the two fits (one permutation per refill), nothing else
    np.random.seed(3)
    for f in fits:
        for _ in range(f['refills']):
            np.random.permutation(f['n'])
    assert np.random.rand() == tail


def test_dir_name_and_the_views_are_restored_when_a_fold_raises(tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    net = _model(dir_name='broken', eval_frequency=200)
    fits, staged = _instrument(net, monkeypatch, break_fold=1)
    runs, starts = _runs(net._M0), _starts()
    labels = np.concatenate([np.arange(len(s)) % 3 for s in starts])
    labels[labels == 2] = np.where(np.arange((labels == 2).sum()) % 4 == 0, 2, 0)          # unbalanced: there is a plan
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 3\)'):
        net.cross_validate_series(runs, starts, labels, groups=SUBJECTS, n_folds=3, sampling=1, augment=1, drop_rate=0.2,
                                  jitter=1, fold_seed=1)
    assert net.dir_name == 'broken' and len(staged) == 9
    assert len(fits) == 2 and 'idx' in fits[0] and 'idx' not in fits[1]                    # fold 0 ran, fold 1 raised, fold 2 never began
    for f in fits:
        view = f['train']
        assert view.plan is None and view.aug is None and view.jitter == 0 and len(view) == view.shape_base[0]
        assert np.array_equal(view.rows_host, view.base_rows)
    assert os.path.isdir(os.path.join(str(tmp_path), 'checkpoints', 'broken', 'fold0', 'model'))
