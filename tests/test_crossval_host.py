"""Cross-validation on the host: every refusal of ``cross_validate_series`` / ``cross_validate_events`` (raised before any
device work, on a shape-only model), the table arithmetic of ``WindowSet.select`` on hand-made tables, views over CPU tensors
with a stub owner (both kinds, an event table with fold 2), and the arithmetic of ``CVResult.summary``.  No GPU."""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import crossval, decode, models_gcn, series
from gcn_fmri_decoding_amd import graph as graph_mod


def _meta_model(**kw):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=3, batch_size=4,
                            verbose=False, dir_name='cv', **kw)


RUNS = [np.zeros((T, 60), np.float32) for T in (9, 11, 10, 12, 13, 14)]
DESIGN = lambda T: (['rest'] * 2 + ['a'] * 3 + ['b'] * 3 + ['rest'] * T)[:T]
DESIGNS = [DESIGN(len(r)) for r in RUNS]
EV = dict(series=RUNS, label_runs=DESIGNS, target_name=['a', 'b'], block_dura=3, groups=[0, 1, 2, 3, 4, 5], n_folds=2,
          flag_event=1)
SE = dict(series=RUNS, starts=[[0, 3]] * 6, labels=[0, 1] * 6, groups=['a', 'b', 'c', 'd', 'e', 'f'], n_folds=2)
BAD_BOTH = [
    (dict(groups=[0, 1, 2]), 'groups'),
    (dict(groups=[0.5] * 6), 'groups'),
    (dict(groups=[0, 0, 0, 1, 1, 1]), 'refused'),                    # two subjects: one test subject, a pool of one
    (dict(n_folds=0), 'n_folds'),
    (dict(test_size=1.5), 'test_size'),
    (dict(val_size=0), 'validation'),
    (dict(split_seed=-1), 'seed'),
    (dict(scheme='loo'), 'scheme'),
    (dict(scheme='kfold', n_folds=5), 'kfold'),
    (dict(standardize=1), 'standardize'),
    (dict(scaler='run'), 'scaler'),
    (dict(fold_seed=-3), 'fold_seed'),
    (dict(fold_seed=2 ** 32 - 1), 'fold_seed'),                      # fold 1 would seed with 2**32
    (dict(fold_seed=1.0), 'fold_seed'),
    (dict(sampling=17), 'sampling'),
    (dict(seed=2 ** 32 - 1), 'seed'),
    (dict(augment=65), 'copies'),
    (dict(augment=1, drop_rate=2.0), 'drop_rate'),
    (dict(augment=1, time_shift=True, sampling=2), 'time_shift'),
    (dict(augment_seed='x'), 'augment_seed'),
]


@pytest.mark.parametrize('kw,word', BAD_BOTH + [
    (dict(block_dura=4), 'channel'),
    (dict(label_runs=DESIGNS[:5]), 'designs'),
    (dict(target_name=['zzz']), 'no run yields'),
    (dict(jitter=1), 'jitter'),                                      # (not a keyword of match_events)
    (dict(TRstep=2), 'TRstep'),
])
def test_cross_validate_events_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word) as e:
        net.cross_validate_events(**dict(EV, **kw))
    assert 'cross_validate_events' in str(e.value) and net.dir_name == 'cv'


@pytest.mark.parametrize('kw,word', BAD_BOTH + [
    (dict(starts=[[0, 9]] * 6), 'start'),
    (dict(labels=[0, 1] * 5), 'labels'),
    (dict(jitter=-1), 'jitter'),
    (dict(jitter_seed=2 ** 32 - 1), 'jitter_seed'),
    (dict(resample=2), 'resample'),
    (dict(series=RUNS[:5] + [np.zeros((2, 60))]), 'shorter'),
])
def test_cross_validate_series_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word) as e:
        net.cross_validate_series(**dict(SE, **kw))
    assert 'cross_validate_series' in str(e.value) and net.dir_name == 'cv'


def test_valid_arguments_reach_the_device_check_and_data_parallel_is_refused():
    net = _meta_model()
    for call, kw in ((net.cross_validate_events, EV), (net.cross_validate_series, SE)):
        for more in (dict(), dict(scheme='kfold', n_folds=4, standardize=True, scaler='fold', fold_seed=7, sampling=2, augment=2,
                                  drop_rate=0.1), dict(groups=None, test_size=0)):
            with pytest.raises(RuntimeError, match='device'):
                call(**dict(kw, **more))
    net._dp = object()
    for call, kw in ((net.cross_validate_events, EV), (net.cross_validate_series, SE)):
        with pytest.raises(NotImplementedError, match='DataParallel'):
            call(**kw)


# ------------------------------------------------------------------------------------------------ select: table arithmetic

LENGTHS = [12, 9, 15, 10, 11]
STARTS = [np.array([0, 9, 4, 4]), np.array([6, 0]), np.array([0, 12, 3]), np.array([7]), np.array([8, 0, 8, 5])]
M, MP, C = 5, 32, 3


def test_select_runs_on_hand_made_tables():
    offsets = series.run_offsets(LENGTHS)
    assert offsets.tolist() == [0, 12, 21, 36, 46] and offsets.dtype == np.int64
    counts = [len(s) for s in STARTS]
    windows, lengths, offs, cnt = series.select_runs(LENGTHS, offsets, counts, [4, 0, 3])
    assert windows.tolist() == [10, 11, 12, 13, 0, 1, 2, 3, 9] and windows.dtype == np.int64
    assert lengths.tolist() == [11, 12, 10] and offs.tolist() == [46, 0, 36] and cnt.tolist() == [4, 4, 1]
    rows, lo, hi = series.row_table(lengths, [STARTS[r] for r in (4, 0, 3)], C, offs)
    assert rows.tolist() == [54, 46, 54, 51, 0, 9, 4, 4, 43]
    assert lo.tolist() == [46] * 4 + [0] * 4 + [36] and hi.tolist() == [54] * 4 + [9] * 4 + [43]
    # a selection of a selection names the first set's rows
    w2, l2, o2, c2 = series.select_runs(lengths, offs, cnt, [2, 0])
    assert w2.tolist() == [8, 0, 1, 2, 3] and l2.tolist() == [10, 11] and o2.tolist() == [36, 46] and c2.tolist() == [1, 4]
    for bad, word in (([], 'non-empty'), ([0, 0], 'twice'), ([5], r'\[0, 5\)'), ([-1], r'\[0, 5\)'), ([0.5], 'int'),
                      ([[0, 1]], '1-D')):
        with pytest.raises(ValueError, match=word):
            series.select_runs(LENGTHS, offsets, counts, bad)


class _Owner(object):
    """What a ``WindowSet`` asks of its model: sizes, a device, the internal vertex order and the tables in that order."""
    _M0, channel, device = M, C, torch.device('cpu')
    _order = np.array([3, 0, 4, 1, 2])
    _scale_tables = decode.Decode._scale_tables


def _sets(fold=2):
    rs = np.random.RandomState(11)
    runs = [rs.randn(T, M).astype(np.float32) for T in LENGTHS]
    owner = _Owner()
    planes = torch.zeros((sum(LENGTHS), MP), dtype=torch.float32)
    planes[:, :M] = torch.as_tensor(np.concatenate(runs)[:, owner._order])
    index = [rs.randint(0, T, size=(len(s), C * fold)).astype(np.int64) for T, s in zip(LENGTHS, STARTS)]
    ws = series.StartWindowSet(owner, planes, LENGTHS, STARTS, M, C)
    we = series.EventWindowSet(owner, planes, LENGTHS, index, M, C, fold)
    return owner, runs, index, ws, we


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize('kind', ['start', 'event'])
def test_a_view_stands_for_the_parents_rows_and_equals_the_set_staged_alone(kind):
    owner, runs, index, ws, we = _sets()
    parent = ws if kind == 'start' else we
    cut = STARTS if kind == 'start' else index
    pick = [4, 0, 3]
    scale, shift = np.full((M, C), 2.0, np.float32), np.full((M, C), -1.0, np.float32)
    parent.set_tables(scale, shift)
    whole = parent.materialise()
    view, sib = parent.select(pick), parent.select([1, 2])
    assert type(view) is type(parent) and view.planes is parent.planes and view.owner is owner
    assert view.tables is parent.tables and view.scaler is parent.scaler
    w = parent.windows_of(pick)
    assert w.tolist() == [10, 11, 12, 13, 0, 1, 2, 3, 9] and len(view) == 9 and view.shape == (9, M, C)
    assert np.array_equal(_bits(view.materialise()), _bits(whole[w]))
    assert view.run_lengths == [11, 12, 10] and view.run_windows == [4, 4, 1]
    assert np.array_equal(view.starts, np.concatenate([cut[r] for r in pick]))
    # ... and the set over those runs alone, staged one behind the other
    alone_planes = torch.zeros((33, MP), dtype=torch.float32)
    alone_planes[:, :M] = torch.as_tensor(np.concatenate([runs[r] for r in pick])[:, owner._order])
    more = dict(fold=we.fold) if kind == 'event' else {}
    alone = type(parent)(owner, alone_planes, [LENGTHS[r] for r in pick], [cut[r] for r in pick], M, C, **more)
    alone.set_tables(scale, shift)
    assert np.array_equal(_bits(view.materialise()), _bits(alone.materialise()))
    if kind == 'event':
        assert view.fold == 2 and np.array_equal(view.index_host - view.offsets[:, None], alone.index_host - alone.offsets[:, None])
    else:
        assert np.array_equal(view.lo - view.offsets, alone.lo - alone.offsets)
        assert np.array_equal(view.hi - view.offsets, alone.hi - alone.offsets)
        assert (view.hi == view.offsets + np.repeat([11, 12, 10], [4, 4, 1]) - C).all()
    # perturbing the view: the same as perturbing the set staged alone, and nobody else moves
    labels = np.array([0, 0, 1, 0, 2, 0, 0, 0, 1])
    groups = [7, 3, 7]
    sib_before = sib.materialise()
    la, lb = view.balance(labels, 2, 5, groups), alone.balance(labels, 2, 5, groups)
    assert np.array_equal(la, lb) and len(view) == len(alone) > 9
    la, lb = view.augment(la, 2, drop_rate=0.4, seed=3), alone.augment(lb, 2, drop_rate=0.4, seed=3)
    assert np.array_equal(la, lb) and np.array_equal(_bits(view.materialise()), _bits(alone.materialise()))
    if kind == 'start':
        for s in (view, alone):
            s.jitter, s.jitter_rng = 2, np.random.RandomState(4)
        assert np.array_equal(view.refill(), alone.refill())
        assert np.array_equal(_bits(view.materialise()), _bits(alone.materialise()))
        assert (view.rows_host >= view.lo).all() and (view.rows_host <= view.hi).all()
    with pytest.raises(ValueError, match='select first'):
        view.select([0])
    assert np.array_equal(_bits(parent.materialise()), _bits(whole)) and np.array_equal(_bits(sib.materialise()), _bits(sib_before))
    assert parent.plan is None and parent.aug is None and sib.plan is None and len(parent) == 14
    view.augment(None, 0)
    if kind == 'start':
        view.reset_rows()
    view.balance(None, 0)
    assert np.array_equal(_bits(view.materialise()), _bits(whole[w]))
    # time shifts on a view (no plan)
    la, lb = view.augment(labels, 2, time_shift=True, seed=9), alone.augment(None, 0)
    alone.balance(None, 0)
    if kind == 'start':
        alone.reset_rows()
    alone.augment(labels, 2, time_shift=True, seed=9)
    assert np.array_equal(_bits(view.materialise()), _bits(alone.materialise()))
    view.augment(None, 0)
    # a view of a view is a view of the first set
    vv = view.select([2, 0])
    assert vv.planes is parent.planes and np.array_equal(_bits(vv.materialise()), _bits(whole[[9, 10, 11, 12, 13]]))
    assert np.array_equal(view.windows_of([2, 0]), [8, 0, 1, 2, 3])
    # new tables on the view stay on the view
    view.set_tables(scale * 2, shift)
    assert parent.scaler[0][0, 0] == 2.0 and sib.scaler[0][0, 0] == 2.0 and view.scaler[0][0, 0] == 4.0
    # the planes are counted once per set, as in the parent
    assert view.nbytes >= parent.planes.numel() * 4 and view.nbytes < 2 * parent.planes.numel() * 4


def test_select_refuses_a_perturbed_parent():
    _, _, _, ws, we = _sets()
    labels = np.array([0, 0, 1, 0, 2, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    for s in (ws, we):
        s.balance(labels, 1, 0)
        with pytest.raises(ValueError, match='a plan'):
            s.select([0])
        s.balance(None, 0)
        s.augment(labels, 1, drop_rate=0.5)
        with pytest.raises(ValueError, match='an augmentation'):
            s.select([0])
        s.augment(None, 0)
        assert len(s.select([0])) == 4
    ws.set_rows(ws.base_rows + np.where(ws.base_rows < ws.hi, 1, 0))
    with pytest.raises(ValueError, match='displaced'):
        ws.select([0])
    ws.reset_rows()
    ws.jitter = 1
    with pytest.raises(ValueError, match='displaced'):
        ws.select([0])


def test_stat_planes_are_the_views_runs_alone():
    """What the statistics kernels are handed: the set's own planes, a slice of them where the view's runs lie one behind the
    other, else a compact copy -- always the view's runs in the view's order and nothing else."""
    _, _, _, ws, _ = _sets()
    p, d = ws._stat_planes()
    assert p is ws.planes and (d == 0).all()
    p, d = ws.select([1, 2])._stat_planes()
    assert p.data_ptr() == ws.planes[12:].data_ptr() and p.shape[0] == 24 and d.tolist() == [-12, -12]
    p, d = ws.select([0, 1])._stat_planes()                         # (the head of the planes, but not all of them)
    assert p.data_ptr() == ws.planes.data_ptr() and p.shape[0] == 21 and d.tolist() == [0, 0]
    v = ws.select([4, 0, 3])
    p, d = v._stat_planes()
    assert p.shape[0] == 33 and d.tolist() == [-46, 11, -13]
    assert torch.equal(p, torch.cat([ws.planes[46:57], ws.planes[0:12], ws.planes[36:46]]))
    assert (v.base_rows + np.repeat(d, v.run_windows)).tolist() == [8, 0, 8, 5, 11, 20, 15, 15, 30]


# ------------------------------------------------------------------------------------------------ CVResult.summary

def test_cv_result_summary_arithmetic():
    F = crossval.FoldResult
    folds = [F(train=(90.0, 88.0, 0.3), test=(70.0, 69.0, 0.9), fit_accuracies=[50.0, 80.0, 60.0]),
             F(train=(80.0, 78.0, 0.4), test=(60.0, 59.0, 1.1), fit_accuracies=[40.0, 30.0]),
             F(train=(100.0, 99.0, 0.1), test=(80.0, 80.0, 0.5), fit_accuracies=[90.0])]
    s = crossval.CVResult(None, np.zeros(4), np.zeros(2), folds).summary()
    assert s['train_accuracy'] == 90.0 and s['test_accuracy'] == 70.0 and s['val_accuracy'] == 70.0    # peaks 80, 40, 90
    assert s['train_accuracy_std'] == pytest.approx(np.sqrt(200 / 3)) and s['test_accuracy_std'] == pytest.approx(np.sqrt(200 / 3))
    assert s['val_accuracy_std'] == pytest.approx(np.std([80.0, 40.0, 90.0]))
    for f in folds:
        f.test = None
    s = crossval.CVResult(None, np.zeros(4), None, folds).summary()
    assert s['test_accuracy'] is None and s['test_accuracy_std'] is None and s['train_accuracy'] == 90.0
    with pytest.raises(ValueError, match='no test set'):
        crossval.CVResult(None, np.zeros(4), None, folds).ensemble()
