"""Event designs on the host: ``events.match_events`` against what the reference's ``matching_fmri_data_to_trials_event``
returned on recorded designs (tests/golden/events_*.npz, written by tools/gen_events_golden.py), against a plain per-trial
restatement on ragged designs the reference cannot run under NumPy 2, every refusal of ``match_events`` / ``stage_windows(index=)``
/ ``stage_events`` / ``fit_events`` before device work, and the new library entry points in the ABI test's style.  No GPU."""
import ctypes
import glob
import os

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, events, models_gcn
from gcn_fmri_decoding_amd import graph as graph_mod
from test_abi_and_host import declared_symbols

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = sorted(os.path.basename(p)[len('events_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'events_*.npz')))
MATCH_KW = ('start_trial', 'hrf_delay', 'flag_event', 'TRstep')


def _load(name):
    z = np.load(os.path.join(GOLDEN, 'events_%s.npz' % name))
    n = int(z['nruns'])
    runs = [z['run%d' % i] for i in range(n)]
    designs = [z['design%d' % i].tolist() for i in range(n)]
    kw = {k: int(z[k]) for k in MATCH_KW}
    return z, runs, designs, z['target_name'].tolist(), int(z['block_dura']), kw


def _fold_by_hand(run, index, fold):
    """The gather's formula in float32, element by element: adds in ascending f, one division."""
    S, Cin = index.shape
    C = Cin // fold
    out = np.empty((S, run.shape[1], C), np.float32)
    for s in range(S):
        for c in range(C):
            acc = run[index[s, c]].astype(np.float32)
            for f in range(1, fold):
                acc = (acc + run[index[s, f * C + c]]).astype(np.float32)
            out[s, :, c] = acc / np.float32(fold) if fold > 1 else acc
    return out


def test_the_fixtures_are_there():
    assert set(FIXTURES) >= {'base', 'start_plus2', 'start_minus2', 'remainder', 'clip', 'trstep2', 'adjacent', 'hrf2', 'merge',
                             'merge_trstep3'}


@pytest.mark.parametrize('name', FIXTURES)
def test_match_events_reproduces_the_reference(name):
    z, runs, designs, targets, block_dura, kw = _load(name)
    ev = events.match_events(designs, targets, block_dura, **kw)
    fold = kw['TRstep']
    assert ev.kept == list(range(len(runs))) and ev.fold == fold and ev.channel == block_dura // fold
    assert ev.block_dura == block_dura and ev.trial_dura == int(z['trial_dura'])
    assert ev.classes == sorted(set(targets)) and len(ev) == z['labels'].size
    for r, run in enumerate(runs):
        idx, lab = ev.index[r], ev.labels[r]
        want = z['windows'][r]                                              # [S, M, channel]
        assert idx.dtype == np.int64 and idx.shape == (want.shape[0], block_dura) and idx.min() >= 0 and idx.max() < len(run)
        assert lab.dtype == np.int64 and np.array_equal(lab, z['labels'][r])
        assert [ev.classes[i] for i in lab] == z['label_names'][r].tolist()
        got = events.host_windows(run, idx, fold)
        assert got.dtype == np.float32 and got.shape == want.shape
        if fold == 1:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        else:
            assert np.array_equal(got.view(np.uint32), _fold_by_hand(run, idx, fold).view(np.uint32))
            ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()     # np.mean's order is NumPy's own


def test_what_the_fixtures_exercise():
    """The recorded designs really hold the cases a contiguous window cannot express."""
    ev = {n: events.match_events(*_load(n)[2:5], **_load(n)[5]) for n in ('clip', 'merge', 'adjacent', 'remainder', 'hrf2')}
    clip = ev['clip'].index[0]
    assert (np.diff(clip, axis=1)[:, :7] == 1).all() and (np.diff(clip, axis=1)[:, 7:] == 0).all()      # 8 TRs, the last x 5
    steps = np.concatenate([np.diff(i, axis=1).ravel() for i in ev['merge'].index])
    assert (steps > 1).any() and (steps >= 1).all()                          # a chunk straddles the rest between two trials
    assert all((np.diff(i, axis=1) == 1).all() for i in ev['adjacent'].index)
    assert len(set(ev['adjacent'].labels[0][:4].tolist())) == 2              # two adjacent trials, two conditions, split
    assert all(len(i) == 4 for i in ev['remainder'].index)                   # 8 // 6 = 1 window per trial, 2 TRs dropped
    z, runs, designs, targets, bd, kw = _load('hrf2')
    plain = events.match_events(designs, targets, bd)
    assert all(np.array_equal(a, b + 2) for a, b in zip(ev['hrf2'].index, plain.index))


# ------------------------------------------------------------------------------------------------ ragged designs

def _restate(run, names, targets, block_dura):
    """The rules per trial, on the data: keep the target TRs, split where the condition changes, drop a short last trial, cut
    chunks or pad by repeating the last volume.  (start_trial = hrf_delay = 0, TRstep = 1.)"""
    classes = sorted(set(targets))
    keep = [t for t, n in enumerate(names) if n in targets]
    trials = []
    for t in keep:
        if trials and names[trials[-1][-1]] == names[t]:
            trials[-1].append(t)
        else:
            trials.append([t])
    if not trials or len(trials[-1]) < block_dura or len(trials[-1]) < 4:
        trials = trials[:-1]
    xs, ys = [], []
    for tr in trials:
        if len(tr) < block_dura:
            rows = tr + [tr[-1]] * (block_dura - len(tr))
            xs.append(run[rows].T)
            ys.append(classes.index(names[tr[0]]))
        for k in range(len(tr) // block_dura):
            xs.append(run[tr[k * block_dura:(k + 1) * block_dura]].T)
            ys.append(classes.index(names[tr[0]]))
    return xs, ys, [len(tr) for tr in trials]


def _ragged():
    rs = np.random.RandomState(5)
    targets = ['b', 'a', 'c']
    designs = [
        ['rest'] * 2 + ['a'] * 7 + ['rest'] + ['b'] * 3 + ['c'] * 11 + ['rest'] * 2 + ['a'] * 5 + ['rest'] + ['a'] * 4 + ['b'] * 9,
        ['rest'] * 9 + ['x'] * 4,                                            # no target at all: skipped
        ['c'] * 13 + ['rest'] + ['b'] * 2 + ['rest'] * 3 + ['a'] * 6 + ['rest'],
        ['a'] * 3,                                                           # one trial, shorter than 4: skipped
        ['b'] * 5 + ['a'] * 2 + ['rest', 'c', 'rest', 'c', 'c', 'c'] + ['b'] * 4,
    ]
    runs = [rs.randn(len(d), 6).astype(np.float32) for d in designs]
    return runs, designs, targets


@pytest.mark.parametrize('block_dura', [1, 4, 5, 9])
def test_ragged_designs_against_a_per_trial_restatement(block_dura):
    runs, designs, targets = _ragged()
    ev = events.match_events(designs, targets, block_dura, flag_event=1)
    want = [(r,) + _restate(runs[r], designs[r], targets, block_dura) for r in range(len(runs))]
    want = [w for w in want if w[1]]
    assert ev.kept == [w[0] for w in want] and 1 not in ev.kept and 3 not in ev.kept
    assert len({len(l) for l in ev.labels}) > 1                             # runs with different window counts
    for (r, xs, ys, _), idx, lab in zip(want, ev.index, ev.labels):
        assert np.array_equal(events.host_windows(runs[r], idx), np.stack(xs)) and lab.tolist() == ys
    assert ev.trial_dura == min(want[-1][3])                                 # the reference's Trial_dura: of the last run kept


def test_start_trial_and_hrf_delay_on_a_ragged_design():
    names = ['rest'] * 3 + ['a'] * 6 + ['rest'] * 4 + ['b'] * 9 + ['rest'] * 3
    ev = events.match_events([names], ['a', 'b'], 3, flag_event=1)
    assert ev.index[0].tolist() == [[3, 4, 5], [6, 7, 8], [13, 14, 15], [16, 17, 18], [19, 20, 21]]
    assert ev.labels[0].tolist() == [0, 0, 1, 1, 1] and ev.trial_dura == 6
    # start_trial > 0: every trial loses its first TRs;  < 0: it starts earlier, and the rest entries take the trial's label
    ev = events.match_events([names], ['a', 'b'], 3, start_trial=2, flag_event=1)
    assert ev.index[0].tolist() == [[5, 6, 7], [15, 16, 17], [18, 19, 20]] and ev.labels[0].tolist() == [0, 1, 1]
    ev = events.match_events([names], ['a', 'b'], 4, start_trial=-2, flag_event=1)
    assert ev.index[0].tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [11, 12, 13, 14], [15, 16, 17, 18]]
    assert ev.labels[0].tolist() == [0, 0, 1, 1] and ev.trial_dura == 8
    # hrf_delay wraps around the end of the run: a trial that ends the run continues at its beginning
    names = ['rest'] * 2 + ['a'] * 5 + ['rest'] * 2 + ['b'] * 4
    ev = events.match_events([names], ['a', 'b'], 2, hrf_delay=3, flag_event=1)
    # design rolled right by 3: b b b | rest rest a a a a a rest rest b   ->  kept rows 0 1 2 | 5 .. 9 | 12
    assert ev.index[0].tolist() == [[0, 1], [5, 6], [7, 8]] and ev.labels[0].tolist() == [1, 0, 0]     # the last trial (1 TR) dropped
    assert events.match_events([names], ['a', 'b'], 2, hrf_delay=-3, flag_event=1).index[0].tolist() == \
        events.match_events([names], ['a', 'b'], 2, flag_event=1).index[0].tolist()
    # a custom rest name
    ev = events.match_events([[n if n != 'rest' else 'fix' for n in names]], ['a', 'b'], 2, start_trial=-1, flag_event=1, rest='fix')
    assert ev.index[0][0].tolist() == [1, 2]
    # a kept TR whose label is no target (a cue in front of a trial, start_trial < 0): the reference's encoder raises
    with pytest.raises(ValueError, match='not in target_name'):
        events.match_events([['rest', 'cue', 'a', 'a', 'a', 'a', 'rest']], ['a'], 2, start_trial=-1)
    with pytest.warns(UserWarning, match='only 4 TRs'):
        events.match_events([['a'] * 4 + ['rest']], ['a'], 2)


def test_match_events_refusals():
    good = dict(label_runs=[['rest', 'a', 'a', 'a', 'a', 'rest']], target_name=['a'], block_dura=2, flag_event=1)
    assert len(events.match_events(**good)) == 2
    for kw, word in ((dict(block_dura=0), 'block_dura'), (dict(block_dura=2.0), 'block_dura'), (dict(block_dura=True), 'block_dura'),
                     (dict(block_dura=None), 'block_dura'), (dict(start_trial=1.5), 'start_trial'), (dict(start_trial='1'), 'start_trial'),
                     (dict(hrf_delay=0.5), 'hrf_delay'), (dict(hrf_delay=False), 'hrf_delay'), (dict(TRstep=0), 'TRstep'),
                     (dict(TRstep=17, block_dura=34), 'TRstep'), (dict(TRstep=1.0), 'TRstep'), (dict(flag_event=2), 'flag_event'),
                     (dict(flag_event='no'), 'flag_event'), (dict(block_dura=4, TRstep=3), 'multiple of TRstep'),
                     (dict(block_dura=3, TRstep=2), 'multiple of TRstep'), (dict(rest=0), 'rest'),
                     (dict(target_name=[]), 'target_name'), (dict(target_name='a'), 'target_name'), (dict(target_name=[1]), 'target_name'),
                     (dict(target_name=None), 'target_name'), (dict(label_runs=[]), 'label_runs'), (dict(label_runs='aaaa'), 'label_runs'),
                     (dict(label_runs=None), 'label_runs'), (dict(label_runs=[[]]), 'run 0'), (dict(label_runs=[[0, 1, 1]]), 'run 0'),
                     (dict(label_runs=[good['label_runs'][0], [['a', 'a']]]), 'run 1'), (dict(label_runs=[['a', 1, None]]), 'run 0'),
                     (dict(label_runs=['aaaa']), 'run 0')):
        with pytest.raises(ValueError, match=word) as e:
            events.match_events(**dict(good, **kw))
        assert 'match_events' in str(e.value)
    # nothing kept is a result, not an error
    ev = events.match_events([['rest'] * 5], ['a'], 2)
    assert ev.kept == [] and ev.index == [] and ev.labels == [] and len(ev) == 0 and ev.trial_dura == 0


def test_entry_points_refuse_before_device_work():
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    net = models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 3], channel=3, batch_size=4, verbose=False)
    run = np.zeros((12, 60), np.float32)
    names = ['rest', 'a', 'a', 'a', 'a', 'a', 'a', 'rest', 'b', 'b', 'b', 'b']
    tab = np.array([[0, 1, 2], [5, 5, 5], [11, 3, 0]])
    # stage_windows(index=)
    for kw, word in ((dict(starts=[0]), 'mutually exclusive'), (dict(fold=2), 'index table'), (dict(fold=0), 'fold'),
                     (dict(fold=17), 'fold'), (dict(fold=True), 'fold'), (dict(index=tab.astype(np.float32)), 'index table'),
                     (dict(index=tab[0]), 'index table'), (dict(index=tab[:0]), 'index table'), (dict(index=tab + 10), 'row'),
                     (dict(index=tab - 1), 'row'), (dict(index=[tab, tab]), 'index table'), (dict(series=[run, run]), 'one'),
                     (dict(series=[run, run], index=[tab]), 'one'), (dict(series=run[:, :5]), 'series'), (dict(series=[]), 'empty'),
                     (dict(scale=np.ones((60, 3), np.float32)), 'scale and shift'),
                     (dict(scale=np.ones((60, 2), np.float32), shift=np.ones((60, 2), np.float32)), 'scale')):
        with pytest.raises(ValueError, match=word) as e:
            net.stage_windows(**dict(dict(series=run, index=tab), **kw))
        assert 'stage_windows' in str(e.value)
    with pytest.raises(ValueError, match='fold goes with index'):
        net.stage_windows(run, [0, 1], fold=2)
    for kw in (dict(series=run, index=tab), dict(series=[run, run], index=[tab, tab[:1]]),
               dict(series=run, index=np.tile(tab, 2), fold=2)):
        with pytest.raises(RuntimeError, match='device'):                    # valid: they reach the device check
            net.stage_windows(**kw)
    # stage_events / fit_events
    good = dict(series=[run, run], label_runs=[names, names], target_name=['a', 'b'], block_dura=3, flag_event=1)
    for kw, word in ((dict(block_dura=4), 'channel'), (dict(block_dura=6, TRstep=3), 'channel'), (dict(block_dura=3.0), 'block_dura'),
                     (dict(label_runs=[names]), 'event designs'), (dict(label_runs=[names, names[:-1]]), 'design of 11'),
                     (dict(target_name=['x']), 'no run yields'), (dict(target_name=['a', 'b', 'rest', 'c']), 'classes'),
                     (dict(TRstep=2), 'TRstep'), (dict(jitter=1), 'jitter'), (dict(series=[run[:, :7], run]), 'series')):
        with pytest.raises(ValueError, match=word) as e:
            net.stage_events(**dict(good, **kw))
        assert 'stage_events' in str(e.value)
        fkw = dict(dict(good, **kw))
        fkw.update(train_series=fkw.pop('series'), train_label_runs=fkw.pop('label_runs'), val_series=run, val_label_runs=names)
        with pytest.raises(ValueError, match=word) as e:
            net.fit_events(**fkw)
        assert 'fit_events' in str(e.value)
    fit_good = dict(train_series=[run, run], train_label_runs=[names, names], val_series=run, val_label_runs=names,
                    target_name=['a', 'b'], block_dura=3, flag_event=1)
    for kw, word in ((dict(sampling=17), 'sampling'), (dict(sampling=True), 'sampling'), (dict(sampling=2, seed=-1), 'seed'),
                     (dict(sampling=2, groups=[0]), 'groups'), (dict(sampling=1, groups=[0.5, 1.0]), 'groups'),
                     (dict(val_label_runs=names[:-2]), 'design of 10')):
        with pytest.raises(ValueError, match=word) as e:
            net.fit_events(**dict(fit_good, **kw))
        assert 'fit_events' in str(e.value)
    with pytest.raises(RuntimeError, match='device'):
        net.stage_events(**good)
    for kw in (dict(), dict(standardize=True, sampling=2, seed=3, groups=[7, 7]), dict(start_trial=1, block_dura=3)):
        with pytest.raises(RuntimeError, match='device'):
            net.fit_events(**dict(fit_good, **kw))


def test_indexed_entry_points_abi():
    names = declared_symbols()
    for n in ('chebgcn_gather_windows_indexed', 'chebgcn_window_stats_indexed', 'chebgcn_window_stats_indexed_workspace'):
        assert n in names and n in _lib.SIGNATURES
    lib = _lib.lib()
    # the workspace: 4 * C * Mp doubles (every sum a pair) per chunk of max(16, ceil(S / 32)) windows
    assert lib.chebgcn_window_stats_indexed_workspace(10, 360, 15) == 1 * 4 * 15 * 384 * 8
    assert lib.chebgcn_window_stats_indexed_workspace(17, 33, 1) == 2 * 4 * 1 * 64 * 8
    assert lib.chebgcn_window_stats_indexed_workspace(3888, 360, 15) == 32 * 4 * 15 * 384 * 8
    for bad in ((0, 360, 15), (10, 0, 15), (10, 360, 0), (2 ** 31, 360, 15)):
        assert lib.chebgcn_window_stats_indexed_workspace(*bad) == 0
    buf = (ctypes.c_float * 4096)()
    tab = (ctypes.c_int64 * 16)()
    num = (ctypes.c_int32 * 4)()
    p, t, n = (ctypes.cast(a, ctypes.c_void_p) for a in (buf, tab, num))
    EINVAL = -1

    def gather(series=p, T=8, idx=t, S=2, Cin=6, fold=2, src=None, cnt=None, W=0, smax=0, sample=None, scale=None, shift=None,
               out=p, B=2, M=32, C=3):
        return lib.chebgcn_gather_windows_indexed(series, T, idx, S, Cin, fold, src, cnt, W, smax, sample, scale, shift, out, B,
                                                  M, C, None)
    for kw in (dict(series=None), dict(idx=None), dict(out=None), dict(src=t), dict(cnt=n), dict(src=t, cnt=n, W=2, smax=0),
               dict(src=t, cnt=n, W=2, smax=17), dict(src=t, cnt=n, W=0, smax=2), dict(fold=0), dict(fold=17, Cin=51),
               dict(Cin=5), dict(Cin=3), dict(S=0), dict(T=0), dict(scale=p), dict(shift=p), dict(B=0), dict(B=65536), dict(M=0),
               dict(C=0, Cin=0), dict(series=ctypes.c_void_p(p.value + 4)), dict(out=ctypes.c_void_p(p.value + 8))):
        assert gather(**kw) == EINVAL, kw
        assert b'gather_windows_indexed' in lib.chebgcn_last_error(), kw

    def stats(series=p, T=8, idx=t, S=2, Cin=6, fold=2, scale=p, shift=p, M=32, C=3, ws=p, nbytes=1 << 20):
        return lib.chebgcn_window_stats_indexed(series, T, idx, S, Cin, fold, None, None, scale, shift, M, C, ws, nbytes, None)
    for kw in (dict(series=None), dict(idx=None), dict(scale=None), dict(shift=None), dict(ws=None), dict(S=0), dict(T=0),
               dict(M=0), dict(C=0, Cin=0), dict(fold=0), dict(fold=17, Cin=51), dict(Cin=4), dict(nbytes=16),
               dict(series=ctypes.c_void_p(p.value + 4))):
        assert stats(**kw) == EINVAL, kw
        assert b'window_stats_indexed' in lib.chebgcn_last_error(), kw
