"""Class balancing of a ``WindowSet`` on the host: the plan ``series.balance_plan`` (a pure NumPy function: the top-up rule, the
sources of every extra window, groups, determinism, the global stream left alone), every refusal, and the new library entry
point chebgcn_gather_windows_mix in the ABI test's style.  No GPU."""
import ctypes

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, models_gcn, series
from gcn_fmri_decoding_amd import graph as graph_mod
from test_abi_and_host import declared_symbols


def _labels(counts, seed=0):
    """Shuffled labels with the given number of windows per class."""
    lab = np.concatenate([np.full(n, c, np.int64) for c, n in counts.items()])
    return np.random.RandomState(seed).permutation(lab)


def _groups(S, n, seed=1):
    return np.random.RandomState(seed).randint(0, n, S)


@pytest.mark.parametrize('sampling', [1, 2, 3, 16])
def test_top_up_rule(sampling):
    labels = _labels({0: 10, 1: 5, 2: 4, 3: 6})
    src, cnt, new = series.balance_plan(labels, _groups(25, 4), sampling, np.random.RandomState(0))
    # class 1: 2 * 5 <= 10, 5 * (int(10 / 5) - 1) = 5 extra; class 2: 4 * (int(10 / 4) - 1) = 4; class 3: 2 * 6 > 10, none
    assert len(new) == 25 + 5 + 4 == 34 and src.shape == (34, max(1, sampling)) and cnt.shape == (34,)
    assert src.dtype == np.int64 and cnt.dtype == np.int32
    assert np.array_equal(new[:25], labels)
    assert new[25:].tolist() == [1] * 5 + [2] * 4                            # ascending label order
    assert np.array_equal(src[:25], np.repeat(np.arange(25)[:, None], src.shape[1], 1)) and (cnt[:25] == 1).all()
    assert np.bincount(new).tolist() == [10, 10, 8, 6]
    # {0: 9, 1: 4}: int(9 / 4) - 1 = 1 extra window per window of class 1
    labels = _labels({0: 9, 1: 4})
    src, cnt, new = series.balance_plan(labels, _groups(13, 3), sampling, np.random.RandomState(0))
    assert len(new) == 13 + 4 and new[13:].tolist() == [1] * 4
    # a balanced set (and one whose small class has MORE than half of the largest) gets nothing
    for counts in ({0: 6, 1: 6, 2: 6}, {0: 9, 1: 5}):
        labels = _labels(counts)
        src, cnt, new = series.balance_plan(labels, _groups(len(labels), 3), sampling, np.random.RandomState(0))
        assert len(new) == len(labels) and np.array_equal(new, labels) and (cnt == 1).all()
    # labels need not be 0 .. n-1
    labels = np.array([7] * 6 + [-2] * 2 + [40] * 3)
    src, cnt, new = series.balance_plan(labels, np.zeros(11, np.int64), sampling, np.random.RandomState(0))
    assert new[11:].tolist() == [-2] * 4 + [40] * 3


@pytest.mark.parametrize('sampling', [1, 2, 5])
def test_sources_of_the_extra_windows(sampling):
    labels = _labels({0: 40, 1: 7, 2: 13, 3: 25}, seed=3)
    groups = _groups(len(labels), 6, seed=4)
    S = len(labels)
    np.random.seed(77)
    state = np.random.get_state()[1].copy()
    src, cnt, new = series.balance_plan(labels, groups, sampling, np.random.RandomState(5))
    assert np.array_equal(np.random.get_state()[1], state)                   # the global NumPy stream is untouched
    assert len(new) == S + 7 * 4 + 13 * 2
    assert (src >= 0).all() and (src < S).all()                              # sources are ORIGINAL windows
    assert (labels[src] == new[:, None]).all()                               # every source carries its window's label
    assert (cnt[:S] == 1).all() and (cnt[S:] == (1 if sampling == 1 else sampling)).all()
    # the same seed: the same plan; another seed: another
    again = series.balance_plan(labels, groups, sampling, np.random.RandomState(5))
    other = series.balance_plan(labels, groups, sampling, np.random.RandomState(6))
    assert all(np.array_equal(a, b) for a, b in zip((src, cnt, new), again))
    assert not np.array_equal(src, other[0]) and np.array_equal(cnt, other[1]) and np.array_equal(new, other[2])
    # draws with replacement out of the whole class: with 28 extra windows of a class of 7, several sources occur
    assert len(np.unique(src[S:S + 28])) > 1
    if sampling > 1:
        assert any(len(set(r.tolist())) > 1 for r in src[S:])               # a synthetic window mixes different windows


def test_groups_confine_the_sources():
    labels = _labels({0: 30, 1: 6, 2: 9}, seed=8)
    S = len(labels)
    groups = np.random.RandomState(9).randint(0, 5, S)
    groups[labels == 1] = 3                                                  # every window of class 1 lies in group 3
    groups[labels == 2] = np.where(np.arange(9) % 2 == 0, 0, 4)              # class 2 only in groups 0 and 4
    for sampling in (1, 2, 4):
        src, cnt, new = series.balance_plan(labels, groups, sampling, np.random.RandomState(2))
        assert (groups[src[new == 1]] == 3).all()
        assert set(groups[src[new == 2]].ravel().tolist()) <= {0, 4}
    # one group in all: the pool of a class is that class, and a class of ONE window is averaged with itself
    labels = np.array([0, 0, 0, 0, 1])
    src, cnt, new = series.balance_plan(labels, np.zeros(5, np.int64), 3, np.random.RandomState(0))
    assert len(new) == 5 + 3 and (src[5:] == 4).all() and (cnt[5:] == 3).all()


def test_refusals():
    labels, groups = _labels({0: 9, 1: 4}), _groups(13, 3)
    rs = np.random.RandomState(0)
    for bad in (17, -1, True, 2.0, 0, '2', None):
        with pytest.raises(ValueError, match='sampling'):
            series.balance_plan(labels, groups, bad, rs)
    for kw in (dict(labels=labels.astype(np.float32)), dict(labels=labels[:, None]), dict(groups=groups[:-1]),
               dict(groups=groups.astype(np.float64)), dict(labels=np.zeros(0, np.int64), groups=np.zeros(0, np.int64))):
        args = dict(dict(labels=labels, groups=groups), **kw)
        with pytest.raises(ValueError, match='balance_plan'):
            series.balance_plan(args['labels'], args['groups'], 2, rs)
    assert series.check_sampling(0, 'x') == 0 and series.check_sampling(np.int64(16), 'x') == 16


def test_fit_series_sampling_arguments_raise_before_device_work():
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    net = models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=3, batch_size=4, verbose=False)
    run = np.zeros((9, 60), np.float32)
    good = dict(train_series=[run, run], train_starts=[[0, 3, 6], [1, 2]], train_labels=[0, 1, 0, 0, 0], val_series=run,
                val_starts=[1, 2], val_labels=[0, 1], sampling=2)
    for kw, word in ((dict(sampling=17), 'sampling'), (dict(sampling=-1), 'sampling'), (dict(sampling=True), 'sampling'),
                     (dict(sampling=2.0), 'sampling'), (dict(sampling_seed=-1), 'seed'), (dict(sampling_seed=1.5), 'seed'),
                     (dict(sampling_groups=[0]), 'groups'), (dict(sampling_groups=[0.5, 1.0]), 'groups'),
                     (dict(resample=1), 'resample'), (dict(train_labels=[0., 1., 0., 0., 0.]), 'labels')):
        with pytest.raises(ValueError, match=word) as e:
            net.fit_series(**dict(good, **kw))
        assert 'fit_series' in str(e.value)
    for kw in (dict(), dict(sampling=0), dict(sampling=1, sampling_groups=[4, 4], resample=True, sampling_seed=9)):
        with pytest.raises(RuntimeError, match='device'):                    # valid: they reach the device check
            net.fit_series(**dict(good, **kw))


def test_gather_windows_mix_abi():
    names = declared_symbols()
    assert 'chebgcn_gather_windows_mix' in names and 'chebgcn_gather_windows_mix' in _lib.SIGNATURES
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    tab = (ctypes.c_int64 * 8)()
    num = (ctypes.c_int32 * 4)()
    p, t, n = (ctypes.cast(a, ctypes.c_void_p) for a in (buf, tab, num))
    EINVAL = -1

    def mix(series=p, T=8, rows=t, cnt=n, smax=2, sample=None, scale=None, shift=None, out=p, B=2, M=32, C=3):
        return lib.chebgcn_gather_windows_mix(series, T, rows, cnt, smax, sample, scale, shift, out, B, M, C, None)
    for kw in (dict(smax=0), dict(cnt=None), dict(smax=17), dict(smax=-1), dict(series=None), dict(rows=None), dict(out=None),
               dict(scale=p), dict(shift=p), dict(B=0), dict(B=65536), dict(M=0), dict(C=0), dict(T=2),
               dict(series=ctypes.c_void_p(p.value + 4)), dict(out=ctypes.c_void_p(p.value + 8))):
        assert mix(**kw) == EINVAL, kw
        assert b'gather_windows_mix' in lib.chebgcn_last_error(), kw
