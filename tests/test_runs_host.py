"""``runs``: the one copy of what the analysis entry points do before their kernels -- the run list, the group keys, staging as
planes -- and of the NumPy ``aug_draw``, without a device (``stage`` is plain torch and runs with ``device='cpu'``).  The plane
stride is M rounded up to 32, so M is taken on both sides of it; the runs have 1, 2 and 3 rows, the one-row run first or last."""
import sys

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, glm, runs, searchlight as sl, series, stats

WIDTHS = (1, 31, 32, 33)
ENTRY_POINTS = ('first_level', 'single_trial', 'searchlight_events', 'crossnobis_events')


def make(M, rows=(1, 2, 3), seed=0):
    rng = np.random.RandomState(seed + M)
    return [(100.0 * rng.randn(T, M)).astype(np.float32) for T in rows]


def as_kind(arrays, kind):
    """The same float32 values as arrays, CPU tensors, both in turn, float64 or (rounded) integer arrays."""
    if kind == 'tensors':
        return [torch.as_tensor(a.copy()) for a in arrays]
    if kind == 'mixed':
        return [torch.as_tensor(a.copy()) if i % 2 else a for i, a in enumerate(arrays)]
    if kind == 'float64':
        return [a.astype(np.float64) for a in arrays]
    return list(arrays)


# ---- stage ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows', [(1, 2, 3), (3, 2, 1)])
@pytest.mark.parametrize('kind', ['arrays', 'tensors', 'mixed', 'float64', 'int'])
@pytest.mark.parametrize('M', WIDTHS)
def test_stage_writes_every_run_at_its_offset(M, kind, rows):
    arrays = make(M, rows)
    if kind == 'int':
        arrays = [np.round(a) for a in arrays]
        given = [a.astype(np.int32) for a in arrays]
    else:
        given = as_kind(arrays, kind)
    checked, single, width, tensors = runs.as_runs(given, 't')
    assert not single and width == M and tensors == (kind == 'tensors')
    offs = runs.offsets(checked)
    assert offs.dtype == np.int64 and offs.tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist() and offs[-1] == 6
    dev, planes = runs.stage(checked, M, 'cpu', 't')
    Mp = _lib.plane_stride(M)
    want = np.zeros((6, Mp), np.float32)
    for a, o in zip(arrays, offs):
        want[o:o + a.shape[0], :M] = a
    assert dev == torch.device('cpu') and planes.dtype == torch.float32 and tuple(planes.shape) == (6, Mp)
    assert planes.is_contiguous() and not planes.requires_grad
    assert np.array_equal(planes.numpy(), want)
    assert not planes[:, M:].any()                              # the padding columns: exactly zero


@pytest.mark.parametrize('tensor', [False, True])
@pytest.mark.parametrize('M', WIDTHS)
def test_one_run_and_a_list_of_one_agree(M, tensor):
    y = make(M, rows=(3,))[0]
    y = torch.as_tensor(y) if tensor else y
    one, single, width, tensors = runs.as_runs(y, 't')
    many, listed, _, _ = runs.as_runs([y], 't')
    assert single and not listed and width == M and tensors == tensor and len(one) == len(many) == 1
    assert torch.equal(runs.stage(one, M, 'cpu', 't')[1], runs.stage(many, M, 'cpu', 't')[1])


def test_stage_takes_a_tensor_that_requires_grad():
    arrays = make(33)
    given = [torch.as_tensor(a.copy()).requires_grad_() for a in arrays]
    planes = runs.stage(given, 33, 'cpu', 't')[1]
    assert not planes.requires_grad and torch.equal(planes, runs.stage(arrays, 33, 'cpu', 't')[1])


@pytest.mark.parametrize('who', ENTRY_POINTS)
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_values_are_refused(who, bad, monkeypatch):
    arrays = make(33)
    arrays[1][1, 32] = bad                                      # the last vertex of a middle run
    for kind in ('tensors', 'mixed'):                           # (mixed: run 1 is the tensor)
        with pytest.raises(ValueError) as e:
            runs.stage(as_kind(arrays, kind), 33, 'cpu', who)
        assert str(e.value) == '%s: series hold non-finite values' % who
    monkeypatch.setitem(sys.modules, 'torch', None)             # a host array: refused before torch is so much as imported
    with pytest.raises(ValueError) as e:
        runs.stage(arrays, 33, 'cpu', who)
    assert str(e.value) == '%s: series hold non-finite values' % who
    with pytest.raises(ImportError):
        runs.stage(make(33), 33, 'cpu', who)


@pytest.mark.parametrize('who', ENTRY_POINTS)
def test_series_that_are_no_numbers_are_refused(who, monkeypatch):
    arrays = make(2)
    monkeypatch.setitem(sys.modules, 'torch', None)
    for other, name in ((arrays[1] > 0, 'bool'), (arrays[1].astype(complex), 'complex128'), (arrays[1].astype(str), '<U32')):
        with pytest.raises(ValueError) as e:
            runs.stage([arrays[0], other, arrays[2]], 2, 'cpu', who)
        assert str(e.value) == '%s: series of dtype %s' % (who, name)
    assert runs.host_array(arrays[1] > 0, who, any_dtype=True).dtype == np.float32          # (what connectivity_graph asks for)


# ---- as_runs --------------------------------------------------------------------------------------------------------------------

def test_as_runs_refusals_carry_who():
    y = np.zeros((3, 4), np.float32)
    for given, kw, text in [([], {}, 'who: no runs'),
                            ([y, np.zeros(4)], {}, 'who: every run must be [T, M]'),
                            (np.zeros((2, 3, 4)), {}, 'who: a run must be [T, M], got shape (2, 3, 4)'),
                            (torch.zeros(4), {}, 'who: a run must be [T, M], got shape (4,)'),
                            ([y, np.zeros((3, 5))], {}, 'who: runs differ in the number of vertices (or have none)'),
                            ([np.zeros((3, 0))], {}, 'who: runs differ in the number of vertices (or have none)'),
                            ([y, np.zeros((1, 4))], dict(min_rows=2), 'who: every run needs at least 2 rows'),
                            ([y, np.zeros((1, 4))], dict(min_rows=2, rows='a run is too short'), 'who: a run is too short')]:
        with pytest.raises(ValueError) as e:
            runs.as_runs(given, 'who', **kw)
        assert str(e.value) == text
    assert runs.as_runs([np.zeros((3, 0))], 'who', min_cols=0)[2] == 0
    assert runs.as_runs([y, np.zeros((1, 4))], 'who', min_rows=1)[2] == 4
    assert runs.as_runs([[[1.0, 2.0]], y[:, :2]], 'who')[0][0].shape == (1, 2)              # (a nested list is a run)


# ---- group_keys -----------------------------------------------------------------------------------------------------------------

def test_group_keys():
    groups, keys, members = runs.group_keys(['b', 'a', 'b', ('c', 1), 'a', 'b'], 6, 'who')
    assert groups == ['b', 'a', 'b', ('c', 1), 'a', 'b'] and keys == ['b', 'a', ('c', 1)]    # first appearance, 'b' again after 'a'
    assert members == [[0, 2, 5], [1, 4], [3]]
    assert runs.group_keys(None, 3, 'who') == ([0, 0, 0], [0], [[0, 1, 2]])
    assert runs.group_keys(iter([7, 7]), 2, 'who')[2] == [[0, 1]]
    with pytest.raises(ValueError) as e:
        runs.group_keys(['a', ['b'], 'c'], 3, 'who')
    assert str(e.value) == "who: group key ['b'] of run 1 is not hashable"
    with pytest.raises(ValueError) as e:
        runs.group_keys(['a', 'b'], 3, 'who')
    assert str(e.value) == 'who: groups must hold one key per run (3 runs, 2 keys)'
    with pytest.raises(ValueError) as e:
        runs.group_keys([{}], 1, 'who', 'sample')
    assert str(e.value) == 'who: group key {} of sample 0 is not hashable'
    with pytest.raises(ValueError) as e:
        runs.group_keys([], 2, 'who', 'sample')
    assert str(e.value) == 'who: groups must hold one key per sample (2 samples, 0 keys)'


# ---- the entry points say what they said ----------------------------------------------------------------------------------------

NAMES = ['rest', 'a', 'a', 'rest', 'b', 'b', 'rest', 'a', 'a', 'rest', 'b', 'b']


def entry(who, given, groups=None):
    """The entry point ``who`` on ``given``, with arguments that are in order otherwise (no device is reached)."""
    n = len(given) if isinstance(given, list) else 1
    if who == 'first_level':
        return glm.first_level(given, [glm.design_matrix(names=NAMES, high_pass=None)] * n, groups=groups)
    if who == 'single_trial':
        return glm.single_trial(given, [glm.trial_design(names=NAMES, high_pass=None)] * n, groups=groups)
    fn = sl.searchlight_events if who == 'searchlight_events' else sl.crossnobis_events
    return fn(given, [NAMES] * n, ['a', 'b'], 2, None, groups=groups)


@pytest.mark.parametrize('who', ENTRY_POINTS)
def test_entry_points_keep_their_messages(who):
    y = np.zeros((len(NAMES), 4), np.float32)
    events = who.endswith('_events')
    malformed = '%s: runs must be a non-empty list of [T, M] arrays' % who
    for given, groups, text in [
            ([], None, malformed if events else '%s: no runs' % who),
            ([y, y[0]], None, malformed if events else '%s: every run must be [T, M]' % who),
            (np.zeros((2, 3, 4)), None, '%s: a run must be [T, M], got shape (2, 3, 4)' % who),
            (y[0], None, '%s: a run must be [T, M], got shape (4,)' % who),
            ([y, y[:, :3]], None, '%s: runs differ in the number of vertices (or have none)' % who),
            ([y[:, :0]], None, '%s: runs differ in the number of vertices (or have none)' % who),
            ([y, y], ['s1'], '%s: groups must hold one key per run (2 runs, 1 keys)' % who),
            ([y, y], ['s1', ['s2']], "%s: group key ['s2'] of run 1 is not hashable" % who)]:
        with pytest.raises(ValueError) as e:
            entry(who, given, groups)
        assert str(e.value) == text


# ---- aug_draw -------------------------------------------------------------------------------------------------------------------

# series.aug_draw(seed, refill, i, d) for i (rows) and d (columns) in (0, 1, 2**32 - 1), as it was before it moved here
AUG_RECORDED = {
    (0, 0): [[2926543089, 3818772927, 584422765], [88723713, 4010709068, 2019726839], [2795973851, 1823927873, 806950628]],
    (0, 1): [[2851025512, 1011709769, 2875062983], [643845433, 2670661481, 3141127963], [3962384953, 2033900211, 2248123013]],
    (11, 0): [[1312316894, 261093610, 4068856532], [239242244, 1775796217, 3727531937], [2008167120, 1457991555, 4181105082]],
    (11, 1): [[1883656094, 1728119196, 2499423890], [321002216, 3980586977, 553741696], [1679532823, 2134795012, 1880634386]]}


def test_aug_draw_matches_the_recorded_values():
    assert series.aug_draw is runs.aug_draw and stats.aug_draw is runs.aug_draw
    assert (series.AUG_MUL1, series.AUG_MUL2, series.AUG_KEY, series.AUG_WINDOW) == (0x7FEB352D, 0x846CA68B, 0x9E3779B9, 0x85EBCA6B)
    v = np.array([0, 1, 2 ** 32 - 1], np.uint64)
    for (seed, refill), want in AUG_RECORDED.items():
        got = runs.aug_draw(seed, refill, v[:, None], v[None, :])
        assert got.dtype == np.uint64 and got.tolist() == want
        assert [[int(runs.aug_draw(seed, refill, int(i), int(d))) for d in v] for i in v] == want
