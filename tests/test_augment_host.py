"""Augmented window sets on the host: the reflection against ``np.pad``, the counter-based generator's NumPy restatement
(deterministic, a function of the window and not of its batch, in range, uniform), the arguments of ``augment`` and of
``fit_series`` / ``fit_events``, and what ``augment`` does to a set's length, labels and ``materialise()``.  CPU tensors and a
stub owner with a vertex order of its own.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gcn_fmri_decoding_amd import _lib, decode, series

M, MP, C = 7, 32, 4
LENGTHS = [12, 9]
STARTS = [np.array([0, 8, 4, 4, 7]), np.array([5, 0, 3, 1])]
LABELS = np.array([0, 0, 1, 0, 2, 0, 1, 0, 0])


class _Owner(object):
    _M0, channel, device = M, C, torch.device('cpu')
    _order = np.array([3, 0, 4, 6, 1, 2, 5])                    # internal vertex j is the caller's vertex _order[j]
    _scale_tables = decode.Decode._scale_tables


def _sets(fold=1):
    rs = np.random.RandomState(11)
    runs = [rs.randn(T, M).astype(np.float32) for T in LENGTHS]
    owner = _Owner()
    planes = torch.zeros((sum(LENGTHS), MP), dtype=torch.float32)
    planes[:, :M] = torch.as_tensor(np.concatenate(runs)[:, owner._order])
    index = [np.concatenate([s[:, None] + np.arange(C)[None, :]] + [rs.randint(0, T, (len(s), C)) for _ in range(fold - 1)], axis=1)
             for s, T in zip(STARTS, LENGTHS)]
    ws = series.StartWindowSet(owner, planes, LENGTHS, STARTS, M, C)
    we = series.EventWindowSet(owner, planes, LENGTHS, index, M, C, fold)
    return ws, we, rs.rand(M, C).astype(np.float32) + 0.5, rs.randn(M, C).astype(np.float32)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the reflection

@pytest.mark.parametrize('Cn', [1, 2, 3, 15])
def test_reflection_is_numpy_symmetric_padding(Cn):
    x = np.random.RandomState(Cn).randn(2, 5, Cn).astype(np.float32)
    padded = np.pad(x, ((0, 0), (0, 0), (Cn, Cn)), 'symmetric')
    for r in range(Cn):
        cols = series.reflect_channels(Cn, r)
        assert cols.shape == (Cn,) and cols.min() >= 0 and cols.max() < Cn
        assert np.array_equal(x[:, :, cols], padded[:, :, r + Cn:r + 2 * Cn])
    assert np.array_equal(series.reflect_channels(Cn, np.arange(Cn)), np.stack([series.reflect_channels(Cn, r) for r in range(Cn)]))
    assert np.array_equal(series.reflect_channels(Cn, 0), np.arange(Cn))


# ------------------------------------------------------------------------------------------------ the generator

def _draw_scalar(seed, refill, i, d):
    """The generator written out once more, in Python integers, from the header's text."""
    def fin(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    a = fin((fin(seed) + refill) & 0xFFFFFFFF)
    k0 = fin((a + i) & 0xFFFFFFFF)
    k1 = fin(((a ^ 0x9E3779B9) + i * 0x85EBCA6B) & 0xFFFFFFFF)
    return fin(fin((k0 + d) & 0xFFFFFFFF) ^ k1)


def test_generator_twin_is_the_header_formula_and_deterministic():
    header = dict(re.findall(r'#define CHEBGCN_AUG_(\w+) (0x[0-9A-Fa-f]+)u', open(os.path.join(ROOT, 'include', 'chebgcn.h')).read()))
    assert {k: int(v, 16) for k, v in header.items()} == dict(
        MUL1=series.AUG_MUL1, MUL2=series.AUG_MUL2, KEY=series.AUG_KEY, WINDOW=series.AUG_WINDOW, SHIFT_DRAW=series.AUG_SHIFT_DRAW)
    assert (series.AUG_MUL1, series.AUG_MUL2, series.AUG_KEY, series.AUG_WINDOW, series.AUG_SHIFT_DRAW) \
        == (0x7FEB352D, 0x846CA68B, 0x9E3779B9, 0x85EBCA6B, 0xFFFFFFFF)
    for seed, refill, i, d in [(0, 0, 0, 0), (1, 2, 3, 4), (2 ** 32 - 1, 7, 123456, 99), (5, 2 ** 31, 2 ** 31 + 5, 0xFFFFFFFF)]:
        assert int(series.aug_draw(seed, refill, i, d)) == _draw_scalar(seed, refill, i, d)
    a = series.drop_vertices(3, 1, np.arange(50), 17, 360)
    assert a.shape == (50, 17) and a.dtype == np.int64
    assert np.array_equal(a, series.drop_vertices(3, 1, np.arange(50), 17, 360))
    for i in (0, 7, 49):
        want = [(_draw_scalar(3, 1, i, d) * 360) >> 32 for d in range(17)]
        assert series.drop_vertices(3, 1, i, 17, 360).tolist() == want == a[i].tolist()
    # seed, refill and window each change the draws
    assert not np.array_equal(a, series.drop_vertices(4, 1, np.arange(50), 17, 360))
    assert not np.array_equal(a, series.drop_vertices(3, 2, np.arange(50), 17, 360))
    assert len({tuple(r) for r in a.tolist()}) == 50
    s = series.time_shifts(3, 1, 200, 15)
    assert s.dtype == np.int32 and s.shape == (200,) and np.array_equal(s, series.time_shifts(3, 1, 200, 15))
    assert s.tolist() == [(_draw_scalar(3, 1, i, 0xFFFFFFFF) * 15) >> 32 for i in range(200)]
    assert set(s.tolist()) == set(range(15)) and not np.array_equal(s, series.time_shifts(3, 2, 200, 15))


def test_a_windows_draws_do_not_depend_on_its_batch():
    every = series.drop_vertices(9, 4, np.arange(100), 12, 33)
    rs = np.random.RandomState(0)
    for _ in range(5):
        batch = rs.permutation(100)[:rs.randint(1, 40)]
        got = series.drop_vertices(9, 4, batch, 12, 33)
        assert np.array_equal(got, every[batch])
    assert np.array_equal(series.time_shifts(9, 4, 100, 5)[:40], series.time_shifts(9, 4, 40, 5))


@pytest.mark.parametrize('Mv', [1, 2, 33, 360, 20000])
def test_draws_lie_in_range(Mv):
    v = series.drop_vertices(1, 0, np.arange(64), 2 * min(Mv, 500), Mv)
    assert v.min() >= 0 and v.max() < Mv
    if Mv <= 360:
        assert set(v.ravel().tolist()) == set(range(Mv))                         # (thousands of draws: every vertex comes up)
    s = series.time_shifts(1, 0, 1000, Mv)
    assert s.min() >= 0 and s.max() < Mv


def test_draws_are_uniform_at_360_vertices():
    """131072 draws (1024 windows of 128) at M = 360: every vertex count is binomial(n, 1/M), mean n / M = 364.1, sigma
    sqrt(n (1/M) (1 - 1/M)) = 19.05; all 360 counts lie within 6 sigma (for a true uniform source the chance that one of 360
    does not is 360 * 2e-9).  The same over the refills, and for the time shifts."""
    Mv, n_win, D = 360, 1024, 128
    n = n_win * D
    sigma = np.sqrt(n * (1.0 / Mv) * (1 - 1.0 / Mv))
    for seed, refill in [(0, 0), (0, 1), (12345, 7)]:
        counts = np.bincount(series.drop_vertices(seed, refill, np.arange(n_win), D, Mv).ravel(), minlength=Mv)
        assert len(counts) == Mv and np.abs(counts - n / Mv).max() <= 6 * sigma, np.abs(counts - n / Mv).max() / sigma
    # one window over many refills: the refill number alone decorrelates as well
    v = np.concatenate([series.drop_vertices(0, r, 5, D, Mv) for r in range(1024)])
    counts = np.bincount(v, minlength=Mv)
    assert np.abs(counts - n / Mv).max() <= 6 * sigma
    Cn = 15
    s = series.time_shifts(0, 3, n, Cn)
    sig = np.sqrt(n * (1.0 / Cn) * (1 - 1.0 / Cn))
    assert np.abs(np.bincount(s, minlength=Cn) - n / Cn).max() <= 6 * sig


# ------------------------------------------------------------------------------------------------ arguments

@pytest.mark.parametrize('kw,match', [
    (dict(copies=-1), 'copies'), (dict(copies=65), 'copies'), (dict(copies=True), 'copies'), (dict(copies=1.0), 'copies'),
    (dict(drop_rate=-0.1), 'drop_rate'), (dict(drop_rate=1.5), 'drop_rate'), (dict(drop_rate='a'), 'drop_rate'),
    (dict(drop_rate=True), 'drop_rate'), (dict(time_shift=1), 'time_shift'), (dict(drop_value=float('nan')), 'drop_value'),
    (dict(drop_value=None), 'drop_value'), (dict(seed=-1), 'seed'), (dict(seed=2 ** 32), 'seed'), (dict(seed=0.5), 'seed'),
])
def test_augment_refuses_bad_arguments(kw, match):
    ws = _sets()[0]
    args = dict(copies=2, drop_rate=0.5, time_shift=False, drop_value=1.0, seed=0)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        ws.augment(LABELS, **args)
    assert ws.aug is None and len(ws) == len(LABELS)
    with pytest.raises(ValueError, match=match):
        series.check_augment_args('fit_series', args['copies'], args['drop_rate'], args['time_shift'], args['drop_value'],
                                  args['seed'])


def test_fit_entries_take_and_check_the_arguments():
    import inspect
    for entry in (series.Series.fit_series, series.Series.fit_events):
        p = inspect.signature(entry).parameters
        assert [p[k].default for k in ('augment', 'drop_rate', 'time_shift', 'drop_value', 'augment_seed')] == [0, 0.0, False, 1.0, 0]
    args = series.Series._augment_args
    assert args('fit_series', 3, 0.25, True, 0.0, 7, 0) == (3, 0.25, True, 0.0, 7)
    with pytest.raises(ValueError, match='fit_events: the number of augmented copies'):
        args('fit_events', 65, 0.0, False, 1.0, 0, 0)
    with pytest.raises(ValueError, match='time_shift together with sampling'):
        args('fit_series', 2, 0.0, True, 1.0, 0, 2)
    assert args('fit_series', 0, 0.0, True, 1.0, 0, 2)[0] == 0                  # (no augmentation: nothing to refuse)
    with pytest.raises(ValueError, match='labels'):
        _sets()[0].augment(LABELS[:-1], 2)


# ------------------------------------------------------------------------------------------------ the set

@pytest.mark.parametrize('kind', ['start', 'event'])
@pytest.mark.parametrize('tables', [False, True])
def test_augment_tiles_the_set_and_materialise_follows_the_twins(kind, tables):
    ws, we, scale, shift = _sets(fold=2)
    w = ws if kind == 'start' else we
    if tables:
        w.set_tables(scale, shift)
    S = len(LABELS)
    base = w.materialise()
    raw = base if not tables else None
    bytes0 = w.nbytes
    new = w.augment(LABELS, 3, drop_rate=0.5, time_shift=True, drop_value=0.25, seed=6)
    assert np.array_equal(new, np.tile(LABELS, 3)) and len(w) == 3 * S and w.shape == (3 * S, M, C) and w.shape_base == (S, M, C)
    assert w.nbytes > bytes0                                                    # the shifts, the copies' table, the positions
    D = int(0.5 * M)
    assert w.aug['D'] == D == 3 and w.aug['refill'] == 0
    seen = []
    for refill in (0, 1, 2):
        if refill:
            st = w.refill()
            assert len(st) == S                                                 # (the starts stay the originals')
        assert w.aug['refill'] == refill
        shifts = series.time_shifts(6, refill, 3 * S, C)
        assert np.array_equal(w.aug['shifts'], shifts) and np.array_equal(w.aug_shifts.numpy(), shifts)
        x = w.materialise()
        assert x.shape == (3 * S, M, C) and x.dtype == np.float32
        if raw is not None:
            for i in range(3 * S):
                want = np.pad(raw[i % S], ((0, 0), (C, C)), 'symmetric')[:, shifts[i] + C:shifts[i] + 2 * C].copy()
                want[series.drop_vertices(6, refill, i, D, M)] = np.float32(0.25)
                assert np.array_equal(_bits(x[i]), _bits(want)), i
        else:
            w.set_tables(None, None)
            plain = w.materialise()
            w.set_tables(scale, shift)
            assert np.array_equal(_bits(x), _bits((plain * scale[None]).astype(np.float32) + shift[None]))
            v = series.drop_vertices(6, refill, 0, D, M)
            assert np.array_equal(_bits(x[0, v]), _bits((np.float32(0.25) * scale[v]).astype(np.float32) + shift[v]))
        seen.append(x)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    if kind == 'event':
        # the uploaded table is the index table with its columns taken through the reflection, fold by fold
        tab = w.aug_index.numpy()
        assert tab.shape == (3 * S, 2 * C)
        for i in (0, S, 3 * S - 1):
            cols = series.reflect_channels(C, w.aug['shifts'][i])
            assert np.array_equal(tab[i], np.concatenate([w.index_host[i % S][f * C + cols] for f in range(2)]))
    else:
        assert np.array_equal(w.aug_rows.numpy(), np.tile(w.rows_host, 3))
    # removed: the set it was
    assert w.augment(None, 0) is None and w.aug is None and len(w) == S and w.shape == (S, M, C)
    assert w.aug_shifts is None and w.aug_pos is None and w.nbytes == bytes0
    assert np.array_equal(_bits(w.materialise()), _bits(base))
    assert w.augment(LABELS, 0).tolist() == LABELS.tolist()


def test_positions_invert_the_owners_order_and_copies_of_one_redraw():
    ws = _sets()[0]
    base = ws.materialise()
    new = ws.augment(LABELS, 1, drop_rate=1.0)
    assert np.array_equal(new, LABELS) and len(ws) == len(LABELS) and ws.aug['D'] == M and ws.aug['shifts'] is None
    pos = ws.aug_pos.numpy()
    assert pos.dtype == np.int32 and np.array_equal(_Owner._order[pos], np.arange(M))         # position pos[v] holds vertex v
    a = ws.materialise()
    ws.refill()
    b = ws.materialise()
    assert (a == 1.0).any() and not np.array_equal(a, b)
    for i in range(len(ws)):
        v = series.drop_vertices(0, 1, i, M, M)
        assert (b[i, v] == 1.0).all()
        rest = np.setdiff1d(np.arange(M), v)
        assert np.array_equal(_bits(b[i, rest]), _bits(base[i, rest]))


def test_augment_goes_on_top_of_a_plan_and_time_shift_with_a_plan_raises():
    ws, we, _, _ = _sets()
    for w in (ws, we):
        bal = w.balance(LABELS, 2, 5, [4, 9])
        S2 = len(bal)
        assert S2 > len(LABELS)
        with pytest.raises(ValueError, match='time_shift on a balanced set'):
            w.augment(bal, 2, drop_rate=0.3, time_shift=True)
        assert w.aug is None and len(w) == S2
        mixed = w.materialise()
        new = w.augment(bal, 2, drop_rate=0.3, seed=1)
        assert np.array_equal(new, np.tile(bal, 2)) and len(w) == 2 * S2 and w.shape_base[0] == len(LABELS)
        x = w.materialise()
        D = int(0.3 * M)
        for i in range(2 * S2):
            want = mixed[i % S2].copy()
            want[series.drop_vertices(1, 0, i, D, M)] = 1.0
            assert np.array_equal(_bits(x[i]), _bits(want))
        with pytest.raises(ValueError, match='augmented'):
            w.balance(None, 0)
        with pytest.raises(ValueError, match='augmented'):
            w.balance(LABELS, 1)
        w.augment(None, 0)
        assert len(w) == S2 and np.array_equal(_bits(w.materialise()), _bits(mixed))
        assert w.balance(None, 0) is None and len(w) == len(LABELS)


def test_jitter_moves_the_copies_rows_with_the_originals():
    ws = _sets()[0]
    ws.augment(LABELS, 2, time_shift=True, seed=3)
    ws.jitter, ws.jitter_rng = 1, np.random.RandomState(0)
    ws.refill()
    assert not np.array_equal(ws.rows_host, ws.base_rows)
    assert np.array_equal(ws.aug_rows.numpy(), np.tile(ws.rows_host, 2)) and ws.aug['refill'] == 1
    ws.reset_rows()
    assert np.array_equal(ws.aug_rows.numpy(), np.tile(ws.base_rows, 2))


# ------------------------------------------------------------------------------------------------ the entries, without a GPU

def test_window_drop_entry_checks_and_launches_nothing_for_no_draws():
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    win = (ctypes.c_int32 * 2)()
    x, w = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(win, ctypes.c_void_p)
    assert lib.chebgcn_window_drop(x, w, 2, 7, 1, 0, 0, 0, None, None, None, 1.0, None) == 0          # D = 0
    assert _lib.last_dispatch() == ''
    assert lib.chebgcn_window_drop(x, w, 0, 7, 1, 3, 0, 0, None, None, None, 1.0, None) == 0          # B = 0
    assert _lib.last_dispatch() == ''
    assert lib.chebgcn_window_drop(None, w, 2, 7, 1, 3, 0, 0, None, None, None, 1.0, None) != 0
    assert b'NULL' in lib.chebgcn_last_error()
    assert lib.chebgcn_window_drop(x, w, 2, 0, 1, 3, 0, 0, None, None, None, 1.0, None) != 0
    assert lib.chebgcn_window_drop(x, w, 2, 7, 1, 3, 0, 0, None, x, None, 1.0, None) != 0
    assert b'both or neither' in lib.chebgcn_last_error()
    assert lib.chebgcn_gather_windows_reflect(None, 10, w, None, None, None, None, x, 1, 7, 2, None) != 0
    assert lib.chebgcn_gather_windows_reflect(x, 1, w, None, None, None, None, x, 1, 7, 2, None) != 0
    assert b'holds no window' in lib.chebgcn_last_error()
