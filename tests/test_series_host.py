"""stage_windows / fit_series on the host: every refusal of the two public methods (raised before any device work, on a
shape-only model), the row table of a list of runs, the start displacement of ``jitter`` (a pure NumPy function), the two new
library entry points in the ABI test's style, and the optional ``window_scaler`` key of a checkpoint.  No GPU."""
import ctypes
import io

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, models_gcn, series
from gcn_fmri_decoding_amd import graph as graph_mod
from test_abi_and_host import declared_symbols


def _meta_model(**kw):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=3, batch_size=4,
                            verbose=False, **kw)


OK = np.zeros((9, 60), np.float32)
BAD_STAGE = [
    (dict(series=np.zeros((2, 60))), 'shorter'),
    (dict(series=np.zeros((9, 59))), 'series'),
    (dict(series=np.zeros((9, 60, 3))), 'series'),
    (dict(series=[]), 'empty'),
    (dict(series=np.array([['a'] * 60] * 9)), 'numeric'),
    (dict(series=OK, starts=[7]), 'start'),
    (dict(series=OK, starts=[-1]), 'start'),
    (dict(series=OK, starts=[0.5]), 'starts'),
    (dict(series=OK, starts=[]), 'starts'),
    (dict(series=[OK, OK], starts=[0, 1]), 'list'),
    (dict(series=[OK, np.zeros((2, 60))]), 'shorter'),
    (dict(series=OK, scale=np.ones((60, 2)), shift=np.ones((60, 3))), 'scale'),
    (dict(series=OK, scale=np.ones((60, 3)), shift=np.ones((3, 60))), 'shift'),
    (dict(series=OK, scale=np.ones((60, 3))), 'both or neither'),
    (dict(series=OK, shift=np.ones((60, 3))), 'both or neither'),
]


@pytest.mark.parametrize('kw,word', BAD_STAGE)
def test_stage_windows_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word) as e:
        net.stage_windows(**kw)
    assert 'stage_windows' in str(e.value) and 'decode_series' not in str(e.value)


def test_valid_stage_windows_arguments_reach_the_device_check():
    net = _meta_model()
    for kw in (dict(), dict(starts=[6, 0, 6]), dict(scale=np.ones((60, 3)), shift=np.zeros((60, 3)))):
        with pytest.raises(RuntimeError, match='device'):
            net.stage_windows(OK, **kw)
    with pytest.raises(RuntimeError, match='device'):
        net.stage_windows([OK, np.zeros((3, 60))], starts=[[0, 1], [0]])


def test_fit_series_arguments_raise_before_device_work():
    net = _meta_model()
    good = dict(train_series=OK, train_starts=[0, 3, 6], train_labels=[0, 1, 2], val_series=OK, val_starts=[1, 2],
                val_labels=[0, 1])
    for kw, word in ((dict(train_series=np.zeros((2, 60))), 'shorter'), (dict(val_starts=[7]), 'start'),
                     (dict(train_labels=[0, 1]), 'train_labels'), (dict(val_labels=[[0, 1]]), 'val_labels'),
                     (dict(jitter=-1), 'jitter'), (dict(jitter=1.5), 'jitter'), (dict(jitter=True), 'jitter'),
                     (dict(jitter_seed=-1), 'jitter_seed'), (dict(jitter_seed='a'), 'jitter_seed')):
        with pytest.raises(ValueError, match=word) as e:
            net.fit_series(**dict(good, **kw))
        assert 'fit_series' in str(e.value)
    with pytest.raises(RuntimeError, match='device'):
        net.fit_series(**good)
    assert net.window_scaler is None


def test_row_table_of_several_runs():
    rows, lo, hi = series.row_table([20, 9, 15], [[5, 0, 5, 3], [1], [0, 7, 7]], 8)
    assert rows.dtype == lo.dtype == hi.dtype == np.int64
    assert rows.tolist() == [5, 0, 5, 3, 21, 29, 36, 36]           # run offsets 0, 20, 29; the caller's order, repeats kept
    assert lo.tolist() == [0, 0, 0, 0, 20, 29, 29, 29]
    assert hi.tolist() == [12, 12, 12, 12, 21, 36, 36, 36]         # offset + T - C: the last row a window of the run starts at
    assert (rows >= lo).all() and (rows <= hi).all()
    rows, lo, hi = series.row_table([8], [np.array([0], np.int32)], 8)
    assert rows.tolist() == lo.tolist() == hi.tolist() == [0] and rows.dtype == np.int64


def test_jitter_rows_bounds_clipping_and_determinism():
    rows, lo, hi = series.row_table([40, 12, 30], [np.arange(0, 33, 4), [0, 4], np.arange(0, 23)], 8)
    j = 3
    seen = set()
    for seed in range(20):
        out = series.jitter_rows(rows, lo, hi, j, np.random.RandomState(seed))
        assert out.dtype == np.int64 and out.shape == rows.shape
        assert (out >= lo).all() and (out <= hi).all()                      # the window stays inside its own run
        inner = (rows - j >= lo) & (rows + j <= hi)
        assert (np.abs(out - rows)[inner] <= j).all() and (np.abs(out - rows) <= j).all()
        seen.update((out - rows)[inner].tolist())
        again = series.jitter_rows(rows, lo, hi, j, np.random.RandomState(seed))
        assert np.array_equal(out, again)                                   # a function of the seed alone
    assert seen == set(range(-j, j + 1))                                    # every displacement of [-j, j] occurs
    a = series.jitter_rows(rows, lo, hi, j, np.random.RandomState(0))
    b = series.jitter_rows(rows, lo, hi, j, np.random.RandomState(1))
    assert not np.array_equal(a, b)
    # at the edges of a run the displaced start is clipped, not wrapped into the neighbouring run
    edge = series.jitter_rows(np.array([40, 44]), np.array([40, 40]), np.array([44, 44]), 50, np.random.RandomState(3))
    assert set(edge.tolist()) <= {40, 44}
    rs = np.random.RandomState(5)
    state = rs.get_state()[1].copy()
    same = series.jitter_rows(rows, lo, hi, 0, rs)
    assert np.array_equal(same, rows) and same is not rows and np.array_equal(rs.get_state()[1], state)    # j = 0 draws nothing
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='jitter'):
            series.jitter_rows(rows, lo, hi, bad, rs)


def test_jitter_leaves_the_global_numpy_stream_alone():
    rows, lo, hi = series.row_table([50], [np.arange(0, 40)], 8)
    np.random.seed(123)
    want = np.random.permutation(17)
    np.random.seed(123)
    series.jitter_rows(rows, lo, hi, 4, np.random.RandomState(9))
    assert np.array_equal(np.random.permutation(17), want)


def test_series_entry_points_abi():
    names = declared_symbols()
    for n in ('chebgcn_gather_windows', 'chebgcn_window_stats', 'chebgcn_window_stats_workspace'):
        assert n in names and n in _lib.SIGNATURES
    lib = _lib.lib()
    # workspace arithmetic: the count table (Ttot + C - 1 + 8 + 4 ints, rounded to 16 bytes) + ceil(Ttot / 512) chunks of
    # 4 * C * Mp float64 partials (every sum a pair of doubles)
    assert lib.chebgcn_window_stats_workspace(1000, 360, 15) == ((1000 + 14 + 12) * 4 + 15) // 16 * 16 + 2 * 4 * 15 * 384 * 8
    assert lib.chebgcn_window_stats_workspace(512, 33, 1) == (512 + 12) * 4 + 1 * 4 * 1 * 64 * 8
    for bad in ((0, 360, 15), (1000, 0, 15), (1000, 360, 0), (1 << 31, 360, 15)):
        assert lib.chebgcn_window_stats_workspace(*bad) == 0
    buf = (ctypes.c_float * 4096)()
    tab = (ctypes.c_int64 * 4)()
    p, t = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(tab, ctypes.c_void_p)
    EINVAL = -1

    def gather(series=p, T=8, rows=t, sample=None, scale=None, shift=None, out=p, B=2, M=32, C=3):
        return lib.chebgcn_gather_windows(series, T, rows, sample, scale, shift, out, B, M, C, None)
    for kw in (dict(series=None), dict(rows=None), dict(out=None), dict(scale=p), dict(shift=p), dict(B=0), dict(B=65536),
               dict(M=0), dict(C=0), dict(T=2), dict(series=ctypes.c_void_p(p.value + 4))):
        assert gather(**kw) == EINVAL, kw
        assert b'gather_windows' in lib.chebgcn_last_error()

    def stats(series=p, T=8, rows=t, S=4, scale=p, shift=p, M=32, C=3, ws=p, nbytes=4096 * 4):
        return lib.chebgcn_window_stats(series, T, rows, S, None, None, scale, shift, M, C, ws, nbytes, None)
    for kw in (dict(series=None), dict(rows=None), dict(scale=None), dict(shift=None), dict(ws=None), dict(S=0), dict(M=0),
               dict(C=0), dict(T=2), dict(nbytes=64)):
        assert stats(**kw) == EINVAL, kw
        assert b'window_stats' in lib.chebgcn_last_error()


def test_window_scaler_round_trips_through_a_checkpoint():
    net = _meta_model()
    assert net.window_scaler is None
    sd = {n: torch.zeros(net._spec(n).ref_shape) for n in net.variables()}
    assert 'window_scaler' not in net._scaler_to_sd({})                  # no scaler: the checkpoint is what it was
    net.load_state_dict(sd)                                              # a checkpoint without the key loads
    assert net.window_scaler is None
    rs = np.random.RandomState(0)
    scale, shift = rs.rand(60, 3).astype(np.float32) + 0.5, rs.randn(60, 3).astype(np.float32)
    net.window_scaler = (scale, shift)
    extra = net._scaler_to_sd({})
    assert list(extra) == ['window_scaler'] and tuple(extra['window_scaler'].shape) == (2, 60, 3)
    f = io.BytesIO()
    torch.save(dict(sd, **extra), f)                                     # (the form _save_best writes and _restore reads)
    f.seek(0)
    back = torch.load(f, weights_only=True)
    other = _meta_model()
    other.load_state_dict(back)
    assert np.array_equal(other.window_scaler[0], scale) and np.array_equal(other.window_scaler[1], shift)
    other.load_state_dict(sd)                                            # ... and a later one without it clears them
    assert other.window_scaler is None
    with pytest.raises(ValueError, match='window_scaler'):
        other.load_state_dict(dict(sd, window_scaler=torch.zeros(2, 59, 3)))
