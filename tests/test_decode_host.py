"""decode_series on the host: the window-start arithmetic and the chunk plan of the shared path, every ValueError of the public
method (raised before any device work, on a shape-only model), the float64 reference on host-cut windows the GPU tests compare
against, checked here against a literal per-window loop, and the two new library entry points in the ABI test's style.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, decode, models_gcn
from gcn_fmri_decoding_amd import graph as graph_mod
from test_saliency_host import SPECS, RefNet, random_params


def host_windows(series, starts, C):
    """The model inputs decode_series stands for, cut on the host: x[w][v][c] = series[starts[w] + c][v]."""
    series, starts = np.asarray(series), np.asarray(starts, np.int64)
    return np.ascontiguousarray(series[starts[:, None] + np.arange(C)[None, :]].transpose(0, 2, 1))


def reference_logits(ref, P, series, starts, C):
    """Float64 logits [W, classes] of RefNet on the host-cut windows."""
    ref.margin = None                   # (RefNet keeps a per-window minimum over its calls: another number of windows starts afresh)
    with torch.no_grad():
        return ref.logits(P, torch.as_tensor(host_windows(np.asarray(series, np.float64), starts, C))).numpy()


def test_window_starts():
    ws = decode.window_starts
    assert ws(20, 15).tolist() == [0, 1, 2, 3, 4, 5] and ws(20, 15).dtype == np.int64
    assert ws(20, 15, stride=2).tolist() == [0, 2, 4]
    assert ws(20, 15, stride=15).tolist() == [0]
    assert ws(46, 15, stride=15).tolist() == [0, 15, 30]
    assert ws(46, 15, stride=20).tolist() == [0, 20]
    assert ws(15, 15).tolist() == [0]
    assert ws(7, 1).tolist() == list(range(7))
    assert ws(20, 15, starts=[5, 0, 5, 3]).tolist() == [5, 0, 5, 3]           # the caller's order, repeats kept
    assert ws(20, 15, starts=np.array([5], np.int32)).dtype == np.int64
    for kw in (dict(T=14, C=15), dict(T=20, C=15, stride=0), dict(T=20, C=15, stride=1.5), dict(T=20, C=15, stride=True),
               dict(T=20, C=15, starts=[6]), dict(T=20, C=15, starts=[-1]), dict(T=20, C=15, starts=[]),
               dict(T=20, C=15, starts=[0.0]), dict(T=20, C=15, starts=[[0]]), dict(T=20, C=15, starts=[True])):
        with pytest.raises(ValueError, match='decode_series'):
            ws(**kw)


@pytest.mark.parametrize('T,C,chunk', [(100, 15, 40), (100, 15, 15), (100, 15, 100), (100, 15, 1000), (31, 3, 4), (50, 1, 7)])
def test_chunk_plan_covers_every_window_once(T, C, chunk):
    rs = np.random.RandomState(T + C + chunk)
    for starts in (np.arange(T - C + 1), rs.randint(0, T - C + 1, 64), np.array([T - C, 0, T - C])):
        plan = decode.chunk_plan(starts, T, C, chunk)
        seen = np.concatenate([idx for _, _, idx in plan])
        assert sorted(seen.tolist()) == list(range(len(starts)))
        for (t0, t1, idx), nxt in zip(plan, plan[1:] + [None]):
            assert 0 <= t0 < t1 <= T and t1 - t0 <= max(chunk, C) and len(idx)
            assert (starts[idx] >= t0).all() and (starts[idx] + C <= t1).all()
            assert t0 % (min(chunk, 10 ** 9) - (C - 1)) == 0          # chunk origins step by chunk - (C - 1): an overlap of C - 1
    with pytest.raises(ValueError, match='chunk'):
        decode.chunk_plan(np.arange(3), 20, 15, 14)


def _meta_model(**kw):
    Ls = graph_mod.synthetic_graph(60, k=4, levels=0, seed=1)[0]
    return models_gcn.cgcnn({'device': 'meta'}, Ls * 2, [4, 4], [3, 3], [1, 1], [8, 5], channel=3, batch_size=4,
                            verbose=False, **kw)


OK = np.zeros((9, 60), np.float32)
BAD = [
    (dict(series=np.zeros((2, 60))), 'shorter'),
    (dict(series=np.zeros((9, 59))), 'series'),
    (dict(series=np.zeros((9, 60, 3))), 'series'),
    (dict(series=np.zeros(60)), 'series'),
    (dict(series=[]), 'empty'),
    (dict(series=np.array([['a'] * 60] * 9)), 'numeric'),
    (dict(series=OK, starts=[7]), 'start'),
    (dict(series=OK, starts=[-1]), 'start'),
    (dict(series=OK, starts=[0.5]), 'starts'),
    (dict(series=OK, starts=[]), 'starts'),
    (dict(series=[OK, OK], starts=[0, 1]), 'list'),
    (dict(series=[OK, OK], starts=[[0]]), 'list'),
    (dict(series=[OK, np.zeros((2, 60))]), 'shorter'),
    (dict(series=OK, stride=0), 'stride'),
    (dict(series=OK, stride=2.0), 'stride'),
    (dict(series=OK, scale=np.ones((60, 2))), 'scale'),
    (dict(series=OK, shift=np.ones((3, 60))), 'shift'),
    (dict(series=OK, share='yes'), 'share'),
    (dict(series=OK, share=1.5), 'share'),
    (dict(series=OK, batch_size=0), 'batch_size'),
    (dict(series=OK, batch_size=2.0), 'batch_size'),
    (dict(series=OK, output='argmax'), 'output'),
    (dict(series=OK, max_stack_bytes=0), 'max_stack_bytes'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_decode_series_arguments_raise_before_device_work(kw, word):
    net = _meta_model()
    with pytest.raises(ValueError, match=word):
        net.decode_series(**kw)
    assert net.last_decode_path is None and net._windows is None


def test_valid_arguments_reach_the_device_check():
    net = _meta_model()
    for kw in (dict(), dict(starts=[6, 0, 6]), dict(stride=4, output='labels'), dict(scale=np.ones((60, 3)), share=False),
               dict(share=True, batch_size=7, output='probabilities')):
        with pytest.raises(RuntimeError, match='device'):
            net.decode_series(OK, **kw)
    with pytest.raises(RuntimeError, match='device'):
        net.decode_series([OK, np.zeros((3, 60))], starts=[[0, 1], [0]])
    with pytest.raises(RuntimeError, match='device'):
        net.decode_series(torch.zeros((9, 60), dtype=torch.float64))


def test_host_windows_is_the_literal_cut():
    rs = np.random.RandomState(0)
    series = rs.randn(23, 11)
    starts = np.array([8, 0, 3, 8, 19])
    x = host_windows(series, starts, 4)
    assert x.shape == (5, 11, 4)
    for w, s in enumerate(starts):
        for v in range(11):
            for c in range(4):
                assert x[w, v, c] == series[s + c, v]


@pytest.mark.parametrize('name', sorted(SPECS))
def test_reference_on_windows_is_the_per_window_loop(name):
    """The float64 reference evaluated on all host-cut windows at once equals a literal loop that cuts and runs one window at
    a time (to float64 round-off: the batched matrix products may sum in another order)."""
    s = SPECS[name]
    Ls = graph_mod.synthetic_graph(s['N'], k=4, levels=s['levels'], seed=0)[0]
    L = Ls + [Ls[-1]] * max(0, len(s['p']) - len(Ls))
    C = 3
    ref = RefNet(L, s['F'], s['K'], s['p'], s['M'], s['filter'], s['brelu'], s['pool'])
    P = random_params(s, C, L[0].shape[0], 1)
    series = np.random.RandomState(2).randn(12, L[0].shape[0])
    starts = decode.window_starts(12, C, stride=2)
    z = reference_logits(ref, P, series, starts, C)
    assert z.shape == (len(starts), s['M'][-1])
    for w, st in enumerate(starts):
        x = np.stack([series[st + c] for c in range(C)], axis=1)[None]          # [1, M, C]
        with torch.no_grad():
            one = ref.logits(P, torch.as_tensor(x)).numpy()[0]
        assert np.abs(one - z[w]).max() <= 1e-12 * max(np.abs(z[w]).max(), 1.0)


def test_windows_entry_points_abi():
    lib = _lib.lib()
    assert lib.chebgcn_contract_fwd_windows_supported(64, 10466, 15, 5, 32, 1) == 1
    assert lib.chebgcn_contract_fwd_windows_supported(3, 360, 1, 1, 1, 4) == 1
    for bad in ((64, 10466, 15, 5, 33, 1), (64, 10466, 15, 5, 256, 1), (0, 100, 3, 3, 4, 1), (65536, 100, 3, 3, 4, 1),
                (4, 0, 3, 3, 4, 1), (4, 100, 0, 3, 4, 1), (4, 100, 3, 0, 4, 1), (4, 100, 3, 3, 0, 1), (4, 100, 3, 3, 4, 3),
                (4, 100, 3, 3, 4, 8), (4, 100, 3, 3, 4, 256), (4, 100, 3, 3, 4, 0)):
        assert lib.chebgcn_contract_fwd_windows_supported(*bad) == 0, bad
    buf = (ctypes.c_float * 4096)()
    tab = (ctypes.c_int32 * 4)()
    p, t = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(tab, ctypes.c_void_p)

    def call(stack=p, T=8, starts=t, W=p, bias=None, bias_kind=0, out=p, B=2, M=32, C=3, K=2, Fout=4, pool=1, pool_kind=0):
        return lib.chebgcn_contract_fwd_windows(stack, T, starts, W, bias, bias_kind, out, None, B, M, C, K, Fout, pool, pool_kind,
                                                1, None)
    EINVAL, EUNSUPPORTED = -1, -4
    for kw in (dict(stack=None), dict(starts=None), dict(W=None), dict(out=None), dict(B=0), dict(M=0), dict(C=0), dict(K=0),
               dict(Fout=0), dict(B=65536), dict(T=2), dict(T=1 << 31), dict(pool=3), dict(pool=64), dict(bias_kind=1),
               dict(bias_kind=3, bias=p), dict(pool_kind=2)):
        assert call(**kw) == EINVAL, kw
        assert b'contract_fwd_windows' in lib.chebgcn_last_error()
    assert call(Fout=33) == EUNSUPPORTED                       # valid, not served: never a launch
    assert b'not served' in lib.chebgcn_last_error()
