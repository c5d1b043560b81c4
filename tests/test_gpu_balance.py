"""Class balancing of a ``WindowSet`` on the MI355X.  (1) chebgcn_gather_windows_mix by name: bit for bit against its float32
restatement in NumPy (sequential adds, one division, a rounded product, a rounded sum), its ``cnt == 1`` windows bit for bit
against chebgcn_gather_windows, every output within the rounding bound of the float64 mean, zero pads whatever the operands
hold in theirs.  (2) ``fit_series(sampling=2)`` against ``fit`` on the materialised balanced set: equal, not close.
(3) ``fit_series`` with ``sampling`` and ``jitter`` / ``resample``: the training replayed refill by refill on the host arrays of
a twin set.  (4) ``fit_series(sampling=0)`` is the training it was, on the kernels it ran on."""
import ctypes

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops, series

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(a).to(DEV)


# ------------------------------------------------------------------------------------------------ (1) the kernel

def _restate(planes, rows, cnt, pick, C, M, scale, shift):
    """The contract of chebgcn_gather_windows_mix in float32 NumPy, window by window."""
    out = np.zeros((len(pick), C, planes.shape[1]), np.float32)
    for b, w in enumerate(pick):
        acc = planes[rows[w, 0]:rows[w, 0] + C].copy()
        for j in range(1, cnt[w]):
            acc = acc + planes[rows[w, j]:rows[w, j] + C]                   # float32 + float32, ascending j
        acc = acc / np.float32(cnt[w])                                      # one correctly rounded division
        if scale is not None:
            acc = (acc * scale).astype(np.float32) + shift                  # a rounded product, then a rounded sum
        out[b, :, :M] = acc[:, :M]
    assert out.dtype == np.float32
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('C', [1, 3, 15])
@pytest.mark.parametrize('M', [30, 33, 64, 360])
def test_gather_windows_mix_against_float32_numpy(M, C):
    """M = 30: the pad inside the last 16-byte piece; 33: whole pieces of pad; 64: none; 360 with C = 15: 1440 pieces per
    window, two blocks, the second partly filled.  The bound against the float64 mean: n - 1 float32 adds of terms of at most
    ``a = max_j |x_j|`` lose at most (n - 1) * 2^-24 * n a (to first order; every partial sum is at most n a), the division
    by n leaves (n - 1) * 2^-24 a and adds its own rounding 2^-24 a: n * 2^-24 a -- stated as n * 2^-23 a, which covers the
    higher-order terms."""
    lib = _lib.lib()
    Mp = ops.plane_stride(M)
    Ttot, S = 100, 41
    rs = np.random.RandomState(1000 * M + C)
    planes = (rs.randn(Ttot, Mp) * (1 + rs.rand(Mp)) + rs.randn(Mp)).astype(np.float32)     # garbage in the pad as well
    scale = (rs.rand(C, Mp) + 0.5).astype(np.float32)
    shift = rs.randn(C, Mp).astype(np.float32)
    planes_d, scale_d, shift_d = dev(planes), dev(scale), dev(shift)
    perm = np.concatenate([rs.permutation(S), rs.randint(0, S, 7)]).astype(np.int32)       # a permutation with repeats
    for smax in (1, 2, 3, 8):
        rows = rs.randint(0, Ttot - C + 1, size=(S, smax)).astype(np.int64)                # entries past cnt: other valid rows
        rows[0, 0], rows[1, -1], rows[2, 0], rows[3, -1] = 0, 0, Ttot - C, Ttot - C
        cnt = rs.randint(1, smax + 1, size=S).astype(np.int32)
        cnt[:4] = [1, smax, 1, smax]
        rows_d, cnt_d = dev(rows), dev(cnt)
        rows1_d = dev(np.ascontiguousarray(rows[:, 0]))
        for sample in (None, perm):
            pick = np.arange(S) if sample is None else sample
            B = len(pick)
            sample_d = None if sample is None else dev(sample)
            for tables in (False, True):
                sc, sh = (scale_d, shift_d) if tables else (None, None)
                kind = 'tables' if tables else 'plain'
                got_d = torch.full((B, C, Mp), float('nan'), device=DEV)
                _lib.check(lib.chebgcn_gather_windows_mix(P(planes_d), Ttot, P(rows_d), P(cnt_d), smax, P(sample_d), P(sc), P(sh),
                                                          P(got_d), B, M, C, stream()), 'gather_windows_mix')
                assert _lib.last_dispatch() == 'gather_windows_mix_kernel<%s>' % kind
                got = got_d.cpu().numpy()
                want = _restate(planes, rows, cnt, pick, C, M, scale if tables else None, shift if tables else None)
                assert np.array_equal(_bits(got), _bits(want)), (smax, kind, 'differs from the float32 restatement')
                assert (got[..., M:] == 0).all()
                # cnt == 1: the plain gather on the same row, bit for bit
                one_d = torch.full((B, C, Mp), float('nan'), device=DEV)
                _lib.check(lib.chebgcn_gather_windows(P(planes_d), Ttot, P(rows1_d), P(sample_d), P(sc), P(sh), P(one_d), B, M, C,
                                                      stream()), 'gather_windows')
                assert _lib.last_dispatch() == 'gather_windows_kernel<%s>' % kind
                single = cnt[pick] == 1
                assert single.any() and np.array_equal(_bits(got[single]), _bits(one_d.cpu().numpy()[single]))
                if not tables:
                    for b, w in enumerate(pick):
                        x = np.stack([planes[r:r + C, :M] for r in rows[w, :cnt[w]]]).astype(np.float64)
                        bound = cnt[w] * 2.0 ** -23 * np.abs(x).max(axis=0)
                        assert (np.abs(got[b, :, :M] - x.mean(axis=0)) <= bound).all(), (smax, w)
    # a count outside [1, smax] is clamped into it, a row outside [0, Ttot - C] moved into it
    smax = 3
    rows = rs.randint(0, Ttot - C + 1, size=(4, smax)).astype(np.int64)
    cnt = np.array([0, -5, 9, 2], np.int32)
    rows[3] = [-4, Ttot, 5]
    got_d = torch.full((4, C, Mp), float('nan'), device=DEV)
    rows_d, cnt_d = dev(rows), dev(cnt)
    _lib.check(lib.chebgcn_gather_windows_mix(P(planes_d), Ttot, P(rows_d), P(cnt_d), smax, None, None, None, P(got_d), 4, M, C,
                                              stream()), 'gather_windows_mix')
    want = _restate(planes, np.clip(rows, 0, Ttot - C), np.clip(cnt, 1, smax), np.arange(4), C, M, None, None)
    assert np.array_equal(_bits(got_d.cpu().numpy()), _bits(want))


def test_ops_gather_windows_mix_shapes_and_refusals():
    M, C, Ttot = 33, 3, 40
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(2)
    planes = np.zeros((Ttot, Mp), np.float32)
    planes[:, :M] = rs.randn(Ttot, M)
    rows = rs.randint(0, Ttot - C + 1, size=(9, 2)).astype(np.int64)
    cnt = rs.randint(1, 3, size=9).astype(np.int32)
    out = ops.gather_windows_mix(dev(planes), dev(rows), dev(cnt), M, C)
    assert _lib.last_dispatch() == 'gather_windows_mix_kernel<plain>' and tuple(out.shape) == (9, C, Mp)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(_restate(planes, rows, cnt, np.arange(9), C, M, None, None)))
    buf = torch.empty((2, C, Mp), device=DEV)
    idx = dev(np.array([8, 8], np.int32))
    assert ops.gather_windows_mix(dev(planes), dev(rows), dev(cnt), M, C, idx, out=buf).data_ptr() == buf.data_ptr()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(_restate(planes, rows, cnt, [8, 8], C, M, None, None)))
    with pytest.raises(_lib.ChebgcnError, match='gather_windows_mix'):
        ops.gather_windows_mix(dev(planes), dev(rows[:, 0]), dev(cnt), M, C)
    with pytest.raises(_lib.ChebgcnError, match='gather_windows_mix'):
        ops.gather_windows_mix(dev(planes), dev(np.zeros((9, 17), np.int64)), dev(cnt), M, C)
    with pytest.raises(_lib.ChebgcnError, match='no CPU path'):
        ops.gather_windows_mix(dev(planes), torch.as_tensor(rows), dev(cnt), M, C)


# ------------------------------------------------------------------------------------------------ (2) - (4) training

M0, CH, NCLASS, BATCH = 30, 3, 3, 8
LENGTHS = [20, 14, 17]
_L = []


def _model(tmp_path, monkeypatch, **kw):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    if not _L:
        _L.append(graph.synthetic_graph(M0, k=4, levels=0, seed=3)[0][0])
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, [_L[0]], [4], [3], [1], [NCLASS], channel=CH, batch_size=BATCH, verbose=False,
                           dropout=1, eval_frequency=50, **kw)
    net.contraction = 'f32'
    return net


def _dataset():
    """Three runs, every window at stride 1 (45 windows), labels 28 / 6 / 11: class 1 gets 6 * (28 // 6 - 1) = 18 extra
    windows, class 2 gets 11 * (28 // 11 - 1) = 11: S' = 74."""
    rs = np.random.RandomState(11)
    runs = [(rs.randn(T, M0) * (1 + rs.rand(M0)) + rs.randn(M0)).astype(np.float32) for T in LENGTHS]
    starts = [np.arange(T - CH + 1) for T in LENGTHS]
    labels = rs.permutation(np.repeat([0, 1, 2], [28, 6, 11]))
    vrun = rs.randn(12, M0).astype(np.float32)
    vstarts = np.arange(10)
    vlabels = rs.randint(0, NCLASS, 10)
    return runs, starts, labels, vrun, vstarts, vlabels


def _fit(net, call, seed=2024):
    torch.manual_seed(7)
    np.random.seed(seed)
    net.record_fit = True
    _lib.dispatch_log = []
    try:
        out = call()
        log = list(_lib.dispatch_log)
    finally:
        _lib.dispatch_log = None
    variables = {k: net.get_var(k).copy() for k in net.variables()}
    return net.fit_log, variables, out, log


def _same_training(a, b):
    assert [i.tolist() for i in a[0]['idx']] == [i.tolist() for i in b[0]['idx']]
    assert np.array_equal(_bits(np.asarray(a[0]['loss_average'], np.float32)),
                          _bits(np.asarray(b[0]['loss_average'], np.float32))), 'loss_average streams differ'
    for k in a[1]:
        assert np.array_equal(_bits(a[1][k]), _bits(b[1][k])), k
    assert a[2][0] == b[2][0] and a[2][1] == b[2][1]


def _host_mix(runs, ws):
    """The balanced set's windows from the runs themselves (caller's vertex order, no tables): float32 adds in source order,
    one float32 division."""
    cat = np.concatenate(runs)
    (src, cnt), tab = ws.sources, ws.mix_rows_host
    x = np.empty((len(cnt), M0, CH), np.float32)
    for w in range(len(cnt)):
        acc = cat[tab[w, 0]:tab[w, 0] + CH].copy()
        for j in range(1, cnt[w]):
            acc = acc + cat[tab[w, j]:tab[w, j] + CH]
        x[w] = (acc / np.float32(cnt[w])).T
    return x


@pytest.mark.parametrize('standardize', [False, True])
def test_fit_series_sampling_equals_fit_on_the_materialised_set(standardize, tmp_path, monkeypatch):
    net = _model(tmp_path, monkeypatch, num_epochs=2, dir_name='bal')
    runs, starts, labels, vrun, vstarts, vlabels = _dataset()
    groups = [0, 0, 1]
    a = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, standardize=standardize, sampling=2,
                                         sampling_seed=5, sampling_groups=groups))
    tail = np.random.rand()
    kernels = {k for what, k in a[3] if what.startswith('gather_windows')}
    mix = 'gather_windows_mix_kernel<%s>' % ('tables' if standardize else 'plain')
    assert mix in kernels                                               # (the validation set is a plain one: the plain gather)
    assert {k for what, k in a[3] if what == 'gather_windows_mix'} == {mix}
    # the twin: the same plan from the same seed, its windows on the host
    ws, wv = net.stage_windows(runs, starts), net.stage_windows(vrun, vstarts)
    if standardize:
        ws.fit_scaler()
        wv.share_tables(ws)
    new = ws.balance(labels, 2, seed=5, groups=groups)
    S, S2 = len(labels), len(new)
    assert S2 == 74 and len(ws) == S2 and ws.shape == (S2, M0, CH) and np.bincount(new).tolist() == [28, 24, 22]
    src, cnt = ws.sources
    assert all(np.array_equal(s, src) and np.array_equal(c, cnt) for s, c in a[0]['sources']) and len(a[0]['sources']) == 2
    assert (labels[src] == new[:, None]).all() and (cnt[:S] == 1).all() and (cnt[S:] == 2).all()
    assert np.array_equal(ws.starts, np.concatenate(starts)) and all(np.array_equal(s, ws.starts) for s in a[0]['starts'])
    x = ws.materialise()
    assert x.shape == (S2, M0, CH) and x.dtype == np.float32
    raw = _host_mix(runs, ws)
    if standardize:
        scale, shift = net.window_scaler
        raw = (raw * scale[None]).astype(np.float32) + shift[None]
    assert np.array_equal(_bits(x), _bits(raw)), 'materialise() differs from the windows mixed on the host'
    got = ws.gather(net, None).planes[:, :, :M0].permute(0, 2, 1).cpu().numpy()       # the kernel, through the set
    order = np.arange(M0) if net._order is None else np.asarray(net._order)           # internal position -> vertex
    back = np.empty_like(got)
    back[:, order] = got
    assert np.array_equal(_bits(back), _bits(x))
    # over one refill every index of [0, S') is drawn once
    drawn = np.concatenate(a[0]['idx'])
    assert sorted(drawn[:S2].tolist()) == list(range(S2)) and drawn.max() == S2 - 1
    b = _fit(net, lambda: net.fit(x, new, wv.materialise(), vlabels))
    assert np.random.rand() == tail                                     # the global stream saw fit's draws only
    _same_training(a, b)
    # balance(sampling = 0) removes the plan
    assert ws.balance(labels, 0).tolist() == labels.tolist() and len(ws) == S and ws.sources is None
    ws.gather(net, None)
    assert _lib.last_dispatch().startswith('gather_windows_kernel<')


@pytest.mark.parametrize('sampling,jitter,resample', [(1, 2, False), (3, 1, True), (2, 0, True)])
def test_fit_series_sampling_with_jitter_and_resample_refill_by_refill(sampling, jitter, resample, tmp_path, monkeypatch):
    """The set changes at every refill, so the comparison is a replay: a twin set driven by hand through the same refills
    gives the host array of every epoch (``materialise()``), and the recorded batches are trained again, step by step, out
    of those arrays.  Both runs are eager (a replay cannot share fit's captured step)."""
    monkeypatch.setenv('CHEBGCN_STEP_GRAPH', '0')
    net = _model(tmp_path, monkeypatch, num_epochs=2, dir_name='balj')
    runs, starts, labels, vrun, vstarts, vlabels = _dataset()
    kw = dict(jitter=jitter, jitter_seed=4)
    a = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, sampling=sampling, sampling_seed=3,
                                         resample=resample, **kw))
    assert not net.fit_captured
    assert any(k == 'gather_windows_mix_kernel<plain>' for _, k in a[3])
    log = a[0]
    nrefill = len(log['starts'])
    assert nrefill == 2 and len(log['sources']) == 2
    ws = net.stage_windows(runs, starts)
    new = ws.balance(labels, sampling, seed=3, resample=resample)
    S, S2 = len(labels), len(new)
    assert S2 == 74
    ws.jitter, ws.jitter_rng = jitter, np.random.RandomState(4)
    base = np.concatenate(starts)
    hi = np.concatenate([np.full(len(s), T - CH) for s, T in zip(starts, LENGTHS)])
    arrays, plans = [], []
    for r in range(nrefill):
        st = ws.refill()
        assert np.array_equal(st, log['starts'][r]) and st.shape == (S,)
        src, cnt = ws.sources
        assert np.array_equal(src, log['sources'][r][0]) and np.array_equal(cnt, log['sources'][r][1])
        assert (labels[src] == new[:, None]).all()
        # every source of an extra window starts within `jitter` of its source's start, inside the source's run
        got = ws.mix_rows_host[S:] - ws.offsets[src[S:]]
        assert (np.abs(got - base[src[S:]]) <= jitter).all() and (got >= 0).all() and (got <= hi[src[S:]]).all()
        assert np.array_equal(ws.mix_rows_host[:S], np.repeat((st + ws.offsets)[:, None], src.shape[1], 1))
        x = ws.materialise()
        assert np.array_equal(_bits(x), _bits(_host_mix(runs, ws)))
        arrays.append(net.stage(x))
        plans.append((src.copy(), ws.mix_rows_host.copy()))
    if resample:
        assert not np.array_equal(plans[0][0], plans[1][0])
    if jitter:
        assert not np.array_equal(plans[0][1][S:], plans[1][1][S:])
        moved = plans[0][1][S:] - ws.base_rows[plans[0][0][S:]]
        assert moved.min() < 0 < moved.max()                                # the copies move, each on its own
    # the originals move exactly as in a run without balancing under the same jitter_seed
    c = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, **kw))
    assert len(c[0]['starts']) >= 2 and 'sources' not in c[0]
    assert all(np.array_equal(s, t) for s, t in zip(log['starts'], c[0]['starts']))
    assert not any(k.startswith('gather_windows_mix') for _, k in c[3])
    # the replay
    drawn = np.concatenate(log['idx'])
    assert sorted(drawn[:S2].tolist()) == list(range(S2))
    torch.manual_seed(7)
    net._init_variables()
    labels_d = dev(new.astype(np.int64))
    trace, have, r = [], 0, -1
    for idx in log['idx']:
        if have < BATCH:
            have += S2
            r += 1
        have -= BATCH
        idx_d = dev(idx.astype(np.int32))
        _, la = net.train_step(net._gather(arrays[r], idx_d), labels_d[idx_d.long()])
        trace.append(float(la))
    assert r == nrefill - 1
    assert np.array_equal(_bits(np.asarray(trace, np.float32)), _bits(np.asarray(log['loss_average'], np.float32)))
    for k, v in a[1].items():
        assert np.array_equal(_bits(net.get_var(k)), _bits(v)), k


def test_fit_series_without_sampling_is_the_training_it_was(tmp_path, monkeypatch):
    net = _model(tmp_path, monkeypatch, num_epochs=2, dir_name='bal0')
    runs, starts, labels, vrun, vstarts, vlabels = _dataset()
    a = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, sampling=0))
    kernels = {k for what, k in a[3] if what.startswith('gather_windows')}
    assert kernels == {'gather_windows_kernel<plain>'}
    assert not any('gather_windows_mix' in what or 'gather_windows_mix' in k for what, k in a[3])
    assert 'sources' not in a[0]
    ws, wv = net.stage_windows(runs, starts), net.stage_windows(vrun, vstarts)
    b = _fit(net, lambda: net.fit(ws, labels, wv, vlabels))
    _same_training(a, b)
