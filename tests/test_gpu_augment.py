"""Augmented training windows on the MI355X.  (1) chebgcn_window_drop and chebgcn_gather_windows_reflect through ``ops``, bit for
bit against the NumPy twins (``series.drop_vertices``, ``series.reflect_channels``): integer draws and float32 operations of one
rounding each on both sides, so the comparison is ``np.array_equal`` on the bit patterns -- no tolerance.  (2) augmented
``StartWindowSet`` / ``EventWindowSet``: ``gather`` of every index equals ``materialise()`` over two refills, on top of a balance
plan, and on a model whose input level is relabelled.  (3) ``fit_series(augment=...)`` trains on the copies, and
``augment = 0`` is the training it was, on the kernels it ran on."""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops, series

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def dev(a):
    return torch.as_tensor(a).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ (1) the kernels

@pytest.mark.parametrize('C', [1, 3, 15])
@pytest.mark.parametrize('M', [1, 33, 360, 1030])
def test_window_drop_against_the_numpy_twin(M, C):
    """M = 1: every draw is vertex 0; 33: one real vertex in the last plane piece; 1030: a level the model would relabel.
    B * D from 0 over one partly filled block (B = 1, D = 1) to many (64 * 2060 draws), D = 2 M: more draws than vertices,
    repeats certain.  The batch holds garbage in its pad: whatever is not a drawn (vertex, channel) entry must keep its bits."""
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(100 * M + C)
    scale = (rs.rand(C, Mp) + 0.5).astype(np.float32)
    shift = rs.randn(C, Mp).astype(np.float32)
    pos = rs.permutation(M).astype(np.int32)
    scale_d, shift_d, pos_d = dev(scale), dev(shift), dev(pos)
    for B in (1, 5, 64):
        x0 = rs.randn(B, C, Mp).astype(np.float32)
        win = rs.randint(0, 2 ** 31 - 1, size=B).astype(np.int32)
        win[0] = 0
        win_d = dev(win)
        for D in (0, 1, M // 2, M, 2 * M):
            seed, refill = int(rs.randint(0, 2 ** 32, dtype=np.uint64)), int(rs.randint(0, 1000))
            v = series.drop_vertices(seed, refill, win.astype(np.int64), D, M)          # [B, D]
            assert v.shape == (B, D)
            for tables, dv in ((False, 1.0), (True, 1.0), (True, 0.0)):
                for relabel in (False, True):
                    x_d = dev(x0.copy())
                    got_d = ops.window_drop(x_d, win_d, M, D, seed, refill, pos_d if relabel else None,
                                            scale_d if tables else None, shift_d if tables else None, dv)
                    assert got_d.data_ptr() == x_d.data_ptr()
                    name = '' if D == 0 else 'window_drop_kernel<%s>' % ('tables' if tables else 'plain')
                    assert _lib.last_dispatch() == name
                    want = x0.copy()
                    touched = np.zeros((B, Mp), bool)
                    for b in range(B):
                        p = pos[v[b]] if relabel else v[b]
                        if tables:
                            want[b][:, p] = (np.float32(dv) * scale[:, p]).astype(np.float32) + shift[:, p]
                        else:
                            want[b][:, p] = np.float32(dv)
                        touched[b, p] = True
                    got = got_d.cpu().numpy()
                    assert np.array_equal(_bits(got), _bits(want)), (B, D, tables, dv, relabel)
                    assert not touched[:, M:].any()
                    keep = np.broadcast_to(~touched[:, None, :], got.shape)
                    assert np.array_equal(_bits(got[keep]), _bits(x0[keep]))            # untouched entries and the pad


def test_window_drop_refusals_and_a_position_table_out_of_range():
    M, C, B = 33, 2, 3
    Mp = ops.plane_stride(M)
    x = torch.zeros((B, C, Mp), device=DEV)
    win = dev(np.arange(B, dtype=np.int32))
    with pytest.raises(_lib.ChebgcnError, match='window_drop'):
        ops.window_drop(x[:, :, :M], win, M, 4, 0, 0)
    with pytest.raises(_lib.ChebgcnError, match='win'):
        ops.window_drop(x, win[:2], M, 4, 0, 0)
    with pytest.raises(_lib.ChebgcnError, match='pos'):
        ops.window_drop(x, win, M, 4, 0, 0, pos=win)
    with pytest.raises(_lib.ChebgcnError, match='no CPU path'):
        ops.window_drop(x.cpu(), win, M, 4, 0, 0)
    with pytest.raises(_lib.ChebgcnError, match='both or neither'):
        ops.window_drop(x, win, M, 4, 0, 0, scale=torch.ones((C, Mp), device=DEV))
    # entries of pos outside [0, M - 1] are moved into it: nothing is written outside the M real vertices
    bad = np.full(M, 10 ** 6, np.int32)
    bad[::2] = -7
    ops.window_drop(x, win, M, 2 * M, 1, 0, pos=dev(bad), drop_value=3.0)
    got = x.cpu().numpy()
    assert (got[:, :, 0] == 3.0).all() and (got[:, :, M - 1] == 3.0).all() and (got[:, :, 1:M - 1] == 0).all()
    assert (got[:, :, M:] == 0).all()


@pytest.mark.parametrize('C', [1, 3, 15])
@pytest.mark.parametrize('M', [1, 33, 360, 1030])
def test_gather_windows_reflect_against_numpy(M, C):
    Mp = ops.plane_stride(M)
    Ttot, S = C + 20, 41
    rs = np.random.RandomState(7 * M + C)
    planes = (rs.randn(Ttot, Mp) * (1 + rs.rand(Mp))).astype(np.float32)                # garbage in the pad as well
    scale = (rs.rand(C, Mp) + 0.5).astype(np.float32)
    shift = rs.randn(C, Mp).astype(np.float32)
    rows = rs.randint(0, Ttot - C + 1, size=S).astype(np.int64)
    rows[0], rows[1] = 0, Ttot - C
    tshift = rs.randint(0, C, size=S).astype(np.int32)
    tshift[0], tshift[1], tshift[2] = C - 1, 0, C - 1
    perm = np.concatenate([rs.permutation(S), rs.randint(0, S, 7)]).astype(np.int32)
    planes_d, rows_d, tshift_d, scale_d, shift_d = dev(planes), dev(rows), dev(tshift), dev(scale), dev(shift)
    zero_d = dev(np.zeros(S, np.int32))
    for sample in (None, perm):
        pick = np.arange(S) if sample is None else sample
        sample_d = None if sample is None else dev(sample)
        for tables in (False, True):
            sc, sh = (scale_d, shift_d) if tables else (None, None)
            kind = 'tables' if tables else 'plain'
            got = ops.gather_windows_reflect(planes_d, rows_d, tshift_d, M, C, sample_d, sc, sh).cpu().numpy()
            assert _lib.last_dispatch() == 'gather_windows_reflect_kernel<%s>' % kind
            src = rows[pick][:, None] + series.reflect_channels(C, tshift[pick])        # [B, C] rows of the series
            want = np.zeros((len(pick), C, Mp), np.float32)
            x = planes[src]
            if tables:
                x = (x * scale[None]).astype(np.float32) + shift[None]
            want[..., :M] = x[..., :M]
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), kind
            assert (got[..., M:] == 0).all()
            # no shift -- a NULL table or zeros -- is chebgcn_gather_windows, bit for bit
            plain = ops.gather_windows(planes_d, rows_d, M, C, sample_d, sc, sh).cpu().numpy()
            assert _lib.last_dispatch() == 'gather_windows_kernel<%s>' % kind
            for t in (None, zero_d):
                same = ops.gather_windows_reflect(planes_d, rows_d, t, M, C, sample_d, sc, sh).cpu().numpy()
                assert np.array_equal(_bits(same), _bits(plain))
    # a shift outside [0, C - 1] and a row outside [0, Ttot - C] are moved into them
    rows2 = np.array([-5, Ttot, 3], np.int64)
    ts2 = np.array([-2, C + 4, 10 ** 6], np.int32)
    got = ops.gather_windows_reflect(planes_d, dev(rows2), dev(ts2), M, C).cpu().numpy()
    src = np.clip(rows2, 0, Ttot - C)[:, None] + series.reflect_channels(C, np.clip(ts2, 0, C - 1))
    assert np.array_equal(_bits(got[..., :M]), _bits(planes[src][..., :M]))
    with pytest.raises(_lib.ChebgcnError, match='tshift'):
        ops.gather_windows_reflect(planes_d, rows_d, tshift_d[:5], M, C)


# ------------------------------------------------------------------------------------------------ (2) the sets

SETS = {
    'small': dict(N=40, levels=0, F=[4], K=[3], p=[1], M=[3], channel=4),
    # more than 1024 vertices: the input level is relabelled, the dropout takes its positions from a table
    'big': dict(N=1200, levels=1, F=[4, 6], K=[3, 3], p=[2, 1], M=[9, 3], channel=3),
}
_graphs = {}


def _model(name, tmp_path, monkeypatch, batch_size=8, **kw):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    s = SETS[name]
    if name not in _graphs:
        Ls = graph.synthetic_graph(s['N'], k=4 if name == 'small' else 6, levels=s['levels'], seed=3)[0]
        _graphs[name] = Ls + [Ls[-1]] * max(0, len(s['p']) - len(Ls))
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, _graphs[name], s['F'], s['K'], s['p'], s['M'], channel=s['channel'],
                           batch_size=batch_size, verbose=False, dropout=1, eval_frequency=50, **kw)
    net.contraction = 'f32'
    return net


def _stage(net, kind, seed=5):
    """About 20 windows over two runs: a start-cut set, or an event set of ``fold = 2`` (two lists of rows per window)."""
    M0, C = int(net._M0), int(net.channel)
    rs = np.random.RandomState(seed)
    lengths = [C + 9, C + 8]
    runs = [(rs.randn(T, M0) * (1 + rs.rand(M0)) + rs.randn(M0)).astype(np.float32) for T in lengths]
    labels = rs.randint(0, 3, sum(T - C + 1 for T in lengths))
    labels[:3] = [0, 1, 2]
    if kind == 'start':
        return net.stage_windows(runs, [np.arange(T - C + 1) for T in lengths]), labels
    index = [np.concatenate([np.arange(T - C + 1)[:, None] + np.arange(C)[None, :], rs.randint(0, T, (T - C + 1, C))], axis=1)
             for T in lengths]
    return net.stage_windows(runs, index=index, fold=2), labels


def _gathered(net, ws, idx=None):
    """``ws.gather`` in the caller's vertex order, ``[B, M, C]``; the pad of what the kernels wrote must be zero."""
    M0 = int(net._M0)
    planes = ws.gather(net, None if idx is None else dev(np.asarray(idx, np.int32))).planes
    assert (planes[:, :, M0:] == 0).all()
    got = planes[:, :, :M0].permute(0, 2, 1).cpu().numpy()
    order = np.arange(M0) if net._order is None else np.asarray(net._order)
    back = np.empty_like(got)
    back[:, order] = got
    return back


@pytest.mark.parametrize('tables', [False, True])
@pytest.mark.parametrize('kind', ['start', 'event'])
def test_gather_of_an_augmented_set_is_its_materialised_array(kind, tables, tmp_path, monkeypatch):
    net = _model('small', tmp_path, monkeypatch)
    ws, labels = _stage(net, kind)
    S, M0, C = len(labels), 40, 4
    assert len(ws) == S == 19 and ws.shape == (S, M0, C)
    if tables:
        ws.fit_scaler()
    base = ws.materialise()
    bytes0 = ws.nbytes
    new = ws.augment(labels, 3, drop_rate=0.25, time_shift=True, drop_value=0.0 if tables else 1.0, seed=9)
    assert np.array_equal(new, np.tile(labels, 3)) and len(ws) == 3 * S and ws.shape_base == (S, M0, C)
    assert ws.nbytes >= bytes0 + 4 * 3 * S
    kinds = 'tables' if tables else 'plain'
    arrays = []
    for refill in range(2):
        if refill:
            ws.refill()
        x = ws.materialise()
        assert x.shape == (3 * S, M0, C)
        _lib.dispatch_log = []
        try:
            got = _gathered(net, ws)
            log = [k for _, k in _lib.dispatch_log]
        finally:
            _lib.dispatch_log = None
        first = 'gather_windows_reflect_kernel<%s>' if kind == 'start' else 'gather_windows_indexed_kernel<%s>'
        assert log == [first % kinds, 'window_drop_kernel<%s>' % kinds]
        assert np.array_equal(_bits(got), _bits(x)), 'gather() and materialise() differ at refill %d' % refill
        # a window is the same whatever batch it comes in
        pick = np.random.RandomState(refill).permutation(3 * S)[:11]
        assert np.array_equal(_bits(_gathered(net, ws, pick)), _bits(x[pick]))
        # ... and is its base window but for the shift and D = 10 dropped vertices
        D = int(0.25 * M0)
        for i in (0, S, 3 * S - 1):
            v = series.drop_vertices(9, refill, i, D, M0)
            rest = np.setdiff1d(np.arange(M0), v)
            cols = series.reflect_channels(C, ws.aug['shifts'][i])
            if not tables:
                assert np.array_equal(_bits(x[i][rest]), _bits(base[i % S][rest][:, cols])) and (x[i][v] == 1.0).all()
            else:
                assert np.array_equal(_bits(x[i][v]), _bits(np.broadcast_to(ws.scaler[1][v], (D, C))))     # 0 * scale + shift
        arrays.append(x)
    assert not np.array_equal(arrays[0], arrays[1])
    ws.augment(None, 0)
    assert len(ws) == S and ws.nbytes == bytes0
    assert np.array_equal(_bits(_gathered(net, ws)), _bits(base))
    assert _lib.last_dispatch() == ('gather_windows_kernel<%s>' if kind == 'start' else 'gather_windows_indexed_kernel<%s>') % kinds


@pytest.mark.parametrize('kind', ['start', 'event'])
def test_dropout_on_top_of_a_balance_plan(kind, tmp_path, monkeypatch):
    net = _model('small', tmp_path, monkeypatch)
    ws, labels = _stage(net, kind)
    labels = np.where(np.arange(len(labels)) < 14, 0, labels)                   # class 0 large: the others are topped up
    labels[-4:] = [1, 2, 1, 2]
    bal = ws.balance(labels, 2, seed=4)
    S2 = len(bal)
    assert S2 > len(labels)
    mixed = ws.materialise()
    with pytest.raises(ValueError, match='time_shift on a balanced set'):
        ws.augment(bal, 2, drop_rate=0.25, time_shift=True)
    new = ws.augment(bal, 2, drop_rate=0.25, seed=2)
    assert np.array_equal(new, np.tile(bal, 2)) and len(ws) == 2 * S2
    for refill in range(2):
        if refill:
            ws.refill()
        x = ws.materialise()
        got = _gathered(net, ws)
        want_first = 'gather_windows_mix_kernel<plain>' if kind == 'start' else 'gather_windows_indexed_kernel<plain>'
        assert _lib.last_dispatch() == 'window_drop_kernel<plain>'
        assert np.array_equal(_bits(got), _bits(x))
        for i in (0, S2 - 1, S2, 2 * S2 - 1):
            want = mixed[i % S2].copy()
            want[series.drop_vertices(2, refill, i, 10, 40)] = 1.0
            assert np.array_equal(_bits(x[i]), _bits(want))
        _lib.dispatch_log = []
        try:
            _gathered(net, ws, [0, 2 * S2 - 1])
            assert [k for _, k in _lib.dispatch_log] == [want_first, 'window_drop_kernel<plain>']
        finally:
            _lib.dispatch_log = None


def test_dropout_and_shift_on_a_relabelled_model(tmp_path, monkeypatch):
    net = _model('big', tmp_path, monkeypatch)
    assert net._relabelled and net._M0 > 1024 and net._order is not None
    ws, labels = _stage(net, 'start')
    M0, C = int(net._M0), 3
    ws.fit_scaler()
    ws.augment(labels, 2, drop_rate=0.1, time_shift=True, seed=1)
    pos = ws.aug_pos.cpu().numpy()
    assert not np.array_equal(pos, np.arange(M0)) and np.array_equal(np.asarray(net._order)[pos], np.arange(M0))
    for refill in range(2):
        if refill:
            ws.refill()
        x = ws.materialise()
        assert np.array_equal(_bits(_gathered(net, ws)), _bits(x))
        v = series.drop_vertices(1, refill, 5, int(0.1 * M0), M0)
        assert np.array_equal(_bits(x[5][v]), _bits((np.float32(1.0) * ws.scaler[0][v]).astype(np.float32) + ws.scaler[1][v]))


# ------------------------------------------------------------------------------------------------ (3) training

M0, CH, NCLASS, BATCH = 30, 3, 3, 8
LENGTHS = [20, 14, 17]
_L = []


def _fit_model(tmp_path, monkeypatch, **kw):
    """The smallest synthetic graph the series tests train on (30 vertices, one layer)."""
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    if not _L:
        _L.append(graph.synthetic_graph(M0, k=4, levels=0, seed=3)[0][0])
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, [_L[0]], [4], [3], [1], [NCLASS], channel=CH, batch_size=BATCH, verbose=False,
                           dropout=1, eval_frequency=50, **kw)
    net.contraction = 'f32'
    return net


def _dataset():
    rs = np.random.RandomState(11)
    runs = [(rs.randn(T, M0) * (1 + rs.rand(M0)) + rs.randn(M0)).astype(np.float32) for T in LENGTHS]
    starts = [np.arange(T - CH + 1) for T in LENGTHS]
    labels = rs.randint(0, NCLASS, sum(len(s) for s in starts))
    vrun = rs.randn(12, M0).astype(np.float32)
    return runs, starts, labels, vrun, np.arange(10), rs.randint(0, NCLASS, 10)


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
    return net.fit_log, out, log


def test_fit_series_trains_on_the_augmented_copies(tmp_path, monkeypatch):
    net = _fit_model(tmp_path, monkeypatch, num_epochs=2, dir_name='aug')
    runs, starts, labels, vrun, vstarts, vlabels = _dataset()
    S = len(labels)
    kw = dict(augment=2, drop_rate=0.25, time_shift=True, augment_seed=3)
    log, out, disp = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, **kw))
    steps = int(2 * 2 * S / BATCH)
    assert len(log['idx']) == steps == 22                                       # trains on 2 S = 90 windows
    drawn = np.concatenate(log['idx'])
    assert sorted(drawn[:2 * S].tolist()) == list(range(2 * S))
    assert np.isfinite(np.asarray(log['loss_average'])).all() and np.isfinite(out[1]).all()
    kernels = {k for _, k in disp}
    assert 'gather_windows_reflect_kernel<plain>' in kernels and 'window_drop_kernel<plain>' in kernels
    # one entry per refill: the refill number and that refill's shifts, the twin's
    assert len(log['augment']) == len(log['starts']) == 2
    for n, (refill, shifts) in enumerate(log['augment'], 1):
        assert refill == n and np.array_equal(shifts, series.time_shifts(3, n, 2 * S, CH))
    # the same training through the sets themselves: they are left as they were staged
    ws, wv = net.stage_windows(runs, starts), net.stage_windows(vrun, vstarts)
    before, bytes0 = ws.materialise(), ws.nbytes
    aug = series.check_augment_args('fit_series', 2, 0.25, True, 1.0, 3)
    log2, out2, _ = _fit(net, lambda: net._fit_sets(ws, labels, wv, vlabels, False, None, (0, 0, None, False), aug))
    assert ws.aug is None and ws.plan is None and len(ws) == S and ws.shape == (S, M0, CH) and ws.nbytes == bytes0
    assert np.array_equal(_bits(ws.materialise()), _bits(before))
    assert [i.tolist() for i in log['idx']] == [i.tolist() for i in log2['idx']]
    assert np.array_equal(_bits(np.asarray(log['loss_average'], np.float32)), _bits(np.asarray(log2['loss_average'], np.float32)))
    # dropout alone, no shifts: the log says None
    log3, _, disp3 = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, augment=1, drop_rate=0.5))
    assert [s for _, s in log3['augment']] == [None] * len(log3['starts']) and len(log3['idx']) == int(2 * S / BATCH)
    k3 = {k for _, k in disp3}
    assert 'window_drop_kernel<plain>' in k3 and not any('reflect' in k for k in k3)
    assert not np.array_equal(np.asarray(log3['loss_average']), np.asarray(log['loss_average'][:len(log3['idx'])]))


def test_fit_series_without_augmentation_is_the_training_it_was(tmp_path, monkeypatch):
    net = _fit_model(tmp_path, monkeypatch, num_epochs=2, dir_name='aug0')
    runs, starts, labels, vrun, vstarts, vlabels = _dataset()
    a = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels, augment=0, drop_rate=0.25, time_shift=True))
    b = _fit(net, lambda: net.fit_series(runs, starts, labels, vrun, vstarts, vlabels))
    for log, _, disp in (a, b):
        assert 'augment' not in log
        assert {k for what, k in disp if what.startswith('gather_windows')} == {'gather_windows_kernel<plain>'}
        assert not any('window_drop' in what or 'window_drop' in k or 'reflect' in k for what, k in disp)
    assert [i.tolist() for i in a[0]['idx']] == [i.tolist() for i in b[0]['idx']]
    assert np.array_equal(_bits(np.asarray(a[0]['loss_average'], np.float32)), _bits(np.asarray(b[0]['loss_average'], np.float32)))
    assert a[1][0] == b[1][0] and a[1][1] == b[1][1]
