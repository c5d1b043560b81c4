"""Training on scans on the MI355X.  (1) chebgcn_gather_windows by name: bit for bit against chebgcn_perm_data on the windows cut
on the host, and with tables against float32 NumPy (two roundings).  (2) chebgcn_window_stats by name against NumPy float64 and
sklearn's StandardScaler on the host-cut windows; reruns and permuted rows bit-identical.  (3) ``fit`` on a ``WindowSet`` against
``fit`` on its materialised array: equal, not close.  (4) ``fit_series(standardize=True)`` against ``fit`` on host-scaled
windows, and ``decode_series`` with ``model.window_scaler`` against the model's logits on the scaled set.  (5) predict /
evaluate / model_perf.predict with a padded last batch.  (6) jitter."""
import ctypes

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops, series
from test_decode_host import host_windows

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
NETS = {
    # the atlas shape: fit() captures the step (graphs of at most 512 vertices)
    'atlas': dict(N=360, levels=0, F=[8, 8], K=[4, 3], p=[1, 1], M=[12, 5], channel=15, brelu='b2relu'),
    # more than 1024 vertices, relabelled input level, pooling through index maps
    'big': dict(N=1200, levels=1, F=[4, 6], K=[3, 3], p=[2, 1], M=[9, 5], channel=3, brelu='b1relu'),
}
_graphs = {}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _laplacians(name):
    s = NETS[name]
    if name not in _graphs:
        _graphs[name] = graph.synthetic_graph(s['N'], k=6, levels=s['levels'], seed=3)[0]
    Ls = _graphs[name]
    return Ls + [Ls[-1]] * max(0, len(s['p']) - len(Ls))


def _model(name, batch_size=8, **kw):
    s = NETS[name]
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, _laplacians(name), s['F'], s['K'], s['p'], s['M'], channel=s['channel'],
                           brelu=s['brelu'], batch_size=batch_size, verbose=False, dropout=1, **kw)
    net.contraction = 'f32'
    return net


def _runs(M, lengths, seed, C):
    """Seeded runs and starts: overlapping, repeated and unsorted starts, the first and the last window of every run."""
    rs = np.random.RandomState(seed)
    runs = [(rs.randn(T, M) * (1 + rs.rand(M)) + rs.randn(M)).astype(np.float32) for T in lengths]
    starts = []
    for T in lengths:
        st = rs.randint(0, T - C + 1, size=max(3, T // 2))
        st[0], st[1], st[-1] = T - C, 0, st[2]
        starts.append(st.astype(np.int64))
    return runs, starts


def _host_windows(runs, starts, C):
    return np.concatenate([host_windows(r, s, C) for r, s in zip(runs, starts)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ (1) gather_windows

@pytest.mark.parametrize('M,relabel', [(360, False), (1031, True)])
@pytest.mark.parametrize('C', [1, 15])
def test_gather_windows_bit_identical_to_perm_data(M, relabel, C):
    lib = _lib.lib()
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(M + C)
    order = rs.permutation(M).astype(np.int32) if relabel else np.arange(M, dtype=np.int32)      # internal position -> vertex
    runs, starts = _runs(M, [C + 20, C, C + 7], M * 3 + C, C)
    x_host = _host_windows(runs, starts, C)                                                        # [S, M, C]
    S = len(x_host)
    order_dev = torch.as_tensor(order).to(DEV)
    # the series staged as decode_series stages it: perm_data with one channel per time point, every run concatenated
    cat = torch.as_tensor(np.concatenate(runs)).to(DEV)
    planes = ops.perm_data(cat.unsqueeze(2), order_dev).view(len(cat), Mp)
    rows_host, _, _ = series.row_table([len(r) for r in runs], starts, C)
    rows = torch.as_tensor(rows_host).to(DEV)
    x_dev = torch.as_tensor(x_host).to(DEV)
    perm = torch.as_tensor(rs.permutation(S)[:max(1, S - 2)].astype(np.int32)).to(DEV)
    scale = np.zeros((C, Mp), np.float32)
    shift = np.zeros((C, Mp), np.float32)
    scale[:, :M] = rs.rand(C, M) + 0.5
    shift[:, :M] = rs.randn(C, M)
    scale_dev, shift_dev = torch.as_tensor(scale).to(DEV), torch.as_tensor(shift).to(DEV)
    for sample in (None, perm):
        B = S if sample is None else int(sample.numel())
        want = ops.perm_data(x_dev, order_dev, sample)
        got = torch.full((B, C, Mp), float('nan'), device=DEV)
        _lib.check(lib.chebgcn_gather_windows(P(planes), len(cat), P(rows), P(sample), None, None, P(got), B, M, C, stream()),
                   'gather_windows')
        assert _lib.last_dispatch() == 'gather_windows_kernel<plain>'
        assert torch.equal(got, want), 'gather_windows and perm_data on the host-cut windows differ'
        assert (got[..., M:] == 0).all()
        # ... and against the literal definition, in NumPy
        pick = np.arange(S) if sample is None else sample.cpu().numpy()
        lit = np.zeros((B, C, Mp), np.float32)
        lit[..., :M] = x_host[pick][:, order, :].transpose(0, 2, 1)
        assert np.array_equal(got.cpu().numpy(), lit)
        # with tables: a rounded product, then a rounded sum, like float32 NumPy
        got_t = torch.full((B, C, Mp), float('nan'), device=DEV)
        _lib.check(lib.chebgcn_gather_windows(P(planes), len(cat), P(rows), P(sample), P(scale_dev), P(shift_dev), P(got_t), B, M,
                                              C, stream()), 'gather_windows')
        assert _lib.last_dispatch() == 'gather_windows_kernel<tables>'
        prod = (lit * scale[None]).astype(np.float32)
        want_t = (prod + shift[None]).astype(np.float32)
        assert np.array_equal(got_t.cpu().numpy().view(np.uint32), want_t.view(np.uint32)), 'scaled windows differ from float32 NumPy'
        assert (got_t[..., M:] == 0).all()
    # a pad that holds something else in the operands still comes out zero
    dirty = planes.clone()
    dirty[:, M:] = 7.0
    got = torch.full((S, C, Mp), float('nan'), device=DEV)
    _lib.check(lib.chebgcn_gather_windows(P(dirty), len(cat), P(rows), None, None, None, P(got), S, M, C, stream()), 'gather_windows')
    assert (got[..., M:] == 0).all() and torch.equal(got[..., :M], ops.perm_data(x_dev, order_dev)[..., :M])


# ------------------------------------------------------------------------------------------------ (2) window_stats

def _stats(planes, rows, M, C):
    mean, var, scale, shift = ops.window_stats(planes, rows, M, C)
    assert _lib.last_dispatch() == 'window_count_kernel + window_stats_partial_kernel + window_stats_finish_kernel'
    return [t.cpu().numpy() for t in (mean, var, scale, shift)]


@pytest.mark.parametrize('M,C,lengths', [(360, 15, [700, 15, 420]), (1031, 3, [90, 40]), (77, 1, [33])])
def test_window_stats_against_float64_and_sklearn(M, C, lengths):
    """Bounds.  The kernel and NumPy sum the same S float64 terms per entry in different orders: two orderings of a float64 sum of
    S terms differ by at most S * 2^-52 * sum|x| (each by (S - 1) * 2^-53 * sum|x| from the exact sum), so the means (the sums
    over S) by 2^-52 * sum|x|, the second moments by 2^-52 * sum x^2, and the variance  m2 - mean^2  by
    2^-52 * sum x^2 + 2 |mean| * 2^-52 * sum|x|  (+ the rounding of the final operations, 4 * 2^-53 * (m2 + mean^2)).  The
    float32 tables are the float64 results rounded once: against sklearn's float64 they may differ by that rounding, 2^-24
    relative, plus what the variance bound above moves 1/std by."""
    from sklearn.preprocessing import StandardScaler
    Mp = ops.plane_stride(M)
    runs, starts = _runs(M, lengths, 11 * M + C, C)
    const_v = 5
    for r in runs:
        r[:, const_v] = np.float32(0.125)                                  # one vertex constant over time: the zero-variance rule
    x = _host_windows(runs, starts, C).astype(np.float64)                  # [S, M, C]
    S = len(x)
    ref_var = x.var(axis=0)
    assert (ref_var[const_v] == 0).all() and (np.delete(ref_var, const_v, axis=0) > 1e-3).all()     # no other zero-variance entry
    cat = torch.as_tensor(np.concatenate(runs)).to(DEV)
    planes = ops.perm_data(cat.unsqueeze(2), torch.arange(M, dtype=torch.int32, device=DEV)).view(len(cat), Mp)
    rows_host, _, _ = series.row_table(lengths, starts, C)
    rows = torch.as_tensor(rows_host).to(DEV)
    mean, var, scale, shift = _stats(planes, rows, M, C)
    u = 2.0 ** -52
    sum_abs, sum_sq = np.abs(x).sum(axis=0).T, (x * x).sum(axis=0).T      # [C, M]
    ref_mean, ref_m2 = x.mean(axis=0).T, (x * x).mean(axis=0).T
    ref_var = ref_var.T
    b_mean = u * sum_abs
    b_var = u * sum_sq + 2 * np.abs(ref_mean) * b_mean + 4 * (u / 2) * (ref_m2 + ref_mean ** 2)
    e_mean, e_var = np.abs(mean[:, :M] - ref_mean), np.abs(var[:, :M] - ref_var)
    print('window_stats M=%d C=%d S=%d: mean err / bound %.3g, var err / bound %.3g'
          % (M, C, S, (e_mean / b_mean).max(), (e_var / b_var).max()))
    assert (e_mean <= b_mean).all(), (e_mean / b_mean).max()
    assert (e_var <= b_var).all(), (e_var / b_var).max()
    assert (var[:, const_v] == 0).all() and (mean[:, const_v] == 0.125).all()
    # sklearn on the flattened windows (the NDStandardScaler construction): [S, M * C]
    sk = StandardScaler().fit(x.reshape(S, M * C))
    sk_scale = (1.0 / sk.scale_).reshape(M, C).T
    sk_shift = (-sk.mean_ / sk.scale_).reshape(M, C).T
    assert (sk.scale_.reshape(M, C)[const_v] == 1).all()
    live = np.ones(M, bool)
    live[const_v] = False
    rel_std = 0.5 * b_var[:, live] / ref_var[:, live]                      # d(1/std) / (1/std) = d(var) / (2 var)
    tol = 2.0 ** -24 + rel_std
    assert (np.abs(scale[:, :M][:, live] - sk_scale[:, live]) <= tol * np.abs(sk_scale[:, live])).all()
    tol_shift = (2.0 ** -24 + rel_std) * np.abs(sk_shift[:, live]) + b_mean[:, live] * sk_scale[:, live]
    assert (np.abs(shift[:, :M][:, live] - sk_shift[:, live]) <= tol_shift).all()
    assert (scale[:, const_v] == 1).all() and (shift[:, const_v] == np.float32(-0.125)).all()
    for t in (mean, var, scale, shift):
        assert (t[:, M:] == 0).all()
    # twice, and with the rows permuted: bit for bit
    again = _stats(planes, rows, M, C)
    shuffled = _stats(planes, torch.as_tensor(np.random.RandomState(1).permutation(rows_host)).to(DEV), M, C)
    for a, b, c in zip((mean, var, scale, shift), again, shuffled):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ------------------------------------------------------------------------------------------------ (3) - (6) training

def _dataset(name, seed=0):
    s = NETS[name]
    net_M = _laplacians(name)[0].shape[0]
    C = s['channel']
    runs, starts = _runs(net_M, [C + 30, C + 12], 100 + seed, C)
    vruns, vstarts = _runs(net_M, [C + 9], 200 + seed, C)
    rs = np.random.RandomState(300 + seed)
    labels = rs.randint(0, s['M'][-1], sum(len(t) for t in starts))
    vlabels = rs.randint(0, s['M'][-1], sum(len(t) for t in vstarts))
    return runs, starts, labels, vruns, vstarts, vlabels


def _fit(net, call, seed=2024):
    """One seeded fit: returns (fit_log, variables, fit's own return)."""
    torch.manual_seed(7)
    np.random.seed(seed)
    net.record_fit = True
    out = call()
    variables = {k: net.get_var(k).copy() for k in net.variables()}
    return net.fit_log, variables, out


def _same_training(a, b):
    (la, va, oa), (lb, vb, ob) = a, b
    assert [i.tolist() for i in la['idx']] == [i.tolist() for i in lb['idx']]
    assert np.array_equal(np.asarray(la['loss_average'], np.float32).view(np.uint32),
                          np.asarray(lb['loss_average'], np.float32).view(np.uint32)), 'loss_average streams differ'
    for k in va:
        assert np.array_equal(va[k].view(np.uint32), vb[k].view(np.uint32)), k
    assert oa[0] == ob[0] and oa[1] == ob[1]                    # validation accuracies and losses of every evaluation


@pytest.mark.parametrize('name', ['atlas', 'big'])
def test_fit_on_a_window_set_equals_fit_on_its_array(name, tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    net = _model(name, num_epochs=2.5, eval_frequency=4, dir_name='ws')
    runs, starts, labels, vruns, vstarts, vlabels = _dataset(name)
    ws, wv = net.stage_windows(runs, starts), net.stage_windows(vruns, vstarts)
    C = NETS[name]['channel']
    assert ws.shape == (len(labels), net._M0, C) and len(ws) == len(labels)
    x, xv = ws.materialise(), wv.materialise()
    assert x.dtype == np.float32 and np.array_equal(x, _host_windows(runs, starts, C))
    assert net.stage(ws) is ws
    if name == 'big':
        assert net._relabelled and net._pool_maps[0] is not None and net._M0 > 1024
    _lib.dispatch_log = []
    try:
        a = _fit(net, lambda: net.fit(ws, labels, wv, vlabels))
        kinds = {what for what, _ in _lib.dispatch_log}
    finally:
        _lib.dispatch_log = None
    assert 'gather_windows' in kinds and 'perm_data' not in kinds
    assert net.fit_captured == (name == 'atlas')
    assert len(a[0]['starts']) >= 2 and all(np.array_equal(s, np.concatenate(starts)) for s in a[0]['starts'])
    b = _fit(net, lambda: net.fit(x, labels, xv, vlabels))
    assert 'starts' not in b[0]
    _same_training(a, b)
    # fit_series without scaler or jitter is the same training, and consumes the same global random numbers
    c = _fit(net, lambda: net.fit_series(runs, starts, labels, vruns, vstarts, vlabels))
    tail = np.random.rand()
    _same_training(a, c)
    np.random.seed(2024)
    net.fit(x, labels, xv, vlabels)
    assert np.random.rand() == tail
    assert net.window_scaler is None and 'window_scaler' not in net.state_dict()
    # a set staged by a model with another internal order is refused
    if name == 'big':
        monkeypatch.setenv('CHEBGCN_VERTEX_ORDER', 'reference')
        other = _model('big')
        assert not other._relabelled and not other._same_order(net)
        with pytest.raises(ValueError, match='another model'):
            other.predict(ws)


def test_fit_series_standardize_and_decode_with_the_scaler(tmp_path, monkeypatch):
    """The decode comparison runs on the atlas shape with a number of windows that is a multiple of the batch size and
    ``decode_series(batch_size=model.batch_size, share=False)``: both sides then hand bit-identical batches of the same size
    to the same ``_inference_storage`` -- the same first-layer kernel (the on-chip fused layer) at the same launch size."""
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    name = 'atlas'
    net = _model(name, num_epochs=2, eval_frequency=5, dir_name='std')
    runs, starts, labels, vruns, vstarts, vlabels = _dataset(name, seed=1)
    a = _fit(net, lambda: net.fit_series(runs, starts, labels, vruns, vstarts, vlabels, standardize=True))
    scale, shift = net.window_scaler
    C, M = NETS[name]['channel'], net._M0
    assert scale.shape == shift.shape == (M, C) and scale.dtype == shift.dtype == np.float32
    sd = net.state_dict()
    assert np.array_equal(sd['window_scaler'].numpy(), np.stack([scale, shift]))
    twin = models_gcn.cgcnn.from_checkpoint(sd, config={'device': DEV})
    assert np.array_equal(twin.window_scaler[0], scale) and np.array_equal(twin.window_scaler[1], shift)
    # the same tables from a set of its own, and the host-scaled windows
    ws = net.stage_windows(runs, starts)
    s2, h2 = ws.fit_scaler()
    assert np.array_equal(s2, scale) and np.array_equal(h2, shift)
    raw, vraw = _host_windows(runs, starts, C), _host_windows(vruns, vstarts, C)
    x = (raw * scale[None]).astype(np.float32) + shift[None]
    xv = (vraw * scale[None]).astype(np.float32) + shift[None]
    assert np.array_equal(ws.materialise(), x)
    b = _fit(net, lambda: net.fit(x, labels, xv, vlabels))
    _same_training(a, b)
    # decode_series with the model's scaler against the model's logits on the scaled set
    bs = net.batch_size
    T = C + 2 * bs - 1                                                         # 2 * bs windows at stride 1
    run = _runs(M, [T], 9, C)[0][0]
    st = np.arange(T - C + 1)
    assert len(st) % bs == 0
    dec = net.decode_series(run, st, scale=scale, shift=shift, share=False, batch_size=bs)
    assert net.last_decode_path == 'materialised'
    wd = net.stage_windows(run, st, scale=scale, shift=shift)
    logits = []
    net.training_mode = False
    with torch.no_grad():
        for b0 in range(0, len(st), bs):
            idx = torch.arange(b0, b0 + bs, dtype=torch.int32, device=DEV)
            logits.append(net._inference_storage(net.as_internal(net._gather_padded(wd, idx, bs)), 1).cpu().numpy())
    assert np.array_equal(np.concatenate(logits).view(np.uint32), dec.view(np.uint32))


@pytest.mark.parametrize('name', ['atlas', 'big'])
def test_predict_and_evaluate_on_a_window_set_with_a_padded_last_batch(name, tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    monkeypatch.chdir(tmp_path)
    net = _model(name, num_epochs=1, eval_frequency=3, dir_name='pred')
    runs, starts, labels, vruns, vstarts, vlabels = _dataset(name, seed=2)
    ws, wv = net.stage_windows(runs, starts), net.stage_windows(vruns, vstarts)
    assert len(wv) % net.batch_size != 0 and len(ws) % net.batch_size != 0
    torch.manual_seed(3)
    np.random.seed(5)
    net.fit(ws, labels, wv, vlabels)
    xv = wv.materialise()
    pa, la = net.predict(wv, vlabels)
    pb, lb = net.predict(xv, vlabels)
    assert np.array_equal(pa, pb) and la == lb
    assert np.array_equal(net.predict(wv), pb)
    ea, eb = net.evaluate(wv, vlabels), net.evaluate(xv, vlabels)
    assert ea == eb
    perf = models_gcn.model_perf()
    ckp = net._get_path('checkpoints')
    ra = perf.predict(ckp, wv, vlabels, batch_size=net.batch_size, model=net)
    rb = perf.predict(ckp, xv, vlabels, batch_size=net.batch_size, model=net)
    assert np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32)) and np.array_equal(ra[1], rb[1])
    assert ra[2] == rb[2] and ra[3] == rb[3]


def test_jitter_moves_the_training_windows_inside_their_runs(tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    name = 'atlas'
    net = _model(name, num_epochs=3, eval_frequency=50, dir_name='jit')
    runs, starts, labels, vruns, vstarts, vlabels = _dataset(name, seed=3)
    C = NETS[name]['channel']
    a = _fit(net, lambda: net.fit_series(runs, starts, labels, vruns, vstarts, vlabels, jitter=2, jitter_seed=4))
    tail = np.random.rand()
    used = a[0]['starts']
    assert len(used) == 3                                                       # one table per refill of the deque
    base = np.concatenate(starts)
    hi = np.concatenate([np.full(len(s), len(r) - C) for r, s in zip(runs, starts)])
    for u in used:
        assert u.shape == base.shape and (u >= 0).all() and (u <= hi).all() and (np.abs(u - base) <= 2).all()
    assert not np.array_equal(used[0], used[1]) and not np.array_equal(used[1], used[2]) and not np.array_equal(used[0], base)
    # the same seed again: the same training; the global stream saw fit's draws only
    b = _fit(net, lambda: net.fit_series(runs, starts, labels, vruns, vstarts, vlabels, jitter=2, jitter_seed=4))
    assert np.random.rand() == tail
    _same_training(a, b)
    assert all(np.array_equal(s, t) for s, t in zip(used, b[0]['starts']))
    # jitter = 0 is the plain training (test 3), with the same samples as the displaced one
    c = _fit(net, lambda: net.fit_series(runs, starts, labels, vruns, vstarts, vlabels, jitter=0))
    d = _fit(net, lambda: net.fit(_host_windows(runs, starts, C), labels, _host_windows(vruns, vstarts, C), vlabels))
    _same_training(c, d)
    assert [i.tolist() for i in a[0]['idx']] == [i.tolist() for i in c[0]['idx']]
    assert not np.array_equal(np.asarray(a[0]['loss_average']), np.asarray(c[0]['loss_average']))
