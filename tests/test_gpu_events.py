"""Windows of event designs on the MI355X.  (1) chebgcn_gather_windows_indexed by name: bit for bit against its float32 NumPy
restatement over pad lanes, tile edges, folds, sources, samples and tables; on contiguous rows bit for bit against
chebgcn_gather_windows and chebgcn_gather_windows_mix.  (2) chebgcn_window_stats_indexed against float64 NumPy and sklearn's
StandardScaler on the materialised windows (the bounds of test_window_stats_against_float64_and_sklearn), reruns bit-identical.
(3) ``fit_events`` against ``fit`` on the materialised array: equal, not close.  (4) predict / evaluate with a padded last batch.
(5) jitter is refused."""
import ctypes

import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import _lib, events, graph, models_gcn, ops
from test_gpu_fit_series import _fit, _same_training

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TILE = 4096                             # floats of one workgroup of the gather (GW_T * GW_U float4s)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _planes(Ttot, M, seed):
    """A staged series with something else than zero in its pad lanes."""
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(seed)
    planes = np.full((Ttot, Mp), 7.0, np.float32)
    planes[:, :M] = (rs.randn(Ttot, M) * (1 + rs.rand(M)) + rs.randn(M)).astype(np.float32)
    return planes


def _pieces(planes, idx, C, fold):
    """piece(s)[c][m] in float32: adds in ascending f, one rounded division."""
    x = planes[idx[:, :C]]                                                   # [S, C, Mp]
    for f in range(1, fold):
        x = x + planes[idx[:, f * C:(f + 1) * C]]
    return x / np.float32(fold) if fold > 1 else x


def _indexed_ref(planes, idx, M, C, fold, src, cnt, pick, scale, shift):
    """The contract of chebgcn_gather_windows_indexed in float32 NumPy, window by window."""
    piece = _pieces(planes, idx, C, fold)
    assert piece.dtype == np.float32
    out = np.empty((len(pick), C, planes.shape[1]), np.float32)
    for b, w in enumerate(pick):
        if src is None:
            acc = piece[w]
        else:
            acc = piece[src[w, 0]]
            for j in range(1, cnt[w]):
                acc = acc + piece[src[w, j]]
            if cnt[w] > 1:
                acc = acc / np.float32(cnt[w])
        out[b] = acc
    if scale is not None:
        out = (out * scale[None]).astype(np.float32) + shift[None]
    out[..., M:] = 0
    return out.astype(np.float32)


def _index_table(rs, S, Ttot, Cin):
    """Rows that repeat (a clipped trial), decrease, jump (cross run boundaries) and the ends of the series."""
    idx = rs.randint(0, Ttot, size=(S, Cin)).astype(np.int64)
    idx[0] = np.clip(np.arange(Cin) + Ttot - 1 - Cin // 2, 0, Ttot - 1)      # ... the last row repeated
    idx[1] = np.maximum(Ttot - 1 - np.arange(Cin), 0)                        # decreasing
    idx[2] = 0
    return idx


CASES = [(M, C, fold) for M in (5, 360, 1030) for C, fold in ((1, 1), (15, 1), (3, 2), (2, 8), (1, 16))]
# C * Mp just below, at and just above one workgroup's tile, and a second tile that holds one plane only
CASES += [(5, TILE // 32 - 1, 1), (5, TILE // 32, 2), (5, TILE // 32 + 1, 1), (5, 2 * TILE // 32 + 1, 3)]


@pytest.mark.parametrize('M,C,fold', CASES)
def test_gather_windows_indexed_against_float32_numpy(M, C, fold):
    lib = _lib.lib()
    Mp = ops.plane_stride(M)
    assert (M, Mp) in ((5, 32), (360, 384), (1030, 1056))
    rs = np.random.RandomState(1000 * M + 10 * C + fold)
    S, Ttot, Cin, smax = 9, 37, C * fold, 16
    planes = _planes(Ttot, M, M + C)
    idx = _index_table(rs, S, Ttot, Cin)
    scale, shift = np.full((C, Mp), 3.0, np.float32), np.full((C, Mp), -2.0, np.float32)     # (nonzero in the pad as well)
    scale[:, :M], shift[:, :M] = rs.rand(C, M) + 0.5, rs.randn(C, M)
    # sources: the originals first (cnt 1), then windows of 2, 3 and 16 sources
    cnt = np.array([1] * S + [2, 3, 16, 2, 16, 1, 3], np.int32)
    W = len(cnt)
    src = rs.randint(0, S, size=(W, smax)).astype(np.int64)
    src[:S, 0] = np.arange(S)
    planes_d, idx_d, src_d, cnt_d = dev(planes), dev(idx), dev(src), dev(cnt)
    tabs = {'plain': (None, None), 'tables': (scale, shift)}
    for with_src in (False, True):
        n_win = W if with_src else S
        for sample in (None, np.array([n_win - 1, 0, 3, 3, n_win - 2, 0, 1], np.int32)):
            pick = np.arange(n_win) if sample is None else sample
            B = len(pick)
            sample_d = dev(sample)
            for kind, (sc, sh) in tabs.items():
                sc_d, sh_d = dev(sc), dev(sh)                                # (held: the call takes their addresses)
                got = torch.full((B, C, Mp), float('nan'), device=DEV)
                _lib.check(lib.chebgcn_gather_windows_indexed(
                    P(planes_d), Ttot, P(idx_d), S, Cin, fold, P(src_d) if with_src else None, P(cnt_d) if with_src else None,
                    W if with_src else 0, smax if with_src else 0, P(sample_d), P(sc_d), P(sh_d), P(got), B, M, C,
                    stream()), 'gather_windows_indexed')
                assert _lib.last_dispatch() == 'gather_windows_indexed_kernel<%s>' % kind
                want = _indexed_ref(planes, idx, M, C, fold, src if with_src else None, cnt, pick, sc, sh)
                got = got.cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (with_src, sample is None, kind)
                assert (got[..., M:].view(np.uint32) == 0).all()
    # the ops wrapper: shapes, the out buffer, refusals
    out = ops.gather_windows_indexed(planes_d, idx_d, M, C, fold, src_d, cnt_d)
    assert tuple(out.shape) == (W, C, Mp)
    buf = torch.empty((2, C, Mp), device=DEV)
    pick = dev(np.array([4, 0], np.int32))
    assert ops.gather_windows_indexed(planes_d, idx_d, M, C, fold, sample=pick, out=buf).data_ptr() == buf.data_ptr()
    assert np.array_equal(buf.cpu().numpy(), _indexed_ref(planes, idx, M, C, fold, None, None, [4, 0], None, None))
    with pytest.raises(_lib.ChebgcnError, match='gather_windows_indexed'):
        ops.gather_windows_indexed(planes_d, idx_d, M, C, fold + 1)
    with pytest.raises(_lib.ChebgcnError, match='gather_windows_indexed'):
        ops.gather_windows_indexed(planes_d, idx_d, M, C, fold, src_d)
    with pytest.raises(_lib.ChebgcnError, match='ROCm device tensors'):
        ops.gather_windows_indexed(planes_d, torch.as_tensor(idx), M, C, fold)


def test_indices_and_counts_out_of_range_are_clamped():
    """Nothing read from memory is an address or a trip count unchecked: rows, sources, counts and samples outside their range
    read what the clamped value reads."""
    lib = _lib.lib()
    M, C, fold, S, Ttot, smax = 40, 2, 2, 4, 11, 3
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(3)
    planes = _planes(Ttot, M, 1)
    idx = rs.randint(0, Ttot, size=(S, C * fold)).astype(np.int64)
    src = rs.randint(0, S, size=(5, smax)).astype(np.int64)
    cnt = np.array([1, 2, 3, 3, 1], np.int32)
    sample = np.array([0, 4, 2, 3], np.int32)
    bad_idx, bad_src, bad_cnt, bad_sample = idx.copy(), src.copy(), cnt.copy(), sample.copy()
    bad_idx[0, 0], bad_idx[1, 1], idx[0, 0], idx[1, 1] = -5, 2 ** 40, 0, Ttot - 1
    bad_src[1, 0], bad_src[2, 2], src[1, 0], src[2, 2] = -1, 2 ** 33, 0, S - 1
    bad_cnt[2], bad_cnt[4], cnt[2], cnt[4] = 99, -7, 3, 1
    bad_sample[1], bad_sample[0], sample[1], sample[0] = 2 ** 20, -3, 4, 0
    want = _indexed_ref(planes, idx, M, C, fold, src, cnt, sample, None, None)
    got = torch.full((4, C, Mp), float('nan'), device=DEV)
    held = [dev(a) for a in (planes, bad_idx, bad_src, bad_cnt, bad_sample)]
    _lib.check(lib.chebgcn_gather_windows_indexed(P(held[0]), Ttot, P(held[1]), S, C * fold, fold, P(held[2]), P(held[3]), 5, smax,
                                                  P(held[4]), None, None, P(got), 4, M, C, stream()), 'gather_windows_indexed')
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('M,C', [(360, 15), (1030, 3)])
def test_contiguous_indices_agree_with_the_existing_gathers(M, C):
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(M)
    S, Ttot, smax = 11, 60, 16
    planes = _planes(Ttot, M, 2)
    planes[:, M:] = 0
    rows = rs.randint(0, Ttot - C + 1, size=S).astype(np.int64)
    rows[0], rows[1] = Ttot - C, 0
    idx = rows[:, None] + np.arange(C)[None, :]
    scale, shift = (rs.rand(C, Mp) + 0.5).astype(np.float32), rs.randn(C, Mp).astype(np.float32)
    cnt = np.array([1] * S + [2, 3, 16, 4, 5, 8, 9], np.int32)
    src = rs.randint(0, S, size=(len(cnt), smax)).astype(np.int64)
    src[:S, 0] = np.arange(S)
    planes_d, rows_d, idx_d, src_d, cnt_d = dev(planes), dev(rows), dev(idx), dev(src), dev(cnt)
    mix_rows_d = dev(rows[src])
    for sample in (None, dev(np.array([5, 5, 0, S - 1, 2], np.int32))):
        for sc, sh in ((None, None), (dev(scale), dev(shift))):
            a = ops.gather_windows_indexed(planes_d, idx_d, M, C, 1, sample=sample, scale=sc, shift=sh)
            assert _lib.last_dispatch().startswith('gather_windows_indexed_kernel<')
            b = ops.gather_windows(planes_d, rows_d, M, C, sample, sc, sh)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for sample in (None, dev(np.array([S + 2, 0, S + 6, S, S, 3], np.int32))):
        for sc, sh in ((None, None), (dev(scale), dev(shift))):
            a = ops.gather_windows_indexed(planes_d, idx_d, M, C, 1, src_d, cnt_d, sample, sc, sh)
            b = ops.gather_windows_mix(planes_d, mix_rows_d, cnt_d, M, C, sample, sc, sh)
            assert _lib.last_dispatch().startswith('gather_windows_mix_kernel<')
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ (2) window_stats_indexed

def _stats(planes, idx, M, C, fold):
    mean, var, scale, shift = ops.window_stats_indexed(planes, idx, M, C, fold)
    assert _lib.last_dispatch() == 'window_stats_indexed_partial_kernel + window_stats_finish_kernel'
    return [t.cpu().numpy() for t in (mean, var, scale, shift)]


@pytest.mark.parametrize('M,C,fold,S', [(360, 15, 1, 701), (1031, 3, 2, 90), (77, 1, 5, 33), (40, 2, 1, 10)])
def test_window_stats_indexed_against_float64_and_sklearn(M, C, fold, S):
    """The bounds of test_window_stats_against_float64_and_sklearn (tests/test_gpu_fit_series.py): the kernel and NumPy sum the
    same S float64 terms per entry in different orders -- the terms are the FOLDED float32 values, formed here exactly as the
    gather forms them.  Two orderings of a float64 sum of S terms differ by at most S * 2^-52 * sum|x|, so the means by
    2^-52 * sum|x|, the second moments by 2^-52 * sum x^2, the variance  m2 - mean^2  by
    2^-52 * sum x^2 + 2 |mean| * 2^-52 * sum|x| + 4 * 2^-53 * (m2 + mean^2); the float32 tables are the float64 results
    rounded once.  S covers one chunk (10), chunks with a partial last one (33, 90) and 32 chunks of 22 (701)."""
    from sklearn.preprocessing import StandardScaler
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(7 * M + C)
    Ttot = 150
    planes = _planes(Ttot, M, 11 * M + C)
    planes[:, M:] = 0
    const_v = 5
    planes[:, const_v] = np.float32(0.125)                                  # one vertex constant over time: the zero-variance rule
    idx = _index_table(rs, S, Ttot, C * fold)
    x = _pieces(planes, idx, C, fold)[..., :M].astype(np.float64)           # [S, C, M]
    ref_var = x.var(axis=0)
    assert (ref_var[:, const_v] == 0).all() and (np.delete(ref_var, const_v, axis=1) > 1e-3).all()
    planes_d, idx_d = dev(planes), dev(idx)
    mean, var, scale, shift = _stats(planes_d, idx_d, M, C, fold)
    u = 2.0 ** -52
    sum_abs, sum_sq = np.abs(x).sum(axis=0), (x * x).sum(axis=0)            # [C, M]
    ref_mean, ref_m2 = x.mean(axis=0), (x * x).mean(axis=0)
    b_mean = u * sum_abs
    b_var = u * sum_sq + 2 * np.abs(ref_mean) * b_mean + 4 * (u / 2) * (ref_m2 + ref_mean ** 2)
    e_mean, e_var = np.abs(mean[:, :M] - ref_mean), np.abs(var[:, :M] - ref_var)
    print('window_stats_indexed M=%d C=%d fold=%d S=%d: mean err / bound %.3g, var err / bound %.3g'
          % (M, C, fold, S, (e_mean / b_mean).max(), (e_var / b_var).max()))
    assert (e_mean <= b_mean).all(), (e_mean / b_mean).max()
    assert (e_var <= b_var).all(), (e_var / b_var).max()
    assert (var[:, const_v] == 0).all() and (mean[:, const_v] == 0.125).all()
    # sklearn on the flattened windows (the NDStandardScaler construction)
    sk = StandardScaler().fit(x.reshape(S, C * M))
    sk_scale = (1.0 / sk.scale_).reshape(C, M)
    sk_shift = (-sk.mean_ / sk.scale_).reshape(C, M)
    assert (sk.scale_.reshape(C, M)[:, const_v] == 1).all()
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
    again = _stats(planes_d, idx_d, M, C, fold)
    for a, b in zip((mean, var, scale, shift), again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ (3) - (5) training

CHANNEL = 6
TARGETS = ['tool', 'face', 'body']
_L = []


def _model(batch_size=8, **kw):
    if not _L:
        _L.append(graph.synthetic_graph(360, k=6, levels=0, seed=3)[0])
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, _L[0] * 2, [8, 8], [4, 3], [1, 1], [12, 3], channel=CHANNEL, brelu='b2relu',
                           batch_size=batch_size, verbose=False, dropout=1, **kw)
    net.contraction = 'f32'
    return net


def _design(rs, bd, n_trials, last):
    """Trials of mixed lengths (shorter than block_dura: padded; longer: several chunks, a remainder dropped), some adjacent,
    some same-condition pairs separated by rest only (merged), 'face' four times as frequent as the others."""
    names = ['rest'] * int(rs.randint(0, 4))
    for _ in range(n_trials):
        cond = TARGETS[int(rs.choice([0, 1, 1, 1, 1, 2]))]
        names += [cond] * int(rs.randint(max(1, bd - 3), 3 * bd)) + ['rest'] * int(rs.randint(0, 4))
    return names + [last] * (bd + 1) + ['rest'] * 2


def _event_data(bd, seed):
    rs = np.random.RandomState(seed)
    designs = [_design(rs, bd, 7, 'tool'), ['rest'] * 9, _design(rs, bd, 5, 'body')]          # the middle run yields nothing
    vdesigns = [_design(rs, bd, 4, 'face')]
    runs = [(rs.randn(len(d), 360) * (1 + rs.rand(360)) + rs.randn(360)).astype(np.float32) for d in designs]
    vruns = [(rs.randn(len(d), 360) * (1 + rs.rand(360)) + rs.randn(360)).astype(np.float32) for d in vdesigns]
    return runs, designs, vruns, vdesigns


@pytest.mark.parametrize('standardize,sampling,TRstep', [(False, 0, 1), (True, 2, 2)])
def test_fit_events_equals_fit_on_the_materialised_array(standardize, sampling, TRstep, tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    net = _model(num_epochs=2.5, eval_frequency=4, dir_name='ev')
    bd = CHANNEL * TRstep
    runs, designs, vruns, vdesigns = _event_data(bd, 40 + TRstep)
    kw = dict(TRstep=TRstep, flag_event=1)
    groups = [3, 9, 4] if sampling else None
    _lib.dispatch_log = []
    try:
        a = _fit(net, lambda: net.fit_events(runs, designs, vruns, vdesigns, TARGETS, bd, standardize=standardize,
                                             sampling=sampling, seed=5, groups=groups, **kw))
        kinds = {what for what, _ in _lib.dispatch_log}
        kernels = {k for what, k in _lib.dispatch_log if what == 'gather_windows_indexed'}
    finally:
        _lib.dispatch_log = None
    tail = np.random.rand()
    # (perm_data is in the log: fit_events stages the runs with it; no batch is cut by the contiguous gathers)
    assert 'gather_windows_indexed' in kinds and 'gather_windows' not in kinds and 'gather_windows_mix' not in kinds
    assert kernels == {'gather_windows_indexed_kernel<%s>' % ('tables' if standardize else 'plain')}
    assert ('window_stats_indexed' in kinds) == standardize and net.fit_captured
    # the same sets by hand, and the arrays they stand for
    ev = events.match_events(designs, TARGETS, bd, **kw)
    assert ev.kept == [0, 2]
    ws, labels = net.stage_events(runs, designs, TARGETS, bd, **kw)
    wv, vlabels = net.stage_events(vruns, vdesigns, TARGETS, bd, **kw)
    assert isinstance(ws, models_gcn.WindowSet) and net.stage(ws) is ws
    assert len(ws) == len(labels) == len(ev) and ws.shape == (len(ev), 360, CHANNEL) and np.array_equal(labels, np.concatenate(ev.labels))
    raw = np.concatenate([events.host_windows(runs[k], i, TRstep) for k, i in zip(ev.kept, ev.index)])
    assert np.array_equal(ws.materialise().view(np.uint32), raw.view(np.uint32))
    assert np.array_equal(ws.starts, np.concatenate(ev.index)) and ws.nbytes > 0
    if standardize:
        scale, shift = ws.fit_scaler()
        wv.share_tables(ws)
        assert np.array_equal(net.window_scaler[0], scale) and np.array_equal(net.window_scaler[1], shift)
        assert np.array_equal(net.state_dict()['window_scaler'].numpy(), np.stack([scale, shift]))
        assert np.array_equal(ws.materialise(), (raw * scale[None]).astype(np.float32) + shift[None])
        # set_tables with the caller-order tables is the same set
        assert np.array_equal(net.stage_events(runs, designs, TARGETS, bd, **kw)[0].set_tables(scale, shift).materialise(),
                              ws.materialise())
    else:
        assert net.window_scaler is None and 'window_scaler' not in net.state_dict()
    if sampling:
        counts = np.bincount(labels, minlength=3)
        assert 2 * counts.min() <= counts.max()                              # the design is unbalanced: there is a plan
        x_orig = ws.materialise()
        labels = ws.balance(labels, sampling, 5, [3, 4])
        src, cnt = ws.sources
        assert len(ws) == len(labels) == len(src) > len(ev) and (cnt[len(ev):] == sampling).all()
        x = ws.materialise()
        assert np.array_equal(x[:len(ev)], x_orig) and len(a[0]['sources']) >= 2
        assert all(np.array_equal(s, src) and np.array_equal(c, cnt) for s, c in a[0]['sources'])
        # gather() of the balanced set is its materialised array, bit for bit
        got = ws.gather(net, None).planes[..., :360].permute(0, 2, 1).contiguous().cpu().numpy()      # internal vertex order
        xi = x if net._order is None else x[:, np.asarray(net._order), :]
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(xi).view(np.uint32))
    else:
        x = ws.materialise()
    xv = wv.materialise()
    b = _fit(net, lambda: net.fit(x, labels, xv, vlabels))
    assert np.random.rand() == tail                                          # the global stream saw fit's draws only
    _same_training(a, b)
    if sampling:
        assert ws.balance(None, 0) is None and len(ws) == len(ev) and ws.sources is None


def test_predict_and_evaluate_on_an_event_set_with_a_padded_last_batch(tmp_path, monkeypatch):
    monkeypatch.setenv('CHEBGCN_HOME', str(tmp_path))
    monkeypatch.chdir(tmp_path)
    net = _model(num_epochs=1, eval_frequency=3, dir_name='pred')
    runs, designs, vruns, vdesigns = _event_data(CHANNEL, 77)
    ws, labels = net.stage_events(runs, designs, TARGETS, CHANNEL, flag_event=1)
    wv, vlabels = net.stage_events(vruns[0], vdesigns[0], TARGETS, CHANNEL, flag_event=1)       # one run, not a list
    assert len(wv) % net.batch_size != 0 and len(ws) % net.batch_size != 0
    torch.manual_seed(3)
    np.random.seed(5)
    net.fit(ws, labels, wv, vlabels)
    xv = wv.materialise()
    pa, la = net.predict(wv, vlabels)
    pb, lb = net.predict(xv, vlabels)
    assert np.array_equal(pa, pb) and la == lb
    assert np.array_equal(net.predict(wv), pb)
    assert net.evaluate(wv, vlabels) == net.evaluate(xv, vlabels)
    perf = models_gcn.model_perf()
    ckp = net._get_path('checkpoints')
    ra = perf.predict(ckp, wv, vlabels, batch_size=net.batch_size, model=net)
    rb = perf.predict(ckp, xv, vlabels, batch_size=net.batch_size, model=net)
    assert np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32)) and np.array_equal(ra[1], rb[1])
    assert ra[2] == rb[2] and ra[3] == rb[3]
    # the low-level entry with the same tables is the same set
    ev = events.match_events([vdesigns[0]], TARGETS, CHANNEL, flag_event=1)
    again = net.stage_windows(vruns[0], index=ev.index[0])
    assert np.array_equal(again.materialise(), xv) and np.array_equal(net.predict(again), pb)


def test_jitter_on_an_event_set_is_refused():
    net = _model()
    runs, designs, vruns, vdesigns = _event_data(CHANNEL, 78)
    ws, labels = net.stage_events(runs, designs, TARGETS, CHANNEL, flag_event=1)
    assert ws.jitter == 0
    for j in (1, 2, True, 0.5):
        with pytest.raises(ValueError, match='jitter'):
            ws.jitter = j
    ws.jitter = 0
    with pytest.raises(ValueError, match='displaced'):
        ws.set_rows(np.zeros(len(ws), np.int64))
    with pytest.raises(ValueError, match='jitter'):
        net.fit_events(runs, designs, vruns, vdesigns, TARGETS, CHANNEL, flag_event=1, jitter=1)
