"""``glm.single_trial`` on the device (chebgcn_glm_project + chebgcn_glm_trials) against its float64 host restatement
``glm.single_trial_host``, which fits every trial's explicit design and knows nothing of the kernels' algebra.  Shapes come from
``ops.glm_geometry()`` / ``ops.glm_trials_geometry()``; trials are 3 rows long with jittered gaps of 4 to 8 rows, q = 3 (two
confounds and the intercept) unless stated.

The bound, for beta, variance and t at EVERY trial and vertex, in the form and with the constants of ``tests/test_gpu_glm.py``:
``|got - ref| <= 2^-23 |ref| + 1e-10 s`` -- one float32 rounding plus that file's float64 dot-product bound ``T 2^-53`` at
T <= 2000 with its 500x margin, times the natural scale s of what the kernel's chains can lose:

* beta: ``s = sum_l |w_jl| |column of d_l| sqrt(y.y)`` (Cauchy-Schwarz on every projection behind ``d_l``: ``z_j`` for l = 0, the
  projected others column for l > 0);
* variance: ``s = w_j0 y.y / dof`` (``rss = y.y - ssq`` cancels at the scale of ``y.y``);
* ``t = beta / sqrt(variance)``: the first-order propagation ``s = s_b / sqrt(v) + |t| s_v / (2 v)`` with the reference's v and
  t; where the reference's variance is exactly 0 the device's t must be exactly 0.

Measured on an MI355X (``record_measured`` keeps every case's figures), as fractions of the bound: beta at most 0.37, variance
0.10, t 0.13 -- the float32 rounding (half of ``2^-23``) and next to nothing else.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, glm, graph, searchlight, stats

pytestmark = pytest.mark.gpu

EPS32, FLOOR, TR = 2.0 ** -23, 1e-10, 0.72
ALL = ('beta', 'variance', 't')


@pytest.fixture(scope='module')
def geo():
    from gcn_fmri_decoding_amd import ops
    g = dict(ops.glm_geometry())
    t = ops.glm_trials_geometry()
    assert t['vertices'] == g['vertices'] and t['panel'] == g['panel']
    g.update(max_G1=t['max_G1'], max_trials=t['max_trials'])
    return g


def make_run(rng, n=None, T=None, conds=2, confounds=2, M=33, gap=None, mean=100.0, sd=1.0, gain=2.0):
    """A run of n trials (or as many as T rows hold) of 3 rows, gaps of 4 to 8 rows (or ``gap``), conditions in turn; the last
    trial starts at least 12 rows before the end, so every trial is estimable.  ``(series [T, M] float32, TrialDesign)``."""
    on, ev = 1, []
    while (len(ev) < n) if n is not None else (on + 3 + 12 <= T):
        ev.append((on * TR, 3 * TR, 'c%02d' % (len(ev) % conds)))
        on += 3 + (gap if gap is not None else rng.randint(4, 9))
    T = on + 12 if T is None else T
    td = glm.trial_design(events=ev, T=T, tr=TR, conditions=['c%02d' % c for c in range(conds)], high_pass=None,
                          confounds=rng.randn(T, confounds) if confounds else None)
    y = (mean + gain * (td.X @ rng.randn(td.X.shape[1], M)) + sd * rng.randn(T, M)).astype(np.float32)
    return y, td


def trial_names(n, geo):
    """What chebgcn_last_dispatch() reports for a batch whose longest run has n trials."""
    return ' + '.join('glm_trials_kernel<%d>' % min(geo['panel'], n - j0) for j0 in range(0, n, geo['panel']))


def run_device(runs, designs, n_batches=None, geo=None, **kw):
    """``single_trial`` with every map and the dispatch log checked: every batch ran the panels its longest run asks for."""
    kw.setdefault('outputs', ALL)
    _lib.dispatch_log = log = []
    try:
        res = glm.single_trial(runs, designs, **kw)
    finally:
        _lib.dispatch_log = None
    what = [w for w, _ in log]
    assert len(what) >= 2 and what == ['glm_project', 'glm_trials'] * (len(what) // 2), what
    if n_batches is not None:
        assert [d for w, d in log if w == 'glm_trials'] == [trial_names(n, geo) for n in n_batches]
    return res


def host(x):
    return np.asarray(x.cpu() if hasattr(x, 'cpu') else x)


def scales(runs, designs, others, groups=None):
    """The natural scales of the bound per (trial, vertex): ``(s_beta, s_variance)``."""
    pl = glm._trial_plan(runs, designs, others, ALL, groups, 'scales')
    sb, sv = [], []
    for y, tb in zip(pl.runs, pl.tables):
        yy = (host(y).astype(np.float32).astype(np.float64) ** 2).sum(axis=0)
        for j in range(tb.n):
            D = np.concatenate([tb.ZX[:, j:j + 1], tb.ZS], axis=1)
            D[:, 1 + tb.own[j]] -= tb.ZX[:, j]
            sb.append((np.abs(tb.w[j]) * np.linalg.norm(D, axis=0)).sum() * np.sqrt(yy))
            sv.append(tb.w[j, 0] * yy / (tb.T - tb.q - tb.rank[j]))
    return np.stack(sb), np.stack(sv)


def worst(got, ref, s):
    """max over every element of |got - ref| / (2^-23 |ref| + 1e-10 s): the bound holds iff <= 1."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (EPS32 * np.abs(ref) + FLOOR * s + 1e-300)).max())


def against_host(name, res, runs, designs, others='condition', groups=None):
    ref = glm.single_trial_host(runs, designs, others=others, outputs=ALL, groups=groups)
    s_b, s_v = scales(runs, designs, others, groups)
    beta, var, t = host(res.beta), host(res.variance), host(res.t)
    assert beta.dtype == var.dtype == t.dtype == np.float32 and beta.shape == ref.beta.shape
    assert np.array_equal(res.dof, ref.dof) and res.labels.tolist() == ref.labels.tolist() and res.group == ref.group
    assert np.array_equal(res.run, ref.run) and np.array_equal(res.trial, ref.trial) and np.array_equal(res.onset, ref.onset)
    pos = ref.variance > 0
    assert (t[~pos] == 0).all()
    v = np.where(pos, ref.variance, 1.0)
    s_t = np.where(pos, s_b / np.sqrt(v) + np.abs(ref.t) * s_v / (2.0 * v), 0.0)
    m = {'beta': worst(beta, ref.beta, s_b), 'variance': worst(var, ref.variance, s_v),
         't': worst(np.where(pos, t, 0.0), np.where(pos, ref.t, 0.0), s_t)}
    record_measured(name, bound_used=m)
    print(name, m)
    for key, val in m.items():
        assert val <= 1.0, '%s: %s error is %.3f of its bound' % (name, key, val)
    return ref


def same(a, b):
    for name in ALL:
        u, v = host(getattr(a, name)), host(getattr(b, name))
        assert u.dtype == v.dtype and np.array_equal(u, v), '%s differs at %d places' % (name, int((u != v).sum()))
    assert np.array_equal(a.dof, b.dof) and a.group == b.group


@pytest.mark.parametrize('M', ['1', '33', 'VB-1', 'VB', 'VB+1'])
def test_vertex_counts_around_the_tile(M, geo):
    M = {'VB-1': geo['vertices'] - 1, 'VB': geo['vertices'], 'VB+1': geo['vertices'] + 1}.get(M) or int(M)
    rng = np.random.RandomState(M)
    y, td = make_run(rng, T=geo['split'] + 5, M=M)
    res = run_device(y, td, n_batches=[td.X.shape[1]], geo=geo)
    against_host('trials_M%d' % M, res, y, td)
    assert res.beta.shape == (td.X.shape[1], M)


@pytest.mark.parametrize('n', ['1', 'panel-1', 'panel', 'panel+1', '2panel+1'])
def test_trial_counts_around_the_panel(n, geo):
    P = geo['panel']
    n = {'panel-1': P - 1, 'panel': P, 'panel+1': P + 1, '2panel+1': 2 * P + 1}.get(n) or int(n)
    rng = np.random.RandomState(100 + n)
    y, td = make_run(rng, n=n)
    assert td.X.shape[1] == n
    res = run_device(y, td, n_batches=[n], geo=geo)
    against_host('trials_n%d' % n, res, y, td)


@pytest.mark.parametrize('T', ['split-1', 'split', 'split+1', '3slices+5', '4slices+1'])
def test_run_lengths_around_the_split(T, geo):
    T = {'split-1': geo['split'] - 1, 'split': geo['split'], 'split+1': geo['split'] + 1, '3slices+5': 3 * geo['slice'] + 5,
         '4slices+1': 4 * geo['slice'] + 1}[T]
    rng = np.random.RandomState(T)
    y, td = make_run(rng, T=T)
    res = run_device(y, td, n_batches=[td.X.shape[1]], geo=geo)
    against_host('trials_T%d' % T, res, y, td)
    assert set(res.dof.tolist()) == {T - 3 - 3}


def mixed_runs(geo, conds):
    """Three runs of different T, q and trial count: fewer trials than a panel, more than two panels, and a handful."""
    rng = np.random.RandomState(11 + conds)
    P = geo['panel']
    a = make_run(rng, n=P - 3, conds=min(conds, P - 3), confounds=2, M=geo['vertices'] + 1)
    b = make_run(rng, n=2 * P + 3, conds=conds, confounds=4, M=geo['vertices'] + 1)
    c = make_run(rng, T=geo['split'] + 9, conds=min(conds, 2), confounds=1, M=geo['vertices'] + 1)
    names = ['c%02d' % i for i in range(conds)]
    runs, designs = zip(a, b, c)
    return list(runs), [d._replace(conditions=names) for d in designs], ['s1', 's2', 's1']


@pytest.fixture(scope='module')
def mixed(geo):
    return mixed_runs(geo, 2)


@pytest.mark.parametrize('others', ['condition', 'pooled'])
@pytest.mark.parametrize('conds', ['1', '2', 'Gmax'])
def test_one_call_with_runs_of_different_length_rank_and_trial_count(conds, others, geo):
    conds = geo['max_G1'] - 1 if conds == 'Gmax' else int(conds)
    runs, designs, groups = mixed_runs(geo, conds)
    P = geo['panel']
    res = run_device(runs, designs, others=others, groups=groups, n_batches=[2 * P + 3], geo=geo)
    ref = against_host('trials_mixed_G%d_%s' % (conds, others), res, runs, designs, others, groups)
    assert (ref.dof > 0).all() and len({int(ref.dof[ref.run == r][0]) - d.X.shape[0] for r, d in enumerate(designs)}) == 3
    assert res.classes == ['c%02d' % i for i in range(conds)]
    assert res.folds().tolist() == [0] * (P - 3) + [0] * (2 * P + 3) + [1] * int((res.run == 2).sum())


def test_a_condition_with_a_single_trial(geo):
    rng = np.random.RandomState(21)
    ev = [(1 * TR, 3 * TR, 'a'), (9 * TR, 3 * TR, 'b'), (17 * TR, 3 * TR, 'a'), (24 * TR, 3 * TR, 'lone'), (33 * TR, 3 * TR, 'b'),
          (41 * TR, 3 * TR, 'a')]
    T = geo['split'] + 3
    td = glm.trial_design(events=ev, T=T, tr=TR, high_pass=None, confounds=rng.randn(T, 2))
    y = (100.0 + 2.0 * (td.X @ rng.randn(6, 33)) + rng.randn(T, 33)).astype(np.float32)
    res = run_device(y, td, n_batches=[6], geo=geo)
    against_host('trials_lone', res, y, td)
    assert res.dof.tolist() == [T - 3 - 4] * 3 + [T - 3 - 3] + [T - 3 - 4] * 2          # the lone trial's model drops its empty column


def test_results_are_bit_identical(mixed, geo):
    import torch
    runs, designs, groups = mixed
    P = geo['panel']
    res = run_device(runs, designs, groups=groups, geo=geo)
    same(res, run_device(runs, designs, groups=groups, geo=geo))                                # twice in a row
    counts = [d.X.shape[1] for d in designs]
    same(res, run_device(runs, designs, groups=groups, batch_runs=1, n_batches=counts, geo=geo))  # a batch per run: its own nmax and k
    for r in range(3):                                                                            # a run alone
        alone = run_device(runs[r], designs[r], geo=geo)
        for name in ALL:
            assert np.array_equal(getattr(alone, name), getattr(res, name)[res.run == r]), (r, name)
    tens = run_device([torch.as_tensor(r).cuda() for r in runs], designs, groups=groups, geo=geo)
    assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() for x in (tens.beta, tens.variance, tens.t))
    same(res, tens)
    half = run_device([torch.as_tensor(runs[0]).cuda(), runs[1], runs[2]], designs, groups=groups, geo=geo)
    assert isinstance(half.beta, np.ndarray)
    same(res, half)
    only = run_device(runs, designs, groups=groups, outputs=('t',), geo=geo)
    assert only.beta is None and only.variance is None and np.array_equal(only.t, res.t)


def test_bold_scaled_series_where_float32_sums_fail():
    """Mean 1e4, noise sd 50, T = 284, 13 confounds, 40 trials.  The same algebra with float32 projections misses the bound by
    more than 10x (shown here in NumPy), the kernels' float64 sums hold it."""
    rng = np.random.RandomState(5)
    y, td = make_run(rng, n=40, T=284, confounds=13, M=40, gap=4, mean=1e4, sd=50.0, gain=30.0)
    assert td.X.shape == (284, 40) and td.nuisance.shape == (284, 14)
    res = run_device(y, td)
    ref = against_host('trials_bold', res, y, td)
    tb = glm._trial_plan(y, td, 'condition', ALL, None, 't').tables[0]
    p32 = (tb.ZX.T.astype(np.float32) @ y).astype(np.float64)
    c32 = (tb.ZS.T.astype(np.float32) @ y).astype(np.float64)
    b32 = np.stack([tb.w[j] @ np.concatenate([p32[j:j + 1], c32 - np.outer(np.arange(2) == tb.own[j], p32[j])]) for j in range(tb.n)])
    assert worst(b32, ref.beta, scales(y, td, 'condition')[0]) > 10.0


def test_a_vertex_constant_in_time(geo):
    rng = np.random.RandomState(6)
    M = geo['vertices']
    y, td = make_run(rng, T=geo['split'] + 9, M=M)
    y[:, 5] = 100.0
    y[:, 40] = 0.0
    res = run_device(y, td)
    for v in (5, 40):
        assert (res.variance[:, v] == 0).all() and (res.t[:, v] == 0).all()
    assert (res.beta[:, 40] == 0).all()
    against_host('trials_constant', res, y, td)                 # their neighbours in the same wave hold the bound
    others = np.setdiff1d(np.arange(M), [5, 40])
    assert (res.variance[:, others] > 0).all() and np.isfinite(res.t).all()


def test_nan_in_the_pad_columns_stays_there(geo):
    import torch
    from gcn_fmri_decoding_amd import ops
    rng = np.random.RandomState(7)
    M = 33
    Mp = _lib.plane_stride(M)
    y, td = make_run(rng, n=geo['panel'] + 2, M=M)
    res = run_device(y, td)
    pl = glm._trial_plan(y, td, 'condition', ALL, None, 't')
    T = pl.tables[0].T
    planes = np.full((T, Mp), np.nan, np.float32)
    planes[:, :M] = y
    dev = torch.device('cuda')
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    Q, Z, toffs, qrank, own, rank, w, F = (up(a) for a in glm._trial_tables(pl.tables, pl.G))
    offs = up(np.array([0, T], np.int64))
    a, yy = ops.glm_project(up(planes), offs, M, Q)
    out = ops.glm_trials(up(planes), offs, M, Z, toffs, a, yy, qrank, own, rank, w, F, outputs=ALL)
    for got, want in zip(out, (res.beta, res.variance, res.t)):
        assert got.shape == (td.X.shape[1], Mp) and torch.isfinite(got).all() and not got[:, M:].any()
        assert np.array_equal(got[:, :M].cpu().numpy(), want)


def test_two_trials_pooled_agree_with_first_level_on_the_device(geo):
    """[x_1 | x_2 | N] either way: the two device routes agree within the sum of their bounds."""
    rng = np.random.RandomState(8)
    y, td = make_run(rng, n=2, T=geo['split'] + 7, M=geo['vertices'] + 1)
    res = run_device(y, td, others='pooled')
    ref = against_host('trials_two', res, y, td, 'pooled')
    full = glm.Design(np.concatenate([td.X, td.nuisance], axis=1), td.columns, td.conditions)
    fl = glm.first_level(y, full, np.eye(2, full.X.shape[1]), betas=True)
    tb = glm._plan(y, full, np.eye(2, full.X.shape[1]), None, 't').tables[0]
    yy = (y.astype(np.float64) ** 2).sum(axis=0)
    s_b, s_v = scales(y, td, 'pooled')
    for j in range(2):
        s_fl_b = np.linalg.norm(tb.B[j]) * np.sqrt(yy)
        s_fl_v = tb.un2[j] * yy / (tb.T - tb.rank)
        assert (np.abs(res.beta[j].astype(np.float64) - fl.betas[0][j])
                <= 2 * EPS32 * np.abs(ref.beta[j]) + FLOOR * (s_b[j] + s_fl_b)).all()
        assert (np.abs(res.variance[j].astype(np.float64) - fl.variance[0, j])
                <= 2 * EPS32 * ref.variance[j] + FLOOR * (s_v[j] + s_fl_v)).all()
    assert fl.dof.tolist() == [res.dof[0]] and res.dof[0] == res.dof[1]


def planted(seed=4, gain=4.0):
    """Six subjects of two runs on a ring of 64 vertices; conditions a and b with opposite-signed amplitudes on a patch of 10."""
    rng = np.random.RandomState(seed)
    M, T = 64, 150
    patch = np.arange(20, 30)
    runs, designs, groups = [], [], []
    for s in range(6):
        for r in range(2):
            on, ev = 2, []
            while on + 3 + 14 < T:
                ev.append((on * TR, 3 * TR, 'ab'[(len(ev) + r) % 2]))
                on += 3 + rng.randint(4, 9)
            td = glm.trial_design(events=ev, T=T, tr=TR, high_pass=None, confounds=rng.randn(T, 2))
            amp = np.zeros((len(ev), M))
            amp[:, patch] = np.where(td.trials == 0, gain, -gain)[:, None] * (1.0 + 0.2 * rng.rand(patch.size))
            runs.append((1000.0 + td.X @ amp + 4.0 * rng.randn(T, M)).astype(np.float32))
            designs.append(td)
            groups.append(s)
    ring = sp.csr_matrix((np.ones(M), (np.arange(M), (np.arange(M) + 1) % M)), shape=(M, M))
    return runs, designs, groups, patch, ring + ring.T


def test_end_to_end_with_searchlight_and_map_test():
    """``single_trial -> searchlight -> map_test``: the significant centres contain the patch and lie inside the patch widened by
    one hop -- for the host chain by itself (seed and gain were chosen on the CPU so that it does), and then for the device's."""
    runs, designs, groups, patch, ring = planted()
    wide = np.arange(patch[0] - 1, patch[-1] + 2)
    balls = graph.hop_balls(ring, 1)
    for st, sl, mt in ((glm.single_trial_host, searchlight.searchlight_host, stats.map_test_host),
                       (glm.single_trial, searchlight.searchlight, stats.map_test)):
        res = st(runs, designs, groups=groups)
        assert res.variance is None and res.beta.shape == res.t.shape == (len(res.labels), 64)
        acc = sl(res.beta, res.labels, balls, res.folds(), groups=res.group, within=True, classifier='gnb').accuracy
        assert acc.shape == (6, 64)
        test = mt(np.asarray(acc, np.float32) - 0.5, ring, stat='max', tail=1, n_perm=64, seed=1)
        found = np.flatnonzero(test.p <= 0.05)
        assert np.isin(patch, found).all() and np.isin(found, wide).all(), (st.__name__, found)
