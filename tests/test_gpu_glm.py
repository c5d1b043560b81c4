"""``glm.first_level`` on the device (chebgcn_glm_project / _finish / _combine) against its float64 host restatement
``glm.first_level_host``, which forms residuals explicitly and knows nothing of the kernels' projection trick.  Shapes come from
``ops.glm_geometry()``.

The bound, for effect, variance, beta and t at EVERY vertex:  ``|got - ref| <= 2^-23 |ref| + 1e-10 s``  -- one float32 rounding
plus the float64 dot-product bound ``T 2^-53`` at T <= 2000 with a 500x margin, times the natural scale s of the quantity:

* effect of a run: ``s = |u| sqrt(y.y)`` (Cauchy-Schwarz on ``u.a``, ``|a| <= |y|``); a coefficient: ``|B_p| sqrt(y.y)``;
* variance of a run: ``s = |u|^2 y.y / dof`` (the kernel's ``rss = y.y - a.a`` cancels at the scale of ``y.y``);
* a group: the same combination of the scales as of the values (mean of the effects' scales, sum / R_g^2 of the variances');
* ``t = e / sqrt(v)``: its first-order propagation, ``s = s_e / sqrt(v) + |t| s_v / (2 v)`` with the reference's v and t.  Where
  the reference's variance is exactly 0 the device's t must be exactly 0.

Measured on an MI355X (``record_measured`` keeps every case's figures), as fractions of the bound: effect at most 0.49, coefficients
0.49, variance 0.06, t 0.12 -- the float32 rounding (half of ``2^-23``) and next to nothing else; t relative to float64 at most
6e-8 (1.8e-7 in the run with one degree of freedom).
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, glm, stats

pytestmark = pytest.mark.gpu

EPS32, FLOOR = 2.0 ** -23, 1e-10


@pytest.fixture(scope='module')
def geo():
    from gcn_fmri_decoding_amd import ops
    return ops.glm_geometry()


def project_names(k, geo):
    """What chebgcn_last_dispatch() reports for a projection of k columns."""
    widths = [min(geo['panel'], k - j0) for j0 in range(0, k, geo['panel'])]
    return ' + '.join('glm_project_kernel<%d>' % w for w in widths)


def random_design(rng, T, P, C):
    """A full-rank design of P columns (the last the intercept) scaled like regressors, and C random contrasts."""
    X = rng.randn(T, P)
    X[:, -1] = 1.0
    return glm.Design(X, ['x%d' % i for i in range(P - 1)] + ['constant'], ['x0']), rng.randn(C, P)


def series(rng, design, M, mean=100.0, sd=1.0, gain=2.0):
    X = design.X
    return (mean + gain * (X[:, :-1] @ rng.randn(X.shape[1] - 1, M)) + sd * rng.randn(X.shape[0], M)).astype(np.float32)


def run_device(runs, designs, contrasts=None, groups=None, k_batches=None, geo=None, **kw):
    """``first_level(betas=True)`` with the dispatch log checked: every projection ran the panels its batch's k asks for."""
    _lib.dispatch_log = log = []
    try:
        res = glm.first_level(runs, designs, contrasts, groups, betas=True, **kw)
    finally:
        _lib.dispatch_log = None
    what = [w for w, _ in log]
    n = what.count('glm_project')
    assert n >= 1 and what == ['glm_project', 'glm_finish'] * n + ['glm_combine'], what
    assert {d for w, d in log if w == 'glm_finish'} == {'glm_finish_kernel'}
    assert log[-1][1] == 'glm_combine_kernel'
    if k_batches is not None:
        assert [d for w, d in log if w == 'glm_project'] == [project_names(k, geo) for k in k_batches]
    return res


def scales(runs, designs, contrasts, groups):
    """The natural scales of the bound, per group for effect and variance and per run for the coefficients."""
    pl = glm._plan(runs, designs, contrasts, groups, 'scales')
    yy = [(np.asarray(r.cpu() if hasattr(r, 'cpu') else r, np.float32).astype(np.float64) ** 2).sum(axis=0) for r in pl.runs]
    se = [np.sqrt(tb.un2)[:, None] * np.sqrt(y)[None, :] for tb, y in zip(pl.tables, yy)]
    sv = [tb.un2[:, None] * y[None, :] / (tb.T - tb.rank) for tb, y in zip(pl.tables, yy)]
    sb = [np.linalg.norm(tb.B, axis=1)[:, None] * np.sqrt(y)[None, :] for tb, y in zip(pl.tables, yy)]
    s_e = np.stack([sum(se[r] for r in m) / len(m) for m in pl.members])
    s_v = np.stack([sum(sv[r] for r in m) / len(m) ** 2 for m in pl.members])
    return s_e, s_v, sb


def worst(got, ref, s):
    """max over every element of |got - ref| / (2^-23 |ref| + 1e-10 s): the bound holds iff <= 1."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (EPS32 * np.abs(ref) + FLOOR * s + 1e-300)).max())


def against_host(name, res, runs, designs, contrasts=None, groups=None):
    ref = glm.first_level_host(runs, designs, contrasts, groups, betas=True)
    s_e, s_v, s_b = scales(runs, designs, contrasts, groups)
    assert res.effect.dtype == res.variance.dtype == res.t.dtype == np.float32
    assert res.effect.shape == ref.effect.shape and res.groups == ref.groups and np.array_equal(res.dof, ref.dof)
    pos = ref.variance > 0
    assert (res.t[~pos] == 0).all()
    v = np.where(pos, ref.variance, 1.0)
    s_t = np.where(pos, s_e / np.sqrt(v) + np.abs(ref.t) * s_v / (2.0 * v), 0.0)
    m = {'effect': worst(res.effect, ref.effect, s_e), 'variance': worst(res.variance, ref.variance, s_v),
         't': worst(np.where(pos, res.t, 0.0), np.where(pos, ref.t, 0.0), s_t),
         'beta': max(worst(b, rb, s) for b, rb, s in zip(res.betas, ref.betas, s_b))}
    rel_t = float((np.abs(res.t.astype(np.float64) - ref.t)[pos] / np.maximum(np.abs(ref.t[pos]), 1e-300)).max()) if pos.any() else 0.0
    record_measured(name, bound_used=m, t_rel=rel_t)
    print(name, m, 't rel %.3e' % rel_t)
    for key, val in m.items():
        assert val <= 1.0, '%s: %s error is %.3f of its bound' % (name, key, val)
    assert all(b.dtype == np.float32 and b.shape == rb.shape for b, rb in zip(res.betas, ref.betas))
    return ref


def same(a, b):
    for name in ('effect', 'variance', 't'):
        u, v = (np.asarray(x.cpu() if hasattr(x, 'cpu') else x) for x in (getattr(a, name), getattr(b, name)))
        assert u.dtype == v.dtype and np.array_equal(u, v), '%s differs at %d places' % (name, int((u != v).sum()))
    assert np.array_equal(a.dof, b.dof) and a.groups == b.groups
    if a.betas is not None and b.betas is not None:
        for u, v in zip(a.betas, b.betas):
            assert np.array_equal(np.asarray(u.cpu() if hasattr(u, 'cpu') else u), np.asarray(v.cpu() if hasattr(v, 'cpu') else v))


@pytest.mark.parametrize('M', ['1', '31', '32', '33', 'VB-1', 'VB+1'])
def test_vertex_counts_around_the_tile(M, geo):
    M = {'VB-1': geo['vertices'] - 1, 'VB+1': geo['vertices'] + 1}.get(M) or int(M)
    rng = np.random.RandomState(M)
    d, c = random_design(rng, geo['split'] + 5, 3, 2)
    y = series(rng, d, M)
    res = run_device(y, d, c, k_batches=[3], geo=geo)
    against_host('glm_M%d' % M, res, y, d, c)
    assert res.effect.shape == (1, 2, M) and res.betas[0].shape == (3, M)


@pytest.mark.parametrize('C', ['1', 'Cmax'])
@pytest.mark.parametrize('k', ['1', '2', 'panel-1', 'panel', 'panel+1', 'kmax'])
def test_ranks_around_the_panel_and_most_contrasts(k, C, geo):
    k = {'panel-1': geo['panel'] - 1, 'panel': geo['panel'], 'panel+1': geo['panel'] + 1, 'kmax': geo['max_k']}.get(k) or int(k)
    C = geo['max_C'] if C == 'Cmax' else 1
    rng = np.random.RandomState(100 * k + C)
    d, c = random_design(rng, 3 * geo['slice'] + 5 + k, k, C)
    y = series(rng, d, 33)
    res = run_device(y, d, c, k_batches=[k], geo=geo)
    against_host('glm_k%d_C%d' % (k, C), res, y, d, c)
    assert res.effect.shape == (1, C, 33) and res.dof.tolist() == [3 * geo['slice'] + 5]


@pytest.mark.parametrize('T', ['k+1', 'split-1', 'split', 'split+1', '3slices+5'])
def test_run_lengths_around_the_split(T, geo):
    k = 5
    T = {'k+1': k + 1, 'split-1': geo['split'] - 1, 'split': geo['split'], 'split+1': geo['split'] + 1, '3slices+5': 3 * geo['slice'] + 5}[T]
    rng = np.random.RandomState(T)
    d, c = random_design(rng, T, k, 2)
    y = series(rng, d, 33)
    res = run_device(y, d, c, k_batches=[k], geo=geo)
    against_host('glm_T%d' % T, res, y, d, c)


@pytest.fixture(scope='module')
def mixed(geo):
    """Three runs of lengths (k + 1, 7 slices + 3, k + 2) with designs of different width, one group each."""
    rng = np.random.RandomState(11)
    k = 6
    shapes = [(k + 1, k), (7 * geo['slice'] + 3, 4), (k + 2, 5)]
    designs, contrasts = zip(*[random_design(rng, T, P, 2) for T, P in shapes])
    runs = [series(rng, d, geo['vertices'] + 1) for d in designs]
    return runs, list(designs), list(contrasts), ['a', 'b', 'c']


def test_one_call_with_runs_of_different_length_and_design(mixed, geo):
    runs, designs, contrasts, groups = mixed
    res = run_device(runs, designs, contrasts, groups, k_batches=[6], geo=geo)
    against_host('glm_mixed', res, runs, designs, contrasts, groups)
    assert res.dof.tolist() == [1, 7 * geo['slice'] + 3 - 4, 3] and [b.shape[0] for b in res.betas] == [6, 4, 5]


def test_results_are_bit_identical(mixed, geo):
    import torch
    runs, designs, contrasts, groups = mixed
    res = run_device(runs, designs, contrasts, groups, geo=geo)
    same(res, run_device(runs, designs, contrasts, groups, geo=geo))                                  # twice in a row
    one = run_device(runs, designs, contrasts, groups, batch_runs=1, k_batches=[6, 4, 5], geo=geo)    # a batch per run: its own k
    same(res, one)
    for r in range(3):                                                                                # a run alone
        alone = run_device(runs[r], designs[r], contrasts[r], geo=geo)
        for name in ('effect', 'variance', 't'):
            assert np.array_equal(getattr(alone, name)[0], getattr(res, name)[r]), (r, name)
        assert np.array_equal(alone.betas[0], res.betas[r])
    tens = run_device([torch.as_tensor(r).cuda() for r in runs], designs, contrasts, groups, geo=geo)
    assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in (tens.effect, tens.variance, tens.t))
    assert all(torch.is_tensor(b) and b.is_cuda for b in tens.betas)
    same(res, tens)
    half = run_device([torch.as_tensor(runs[0]).cuda(), runs[1], runs[2]], designs, contrasts, groups, geo=geo)
    assert isinstance(half.effect, np.ndarray)
    same(res, half)


def test_bold_scaled_series_where_float32_sums_fail():
    """Mean 1e4, noise sd 50, T = 284, 22 regressors: rss / y.y = 2e-5.  The same algebra with float32 projections misses the
    bound by orders of magnitude (shown here in NumPy), the kernels' float64 sums hold it."""
    rng = np.random.RandomState(5)
    T, M = 284, 40
    names = (['rest'] * 15 + ['a'] * 20 + ['rest'] * 16 + ['b'] * 20 + ['rest'] * 15 + ['c'] * 20 + ['rest'] * 16 + ['d'] * 20) * 2
    d = glm.design_matrix(names=names, tr=0.72, high_pass=0.01, confounds=rng.randn(T, 13))
    assert d.X.shape == (T, 22)
    y = (1e4 + 50.0 * rng.randn(T, M) + 30.0 * (d.X[:, :4] @ rng.randn(4, M))).astype(np.float32)
    res = run_device(y, d)
    ref = against_host('glm_bold', res, y, d)
    yy = (y.astype(np.float64) ** 2).sum(axis=0)
    ratio = ref.variance[0, 0] * (T - 22) / glm._plan(y, d, None, None, 't').tables[0].un2[0] / yy
    assert 1e-5 < ratio.min() and ratio.max() < 5e-5, (ratio.min(), ratio.max())
    tb = glm._plan(y, d, None, None, 't').tables[0]
    e32 = (tb.u.astype(np.float32) @ (tb.Q.T.astype(np.float32) @ y)).astype(np.float64)
    s_e = scales(y, d, None, None)[0]
    assert worst(e32[None], ref.effect, s_e) > 10.0


def test_a_vertex_constant_in_time(geo):
    rng = np.random.RandomState(6)
    M = geo['vertices']
    d, c = random_design(rng, geo['split'] + 9, 4, 3)
    y = series(rng, d, M)
    y[:, 5] = 100.0
    y[:, 40] = 0.0
    res = run_device(y, d, c)
    for v in (5, 40):
        assert (res.variance[0, :, v] == 0).all() and (res.t[0, :, v] == 0).all()
    assert (res.effect[0, :, 40] == 0).all()                # (vertex 5 keeps its effect: the contrasts weigh the intercept)
    against_host('glm_constant', res, y, d, c)              # its neighbours in the same wave hold the bound
    others = np.setdiff1d(np.arange(M), [5, 40])
    assert (res.variance[0][:, others] > 0).all() and np.isfinite(res.t).all()


def test_nan_in_the_pad_columns_stays_there(geo):
    import torch
    from gcn_fmri_decoding_amd import ops
    rng = np.random.RandomState(7)
    M = 33
    Mp = _lib.plane_stride(M)
    d, c = random_design(rng, 2 * geo['split'] + 3, geo['panel'] + 2, 2)
    y = series(rng, d, M)
    res = run_device(y, d, c)
    tb = glm._plan(y, d, c, None, 't').tables[0]
    planes = np.full((tb.T, Mp), np.nan, np.float32)
    planes[:, :M] = y
    dev = torch.device('cuda')
    offs = torch.as_tensor(np.array([0, tb.T], np.int64)).to(dev)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    a, yy = ops.glm_project(up(planes), offs, M, up(tb.Q))
    assert torch.isfinite(a).all() and torch.isfinite(yy).all() and not a[:, :, M:].any() and not yy[:, M:].any()
    e64 = torch.empty((1, 2, Mp), dtype=torch.float64, device=dev)
    v64 = torch.empty_like(e64)
    e32, v32, t32, beta = ops.glm_finish(a, yy, offs, tb.T, up(np.array([tb.rank], np.int32)), up(tb.u[None]), up(tb.un2[None]), M,
                                         B=up(tb.B[None]), out64=(e64, v64), want32=True)
    eff, var, t = ops.glm_combine(e64, v64, up(np.array([0, 1], np.int32)), up(np.array([0], np.int32)), M)
    for got, direct, want in ((eff, e32, res.effect), (var, v32, res.variance), (t, t32, res.t)):
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(direct[:, :, :M].cpu().numpy(), want)
    assert np.array_equal(beta[0, :, :M].cpu().numpy(), res.betas[0])


def test_three_groups_of_one_two_and_three_runs(geo):
    rng = np.random.RandomState(8)
    M = 37
    groups = ['s2', 's1', 's2', 's3', 's3', 's3']
    lengths = [geo['split'] + 3, 40, 3 * geo['slice'] + 5, 50, geo['split'] - 1, 4 * geo['slice'] + 1]
    names = (['rest'] * 4 + ['a'] * 6 + ['rest'] * 3 + ['b'] * 7) * 8
    designs = [glm.design_matrix(names=names[:T], tr=0.72, high_pass=0.02) for T in lengths]
    runs = [series(rng, d, M, mean=1000.0, sd=5.0) for d in designs]
    res = run_device(runs, designs, groups=groups)
    ref = against_host('glm_groups', res, runs, designs, groups=groups)
    assert res.groups == ['s2', 's1', 's3'] and res.effect.shape == (3, 2, M)
    assert res.dof.tolist() == ref.dof.tolist() == [sum(lengths[r] - designs[r].X.shape[1] for r in m) for m in ([0, 2], [1], [3, 4, 5])]
    same(res, run_device(runs, designs, groups=groups, batch_runs=4))


def test_end_to_end_with_map_test():
    """Eight synthetic subjects with condition a > b planted on a patch of a ring of 64 vertices: the effect maps go straight
    into ``map_test`` and the patch is what it finds."""
    rng = np.random.RandomState(9)
    M, S, T = 64, 8, 120
    names = (['rest'] * 5 + ['a'] * 10 + ['rest'] * 5 + ['b'] * 10) * 4
    patch = np.arange(20, 30)
    runs, designs = [], []
    for s in range(S):
        d = glm.design_matrix(names=names, tr=0.72)
        gain = np.zeros((2, M))
        gain[0, patch] = 8.0 + rng.rand(patch.size)
        runs.append((1000.0 + d.X[:, :2] @ gain + 4.0 * rng.randn(T, M)).astype(np.float32))
        designs.append(d)
    res = run_device(runs, designs, groups=list(range(S)))
    assert res.effect.shape == (S, 2, M) and res.effect.dtype == np.float32
    ring = sp.csr_matrix((np.ones(M), (np.arange(M), (np.arange(M) + 1) % M)), shape=(M, M))
    mt = stats.map_test(res.effect, ring, stat='max', n_perm=64, tail=1, seed=3)
    assert mt.t.shape == (2, M) and mt.t.dtype == np.float32 and mt.p.shape == (2, M) and mt.p.dtype == np.float64
    assert mt.null.shape == (2, 64) and mt.n_perm == 64 and not mt.exact
    found = np.flatnonzero(mt.p[0] <= 0.05)                 # class a: a > b
    assert np.array_equal(found, patch), found
    assert not (mt.p[1] <= 0.05).any()                      # class b: b > a nowhere
