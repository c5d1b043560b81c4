"""``glm.first_level(noise='ar1')`` on the device (chebgcn_glm_project_ar1 / _finish_ar1 / _combine) against its float64 host
restatement ``glm.first_level_host(noise='ar1')``, which builds the T x T covariance of every vertex, whitens by its Cholesky
factor and forms residuals, and knows nothing of the kernels' sums.  Inputs, scales and the bound
``|got - ref| <= 2^-23 |ref| + EPS s`` are those of glm_ar1_common.py: EPS = 3.64e-11 is four times what the same algebra costs
in float64 NumPy on these very inputs (measured on the CPU by test_glm_ar1_host.py).

Measured on an MI355X (``record_measured`` keeps every case's figures), as fractions of the bound: effect at most 0.50,
coefficients 0.49, t 0.31, variance 0.25, rho 0.10 -- the float32 rounding (half of ``2^-23``) and next to nothing else."""
import numpy as np
import pytest
import scipy.sparse as sp

import glm_ar1_common as G
from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, glm, stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def geo():
    return G.geometry()


@pytest.fixture(scope='module')
def cases(geo):
    return G.device_cases(geo)


def project_names(k, geo):
    """What chebgcn_last_dispatch() reports for the pass over the 2k columns of [Q | Qs]."""
    widths = [min(geo['panel'], 2 * k - j0) for j0 in range(0, 2 * k, geo['panel'])]
    return ' + '.join('glm_project_ar1_kernel<%d>' % w for w in widths)


def run_device(runs, designs, contrasts=None, groups=None, rho=None, k_batches=None, geo=None, betas=True, **kw):
    """``first_level(noise='ar1')`` with the dispatch log checked: every batch ran the panels and the rank bucket of its k."""
    _lib.dispatch_log = log = []
    try:
        res = glm.first_level(runs, designs, contrasts, groups, betas=betas, noise='ar1', rho=rho, **kw)
    finally:
        _lib.dispatch_log = None
    what = [w for w, _ in log]
    n = what.count('glm_project_ar1')
    assert n >= 1 and what == ['glm_project_ar1', 'glm_finish_ar1'] * n + ['glm_combine'], what
    assert log[-1][1] == 'glm_combine_kernel'
    if k_batches is not None:
        assert [d for w, d in log if w == 'glm_project_ar1'] == [project_names(k, geo) for k in k_batches]
        assert [d for w, d in log if w == 'glm_finish_ar1'] == ['glm_finish_ar1_kernel<%d>' % geo['bucket'](k) for k in k_batches]
    assert isinstance(res, glm.GLMResultAR1)
    return res


def against_host(name, res, runs, designs, contrasts=None, groups=None, rho=None, clamped=()):
    ref = glm.first_level_host(runs, designs, contrasts, groups, betas=True, noise='ar1', rho=rho)
    assert res.effect.dtype == res.variance.dtype == res.t.dtype == np.float32 and all(r.dtype == np.float32 for r in res.rho)
    assert res.effect.shape == ref.effect.shape and res.groups == ref.groups and np.array_equal(res.dof, ref.dof)
    assert len(res.rho) == len(ref.rho) and all(a.shape == b.shape for a, b in zip(res.rho, ref.rho))
    free = np.ones(ref.rho[0].shape, bool)
    free[list(clamped)] = False
    at_clamp = sum(int((np.abs(r[free]) >= G.RHO_FREE).sum()) for r in ref.rho)
    assert at_clamp == 0, '%s: %d vertices of the host sit at the clamp' % (name, at_clamp)
    pos = ref.variance > 0
    assert (res.t[~pos] == 0).all()
    m = G.distances(res, ref, runs, designs, contrasts, groups, G.EPS)
    record_measured(name, bound_used=m)
    print(name, m)
    for key, val in m.items():
        assert val <= 1.0, '%s: %s error is %.3f of its bound' % (name, key, val)
    assert all(b.dtype == np.float32 and b.shape == rb.shape for b, rb in zip(res.betas, ref.betas))
    return ref


def same(a, b):
    get = lambda x: np.asarray(x.cpu() if hasattr(x, 'cpu') else x)
    for name in ('effect', 'variance', 't'):
        u, v = get(getattr(a, name)), get(getattr(b, name))
        assert u.dtype == v.dtype and np.array_equal(u, v), '%s differs at %d places' % (name, int((u != v).sum()))
    assert np.array_equal(a.dof, b.dof) and a.groups == b.groups
    for u, v in zip(a.rho, b.rho):
        assert np.array_equal(get(u), get(v))
    if a.betas is not None and b.betas is not None:
        for u, v in zip(a.betas, b.betas):
            assert np.array_equal(get(u), get(v))


@pytest.mark.parametrize('M', ['1', '33', 'VB+1'])
def test_vertex_counts_around_the_tile(M, geo, cases):
    M = geo['vertices'] + 1 if M == 'VB+1' else int(M)
    y, d, c, _, _ = cases['M%d' % M]
    res = run_device(y, d, c, k_batches=[3], geo=geo)
    against_host('glm_ar1_M%d' % M, res, y, d, c)
    assert res.effect.shape == (1, 2, M) and res.betas[0].shape == (3, M) and res.rho[0].shape == (M,)


@pytest.mark.parametrize('C', ['1', 'Cmax'])
@pytest.mark.parametrize('k', ['1', '2', 'panel/2', 'panel/2+1', 'panel', 'panel+1', '32', '33', 'kmax'])
def test_ranks_where_the_table_crosses_a_panel_and_the_rank_a_bucket(k, C, geo, cases):
    half = geo['panel'] // 2
    k = {'panel/2': half, 'panel/2+1': half + 1, 'panel': geo['panel'], 'panel+1': geo['panel'] + 1, 'kmax': geo['max_k']}.get(k) or int(k)
    C = geo['max_C'] if C == 'Cmax' else 1
    y, d, c, _, _ = cases['k%d_C%d' % (k, C)]
    res = run_device(y, d, c, k_batches=[k], geo=geo)
    against_host('glm_ar1_k%d_C%d' % (k, C), res, y, d, c)
    assert res.effect.shape == (1, C, 33) and res.dof.tolist() == [3 * geo['slice'] + 5]


@pytest.mark.parametrize('T', ['k+2', 'split-1', 'split', 'split+1', '3slices+5'])
def test_run_lengths_around_the_split(T, geo, cases):
    k = 5
    T = {'k+2': k + 2, 'split-1': geo['split'] - 1, 'split': geo['split'], 'split+1': geo['split'] + 1, '3slices+5': 3 * geo['slice'] + 5}[T]
    y, d, c, _, _ = cases['T%d' % T]
    res = run_device(y, d, c, k_batches=[k], geo=geo)
    against_host('glm_ar1_T%d' % T, res, y, d, c)


def test_one_call_with_runs_of_different_length_and_design(geo, cases):
    runs, designs, contrasts, groups, _ = cases['mixed']
    res = run_device(runs, designs, contrasts, groups, k_batches=[6], geo=geo)
    against_host('glm_ar1_mixed', res, runs, designs, contrasts, groups)
    assert res.dof.tolist() == [2, 7 * geo['slice'] + 3 - 4, 4] and [b.shape[0] for b in res.betas] == [6, 4, 5]


def test_results_are_bit_identical_under_every_batching(geo, cases):
    """The run-boundary test of the lag sum: a run gives the same bits alone (its own k, panels and bucket), in a batch of any
    cut, and as a tensor."""
    import torch
    runs, designs, contrasts, groups, _ = cases['mixed']
    res = run_device(runs, designs, contrasts, groups, geo=geo)
    same(res, run_device(runs, designs, contrasts, groups, geo=geo))
    same(res, run_device(runs, designs, contrasts, groups, batch_runs=1, k_batches=[6, 4, 5], geo=geo))
    same(res, run_device(runs, designs, contrasts, groups, batch_runs=2, k_batches=[6, 5], geo=geo))
    same(res, run_device(runs, designs, contrasts, groups, batch_runs=3, k_batches=[6], geo=geo))
    for r in range(3):
        alone = run_device(runs[r], designs[r], contrasts[r], geo=geo)
        for name in ('effect', 'variance', 't'):
            assert np.array_equal(getattr(alone, name)[0], getattr(res, name)[r]), (r, name)
        assert np.array_equal(alone.betas[0], res.betas[r]) and np.array_equal(alone.rho[0], res.rho[r])
    order = [1, 0, 2]                                           # other neighbours in the staged block
    swapped = run_device([runs[i] for i in order], [designs[i] for i in order], [contrasts[i] for i in order],
                         [groups[i] for i in order], geo=geo)
    for j, i in enumerate(order):
        assert np.array_equal(swapped.effect[j], res.effect[i]) and np.array_equal(swapped.rho[j], res.rho[i])
    tens = run_device([torch.as_tensor(r).cuda() for r in runs], designs, contrasts, groups, geo=geo)
    assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in (tens.effect, tens.variance, tens.t) + tuple(tens.rho))
    same(res, tens)


def test_a_given_rho_and_rho_zero_against_the_ols_path(geo, cases):
    y, d, c, _, rho = cases['given']
    res = run_device(y, d, c, rho=rho, k_batches=[6], geo=geo)
    against_host('glm_ar1_given', res, y, d, c, rho=rho)
    assert (res.rho[0] == np.float32(0.3)).all()
    zero = run_device(y, d, c, rho=0.0, geo=geo)
    ols = glm.first_level(y, d, c, betas=True)
    assert isinstance(ols, glm.GLMResult) and not isinstance(ols, glm.GLMResultAR1) and len(ols) == 6
    assert not zero.rho[0].any()
    for name, a, b in [(n, getattr(zero, n), getattr(ols, n)) for n in ('effect', 'variance', 't')] + [('beta', zero.betas[0], ols.betas[0])]:
        assert (np.abs(a - b) <= np.spacing(np.abs(b))).all(), name        # one float32 ulp


def test_three_groups_of_one_two_and_three_runs(geo, cases):
    runs, designs, contrasts, groups, _ = cases['groups']
    res = run_device(runs, designs, groups=groups)
    ref = against_host('glm_ar1_groups', res, runs, designs, groups=groups)
    assert res.groups == ['s2', 's1', 's3'] and res.effect.shape == (3, 2, 37) and len(res.rho) == 6
    assert res.dof.tolist() == ref.dof.tolist() == [sum(runs[r].shape[0] - designs[r].X.shape[1] for r in m) for m in ([0, 2], [1], [3, 4, 5])]
    same(res, run_device(runs, designs, groups=groups, batch_runs=4))


def test_a_vertex_constant_in_time(geo, cases):
    y, d, c, _, _ = cases['constant']
    res = run_device(y, d, c)
    for v in (5, 40):
        assert (res.variance[0, :, v] == 0).all() and (res.t[0, :, v] == 0).all() and res.rho[0][v] == 0
    assert (res.effect[0, :, 40] == 0).all() and (res.betas[0][:, 40] == 0).all()
    against_host('glm_ar1_constant', res, y, d, c)
    others = np.setdiff1d(np.arange(y.shape[1]), [5, 40])
    assert (res.variance[0][:, others] > 0).all() and np.isfinite(res.t).all() and np.isfinite(res.rho[0]).all()
    given = run_device(y, d, c, rho=0.3)                        # the floor of rss* alone
    for v in (5, 40):
        assert (given.variance[0, :, v] == 0).all() and (given.t[0, :, v] == 0).all()
    assert np.isfinite(given.t).all() and np.isfinite(given.effect).all()


def test_nan_in_the_pad_columns_stays_there(geo):
    import torch
    from gcn_fmri_decoding_amd import ops
    rng = np.random.RandomState(7)
    M = 33
    Mp = _lib.plane_stride(M)
    d, c = G.random_design(rng, 2 * geo['split'] + 3, geo['panel'] + 2, 2)
    y = G.series(rng, d, M)
    res = run_device(y, d, c)
    tb = glm._plan(y, d, c, None, 't').tables[0]
    planes = np.full((tb.T, Mp), np.nan, np.float32)
    planes[:, :M] = y
    dev = torch.device('cuda')
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    offs = up(np.array([0, tb.T], np.int64))
    W, D, E = (up(a) for a in glm._ar1_tables([tb], tb.rank))
    rows = up(planes)
    ah, s0, s1 = ops.glm_project_ar1(rows, offs, M, W)
    for x in (ah, s0, s1):
        assert torch.isfinite(x).all() and not x[..., M:].any()
    e64 = torch.empty((1, 2, Mp), dtype=torch.float64, device=dev)
    v64 = torch.empty_like(e64)
    e32, v32, t32, beta, rho = ops.glm_finish_ar1(ah, s0, s1, rows, W, offs, up(np.array([tb.rank], np.int32)), D, E, up(tb.u[None]), M,
                                                  B=up(tb.B[None]), out64=(e64, v64), want32=True)
    for x in (e64, v64, e32, v32, t32, beta, rho):
        assert torch.isfinite(x).all() and not x[..., M:].any()
    eff, var, t = ops.glm_combine(e64, v64, up(np.array([0, 1], np.int32)), up(np.array([0], np.int32)), M)
    for got, direct, want in ((eff, e32, res.effect), (var, v32, res.variance), (t, t32, res.t)):
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(direct[:, :, :M].cpu().numpy(), want)
    assert np.array_equal(beta[0, :, :M].cpu().numpy(), res.betas[0]) and np.array_equal(rho[0, :M].cpu().numpy(), res.rho[0])


def test_a_slow_sinusoid_sits_at_the_clamp_on_both_sides(geo):
    y, d, c = G.sinusoid(geo)
    res = run_device(y, d, c)
    ref = against_host('glm_ar1_sinusoid', res, y, d, c, clamped=[0])
    assert ref.rho[0][0] == glm.RHO_MAX and res.rho[0][0] == np.float32(glm.RHO_MAX)
    assert (np.abs(res.rho[0][1:]) < G.RHO_FREE).all()


def test_end_to_end_with_map_test():
    """Eight synthetic subjects with a > b planted on a patch of a ring of 64 vertices, under AR(1) noise: the prewhitened
    effect maps go straight into ``map_test`` and the patch is what it finds."""
    rng = np.random.RandomState(9)
    M, S, T = 64, 8, 120
    names = (['rest'] * 5 + ['a'] * 10 + ['rest'] * 5 + ['b'] * 10) * 4
    patch = np.arange(20, 30)
    runs, designs = [], []
    for s in range(S):
        d = glm.design_matrix(names=names, tr=0.72)
        gain = np.zeros((2, M))
        gain[0, patch] = 8.0 + rng.rand(patch.size)
        runs.append((1000.0 + d.X[:, :2] @ gain + 3.0 * G.ar1_noise(rng, T, M, 0.4)).astype(np.float32))
        designs.append(d)
    res = run_device(runs, designs, groups=list(range(S)), betas=False)
    assert res.effect.shape == (S, 2, M) and res.effect.dtype == np.float32 and res.betas is None and len(res.rho) == S
    assert 0.2 < np.mean([r.mean() for r in res.rho]) < 0.5
    ring = sp.csr_matrix((np.ones(M), (np.arange(M), (np.arange(M) + 1) % M)), shape=(M, M))
    mt = stats.map_test(res.effect, ring, stat='max', n_perm=64, tail=1, seed=3)
    assert mt.t.shape == (2, M) and mt.p.shape == (2, M)
    found = np.flatnonzero(mt.p[0] <= 0.05)
    assert np.array_equal(found, patch), found
    assert not (mt.p[1] <= 0.05).any()
