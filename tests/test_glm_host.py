"""Host side of the first-level GLM (``glm.design_matrix``, ``glm.contrasts_one_vs_rest``, ``glm.first_level_host``) and the
argument checks of the ``chebgcn_glm_*`` entry points, which return before any launch: no GPU."""
import ctypes

import numpy as np
import pytest
from scipy import stats as sps

from gcn_fmri_decoding_amd import _lib, events, glm

TR = 0.72
NAMES = ['rest'] * 10 + ['math'] * 20 + ['rest'] * 10 + ['story'] * 25 + ['rest'] * 15 + ['math'] * 7 + ['rest'] * 10 + ['story'] * 1 \
    + ['rest'] * 12
EVENTS = [(10 * TR, 20 * TR, 'math'), (40 * TR, 25 * TR, 'story'), (80 * TR, 7 * TR, 'math'), (97 * TR, 1 * TR, 'story')]


def riemann(names, cond, tr, hrf, sub=200):
    """The regressor of ``cond`` by brute force: the boxcar on a tr / sub grid convolved with the HRF's density."""
    from scipy.stats import gamma
    T, dt = len(names), tr / sub
    box = np.repeat((np.asarray(names) == cond).astype(np.float64), sub)
    s = np.arange(0.0, 60.0, dt)
    a1, a2, ratio = hrf
    h = (gamma.pdf(s, a1) - ratio * gamma.pdf(s, a2)) / (1.0 - ratio)
    return (np.convolve(box, h)[:T * sub] * dt)[::sub]


@pytest.mark.parametrize('hrf', ['spm', (5.0, 14.0, 0.25)])
def test_closed_form_regressors_against_a_riemann_convolution(hrf):
    d = glm.design_matrix(names=NAMES, tr=TR, hrf=hrf)
    shape = glm.HRF_SPM if hrf == 'spm' else hrf
    for i, cond in enumerate(d.conditions):
        err = np.abs(d.X[:, i] - riemann(NAMES, cond, TR, shape)).max()
        assert err <= 1e-3, (cond, err)
    long_block = glm.design_matrix(names=['rest'] * 5 + ['on'] * 120, tr=TR, high_pass=None)
    assert abs(long_block.X[-1, 0] - 1.0) < 1e-9            # plateau 1


def test_names_and_events_give_the_same_design():
    a = glm.design_matrix(names=NAMES, tr=TR)
    b = glm.design_matrix(events=EVENTS, T=len(NAMES), tr=TR)
    assert a.columns == b.columns and a.conditions == b.conditions
    assert np.array_equal(a.X, b.X)
    assert a.X.dtype == np.float64 and a.X.shape == (len(NAMES), len(a.columns))


def test_class_order_is_that_of_match_events():
    ew = events.match_events([NAMES], ['story', 'math'], block_dura=5, flag_event=1)
    d = glm.design_matrix(names=NAMES, tr=TR)
    assert d.conditions == ew.classes == ['math', 'story']
    assert d.columns[:2] == ew.classes and d.columns[-1] == 'constant'
    c = glm.contrasts_one_vs_rest(d)
    assert c.shape == (2, len(d.columns))
    assert np.array_equal(c[:, :2], [[1.0, -1.0], [-1.0, 1.0]]) and not c[:, 2:].any()
    three = glm.design_matrix(names=['a', 'b', 'c', 'rest'] * 6, tr=TR, high_pass=None)
    assert np.array_equal(glm.contrasts_one_vs_rest(three)[:, :3], np.where(np.eye(3) > 0, 1.0, -0.5))
    one = glm.design_matrix(names=['a', 'rest'] * 6, tr=TR, high_pass=None)
    assert np.array_equal(glm.contrasts_one_vs_rest(one), [[1.0, 0.0]])
    picked = glm.design_matrix(names=NAMES, tr=TR, conditions=['story'])
    assert picked.conditions == ['story'] and np.array_equal(picked.X[:, 0], d.X[:, 1])


def test_drift_columns_boxcar_confounds_and_intercept():
    T = 200
    names = ['rest'] * 50 + ['a'] * 50 + ['rest'] * 100
    for hp, order in [(1.0 / 128, int(np.floor(2 * T * TR / 128.0))), (0.01, 2), (None, 0), (0.0, 0), (1e-4, 0)]:
        d = glm.design_matrix(names=names, tr=TR, high_pass=hp)
        drifts = [c for c in d.columns if c.startswith('drift_')]
        assert drifts == ['drift_%d' % j for j in range(1, order + 1)], (hp, drifts)
        k = np.arange(T)
        for j in range(1, order + 1):
            assert np.allclose(d.X[:, d.columns.index('drift_%d' % j)], np.cos(np.pi * (2 * k + 1) * j / (2.0 * T)), rtol=0, atol=1e-15)
        assert np.array_equal(d.X[:, -1], np.ones(T))
    box = glm.design_matrix(names=names, tr=TR, hrf=None, high_pass=None)
    assert np.array_equal(box.X[:, 0], (np.asarray(names) == 'a').astype(np.float64))
    half = glm.design_matrix(events=[(1.5 * TR, 2.0 * TR, 'a')], T=6, tr=TR, hrf=None, high_pass=None)
    assert np.array_equal(half.X[:, 0], [0, 0, 1, 1, 0, 0])                # [1.5, 3.5) tr sampled at k tr
    conf = np.random.RandomState(0).randn(T, 3)
    d = glm.design_matrix(names=names, tr=TR, confounds=conf)
    q0 = d.columns.index('confound_0')
    assert d.columns[q0:] == ['confound_0', 'confound_1', 'confound_2', 'constant'] and np.array_equal(d.X[:, q0:q0 + 3], conf)


@pytest.mark.parametrize('kw', [
    dict(), dict(names=NAMES, events=EVENTS, T=len(NAMES)), dict(events=EVENTS), dict(names=NAMES, T=5), dict(names=[]),
    dict(names='math'), dict(names=[1, 2, 3]), dict(names=[['a', 'b']]), dict(names=NAMES, tr=0), dict(names=NAMES, tr=float('nan')),
    dict(names=NAMES, tr='1'), dict(names=NAMES, hrf='glover'), dict(names=NAMES, hrf=(6, 16)), dict(names=NAMES, hrf=(6, 16, 1.0)),
    dict(names=NAMES, hrf=(-1, 16, 0.1)), dict(names=NAMES, high_pass=-1.0), dict(names=NAMES, high_pass='x'),
    dict(names=NAMES, confounds=np.zeros((3, 2))), dict(names=NAMES, confounds=np.full((len(NAMES), 1), np.nan)),
    dict(names=NAMES, confounds=np.zeros(len(NAMES))), dict(names=NAMES, conditions=[]), dict(names=NAMES, conditions='math'),
    dict(names=NAMES, conditions=['math', 'math']), dict(names=NAMES, conditions=[1]), dict(events=[], T=10),
    dict(events=[(0.0, 1.0)], T=10), dict(events=[(0.0, -1.0, 'a')], T=10), dict(events=[(float('inf'), 1.0, 'a')], T=10),
    dict(events=[(0.0, 1.0, 3)], T=10), dict(events=EVENTS, T=0), dict(events=EVENTS, T=2.5), dict(names=['rest'] * 8),
])
def test_design_matrix_refuses(kw):
    with pytest.raises(ValueError, match='design_matrix'):
        glm.design_matrix(**kw)


def test_one_regressor_against_linregress():
    rng = np.random.RandomState(1)
    T, M = 60, 5
    x = rng.randn(T)
    y = (3.0 + np.outer(x, rng.randn(M)) + rng.randn(T, M)).astype(np.float32)
    d = glm.Design(np.stack([x, np.ones(T)], axis=1), ['x', 'constant'], ['x'])
    res = glm.first_level_host(y, d, betas=True)
    assert res.effect.shape == (1, 1, M) and res.effect.dtype == np.float64 and res.dof.tolist() == [T - 2] and res.groups == [0]
    for m in range(M):
        lr = sps.linregress(x, y[:, m].astype(np.float64))
        assert abs(res.effect[0, 0, m] - lr.slope) <= 1e-12 * abs(lr.slope)
        assert abs(res.variance[0, 0, m] - lr.stderr ** 2) <= 1e-12 * lr.stderr ** 2
        assert abs(res.t[0, 0, m] - lr.slope / lr.stderr) <= 1e-11 * abs(lr.slope / lr.stderr)
        assert abs(res.betas[0][1, m] - lr.intercept) <= 1e-12 * abs(lr.intercept)


def _two_runs():
    rng = np.random.RandomState(2)
    runs, designs = [], []
    for T in (70, 45):
        names = (['rest'] * 5 + ['a'] * 6 + ['rest'] * 4 + ['b'] * 6) * 4
        d = glm.design_matrix(names=names[:T], tr=TR, high_pass=0.02)
        runs.append((100.0 + d.X[:, :2] @ rng.randn(2, 6) + rng.randn(T, 6)).astype(np.float32))
        designs.append(d)
    return runs, designs


def test_fixed_effects_over_runs_of_unequal_length():
    runs, designs = _two_runs()
    both = glm.first_level_host(runs, designs, groups=['s', 's'])
    each = glm.first_level_host(runs, designs, groups=['p', 'q'])
    assert both.groups == ['s'] and each.groups == ['p', 'q']
    assert np.allclose(both.effect[0], (each.effect[0] + each.effect[1]) / 2, rtol=1e-14, atol=0)
    assert np.allclose(both.variance[0], (each.variance[0] + each.variance[1]) / 4, rtol=1e-14, atol=0)
    assert both.dof.tolist() == [int(each.dof.sum())] and each.dof.tolist() == [70 - 5, 45 - 4]
    assert np.allclose(both.t, both.effect / np.sqrt(both.variance), rtol=1e-14, atol=0)
    default = glm.first_level_host(runs, designs)
    assert default.groups == [0] and np.array_equal(default.effect, both.effect)


def test_rank_deficient_design_equals_the_design_without_the_duplicate():
    rng = np.random.RandomState(3)
    names = (['rest'] * 5 + ['a'] * 6 + ['rest'] * 4 + ['b'] * 6) * 3
    conf = rng.randn(len(names), 2)
    full = glm.design_matrix(names=names, tr=TR, confounds=conf[:, [0, 1, 0]])
    lean = glm.design_matrix(names=names, tr=TR, confounds=conf)
    y = (50.0 + rng.randn(len(names), 4)).astype(np.float32)
    cf, cl = glm.contrasts_one_vs_rest(full), glm.contrasts_one_vs_rest(lean)
    a, b = glm.first_level_host(y, full, cf), glm.first_level_host(y, lean, cl)
    assert a.dof.tolist() == b.dof.tolist() == [len(names) - len(lean.columns)]
    for u, v in ((a.effect, b.effect), (a.variance, b.variance), (a.t, b.t)):
        assert np.allclose(u, v, rtol=1e-9, atol=0)


def test_first_level_refuses_before_the_device():
    rng = np.random.RandomState(4)
    names = (['rest'] * 5 + ['a'] * 6 + ['rest'] * 4 + ['b'] * 6) * 3
    d = glm.design_matrix(names=names, tr=TR)
    T, P = d.X.shape
    y = rng.randn(T, 3).astype(np.float32)
    dup = glm.design_matrix(names=names, tr=TR, confounds=np.stack([d.X[:, 0], d.X[:, 0]], axis=1))
    alone = np.zeros((1, len(dup.columns)))
    alone[0, 0] = 1.0                                          # condition a alone is confounded with its copies
    short = glm.Design(rng.randn(4, 4), list('wxyz'), ['w'])
    bad = y.copy()
    bad[3, 1] = np.inf
    for fn in (glm.first_level_host, glm.first_level):
        for args, what in [((y, dup, alone), 'not estimable'), ((rng.randn(4, 3), short), 'degrees of freedom'),
                           ((y[:-1], d), 'rows'), (([y, y[:, :2]], [d, d]), 'vertices'), (([y, y], [d]), 'one Design per run'),
                           ((y, d, np.zeros((1, P))), 'not estimable'), ((y, d, np.ones((1, P + 1))), 'contrasts'),
                           ((bad, d), 'non-finite'), ((y[0], d), r'\[T, M\]'), (([], []), 'no runs')]:
            with pytest.raises(ValueError, match=what):
                fn(*args)
        with pytest.raises(ValueError, match='groups'):
            fn([y, y], [d, d], groups=['a'])
    # the duplicates do not hurt a contrast that stays in the row space: the SUM of the three copies' coefficients against b
    inside = np.array([[1.0 if n in ('a', 'confound_0', 'confound_1') else -1.0 if n == 'b' else 0.0 for n in dup.columns]])
    assert np.isfinite(glm.first_level_host(y, dup, inside).t).all()
    wide = glm.Design(np.concatenate([rng.randn(200, glm.PMAX), np.ones((200, 1))], axis=1), ['c%d' % i for i in range(glm.PMAX)] + ['constant'],
                      ['c0', 'c1'])
    with pytest.raises(ValueError, match='served'):
        glm.first_level(rng.randn(200, 3), wide)
    many = np.eye(glm.CMAX + 1, P)
    with pytest.raises(ValueError, match='served'):
        glm.first_level(y, d, many)
    with pytest.raises(ValueError, match='batch_runs'):
        glm.first_level(y, d, batch_runs=0)


def test_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_glm_query(i) for i in range(9)]
    assert all(v > 0 for v in q) and L.chebgcn_glm_query(9) == -1 and L.chebgcn_glm_query(-1) == -1
    VB, PANEL, KMAX, CMAX, SPLIT, SLICE, NW, PMAX, RMAX = q
    assert KMAX >= 64 and CMAX >= 32 and SPLIT >= SLICE and PANEL <= KMAX
    assert (KMAX, CMAX, PMAX, RMAX) == (glm.KMAX, glm.CMAX, glm.PMAX, glm.RMAX)
    assert L.chebgcn_glm_workspace(3, 33, 5) == 3 * 6 * 64 * 8
    for bad in [(0, 33, 5), (3, 0, 5), (3, 33, 0), (3, 33, KMAX + 1), (RMAX + 1, 33, 5), (-1, 33, 5)]:
        assert L.chebgcn_glm_workspace(*bad) == 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    EINVAL, EUNSUP = -1, -4

    def project(series=p, Ttot=4, offs=p, R=1, M=1, Q=p, k=1, a=p, yy=p):
        return L.chebgcn_glm_project(series, Ttot, offs, R, M, Q, k, a, yy, None)

    for kw in [dict(series=None), dict(offs=None), dict(Q=None), dict(a=None), dict(yy=None), dict(Ttot=0), dict(R=0), dict(R=-2),
               dict(M=0), dict(k=0), dict(k=-1), dict(Q=odd), dict(a=odd), dict(offs=odd), dict(series=odd)]:
        assert project(**kw) == EINVAL, kw
        assert b'glm_project' in L.chebgcn_last_error()
    for kw in [dict(k=KMAX + 1), dict(R=RMAX + 1), dict(Ttot=1 << 40)]:
        assert project(**kw) == EUNSUP, kw

    def finish(a=p, yy=p, offs=p, Ttot=4, rank=p, U=p, un2=p, B=None, R=1, M=1, k=1, C=1, P=0, e64=p, v64=p, e=None, v=None, t=None,
               beta=None):
        return L.chebgcn_glm_finish(a, yy, offs, Ttot, rank, U, un2, B, R, M, k, C, P, e64, v64, e, v, t, beta, None)

    for kw in [dict(a=None), dict(yy=None), dict(offs=None), dict(rank=None), dict(U=None), dict(un2=None), dict(e64=None, v64=None),
               dict(v64=None), dict(e=p), dict(e=p, v=p), dict(beta=p, P=1), dict(B=p, P=1), dict(B=p, beta=p, P=0), dict(Ttot=0),
               dict(R=0), dict(M=0), dict(k=0), dict(C=0), dict(P=-1), dict(U=odd), dict(e64=odd)]:
        assert finish(**kw) == EINVAL, kw
        assert b'glm_finish' in L.chebgcn_last_error()
    for kw in [dict(k=KMAX + 1), dict(C=CMAX + 1), dict(P=PMAX + 1, B=p, beta=p), dict(R=RMAX + 1)]:
        assert finish(**kw) == EUNSUP, kw

    def combine(e64=p, v64=p, gp=p, gr=p, n=1, R=1, S=1, C=1, M=1, e=p, v=p, t=p):
        return L.chebgcn_glm_combine(e64, v64, gp, gr, n, R, S, C, M, e, v, t, None)

    for kw in [dict(e64=None), dict(v64=None), dict(gp=None), dict(gr=None), dict(e=None), dict(v=None), dict(t=None), dict(n=0),
               dict(R=0), dict(S=0), dict(C=0), dict(M=0), dict(e64=odd)]:
        assert combine(**kw) == EINVAL, kw
        assert b'glm_combine' in L.chebgcn_last_error()
    for kw in [dict(C=CMAX + 1), dict(S=65536)]:
        assert combine(**kw) == EUNSUP, kw
