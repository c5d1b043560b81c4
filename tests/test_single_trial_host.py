"""Host side of the single-trial (least squares - separate) estimator: ``glm.trial_design``, ``glm.single_trial_host``, the
closed form the kernels use restated in NumPy against the explicit per-trial fit, every ``ValueError`` of ``single_trial``, and
the argument checks of ``chebgcn_glm_trials``, which return before any launch: no GPU."""
import ctypes
import os

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, glm

TR = 0.72
NAMES = (['rest'] * 4 + ['a'] * 3 + ['rest'] * 5 + ['b'] * 3 + ['rest'] * 6 + ['b'] * 3 + ['rest'] * 4 + ['a'] * 3) * 3
EVENTS = [(30.0, 2.0, 'b'), (4.0, 2.0, 'a'), (12.5, 3.0, 'b'), (21.0, 2.0, 'a'), (40.0, 2.5, 'c'), (50.0, 1.0, 'ignored')]
ALL = ('beta', 'variance', 't')


@pytest.mark.parametrize('how', ['names', 'events'])
def test_trial_columns_sum_to_the_condition_columns(how):
    rng = np.random.RandomState(0)
    if how == 'names':
        kw = dict(names=NAMES, tr=TR, high_pass=0.02, confounds=rng.randn(len(NAMES), 2))
        blocks = 12
    else:
        kw = dict(events=EVENTS, T=90, tr=TR, conditions=['a', 'b', 'c'], confounds=rng.randn(90, 3))
        blocks = 5
    td, d = glm.trial_design(**kw), glm.design_matrix(**kw)
    n, C = td.X.shape[1], len(d.conditions)
    assert n == blocks and td.conditions == d.conditions and td.trials.dtype == np.int64 and td.onsets.dtype == np.float64
    for c in range(C):
        assert np.abs(td.X[:, td.trials == c].sum(axis=1) - d.X[:, c]).max() <= 1e-12
    assert np.array_equal(td.nuisance, d.X[:, C:]) and td.columns[n:] == d.columns[C:] and len(td.columns) == n + td.nuisance.shape[1]
    assert (np.diff(td.onsets) >= 0).all()                     # in order of onset, whatever order the events came in
    if how == 'events':
        assert td.onsets.tolist() == [4.0, 12.5, 21.0, 30.0, 40.0] and td.trials.tolist() == [0, 1, 0, 1, 2]
        assert td.columns[:5] == ['a_0', 'b_0', 'a_1', 'b_1', 'c_0']
    else:
        assert td.onsets[0] == 4 * TR and [d.conditions[c] for c in td.trials[:4]] == ['a', 'b', 'b', 'a']
    with pytest.raises(ValueError, match='trial_design'):
        glm.trial_design(names=NAMES, events=EVENTS)


def bold(rng, td, M, gain=30.0):
    return (1e4 + 50.0 * rng.randn(td.X.shape[0], M) + gain * (td.X @ rng.randn(td.X.shape[1], M))).astype(np.float32)


def test_two_trials_pooled_is_the_two_column_model():
    """[x_1 | x_2 | N] and [x_2 | x_1 | N] are the same model: betas, variances and dof of ``first_level_host``."""
    rng = np.random.RandomState(1)
    td = glm.trial_design(events=[(5.0, 2.0, 'a'), (11.0, 2.0, 'b')], T=60, tr=TR, high_pass=0.03)
    y = bold(rng, td, 7)
    res = glm.single_trial_host(y, td, others='pooled', outputs=ALL)
    full = glm.Design(np.concatenate([td.X, td.nuisance], axis=1), td.columns, td.conditions)
    ref = glm.first_level_host(y, full, np.eye(2, full.X.shape[1]), betas=True)
    assert res.dof.tolist() == [ref.dof[0]] * 2
    for j in range(2):
        assert np.abs(res.beta[j] - ref.betas[0][j]).max() <= 1e-9 * np.abs(ref.betas[0][j]).max()
        assert (np.abs(res.variance[j] - ref.variance[0, j]) <= 1e-9 * ref.variance[0, j]).all()
        assert (np.abs(res.t[j] - ref.t[0, j]) <= 1e-9 * np.abs(ref.t[0, j])).all()


@pytest.mark.parametrize('others', ['condition', 'pooled'])
def test_a_single_trial_run_is_the_one_column_model(others):
    rng = np.random.RandomState(2)
    td = glm.trial_design(events=[(5.0, 2.0, 'a')], T=50, tr=TR, conditions=['a', 'b'], high_pass=0.03)
    y = bold(rng, td, 5)
    res = glm.single_trial_host(y, td, others=others, outputs=ALL)
    one = glm.Design(np.concatenate([td.X, td.nuisance], axis=1), td.columns, ['a'])
    ref = glm.first_level_host(y, one, np.eye(1, one.X.shape[1]), betas=True)
    assert res.dof.tolist() == [ref.dof[0]] and res.beta.shape == (1, 5)
    assert np.abs(res.beta[0] - ref.betas[0][0]).max() <= 1e-9 * np.abs(ref.betas[0][0]).max()
    assert (np.abs(res.variance[0] - ref.variance[0, 0]) <= 1e-9 * ref.variance[0, 0]).all()


def closed_form(y, td, others):
    """The algebra of the kernels, restated: one set of projections of y, then a (1 + G)-sized epilogue per trial."""
    X, N = td.X, td.nuisance
    T, n = X.shape
    U, S, _ = np.linalg.svd(N, full_matrices=False)
    q = int((S > max(N.shape) * np.finfo(np.float64).eps * S[0]).sum())
    Qn = U[:, :q]
    own = td.trials if others == 'condition' else np.zeros(n, np.int64)
    G = len(td.conditions) if others == 'condition' else 1
    Sg = np.stack([X[:, own == g].sum(axis=1) for g in range(G)], axis=1)
    proj = lambda A: A - Qn @ (Qn.T @ A)
    ZX, ZS = proj(X), proj(Sg)
    yd = y.astype(np.float64)
    an, c, p, yy = Qn.T @ yd, ZS.T @ yd, ZX.T @ yd, (yd * yd).sum(axis=0)
    beta, var, dof = np.empty((n, y.shape[1])), np.empty((n, y.shape[1])), np.empty(n, np.int64)
    for j in range(n):
        mine = (np.arange(G) == own[j]).astype(np.float64)
        D = np.concatenate([ZX[:, j:j + 1], ZS - np.outer(ZX[:, j], mine)], axis=1)
        D[:, 1:][:, ~(Sg - np.outer(X[:, j], mine)).any(axis=0)] = 0.0       # an others column that is identically zero
        H = D.T @ D
        Hp = np.linalg.pinv(H, hermitian=True)
        r = np.linalg.matrix_rank(H, hermitian=True)
        d = np.concatenate([p[j:j + 1], c - np.outer(np.arange(G) == own[j], p[j])])
        beta[j] = Hp[0] @ d
        rss = yy - (an * an).sum(axis=0) - np.einsum('lm,lk,km->m', d, Hp, d)
        dof[j] = T - q - r
        var[j] = rss / dof[j] * Hp[0, 0]
    return beta, var, dof


@pytest.mark.parametrize('others', ['condition', 'pooled'])
def test_the_closed_form_agrees_with_the_explicit_fit_on_bold_scaled_data(others):
    """Mean 1e4, sd 50; condition c has ONE trial, whose model drops the empty column: its dof is one higher."""
    rng = np.random.RandomState(3)
    T = 140
    ev = [(3.0 + 7.5 * i + rng.rand(), 2.0, 'ab'[i % 2]) for i in range(12)] + [(47.0, 2.0, 'c')]
    td = glm.trial_design(events=ev, T=T, tr=TR, high_pass=0.02, confounds=rng.randn(T, 5))
    y = bold(rng, td, 9)
    res = glm.single_trial_host(y, td, others=others, outputs=ALL)
    beta, var, dof = closed_form(y, td, others)
    assert np.array_equal(res.dof, dof)
    lone = int(np.flatnonzero(td.trials == 2)[0])
    assert res.dof[lone] == res.dof[lone - 1] + (1 if others == 'condition' else 0)
    assert np.abs(beta - res.beta).max() <= 1e-9 * np.abs(res.beta).max()
    assert (np.abs(var - res.variance) <= 1e-8 * res.variance).all() and (res.variance > 0).all()
    assert res.labels.tolist() == [td.conditions[c] for c in td.trials] and res.classes == ['a', 'b', 'c']
    assert np.array_equal(res.trial, np.arange(13)) and not res.run.any() and np.array_equal(res.onset, td.onsets)
    assert np.allclose(res.t, res.beta / np.sqrt(res.variance), rtol=1e-12)
    only = glm.single_trial_host(y, td, others=others, outputs='beta')
    assert only.variance is None and only.t is None and np.array_equal(only.beta, res.beta)


def test_folds_and_groups_follow_the_runs():
    rng = np.random.RandomState(4)
    tds = [glm.trial_design(events=[(4.0 + 8 * i, 2.0, 'ab'[(i + r) % 2]) for i in range(3 + r)], T=70, tr=TR) for r in range(4)]
    runs = [bold(rng, td, 3) for td in tds]
    res = glm.single_trial_host(runs, tds, groups=['s1', 's2', 's1', 's2'])
    assert res.run.tolist() == [0] * 3 + [1] * 4 + [2] * 5 + [3] * 6
    assert res.group == ['s1'] * 3 + ['s2'] * 4 + ['s1'] * 5 + ['s2'] * 6
    assert res.folds().tolist() == [0] * 3 + [0] * 4 + [1] * 5 + [1] * 6
    assert res.folds(within=False).tolist() == [0] * 3 + [1] * 4 + [0] * 5 + [1] * 6
    assert res.variance is None and res.beta.shape == res.t.shape == (18, 3)


@pytest.mark.parametrize('fn', [glm.single_trial_host, glm.single_trial])
def test_single_trial_refuses_before_the_device(fn):
    rng = np.random.RandomState(5)
    T = 60
    td = glm.trial_design(events=[(5.0, 2.0, 'a'), (15.0, 2.0, 'b'), (25.0, 2.0, 'a')], T=T, tr=TR)
    y = bold(rng, td, 4)
    with pytest.raises(ValueError, match='rows'):
        fn(y[:-1], td)
    empty = glm.trial_design(events=[(5.0, 2.0, 'z')], T=T, tr=TR, conditions=['a'])
    assert empty.X.shape == (T, 0)
    with pytest.raises(ValueError, match='run 1 has no trials'):
        fn([y, y], [td, empty._replace(conditions=td.conditions)])
    late = glm.trial_design(events=[(5.0, 2.0, 'a'), (15.0, 2.0, 'b'), (T * TR + 10.0, 2.0, 'a')], T=T, tr=TR)
    with pytest.raises(ValueError, match='trial 2 of run 1 is not estimable'):
        fn([y, y], [td, late])
    twice = td._replace(X=td.X[:, [1, 1]], trials=td.trials[:2], onsets=td.onsets[:2])      # a trial equal to the sum of its others
    with pytest.raises(ValueError, match='trial 0 of run 0 is not estimable'):
        fn(y, twice, others='pooled')
    short = glm.trial_design(events=[(0.5, 1.5, 'a'), (3.0, 1.5, 'b')], T=8, tr=TR, hrf=None, high_pass=None, confounds=rng.randn(8, 5))
    with pytest.raises(ValueError, match='run 0 has T = 8 rows and trial 0 a model of rank 8: no residual degrees of freedom'):
        fn(y[:8], short)
    with pytest.raises(ValueError, match='one TrialDesign per run'):
        fn([y, y], [td])
    with pytest.raises(ValueError, match='TrialDesign'):
        fn(y, glm.design_matrix(events=[(5.0, 2.0, 'a')], T=T, tr=TR))
    with pytest.raises(ValueError, match='others'):
        fn(y, td, others='all')
    with pytest.raises(ValueError, match='outputs'):
        fn(y, td, outputs=('beta', 'effect'))
    with pytest.raises(ValueError, match='groups'):
        fn(y, td, groups=['a', 'b'])
    with pytest.raises(ValueError, match='conditions'):
        fn([y, y], [td, td._replace(conditions=['a', 'c'])])
    bad = y.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        fn(bad, td)
    if fn is glm.single_trial:                                  # what the kernels serve
        many = [chr(ord('a') + i) for i in range(glm.G1MAX)]
        wide = glm.trial_design(events=[(2.0 + 2.5 * i, 1.0, c) for i, c in enumerate(many)], T=T, tr=TR)
        with pytest.raises(ValueError, match='conditions'):
            fn(y, wide)
        heavy = glm.trial_design(events=[(5.0, 2.0, 'a'), (15.0, 2.0, 'b')], T=80, tr=TR, high_pass=None, confounds=rng.randn(80, glm.KMAX - 2))
        with pytest.raises(ValueError, match='q \\+ G'):
            fn(rng.randn(80, 4), heavy)
        crowd = glm.TrialDesign(np.zeros((10, glm.NMAX + 1)), np.zeros(glm.NMAX + 1, np.int64), np.zeros(glm.NMAX + 1), np.ones((10, 1)),
                                [], ['a'])
        with pytest.raises(ValueError, match='trials; served'):
            fn(rng.randn(10, 4), crowd)
        with pytest.raises(ValueError, match='batch_runs'):
            fn(y, td, batch_runs=0)


def test_the_entry_point_is_declared_bound_and_checks_its_arguments_without_a_gpu():
    L = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'chebgcn.h')) as f:
        header = f.read()
    for name in ('chebgcn_glm_trials', 'chebgcn_glm_trials_query'):
        assert 'int %s(' % name in header and name in _lib.SIGNATURES and hasattr(L, name)
    q = [L.chebgcn_glm_trials_query(i) for i in range(6)]
    VB, PANEL, G1MAX, KMAX, NMAX, RMAX = q
    assert L.chebgcn_glm_trials_query(6) == -1 and L.chebgcn_glm_trials_query(-1) == -1
    assert (VB, PANEL) == (L.chebgcn_glm_query(0), L.chebgcn_glm_query(1))
    assert (G1MAX, KMAX, NMAX, RMAX) == (glm.G1MAX, glm.KMAX, glm.NMAX, glm.RMAX) and G1MAX == 16 and KMAX == 64 and NMAX >= 1024
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    EINVAL, EUNSUP = -1, -4

    def trials(series=p, Ttot=4, offs=p, R=1, M=1, Z=p, nmax=1, toffs=p, a=p, yy=p, k=2, qrank=p, own=p, rank=p, w=p, F=p, G1=2, N=1,
               beta=p, variance=None, t=None):
        return L.chebgcn_glm_trials(series, Ttot, offs, R, M, Z, nmax, toffs, a, yy, k, qrank, own, rank, w, F, G1, N, beta, variance, t,
                                    None)

    for kw in [dict(series=None), dict(offs=None), dict(Z=None), dict(toffs=None), dict(a=None), dict(yy=None), dict(qrank=None),
               dict(own=None), dict(rank=None), dict(w=None), dict(F=None), dict(beta=None), dict(Ttot=0), dict(R=0), dict(R=-3),
               dict(M=0), dict(nmax=0), dict(k=0), dict(G1=0), dict(N=0), dict(k=1, G1=3), dict(series=odd), dict(Z=odd), dict(w=odd),
               dict(beta=odd), dict(t=odd), dict(offs=odd)]:
        assert trials(**kw) == EINVAL, kw
        assert b'glm_trials' in L.chebgcn_last_error()
    for kw in [dict(G1=G1MAX + 1, k=G1MAX), dict(k=KMAX + 1), dict(nmax=NMAX + 1), dict(R=RMAX + 1), dict(Ttot=1 << 40), dict(N=1 << 40)]:
        assert trials(**kw) == EUNSUP, kw
