"""``glm.first_level_host(noise='ar1')`` -- the explicit AR(1) generalised least squares the device is held against -- and what
can be said of the AR(1) entry points without a GPU: the sums algebra of the kernels (restated in float64 NumPy in
glm_ar1_common.py) against it, the null calibration that is the point of prewhitening, and the refusals."""
import ctypes

import numpy as np
import pytest

import glm_ar1_common as G
from gcn_fmri_decoding_amd import _lib, glm


@pytest.fixture(scope='module')
def geo():
    return G.geometry()


def test_rho_zero_is_ordinary_least_squares():
    rng = np.random.RandomState(1)
    d, c = G.random_design(rng, 70, 5, 3)
    y = G.series(rng, d, 11)
    ols = glm.first_level_host(y, d, c, betas=True)
    ar1 = glm.first_level_host(y, d, c, betas=True, noise='ar1', rho=0.0)
    assert isinstance(ar1, glm.GLMResultAR1) and ar1._fields == glm.GLMResult._fields + ('rho',) and len(ols) == 6
    for name in ('effect', 'variance', 't'):
        a, b = getattr(ar1, name), getattr(ols, name)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
    assert np.abs(ar1.betas[0] - ols.betas[0]).max() <= 1e-12 * np.abs(ols.betas[0]).max()
    assert np.array_equal(ar1.dof, ols.dof) and ar1.groups == ols.groups
    assert len(ar1.rho) == 1 and ar1.rho[0].shape == (11,) and not ar1.rho[0].any()


def test_the_sums_algebra_on_bold_scaled_series():
    """Mean 1e4, sd 50, T = 284, 22 regressors, true rho -0.5 .. 0.9: rss is 2.5e-5 of y.y, and the sums statement still meets
    the explicit GLS: to 1e-11 of the natural scales (T 2^-53 = 3e-14 of y.y with room for the conditioning of the design),
    and rho and the variance themselves to 2e-9 = T 2^-53 y.y / rss, the round-off of the cancellation."""
    rng = np.random.RandomState(5)
    T, M = 284, 12
    names = (['rest'] * 15 + ['a'] * 20 + ['rest'] * 16 + ['b'] * 20 + ['rest'] * 15 + ['c'] * 20 + ['rest'] * 16 + ['d'] * 20) * 2
    d = glm.design_matrix(names=names, tr=0.72, high_pass=0.01, confounds=rng.randn(T, 13))
    assert d.X.shape == (T, 22)
    true = np.linspace(-0.5, 0.9, M)
    noise = G.ar1_noise(rng, T, M, true) * np.sqrt(1.0 - true * true)
    y = (1e4 + 50.0 * noise + 30.0 * (d.X[:, :4] @ rng.randn(4, M))).astype(np.float32)
    for rho in (None, 0.4):
        ref = glm.first_level_host(y, d, betas=True, noise='ar1', rho=rho)
        st, _ = G.sums_statement(y, d, rho=rho)
        m = G.distances(st, ref, y, d, None, None, 0)
        print('bold rho=%r' % (rho,), m)
        assert max(m.values()) <= 1e-11, m
        assert np.abs(st.rho[0] - ref.rho[0]).max() <= 2e-9
        rel_v = np.abs(st.variance - ref.variance).max() / ref.variance.max()
        assert rel_v <= 2e-9, rel_v
    assert np.abs(ref.rho[0]).max() == 0.4 and np.corrcoef(glm.first_level_host(y, d, noise='ar1').rho[0], true)[0, 1] > 0.9


def test_the_sums_statement_on_the_inputs_of_the_device_cases(geo):
    """The figure behind EPS of the device tests: the float64 sums statement against the host restatement on every input the
    device tests use, in the units of the bound.  No input but the sinusoid has a vertex near the clamp."""
    top = {}
    cases = dict(G.device_cases(geo))
    cases['sinusoid'] = G.sinusoid(geo) + (None, None)
    for name, (runs, designs, contrasts, groups, rho) in cases.items():
        ref = glm.first_level_host(runs, designs, contrasts, groups, betas=True, noise='ar1', rho=rho)
        st, raws = G.sums_statement(runs, designs, contrasts, groups, rho)
        for key, val in G.distances(st, ref, runs, designs, contrasts, groups, 0).items():
            top[key] = max(top.get(key, 0.0), val)
        if name == 'sinusoid':
            assert raws[0][0] >= 0.995 and ref.rho[0][0] == glm.RHO_MAX == st.rho[0][0]
            assert np.abs(ref.rho[0][1:]).max() < G.RHO_FREE
        else:
            assert max(np.abs(r).max() for r in ref.rho) < G.RHO_FREE, name
    print('sums statement against the host restatement:', top)
    assert max(top.values()) <= G.MEASURED, top
    assert G.EPS == 4.0 * G.MEASURED


def test_null_calibration():
    """AR(1) noise, rho = 0.4, T = 284, the 22-column design with a 20-TR boxcar, no signal: the variance of the t values is 1
    with the true rho (within the sampling interval 1 +- 4 sqrt(2 / (n - 1))), above the interval under OLS, and in between
    with the estimated rho (the residual estimate is biased downward with 22 regressors: out of scope)."""
    rng = np.random.RandomState(2)
    T, n = 284, 200
    names = (['rest'] * 15 + ['a'] * 20 + ['rest'] * 16 + ['b'] * 20 + ['rest'] * 15 + ['c'] * 20 + ['rest'] * 16 + ['d'] * 20) * 2
    d = glm.design_matrix(names=names, tr=0.72, high_pass=0.01, confounds=rng.randn(T, 13))
    y = (100.0 + G.ar1_noise(rng, T, n, 0.4)).astype(np.float32)
    c = np.zeros((1, 22))
    c[0, 0] = 1.0
    half = 4.0 * np.sqrt(2.0 / (n - 1))
    v_true = glm.first_level_host(y, d, c, noise='ar1', rho=0.4).t[0, 0].var(ddof=1)
    v_ols = glm.first_level_host(y, d, c).t[0, 0].var(ddof=1)
    v_est = glm.first_level_host(y, d, c, noise='ar1').t[0, 0].var(ddof=1)
    print('variance of null t: true rho %.3f, estimated %.3f, OLS %.3f, interval 1 +- %.3f' % (v_true, v_est, v_ols, half))
    assert 1.0 - half <= v_true <= 1.0 + half
    assert v_ols > 1.0 + half
    assert v_est < v_ols


def test_a_duplicated_confound_gives_the_same_maps():
    rng = np.random.RandomState(3)
    T, M = 90, 7
    conf = rng.randn(T, 2)
    names = (['rest'] * 5 + ['a'] * 8 + ['rest'] * 4 + ['b'] * 8) * 4
    d1 = glm.design_matrix(names=names[:T], tr=0.72, confounds=conf)
    d2 = glm.design_matrix(names=names[:T], tr=0.72, confounds=np.concatenate([conf, conf[:, :1]], axis=1))
    y = G.series(rng, d1, M)
    for rho in (None, 0.35):
        a = glm.first_level_host(y, d1, noise='ar1', rho=rho)
        b = glm.first_level_host(y, d2, noise='ar1', rho=rho)
        assert np.array_equal(a.dof, b.dof)
        for name in ('effect', 'variance', 't'):
            u, v = getattr(a, name), getattr(b, name)
            assert np.abs(u - v).max() <= 1e-9 * np.abs(u).max(), (name, rho)
        assert np.abs(a.rho[0] - b.rho[0]).max() <= 1e-9
        st, _ = G.sums_statement(y, d2, rho=rho)
        assert np.abs(st.effect - a.effect).max() <= 1e-9 * np.abs(a.effect).max()
        assert np.abs(st.variance - a.variance).max() <= 1e-9 * np.abs(a.variance).max()


def test_arguments_are_refused():
    rng = np.random.RandomState(4)
    d, c = G.random_design(rng, 20, 3, 1)
    y = G.series(rng, d, 4)
    for f in (glm.first_level_host, glm.first_level):
        with pytest.raises(ValueError, match='rho'):
            f(y, d, c, rho=0.2)                                 # rho with the default 'ols'
        with pytest.raises(ValueError, match='rho'):
            f(y, d, c, noise='ols', rho=0.0)
        for bad in (1.0, -1.0, 1.5, float('nan'), float('inf'), 'x', True, [0.1]):
            with pytest.raises(ValueError, match='rho'):
                f(y, d, c, noise='ar1', rho=bad)
        for bad in ('ar2', 'AR1', None, 1):
            with pytest.raises(ValueError, match='noise'):
                f(y, d, c, noise=bad)


def test_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    KMAX, CMAX, PMAX, RMAX = (L.chebgcn_glm_query(i) for i in (2, 3, 7, 8))
    q = L.chebgcn_glm_ar1_query
    assert q(0) >= 1 and q(1) >= 1 and q(2) == -1 and q(-1) == -1 and q(100) == -1 and q(100 + KMAX + 1) == -1 and q(200) == -1
    for k in range(1, KMAX + 1):
        kb = q(100 + k)
        assert kb in (8, 16, 32, 64) and kb >= k and (kb == 8 or kb // 2 < k) and q(200 + k) == q(0) * (64 // kb)
    ws = L.chebgcn_glm_ar1_workspace
    assert ws(3, 33, 5) == 3 * (2 * 5 + 2) * 64 * 8 and ws(3, 33, 5) > L.chebgcn_glm_workspace(3, 33, 5)
    for bad in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, KMAX + 1), (RMAX + 1, 1, 1), (1, 2 ** 31 - 1, 1)]:
        assert ws(*bad) == 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    byte = ctypes.c_void_p(p.value + 2)
    EINVAL, EUNSUP = -1, -4

    def project(series=p, Ttot=4, offs=p, R=1, M=1, W=p, k=1, ah=p, s0=p, s1=p):
        return L.chebgcn_glm_project_ar1(series, Ttot, offs, R, M, W, k, ah, s0, s1, None)

    for kw in [dict(series=None), dict(offs=None), dict(W=None), dict(ah=None), dict(s0=None), dict(s1=None), dict(Ttot=0), dict(R=0),
               dict(R=-2), dict(M=0), dict(k=0), dict(k=-1), dict(W=odd), dict(ah=odd), dict(s1=odd), dict(offs=odd), dict(series=odd)]:
        assert project(**kw) == EINVAL, kw
        assert b'glm_project_ar1' in L.chebgcn_last_error()
    for kw in [dict(k=KMAX + 1), dict(R=RMAX + 1), dict(Ttot=1 << 40)]:
        assert project(**kw) == EUNSUP, kw

    def finish(ah=p, s0=p, s1=p, series=p, W=p, offs=p, Ttot=4, rank=p, D=p, E=p, U=p, B=None, R=1, M=1, k=1, C=1, P=0, given=0, rho=0.0,
               e64=p, v64=p, e=None, v=None, t=None, beta=None, rho_out=p):
        return L.chebgcn_glm_finish_ar1(ah, s0, s1, series, W, offs, Ttot, rank, D, E, U, B, R, M, k, C, P, given, rho, e64, v64, e, v, t,
                                        beta, rho_out, None)

    for kw in [dict(ah=None), dict(s0=None), dict(s1=None), dict(series=None), dict(W=None), dict(offs=None), dict(rank=None), dict(D=None),
               dict(E=None), dict(U=None), dict(rho_out=None), dict(e64=None, v64=None), dict(v64=None), dict(e=p), dict(e=p, v=p),
               dict(beta=p, P=1), dict(B=p, P=1), dict(B=p, beta=p, P=0), dict(Ttot=0), dict(R=0), dict(M=0), dict(k=0), dict(C=0),
               dict(P=-1), dict(U=odd), dict(D=odd), dict(e64=odd), dict(series=byte), dict(rho_out=byte), dict(given=2), dict(given=-1),
               dict(given=1, rho=1.0), dict(given=1, rho=-1.0), dict(given=1, rho=2.5), dict(given=1, rho=float('nan'))]:
        assert finish(**kw) == EINVAL, kw
        assert b'glm_finish_ar1' in L.chebgcn_last_error()
    for kw in [dict(k=KMAX + 1), dict(C=CMAX + 1), dict(P=PMAX + 1, B=p, beta=p), dict(R=RMAX + 1), dict(Ttot=1 << 40)]:
        assert finish(**kw) == EUNSUP, kw
    assert glm.RHO_MAX == 0.99
