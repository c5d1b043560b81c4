"""Tangent-space connectivity on the host: ``tangent_host`` and ``geometric_mean_host`` (NumPy float64, ``numpy.linalg.eigh`` and
``@``) against the properties that define a geometric mean, every refusal of ``tangent`` / ``tangent_host`` / ``eigh``, and the
argument checks and ``query`` values of every C entry of the family -- none of it needs a GPU.
"""
import ctypes

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, connectome as cn
from test_connectome_host import latent


def spd(R, seed, cond=50.0):
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.randn(R, R))[0]
    A = (Q * np.exp(rng.uniform(0.0, np.log(cond), R))) @ Q.T
    return (A + A.T) / 2


def test_commuting_matrices_give_exp_mean_log():
    rng = np.random.RandomState(0)
    d = [np.exp(rng.uniform(-2, 2, 6)) for _ in range(5)]
    G, it, norms, steps, ok = cn.geometric_mean_host([np.diag(v) for v in d], tol=1e-14)
    assert ok and it <= 5 and np.abs(G - np.diag(np.exp(np.mean(np.log(d), axis=0)))).max() <= 1e-12
    assert len(norms) == len(steps) == it and (steps == 1.0).all()


def test_a_matrix_and_its_inverse_give_the_identity():
    A = spd(7, seed=1)
    G, _, _, _, ok = cn.geometric_mean_host([A, np.linalg.inv(A)], tol=1e-14)
    assert ok and np.abs(G - np.eye(7)).max() <= 1e-10


def test_congruence_invariance():
    mats = [spd(6, seed=s) for s in range(4)]
    P = np.random.RandomState(9).randn(6, 6) + 2 * np.eye(6)
    G = cn.geometric_mean_host(mats, tol=1e-13)[0]
    GP = cn.geometric_mean_host([P @ m @ P.T for m in mats], tol=1e-13)[0]
    ref = P @ G @ P.T
    assert np.abs(GP - ref).max() <= 1e-9 * np.abs(ref).max()


def test_the_mean_of_the_tangent_matrices_vanishes_at_convergence():
    runs = [latent(T, 12, seed=T) for T in (60, 45, 80, 52)]
    t = cn.tangent_host(runs)
    assert t.converged and t.iterations == len(t.norms) == len(t.steps) and t.norms[-1] < 1e-7
    assert t.matrices.dtype == np.float32 and t.matrices.shape == (4, 12, 12) and t.mean.dtype == t.whitening.dtype == np.float32
    assert t.reference.dtype == np.float64 and np.array_equal(t.reference.astype(np.float32), t.mean)
    for m in t.matrices:
        assert np.array_equal(m, m.T)
    W = cn._sym_fun_host(t.reference, lambda w: 1 / np.sqrt(w))
    assert np.abs(W @ t.reference @ W - np.eye(12)).max() <= 1e-12 and np.array_equal(W.astype(np.float32), t.whitening)
    logs = [cn._sym_fun_host(cn._congruence_host(W, cn.host_run(x, 'covariance', -1.0)[0]), np.log) for x in runs]
    M = np.mean(logs, axis=0)
    # one more step moved G by less than the step before: the norm at the final G is below the last one recorded
    assert np.sqrt((M * M).sum()) / 12 ** 2 < 1e-7
    assert t.sweeps == 0 and t.eig_converged and not t.degenerate.any()
    assert np.allclose(t.shrinkage, cn.connectome_host(runs, 'covariance').shrinkage, rtol=0, atol=0)


def test_a_single_run_is_its_own_mean():
    x = latent(30, 5, seed=3)
    t = cn.tangent_host(x)
    sigma = cn.host_run(x, 'covariance', -1.0)[0]
    assert t.iterations == 1 and t.converged and np.abs(t.reference - sigma).max() <= 1e-13 * np.abs(sigma).max()
    assert np.abs(t.matrices).max() <= 1e-6           # (float32 of a float64 round-off)
    every = cn.tangent_host(x, tol=0, max_iter=3)
    assert every.iterations == 3 and not every.converged


def test_reference_maps_runs_onto_a_fitted_mean():
    runs = [latent(T, 9, seed=T) for T in (40, 50, 64)]
    t = cn.tangent_host(runs)
    again = cn.tangent_host(runs, reference=t.reference)
    assert np.array_equal(again.matrices, t.matrices) and again.iterations == 0 and again.converged and len(again.norms) == 0
    assert np.array_equal(again.reference, t.reference) and np.array_equal(again.whitening, t.whitening)
    alone = cn.tangent_host(runs[1], reference=t.reference)
    assert np.array_equal(alone.matrices[0], t.matrices[1])
    held_out = cn.tangent_host(latent(33, 9, seed=99), reference=t.reference)
    assert np.isfinite(held_out.matrices).all() and np.abs(held_out.matrices).max() > 1e-3


def test_a_constant_run_is_flagged_and_left_out():
    runs = [latent(40, 8, seed=1), np.full((25, 8), 2.5, np.float32), latent(50, 8, seed=2)]
    t = cn.tangent_host(runs)
    assert t.degenerate.tolist() == [False, True, False] and not t.matrices[1].any() and np.isfinite(t.matrices).all()
    rest = cn.tangent_host([runs[0], runs[2]])
    assert np.array_equal(rest.reference, t.reference) and np.array_equal(rest.matrices, t.matrices[[0, 2]])
    wide = cn.tangent_host(latent(6, 10, seed=3), shrinkage=0.0)       # T <= R without shrinkage
    assert wide.degenerate.tolist() == [True] and not wide.matrices.any() and not wide.converged and wide.iterations == 0
    assert np.array_equal(wide.mean, np.eye(10, dtype=np.float32)) and np.array_equal(wide.whitening, np.eye(10, dtype=np.float32))
    assert cn.degenerate_floor(10) == 40 * 2.0 ** -53


def test_against_nilearn():
    connectome = pytest.importorskip('nilearn.connectome')
    runs = [latent(T, 10, seed=T) for T in (60, 70, 80)]
    measure = connectome.ConnectivityMeasure(kind='tangent')
    ref = measure.fit_transform([r.astype(np.float64) for r in runs])
    t = cn.tangent_host(runs)
    assert np.abs(t.reference - measure.mean_).max() <= 1e-8 * np.abs(measure.mean_).max()
    assert np.abs(t.matrices - ref).max() <= 1e-6


def test_refusals_come_before_the_device():
    x = latent(20, 6, seed=0)
    good = cn.tangent_host(x).reference
    nan = x.copy()
    nan[3, 2] = np.nan
    lopsided = good.copy()
    lopsided[0, 1] += 1e-3
    for call in (cn.tangent, cn.tangent_host):
        for kw, match in [(dict(shrinkage=1.5), 'outside'), (dict(shrinkage='lw'), 'shrinkage'), (dict(shrinkage=None), 'shrinkage'),
                          (dict(max_iter=0), 'max_iter'), (dict(max_iter=2.5), 'max_iter'), (dict(max_iter=True), 'max_iter'),
                          (dict(tol=-1e-9), 'tol'), (dict(tol=float('nan')), 'tol'), (dict(tol=float('inf')), 'tol'),
                          (dict(tol=None), 'tol'), (dict(tol='x'), 'tol'),
                          (dict(reference=np.eye(5)), 'reference'), (dict(reference=-np.eye(6)), 'positive definite'),
                          (dict(reference=lopsided), 'symmetric'), (dict(reference=np.full((6, 6), np.nan)), 'finite'),
                          (dict(reference=np.zeros((6, 6))), 'positive definite'), (dict(reference='G'), 'reference')]:
            with pytest.raises(ValueError, match=match):
                call(x, **kw)
        for runs, match in [(x[:1], 'two time points'), ([x, x[:, :5]], 'differ'), (nan, 'non-finite'), ([], 'no runs'),
                            (np.zeros(5, np.float32), r'\[T, M\]')]:
            with pytest.raises(ValueError, match=match):
                call(runs)
    limit = _lib.lib().chebgcn_connectome_query(0)
    with pytest.raises(ValueError, match='at most %d' % limit):
        cn.tangent(np.zeros((4, limit + 1), np.float32))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='batch_runs'):
            cn.tangent(x, batch_runs=bad)
    for bad, match in [(np.eye(3), 'float64'), (np.zeros((2, 3, 4)), 'float64'), (np.zeros((1, 3, 3), np.float32), 'float64'),
                       (np.zeros((1, 513, 513)), 'at most 512'), (np.full((1, 2, 2), np.nan), 'symmetric'),
                       (np.array([[[1.0, 2.0], [3.0, 1.0]]]), 'symmetric')]:
        with pytest.raises(ValueError, match=match):
            cn.eigh(bad)
    # the pinned refusals of the connectome kinds now point here
    with pytest.raises(ValueError, match='connectome.tangent'):
        cn.connectome_host(x, kind='tangent')


def test_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    q = [L.chebgcn_tangent_query(i) for i in range(8)]
    assert q == [512, 65535, 8, 256, 40, 64, 16, 10] and L.chebgcn_tangent_query(8) == -1 and L.chebgcn_tangent_query(-1) == -1
    RMAX, SMAX = q[0], q[1]
    assert L.chebgcn_connectome_query(8) == -1 and _lib.CONNECTOME_KINDS == ('covariance', 'correlation', 'precision',
                                                                            'partial correlation')
    assert _lib.SYM_FUNCTIONS == ('log', 'exp', 'sqrt', 'rsqrt')
    assert L.chebgcn_tangent_workspace(3, 33) == (3 * 33 * 33 + 3) * 8 + (3 * 3 + 2) * 4
    for bad in [(0, 33), (3, 0), (-1, 33), (3, RMAX + 1), (SMAX + 1, 33)]:
        assert L.chebgcn_tangent_workspace(*bad) == 0
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)
    p2 = ctypes.c_void_p(p.value + 8192)
    p3 = ctypes.c_void_p(p.value + 16384)
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    EINVAL, EUNSUP = -1, -4
    big = 1 << 40

    def sigma(ws=p, nbytes=big, offs=p, Ttot=4, S=1, R=1, shrinkage=-1.0, out=p, so=p):
        return L.chebgcn_connectome_sigma(ws, nbytes, offs, Ttot, S, R, shrinkage, out, so, None)

    for kw in [dict(ws=None), dict(offs=None), dict(out=None), dict(so=None), dict(Ttot=0), dict(S=0), dict(R=0), dict(shrinkage=1.5),
               dict(shrinkage=float('nan')), dict(nbytes=8), dict(ws=ctypes.c_void_p(p.value + 8)), dict(so=odd4), dict(offs=odd4),
               dict(out=odd4)]:
        assert sigma(**kw) == EINVAL, kw
        assert b'connectome_sigma' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=SMAX + 1)]:
        assert sigma(**kw) == EUNSUP, kw

    def eigh(A=p, S=1, R=1, w=p2, Vt=p3, sw=p2, cv=p2, ws=p2, nbytes=big):
        return L.chebgcn_sym_eigh(A, S, R, w, Vt, sw, cv, ws, nbytes, None)

    for kw in [dict(A=None), dict(w=None), dict(Vt=None), dict(sw=None), dict(cv=None), dict(ws=None), dict(S=0), dict(R=0), dict(R=-2),
               dict(nbytes=8), dict(A=odd4), dict(w=odd4), dict(Vt=odd4), dict(ws=odd4), dict(sw=odd2), dict(cv=odd2), dict(Vt=p)]:
        assert eigh(**kw) == EINVAL, kw
        assert b'sym_eigh' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=SMAX + 1)]:
        assert eigh(**kw) == EUNSUP, kw

    def function(w=p, Vt=p, S=1, R=1, func=0, a=1.0, out=p2, f32=0, flags=p3, fvals=p3):
        return L.chebgcn_sym_function(w, Vt, S, R, func, a, out, f32, flags, fvals, None)

    for kw in [dict(w=None), dict(Vt=None), dict(out=None), dict(flags=None), dict(fvals=None), dict(S=0), dict(R=0), dict(func=-1),
               dict(func=4), dict(a=float('nan')), dict(a=float('inf')), dict(f32=2), dict(w=odd4), dict(Vt=odd4), dict(out=odd4),
               dict(fvals=odd4), dict(flags=odd2), dict(out=odd2, f32=1)]:
        assert function(**kw) == EINVAL, kw
        assert b'sym_function' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=SMAX + 1)]:
        assert function(**kw) == EUNSUP, kw

    def congruence(W=p, A=p, S=1, R=1, out=p2, scratch=p3):
        return L.chebgcn_sym_congruence(W, A, S, R, out, scratch, None)

    for kw in [dict(W=None), dict(A=None), dict(out=None), dict(scratch=None), dict(S=0), dict(R=0), dict(W=odd4), dict(A=odd4),
               dict(out=odd4), dict(scratch=odd4), dict(scratch=p), dict(scratch=p2)]:
        assert congruence(**kw) == EINVAL, kw
        assert b'sym_congruence' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=SMAX + 1)]:
        assert congruence(**kw) == EUNSUP, kw

    def mean(m=p, flags=p, S=1, R=1, first=1, n=1, acc=p2, out=p3, norm=p3):
        return L.chebgcn_sym_mean(m, flags, S, R, first, n, acc, out, norm, None)

    for kw in [dict(m=None), dict(flags=None), dict(acc=None), dict(out=None), dict(norm=None), dict(S=0), dict(R=0), dict(first=2),
               dict(n=-1), dict(m=odd4), dict(acc=odd4), dict(out=odd4), dict(norm=odd4), dict(flags=odd2)]:
        assert mean(**kw) == EINVAL, kw
        assert b'sym_mean' in L.chebgcn_last_error()
    for kw in [dict(R=RMAX + 1), dict(S=(1 << 24) + 1)]:
        assert mean(**kw) == EUNSUP, kw
