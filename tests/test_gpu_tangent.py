"""Tangent-space connectivity on the MI355X: every kernel of the chebgcn_sym_* family and ``connectome_sigma_kernel`` by name,
the solver alone against ``numpy.linalg.eigvalsh``, the products against float64 ``@``, ``tangent`` against ``tangent_host``
(NumPy ``eigh`` and ``@`` -- none of the device's algebra).

Bounds.  Solver: ``max|V^T V - I| <= 1e-11``, ``max|A - V L V^T| <= 1e-11 max|A|``, eigenvalues within ``1e-11 max|lambda|`` --
ten times the worst a NumPy model of the method measured on whitened covariances up to R = 512 (1.0e-12 / 1.2e-12 / 8e-13), the
device's chains running in other orders than NumPy's.  Products: ``2 R 2^-53 sum_p |a_ip| |b_pj|`` per product, from the
absolute-value matrices (the bound of a chain of R fused multiply-adds, doubled).  ``tangent``: ``2^-23 |ref| + 1e-10 s`` per
entry, the one float32 rounding plus 1e-10 of the natural scale (1 for the tangent matrices, ``sqrt(G_ii G_jj)`` for the mean,
``max|W|`` for the whitening): the bound of tests/test_gpu_connectome.py.  The norms of the iterations agree to 1e-6 relative,
plus 1e-13 absolute: a norm that is all round-off (one run: M = log(I + round-off), 1e-18 against the tolerance 1e-7) has no
relative accuracy on either side.  Every case asserts on the host trace that no ``norm / R^2`` lies within 1e-3 relative of
``tol`` and no two consecutive norms within 1e-6 of each other, so that neither the stop nor a halving can flip on round-off.

The matrices of the solver tests are the ones the method is for: a covariance whitened by the mean of two (``W Sigma W``,
eigenvalues around 1), its matrix logarithm less its mean eigenvalue (a tangent vector at the mean: traceless, eigenvalues of
both signs), and the structured cases.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_measured
from guarded_buffers import FILLS, Guarded, bits
from gcn_fmri_decoding_amd import _lib, connectome as cn, graph, models_gcn, ops, runs as _runs
from test_connectome_host import latent

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -53

EIGH_KERNELS = ('tangent_eigh_init_kernel + tangent_eigh_step_kernel + tangent_eigh_sweep_kernel + '
                'tangent_eigh_values_kernel')
FUNCTION_KERNELS = 'tangent_fvals_kernel + tangent_product_kernel<lower>'
CONGRUENCE_KERNELS = 'tangent_product_kernel<full> + tangent_product_kernel<lower>'
MEAN_KERNELS = 'tangent_mean_kernel'
MEAN_END_KERNELS = 'tangent_mean_kernel + tangent_norm_kernel'
COV_KERNELS = 'connectome_centre_kernel + connectome_rowsq_kernel + connectome_cov_kernel'

SOLVER_R = (1, 2, 7, 8, 9, 16, 17, 33, 64, 65, 130, 257, 360, 512)


def dev64(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(DEV)


def whitened(R, seed):
    """``W Sigma_1 W`` with ``W = ((Sigma_1 + Sigma_2) / 2)^-1/2`` of two latent-factor runs: symmetric, eigenvalues around 1."""
    T = 2 * R + 20
    s1, s2 = (cn.host_run(latent(T, R, seed=seed + k, mix=0.5), 'covariance', -1.0)[0] for k in (0, 1))
    W = cn._sym_fun_host((s1 + s2) / 2, lambda w: 1 / np.sqrt(w))
    return cn._congruence_host(W, s1)


def solver_cases(R):
    """name -> float64 [3, R, R]: three different matrices of every kind."""
    rng = np.random.RandomState(R)
    spd = np.stack([whitened(R, seed=10 * R + 2 * s) for s in range(3)])
    tangent_vectors = np.stack([cn._sym_fun_host(a, np.log) for a in spd])
    tangent_vectors = tangent_vectors - (np.trace(tangent_vectors, axis1=1, axis2=2) / R)[:, None, None] * np.eye(R)     # traceless
    Q = [np.linalg.qr(rng.randn(R, R))[0] for _ in range(3)]
    repeated = np.stack([(q * np.where(np.arange(R) % 3 == 0, 1.0, 2.0)) @ q.T for q in Q])
    repeated = (repeated + repeated.transpose(0, 2, 1)) / 2
    diagonal = np.stack([np.diag(rng.uniform(0.5, 2.0, R) * np.where(rng.rand(R) < 0.5, -1.0, 1.0)) for _ in range(3)])
    return {'whitened': spd, 'indefinite': tangent_vectors, 'identity': np.stack([np.eye(R)] * 3), 'repeated': repeated,
            'diagonal': diagonal, 'zero': np.zeros((3, R, R)), 'whitened*1e6': spd * 1e6, 'whitened*1e-6': spd * 1e-6,
            'indefinite*1e6': tangent_vectors * 1e6, 'indefinite*1e-6': tangent_vectors * 1e-6}


@pytest.mark.parametrize('R', SOLVER_R)
def test_solver_alone(R):
    worst = {'orthogonality': 0.0, 'reconstruction': 0.0, 'eigenvalues': 0.0, 'sweeps': 0}
    for name, A in solver_cases(R).items():
        if name == 'indefinite' and R > 1:
            ev = np.linalg.eigvalsh(A[0])
            assert ev[0] < 0 < ev[-1]
        _lib.dispatch_log = []
        try:
            w, V, sweeps = cn.eigh(A, device=DEV)
        finally:
            log, _lib.dispatch_log = _lib.dispatch_log, None
        assert [k for _, k in log] == [EIGH_KERNELS], log
        w, V = w.cpu().numpy(), V.cpu().numpy()
        assert w.shape == (3, R) and V.shape == (3, R, R) and sweeps.dtype == np.int32 and (np.diff(w, axis=1) >= 0).all()
        assert (sweeps >= 1).all() and (sweeps <= 40).all(), (name, sweeps)
        for s in range(3):
            scale, ref = np.abs(A[s]).max(), np.linalg.eigvalsh(A[s])
            orth = np.abs(V[s].T @ V[s] - np.eye(R)).max()
            recon = np.abs(A[s] - (V[s] * w[s]) @ V[s].T).max()
            eig = np.abs(w[s] - ref).max()
            print('R=%d %s[%d]: sweeps %d, orthogonality %.2e, reconstruction %.2e of max|A|, eigenvalues %.2e of max|l|' % (
                R, name, s, sweeps[s], orth, recon / max(scale, 1e-300), eig / max(np.abs(ref).max(), 1e-300)))
            assert orth <= 1e-11, (name, s, orth)
            assert recon <= 1e-11 * scale, (name, s, recon, scale)
            assert eig <= 1e-11 * np.abs(ref).max(), (name, s, eig)
            worst['orthogonality'] = max(worst['orthogonality'], orth / 1e-11)
            if scale > 0:
                worst['reconstruction'] = max(worst['reconstruction'], recon / (1e-11 * scale))
                worst['eigenvalues'] = max(worst['eigenvalues'], eig / (1e-11 * np.abs(ref).max()))
        worst['sweeps'] = max(worst['sweeps'], int(sweeps.max()))
        if name in ('identity', 'diagonal', 'zero'):
            assert (sweeps == 1).all(), (name, sweeps)              # nothing to rotate: one idle sweep
        alone = cn.eigh(A[1:2], device=DEV)                         # S = 1: the same bits as among others
        assert np.array_equal(bits(alone[0].cpu().numpy()[0]), bits(w[1])) and np.array_equal(bits(alone[1].cpu().numpy()[0]), bits(V[1]))
        assert alone[2][0] == sweeps[1]
    record_measured('tangent_solver[R%d]' % R, **worst)


def test_the_matrix_the_gram_of_the_columns_cannot_solve():
    """[[0, 1], [1, 0]]: its columns are orthogonal, its eigenvalues are +1 and -1."""
    w, V, sweeps = cn.eigh(np.array([[[0.0, 1.0], [1.0, 0.0]]]), device=DEV)
    assert np.abs(w.cpu().numpy()[0] - [-1.0, 1.0]).max() <= 1e-15 and sweeps[0] == 2
    V = V.cpu().numpy()[0]
    assert np.abs(np.abs(V) - np.sqrt(0.5)).max() <= 1e-15 and V[0, 0] * V[1, 0] < 0 < V[0, 1] * V[1, 1]


# ---------------------------------------------------------------------------------------------- products and mean

def random_sym(S, R, seed):
    a = np.random.RandomState(seed).randn(S, R, R)
    return (a + a.transpose(0, 2, 1)) / 2


@pytest.mark.parametrize('R', (1, 33, 64, 65, 130))
def test_sym_function_against_float64(R):
    rng = np.random.RandomState(R)
    S = 3
    Vt = rng.randn(S, R, R)
    w = rng.uniform(0.2, 3.0, (S, R))
    host = {'log': np.log, 'exp': np.exp, 'sqrt': np.sqrt, 'rsqrt': lambda x: 1 / np.sqrt(x)}
    for func, a in [('log', 1.0), ('exp', -0.5), ('sqrt', 2.0), ('rsqrt', 1.0), ('exp', 1.0)]:
        ww = w - 1.5 if func == 'exp' else w                        # (exp takes both signs)
        out, flags = ops.sym_function(dev64(ww), dev64(Vt), func, a=a)
        assert _lib.last_dispatch() == FUNCTION_KERNELS
        out32, _ = ops.sym_function(dev64(ww), dev64(Vt), func, a=a, float32=True)
        out, out32 = out.cpu().numpy(), out32.cpu().numpy()
        assert not flags.cpu().numpy().any() and out32.dtype == np.float32
        f = host[func](a * ww)
        ref = np.einsum('sp,spi,spj->sij', f, Vt, Vt)
        bound = 2 * R * EPS64 * np.einsum('sp,spi,spj->sij', np.abs(f), np.abs(Vt), np.abs(Vt))
        assert (np.abs(out - ref) <= bound).all(), (func, (np.abs(out - ref) / bound).max())
        assert np.array_equal(bits(out), bits(out.transpose(0, 2, 1))) and np.array_equal(out32, out.astype(np.float32))
    # an eigenvalue the function cannot take flags its matrix, which comes out as zeros; the others are untouched
    bad = w.copy()
    bad[1, R // 2] = -0.25
    for func in ('log', 'sqrt', 'rsqrt'):
        out, flags = ops.sym_function(dev64(bad), dev64(Vt), func)
        good, _ = ops.sym_function(dev64(w), dev64(Vt), func)
        out, good = out.cpu().numpy(), good.cpu().numpy()
        assert flags.cpu().numpy().tolist() == [0, 1, 0] and not out[1].any() and np.isfinite(out).all()
        assert np.array_equal(bits(out[[0, 2]]), bits(good[[0, 2]]))
    out, flags = ops.sym_function(dev64(np.where(bad < 0, np.nan, bad)), dev64(Vt), 'exp')
    assert flags.cpu().numpy().tolist() == [0, 1, 0] and not out.cpu().numpy()[1].any()


@pytest.mark.parametrize('R', (1, 33, 64, 65, 130))
def test_sym_congruence_against_float64(R):
    A = random_sym(3, R, seed=R)
    W = random_sym(1, R, seed=R + 1)[0]
    out = ops.sym_congruence(dev64(W), dev64(A)).cpu().numpy()
    assert _lib.last_dispatch() == CONGRUENCE_KERNELS
    ref = W @ A @ W
    bound = 2 * (2 * R * EPS64) * (np.abs(W) @ np.abs(A) @ np.abs(W))        # two chained products
    assert (np.abs(out - ref) <= bound).all(), (np.abs(out - ref) / bound).max()
    assert np.array_equal(bits(out), bits(out.transpose(0, 2, 1)))
    alone = ops.sym_congruence(dev64(W), dev64(A[2:])).cpu().numpy()
    assert np.array_equal(bits(alone[0]), bits(out[2]))


@pytest.mark.parametrize('R', (1, 33, 130))
def test_sym_mean_is_the_chain_in_ascending_order(R):
    S = 5
    A = random_sym(S, R, seed=R)
    flags = np.array([0, 1, 0, 0, 1], np.int32)
    acc = torch.empty((R, R), dtype=torch.float64, device=DEV)
    mean, norm = ops.sym_mean(dev64(A), torch.as_tensor(flags).to(DEV), acc, first=True, n_total=3)
    assert _lib.last_dispatch() == MEAN_END_KERNELS
    ref = ((A[0] + A[2]) + A[3]) / 3
    assert np.array_equal(bits(mean.cpu().numpy()), bits(ref))
    exact = np.sqrt((ref * ref).sum())
    terms = -(-R * R // 512) + 9 + 1                             # a thread's chain, the tree, the root
    assert abs(float(norm.cpu()[0]) - exact) <= terms * EPS64 * exact
    # in two calls: the chain runs on
    assert ops.sym_mean(dev64(A[:2]), torch.as_tensor(flags[:2]).to(DEV), acc, first=True, n_total=0) is None
    assert _lib.last_dispatch() == MEAN_KERNELS
    mean2, norm2 = ops.sym_mean(dev64(A[2:]), torch.as_tensor(flags[2:]).to(DEV), acc, first=False, n_total=3)
    assert np.array_equal(bits(mean2.cpu().numpy()), bits(ref)) and bits(norm2.cpu().numpy())[0] == bits(norm.cpu().numpy())[0]


# ---------------------------------------------------------------------------------------------- Sigma

def sigma_of(runs, shrinkage=-1.0):
    R = runs[0].shape[1]
    dev, planes = _runs.stage(runs, R, DEV, 'test')
    offs = torch.as_tensor(_runs.offsets(runs)).to(DEV)
    S = len(runs)
    sigma = torch.empty((S, R, R), dtype=torch.float64, device=DEV)
    shrunk = torch.empty((S,), dtype=torch.float64, device=DEV)
    ws = ops.connectome_cov(planes, offs, R)
    ops.connectome_sigma(ws, offs, int(planes.shape[0]), R, shrinkage, sigma, shrunk)
    assert _lib.last_dispatch() == 'connectome_sigma_kernel'
    return sigma.cpu().numpy(), shrunk.cpu().numpy()


@pytest.mark.parametrize('T,R', [(2, 1), (20, 5), (31, 65), (129, 129), (284, 360), (600, 512)])
def test_sigma_is_the_covariance_kind_before_its_rounding(T, R):
    runs = [latent(T, R, seed=T + R), latent(T + 3, R, seed=T + R + 1)]
    for shrinkage in ('auto', 0.3):
        sh = -1.0 if shrinkage == 'auto' else shrinkage
        sigma, shrunk = sigma_of(runs, sh)
        c = cn.connectome(runs, 'covariance', shrinkage, device=DEV)
        assert np.array_equal(bits(sigma.astype(np.float32)), bits(c.matrices.cpu().numpy()))
        assert np.array_equal(bits(shrunk), bits(c.shrinkage))
        for s, x in enumerate(runs):
            ref = cn.host_run(x, 'covariance', sh)[0]
            assert np.abs(sigma[s] - ref).max() <= 1e-12 * np.abs(ref).max()
            assert np.array_equal(bits(sigma[s]), bits(sigma[s].T))


# ---------------------------------------------------------------------------------------------- tangent against the host

def ratio(got, ref, scale):
    got = np.asarray(got, np.float64)
    return float((np.abs(got - ref) / (EPS32 * np.abs(ref) + 1e-10 * scale)).max())


def well_conditioned(h, tol):
    """The host trace stops and halves far from round-off."""
    n = h.norms
    assert all(abs(v - tol) > 1e-3 * tol for v in n) or tol == 0, n
    assert all(abs(a - b) > 1e-6 * max(a, b) for a, b in zip(n[:-1], n[1:])), n


def check_tangent(runs, what, **kw):
    tol = kw.get('tol', 1e-7)
    h = cn.tangent_host(runs, **kw)
    well_conditioned(h, tol)
    _lib.dispatch_log = []
    try:
        t = cn.tangent(runs, device=DEV, **kw)
    finally:
        log, _lib.dispatch_log = _lib.dispatch_log, None
    seen = {k for _, k in log}
    assert seen <= {COV_KERNELS, 'connectome_sigma_kernel', EIGH_KERNELS, FUNCTION_KERNELS, CONGRUENCE_KERNELS, MEAN_KERNELS,
                    MEAN_END_KERNELS}, seen
    assert {COV_KERNELS, 'connectome_sigma_kernel', EIGH_KERNELS, FUNCTION_KERNELS, CONGRUENCE_KERNELS} <= seen, seen
    m = t.matrices.cpu().numpy()
    assert m.dtype == np.float32 and np.isfinite(m).all() and np.array_equal(m, m.transpose(0, 2, 1))
    assert t.degenerate.tolist() == h.degenerate.tolist() and t.eig_converged and 1 <= t.sweeps <= 40
    assert np.abs(t.shrinkage - h.shrinkage).max() <= 1e-10
    assert t.iterations == h.iterations and t.converged == h.converged, (what, t.iterations, h.iterations, t.norms, h.norms)
    assert np.array_equal(t.steps, h.steps), (what, t.steps, h.steps)
    assert (np.abs(t.norms - h.norms) <= 1e-6 * h.norms + 1e-13).all(), (what, t.norms, h.norms)
    G = h.reference
    r = {'matrices': ratio(m, _host_matrices(runs, h, kw), 1.0),
         'mean': ratio(t.mean.cpu().numpy(), G, np.sqrt(np.outer(np.diag(G), np.diag(G)))),
         'whitening': ratio(t.whitening.cpu().numpy(), _host_whitening(G), np.abs(_host_whitening(G)).max()),
         'reference': float((np.abs(t.reference - G) / (1e-10 * np.sqrt(np.outer(np.diag(G), np.diag(G))))).max())}
    print('%s: iterations %d, sweeps %d, of the bound: %s' % (what, t.iterations, t.sweeps, r))
    assert max(r.values()) <= 1.0, (what, r)
    assert np.array_equal(t.reference.astype(np.float32), t.mean.cpu().numpy())
    return t, h, r


def _host_whitening(G):
    return cn._sym_fun_host(G, lambda w: 1 / np.sqrt(w))


def _host_matrices(runs, h, kw):
    """The tangent matrices of the host in float64 (``tangent_host`` returns them rounded)."""
    W = _host_whitening(h.reference)
    s = kw.get('shrinkage', 'auto')
    out = np.zeros(h.matrices.shape)
    for r, x in enumerate(runs):
        if not h.degenerate[r]:
            out[r] = cn._sym_fun_host(cn._congruence_host(W, cn.host_run(x, 'covariance', -1.0 if s == 'auto' else s)[0]), np.log)
    return out


SHAPES = [(1, 20, 5), (5, 40, 17), (4, 60, 24), (6, 100, 33), (4, 30, 40), (3, 284, 130), (2, 600, 360)]


@pytest.mark.parametrize('S,T,R', SHAPES, ids=['S%d-T%d-R%d' % s for s in SHAPES])
def test_tangent_against_the_host(S, T, R):
    runs = [latent(T, R, seed=100 * S + 10 * s + R) for s in range(S)]
    t, h, r = check_tangent(runs, 'S%d T%d R%d' % (S, T, R))
    assert t.converged
    record_measured('tangent[S%d-T%d-R%d]' % (S, T, R), iterations=t.iterations, sweeps=t.sweeps, **r)


def test_tangent_at_the_limit_with_every_iteration():
    runs = [latent(600, 512, seed=s, mix=0.3) for s in (1, 2)]
    t, h, r = check_tangent(runs, 'S2 T600 R512', max_iter=3, tol=0)
    assert t.iterations == 3 and not t.converged
    record_measured('tangent[S2-T600-R512]', sweeps=t.sweeps, **r)


@pytest.fixture(scope='module')
def mixed():
    return [latent(T, 24, seed=T) for T in (90, 40, 284, 33, 129, 64)]


def test_runs_of_mixed_length_in_one_call(mixed):
    check_tangent(mixed, 'mixed lengths')


def same(a, b):
    return all(np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())) for x, y in
               ((a.matrices, b.matrices), (a.mean, b.mean), (a.whitening, b.whitening))) and \
        np.array_equal(bits(a.reference), bits(b.reference)) and np.array_equal(bits(a.norms), bits(b.norms)) and \
        np.array_equal(bits(a.shrinkage), bits(b.shrinkage)) and np.array_equal(a.degenerate, b.degenerate)


def test_results_are_bit_identical(mixed):
    base = cn.tangent(mixed, device=DEV)
    for batch in (1, 2, len(mixed)):
        assert same(cn.tangent(mixed, device=DEV, batch_runs=batch), base), batch
    assert same(cn.tangent(mixed, device=DEV), base)
    for given in ([torch.as_tensor(x) for x in mixed], [torch.as_tensor(x).to(DEV) for x in mixed]):
        assert same(cn.tangent(given, device=DEV), base)
    m = base.matrices.cpu().numpy()
    # onto a fitted mean: the same bits as the fit, for a run alone or among others, in any order
    fitted = cn.tangent(mixed, reference=base.reference, device=DEV)
    assert np.array_equal(bits(fitted.matrices.cpu().numpy()), bits(m)) and fitted.iterations == 0 and fitted.converged
    assert np.array_equal(bits(fitted.whitening.cpu().numpy()), bits(base.whitening.cpu().numpy()))
    order = [4, 0, 5, 2, 1, 3]
    perm = cn.tangent([mixed[i] for i in order], reference=base.reference, device=DEV, batch_runs=4)
    assert np.array_equal(bits(perm.matrices.cpu().numpy()[np.argsort(order)]), bits(m))
    for r in (0, 3):
        alone = cn.tangent(mixed[r], reference=base.reference, device=DEV)
        assert np.array_equal(bits(alone.matrices.cpu().numpy()[0]), bits(m[r]))
    # without a reference the means sum in ascending run order: a permuted order gives the permuted result within the bound only
    free = cn.tangent([mixed[i] for i in order], device=DEV)
    assert free.iterations == base.iterations
    assert ratio(free.matrices.cpu().numpy()[np.argsort(order)], _host_matrices(mixed, cn.tangent_host(mixed), {}), 1.0) <= 1.0


def test_degenerate_runs_are_flagged_zero_and_left_out():
    R = 12
    good = [latent(T, R, seed=T) for T in (50, 64, 41)]
    flat = np.full((30, R), 7.5, np.float32)
    base = cn.tangent(good, device=DEV)
    t = cn.tangent([good[0], flat, good[1], good[2]], device=DEV)
    m = t.matrices.cpu().numpy()
    assert t.degenerate.tolist() == [False, True, False, False] and not m[1].any() and np.isfinite(m).all()
    assert np.array_equal(bits(m[[0, 2, 3]]), bits(base.matrices.cpu().numpy())) and np.array_equal(bits(t.reference), bits(base.reference))
    assert np.isfinite(t.mean.cpu().numpy()).all() and np.isfinite(t.whitening.cpu().numpy()).all() and np.isfinite(t.norms).all()
    # shrinkage 0 with T <= R: singular
    wide = latent(8, R, seed=3)
    base0 = cn.tangent(good, shrinkage=0.0, device=DEV)
    t0 = cn.tangent(good + [wide], shrinkage=0.0, device=DEV)
    h0 = cn.tangent_host(good + [wide], shrinkage=0.0)
    m0 = t0.matrices.cpu().numpy()
    assert t0.degenerate.tolist() == h0.degenerate.tolist() == [False, False, False, True] and not m0[3].any() and np.isfinite(m0).all()
    assert np.array_equal(bits(m0[:3]), bits(base0.matrices.cpu().numpy()))
    none = cn.tangent([flat, wide], shrinkage=0.0, device=DEV)
    assert none.degenerate.all() and not none.converged and none.iterations == 0 and not none.matrices.cpu().numpy().any()
    assert np.array_equal(none.mean.cpu().numpy(), np.eye(R, dtype=np.float32))
    assert np.array_equal(none.whitening.cpu().numpy(), np.eye(R, dtype=np.float32)) and np.array_equal(none.reference, np.eye(R))


# ---------------------------------------------------------------------------------------------- the C entries directly

def bare_entries(A, W, flags, planes, offs, R, fill):
    """Every entry of the family on guarded, poisoned buffers -> the host copies of what they wrote; every guard band checked."""
    L = _lib.lib()
    S = A.shape[0]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = {}

    def buf(name, shape, dtype, align, init=None):
        g[name] = Guarded(shape, dtype, fill, DEV, align=align, init=init)
        return g[name]

    nbytes = int(L.chebgcn_tangent_workspace(S, R))
    buf('A', (S, R, R), 'float64', 8, A)
    buf('w', (S, R), 'float64', 8)
    buf('Vt', (S, R, R), 'float64', 8)
    buf('sweeps', (S,), 'int32', 4)
    buf('converged', (S,), 'int32', 4)
    buf('ws', (nbytes // 4,), 'int32', 8)
    assert L.chebgcn_sym_eigh(g['A'].ptr, S, R, g['w'].ptr, g['Vt'].ptr, g['sweeps'].ptr, g['converged'].ptr, g['ws'].ptr, nbytes,
                              stream) == 0, L.chebgcn_last_error()
    assert _lib.last_dispatch() == EIGH_KERNELS
    buf('flags', (S,), 'int32', 4, flags)
    buf('fvals', (S, R), 'float64', 8)
    buf('exp', (S, R, R), 'float64', 8)
    buf('exp32', (S, R, R), 'float32', 4)
    for out, f32 in (('exp', 0), ('exp32', 1)):
        assert L.chebgcn_sym_function(g['w'].ptr, g['Vt'].ptr, S, R, 1, 0.5, g[out].ptr, f32, g['flags'].ptr, g['fvals'].ptr,
                                      stream) == 0, L.chebgcn_last_error()
        assert _lib.last_dispatch() == FUNCTION_KERNELS
    buf('W', (R, R), 'float64', 8, W)
    buf('scratch', (S, R, R), 'float64', 8)
    buf('cong', (S, R, R), 'float64', 8)
    assert L.chebgcn_sym_congruence(g['W'].ptr, g['A'].ptr, S, R, g['cong'].ptr, g['scratch'].ptr, stream) == 0, L.chebgcn_last_error()
    assert _lib.last_dispatch() == CONGRUENCE_KERNELS
    buf('acc', (R, R), 'float64', 8)
    buf('mean', (R, R), 'float64', 8)
    buf('norm', (1,), 'float64', 8)
    n = int((flags == 0).sum())
    assert L.chebgcn_sym_mean(g['cong'].ptr, g['flags'].ptr, S, R, 1, n, g['acc'].ptr, g['mean'].ptr, g['norm'].ptr, stream) == 0
    assert _lib.last_dispatch() == MEAN_END_KERNELS
    Ttot, Rp = planes.shape
    cbytes = int(L.chebgcn_connectome_workspace(S, R))
    buf('planes', (Ttot, Rp), 'float32', 16, planes)
    buf('offs', (S + 1,), 'int64', 8, offs)
    buf('cws', (cbytes // 8,), 'float64', 16)
    buf('sigma', (S, R, R), 'float64', 8)
    buf('shrunk', (S,), 'float64', 8)
    assert L.chebgcn_connectome_cov(g['planes'].ptr, Ttot, g['offs'].ptr, S, R, g['cws'].ptr, cbytes, stream) == 0
    assert L.chebgcn_connectome_sigma(g['cws'].ptr, cbytes, g['offs'].ptr, Ttot, S, R, -1.0, g['sigma'].ptr, g['shrunk'].ptr,
                                      stream) == 0, L.chebgcn_last_error()
    assert _lib.last_dispatch() == 'connectome_sigma_kernel'
    torch.cuda.synchronize()
    for name, b in g.items():
        b.check(name)
    for name, init in (('A', A), ('W', W), ('offs', offs)):
        assert np.array_equal(bits(g[name].host()), bits(np.ascontiguousarray(init, g[name].np_dtype))), '%s was written' % name
    return {k: g[k].host() for k in ('w', 'Vt', 'sweeps', 'converged', 'flags', 'exp', 'exp32', 'cong', 'mean', 'norm', 'sigma', 'shrunk')}


@pytest.mark.parametrize('R', (9, 33, 130))
def test_guard_bands_poisoned_buffers_and_nan_pads(R):
    S = 3
    A = np.stack([whitened(R, seed=7 * R + 2 * s) for s in range(S)])
    A = np.stack([cn._sym_fun_host(a, np.log) for a in A])
    A = A - (np.trace(A, axis1=1, axis2=2) / R)[:, None, None] * np.eye(R)
    W = random_sym(1, R, seed=R)[0]
    flags = np.array([0, 1, 0], np.int32)
    runs = [latent(T, R, seed=T + R) for T in (40, 2, 97)]
    offs = _runs.offsets(runs)
    planes = np.full((int(offs[-1]), _lib.plane_stride(R)), np.nan, np.float32)
    for x, o in zip(runs, offs):
        planes[o:o + len(x), :R] = x
    out = [bare_entries(A, W, flags, planes, offs, R, fill) for _, fill in FILLS]
    for k in out[0]:
        assert np.array_equal(bits(out[0][k]), bits(out[1][k])), '%s depends on memory nobody wrote' % k
    o = out[0]
    assert (o['converged'] == 1).all() and (o['sweeps'] >= 2).all() and (o['sweeps'] <= 40).all()
    for s in range(S):
        V = o['Vt'][s].T
        assert np.abs(V.T @ V - np.eye(R)).max() <= 1e-11 and np.abs(A[s] - (V * o['w'][s]) @ V.T).max() <= 1e-11 * np.abs(A[s]).max()
    assert o['flags'].tolist() == [0, 1, 0] and not o['exp'][1].any() and not o['exp32'][1].any()
    for s in (0, 2):
        ref = cn._sym_fun_host(A[s], lambda w: np.exp(0.5 * w))
        assert np.abs(o['exp'][s] - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.array_equal(o['exp32'], o['exp'].astype(np.float32))
    assert np.array_equal(bits(o['mean']), bits((o['cong'][0] + o['cong'][2]) / 2))
    for s, x in enumerate(runs):
        ref = cn.host_run(x, 'covariance', -1.0)[0]
        assert np.abs(o['sigma'][s] - ref).max() <= 1e-12 * np.abs(ref).max()
    via = ops.sym_eigh(dev64(A))                                   # the Python path gives the same bits as the bare entry
    assert np.array_equal(bits(via[0].cpu().numpy()), bits(o['w'])) and np.array_equal(bits(via[1].cpu().numpy()), bits(o['Vt']))


# ---------------------------------------------------------------------------------------------- the graph on top

def test_into_the_rsfc_graph_and_a_forward_pass():
    R, k = 33, 8
    rng = np.random.RandomState(1)                               # (a global signal: mean connectivity above 0, as in resting-state scans)
    runs = [latent(T, R, seed=R + T, factors=6) + 1.5 * rng.randn(T, 1).astype(np.float32) for T in (284, 200, 284)]
    t = cn.tangent(runs, device=DEV)
    z = np.tanh(t.mean.cpu().numpy())
    sig = z.mean()
    v, idx = graph.knn_from_similarity(np.exp(z / sig), k)
    v = v.copy()
    v[v < 1] = 0
    A = graph.adjacency(v, idx)
    assert A.shape == (R, R) and abs(A - A.T).max() == 0 and A.diagonal().max() == 0 and A.nnz > 0
    L = graph.laplacian(A.astype(np.float32), normalized=True)
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, [L, L], [4, 6], [3, 3], [1, 1], [9, 5], channel=3, brelu='b1relu', batch_size=8,
                           verbose=False, dropout=1)
    x = torch.as_tensor(np.random.RandomState(0).randn(8, R, 3).astype(np.float32)).to(DEV)
    with torch.no_grad():
        logits = net.inference(x, 1).cpu().numpy()
    assert logits.shape == (8, 5) and np.isfinite(logits).all()
