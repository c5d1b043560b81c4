"""What the AR(1) tests of ``glm.first_level`` share (test_glm_ar1_host.py on the CPU, test_gpu_glm_ar1.py on the device): the
inputs of every device case, built from the kernels' geometry alone so that the CPU test can measure them too; a float64 NumPy
statement of the sums algebra the kernels use; the natural scales of the bound; and EPS, the absolute term of the bound.

The bound, for effect, variance, t, beta and rho at EVERY vertex:  ``|got - ref| <= 2^-23 |ref| + EPS s``  with ref =
``first_level_host(noise='ar1')`` -- explicit covariance, Cholesky whitening, lstsq, residuals -- and s the natural scale:

* effect, variance, beta, t: the scales of test_gpu_glm.py (``|u| sqrt(y.y)``, ``|u|^2 y.y / dof``, ``|B_p| sqrt(y.y)``, and the
  first-order propagation for t);
* rho: ``y.y / rss_ols`` -- numerator and denominator of the estimate are differences of sums of size y.y.

EPS is four times the largest distance, in these units, of the float64 sums statement below from the host restatement over the
inputs of every device case (the sinusoid, whose first vertex sits at the clamp, included): the statement IS the kernels'
algebra, so that distance is what the algebra itself costs in float64 (the cancellations ``y.y - a.a`` and ``y^T K y - z.z``), and the factor 4 is for the order of the sums on the device.
Measured on the CPU (test_glm_ar1_host.py::test_the_sums_statement_on_the_inputs_of_the_device_cases asserts it on every run):
the largest distance is 9.1e-12, a coefficient of the sinusoid's clamped vertex, where rho = 0.99 makes the host's own 137 x 137
covariance ill-conditioned (there: effect 4.2e-13, t 3.9e-13, variance 9.4e-14); over all other vertices and cases it is 2.6e-13
(coefficients; effect 2.4e-13, t 2.2e-14, variance 1.4e-14, rho 7.8e-15).  So EPS = 3.64e-11.
"""
import numpy as np

from gcn_fmri_decoding_amd import glm
from gcn_fmri_decoding_amd.runs import host_array

EPS32 = 2.0 ** -23
MEASURED = 9.1e-12          # the sums statement against the host restatement, largest over the device cases (see above)
EPS = 4.0 * MEASURED
RHO_FREE = 0.98             # every input but the sinusoid keeps the host's |rho| below this: no vertex at the clamp


def geometry():
    """The kernels' constants without a device (the query entry points need none)."""
    from gcn_fmri_decoding_amd import _lib
    L = _lib.lib()
    q = L.chebgcn_glm_query
    geo = {'vertices': q(0), 'panel': q(1), 'max_k': q(2), 'max_C': q(3), 'split': q(4), 'slice': q(5), 'slices': q(6)}
    geo['bucket'] = lambda k: L.chebgcn_glm_ar1_query(100 + k)
    geo['finish_vertices'] = lambda k: L.chebgcn_glm_ar1_query(200 + k)
    return geo


def random_design(rng, T, P, C):
    """A full-rank design of P columns (the last the intercept) and C random contrasts."""
    X = rng.randn(T, P)
    X[:, -1] = 1.0
    return glm.Design(X, ['x%d' % i for i in range(P - 1)] + ['constant'], ['x0']), rng.randn(C, P)


def ar1_noise(rng, T, M, rho):
    """Stationary AR(1) noise of unit innovation variance, [T, M]; ``rho`` a number or one per vertex."""
    rho = np.broadcast_to(np.asarray(rho, np.float64), (M,))
    e = rng.randn(T, M)
    x = np.empty((T, M))
    x[0] = e[0] / np.sqrt(1.0 - rho * rho)
    for t in range(1, T):
        x[t] = rho * x[t - 1] + e[t]
    return x


def series(rng, design, M, mean=100.0, sd=1.0, gain=2.0, rho=None):
    """Signal in the design's span plus AR(1) noise whose coefficient differs from vertex to vertex (-0.3 .. 0.6)."""
    X = design.X
    rho = rng.uniform(-0.3, 0.6, M) if rho is None else rho
    return (mean + gain * (X[:, :-1] @ rng.randn(X.shape[1] - 1, M)) + sd * ar1_noise(rng, X.shape[0], M, rho)).astype(np.float32)


def device_cases(geo):
    """name -> (runs, designs, contrasts, groups, rho): the inputs of every device test that is held against the host."""
    out = {}
    for M in (1, 33, geo['vertices'] + 1):
        rng = np.random.RandomState(M)
        d, c = random_design(rng, geo['split'] + 5, 3, 2)
        out['M%d' % M] = (series(rng, d, M), d, c, None, None)
    half = geo['panel'] // 2
    for k in (1, 2, half, half + 1, geo['panel'], geo['panel'] + 1, 32, 33, geo['max_k']):
        for C in (1, geo['max_C']):
            rng = np.random.RandomState(100 * k + C)
            d, c = random_design(rng, 3 * geo['slice'] + 5 + k, k, C)
            out['k%d_C%d' % (k, C)] = (series(rng, d, 33), d, c, None, None)
    k = 5
    for T in (k + 2, geo['split'] - 1, geo['split'], geo['split'] + 1, 3 * geo['slice'] + 5):
        rng = np.random.RandomState(T)
        d, c = random_design(rng, T, k, 2)
        out['T%d' % T] = (series(rng, d, 33), d, c, None, None)
    out['mixed'] = mixed(geo) + (None,)
    rng = np.random.RandomState(12)
    d, c = random_design(rng, 2 * geo['split'] + 7, 6, 3)
    out['given'] = (series(rng, d, 37), d, c, None, 0.3)
    out['groups'] = grouped(geo) + (None,)
    out['constant'] = constant(geo) + (None, None)
    return out


def mixed(geo):
    """Three runs of different length (two shorter than a slice, one of 7 slices + 3) and rank, a group each."""
    rng = np.random.RandomState(11)
    k = 6
    shapes = [(k + 2, k), (7 * geo['slice'] + 3, 4), (k + 3, 5)]
    designs, contrasts = zip(*[random_design(rng, T, P, 2) for T, P in shapes])
    runs = [series(rng, d, geo['finish_vertices'](k) + 1) for d in designs]
    return runs, list(designs), list(contrasts), ['a', 'b', 'c']


def grouped(geo):
    rng = np.random.RandomState(8)
    groups = ['s2', 's1', 's2', 's3', 's3', 's3']
    lengths = [geo['split'] + 3, 40, 3 * geo['slice'] + 5, 50, geo['split'] - 1, 4 * geo['slice'] + 1]
    names = (['rest'] * 4 + ['a'] * 6 + ['rest'] * 3 + ['b'] * 7) * 8
    designs = [glm.design_matrix(names=names[:T], tr=0.72, high_pass=0.02) for T in lengths]
    runs = [series(rng, d, 37, mean=1000.0, sd=5.0) for d in designs]
    return runs, designs, None, groups


def constant(geo):
    """Vertices 5 (a constant) and 40 (zero) among AR(1) neighbours."""
    rng = np.random.RandomState(6)
    d, c = random_design(rng, geo['split'] + 9, 4, 3)
    y = series(rng, d, 64)
    y[:, 5] = 100.0
    y[:, 40] = 0.0
    return y, d, c


def sinusoid(geo):
    """Vertex 0: a slow sinusoid outside the design (one period over the run) under little noise, whose raw residual
    autocorrelation is above 0.995; the other vertices ordinary."""
    rng = np.random.RandomState(13)
    T = 4 * geo['slice'] + 9
    t = np.arange(T, dtype=np.float64)                                          # slow columns only: they leave no white part
    X = np.stack([np.cos(np.pi * (2.0 * t + 1.0) * j / (2.0 * T)) for j in (2, 4)] + [np.ones(T)], axis=1)     # even about the middle
    d = glm.Design(X, ['x0', 'x1', 'constant'], ['x0', 'x1'])
    y = series(rng, d, 9).astype(np.float64)
    y[:, 0] = 100.0 + 40.0 * np.sin(2.0 * np.pi * np.arange(T) / T) + 0.01 * rng.randn(T)
    return y.astype(np.float32), d, None


# ---- the sums algebra in float64 NumPy ------------------------------------------------------------------------------------------

def sums_statement(runs, designs, contrasts=None, groups=None, rho=None):
    """``first_level(noise='ar1')`` by the algebra of the kernels, in float64 NumPy: the sums a, h, S0, S1 and the end samples
    of every run, rho from them, then per vertex the k x k system M(rho), its Cholesky factor and the triangular solves.
    Returns ``(GLMResultAR1, raw)`` with ``raw`` the unclamped estimate per run (None where rho is given)."""
    from scipy.linalg import cholesky, solve_triangular
    pl = glm._plan(runs, designs, contrasts, groups, 'sums_statement', limits=False)
    eff, var, bs, rhos, raws = [], [], [], [], []
    for y, tb in zip(pl.runs, pl.tables):
        y = host_array(y, 'sums_statement').astype(np.float64)
        Q, k, T = tb.Q, tb.rank, tb.T
        Qs = np.zeros_like(Q)
        Qs[1:] += Q[:-1]
        Qs[:-1] += Q[1:]
        D = Q.T @ Qs
        E = np.outer(Q[0], Q[0]) + np.outer(Q[-1], Q[-1])
        a, h = Q.T @ y, Qs.T @ y
        S0, S1 = (y * y).sum(axis=0), (y[1:] * y[:-1]).sum(axis=0)
        y0, yL = y[0], y[-1]
        if rho is None:
            rss = S0 - (a * a).sum(axis=0)
            rss = np.where(rss < 4.0 * (T + k) * 2.0 ** -53 * S0, 0.0, rss)
            num = S1 - (a * h).sum(axis=0) + 0.5 * np.einsum('im,ij,jm->m', a, D, a)
            raw = np.where(rss > 0, num / np.where(rss > 0, rss, 1.0), 0.0)
            rv = np.clip(raw, -glm.RHO_MAX, glm.RHO_MAX)
        else:
            raw, rv = None, np.full(pl.M, float(rho))
        e, v, b = np.empty((pl.C, pl.M)), np.empty((pl.C, pl.M)), np.empty((tb.X.shape[1], pl.M))
        for m in range(pl.M):
            r = rv[m]
            Mr = (1.0 + r * r) * np.eye(k) - r * D - r * r * E
            g = (1.0 + r * r) * a[:, m] - r * h[:, m] - r * r * (Q[0] * y0[m] + Q[-1] * yL[m])
            yKy = (1.0 + r * r) * S0[m] - 2.0 * r * S1[m] - r * r * (y0[m] ** 2 + yL[m] ** 2)
            Lc = cholesky(Mr, lower=True)
            z = solve_triangular(Lc, g, lower=True)
            w = solve_triangular(Lc, tb.u.T, lower=True)                        # [k, C]
            rs = yKy - z @ z
            if rs < 4.0 * (T + k) * 2.0 ** -53 * (1.0 + abs(r)) ** 4 / (1.0 - abs(r)) ** 2 * S0[m]:
                rs = 0.0
            e[:, m] = w.T @ z
            v[:, m] = rs / (T - k) * (w * w).sum(axis=0)
            b[:, m] = tb.B @ solve_triangular(Lc.T, z, lower=False)
        eff.append(e), var.append(v), bs.append(b), rhos.append(rv), raws.append(raw)
    S = len(pl.keys)
    effect, variance = np.empty((S, pl.C, pl.M)), np.empty((S, pl.C, pl.M))
    for gi, mem in enumerate(pl.members):
        effect[gi] = sum(eff[r] for r in mem) / len(mem)
        variance[gi] = sum(var[r] for r in mem) / float(len(mem)) ** 2
    dof = np.array([sum(pl.tables[r].T - pl.tables[r].rank for r in m) for m in pl.members], np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(variance > 0, effect / np.sqrt(variance), 0.0)
    return glm.GLMResultAR1(effect, variance, t, dof, list(pl.keys), bs, rhos), raws


# ---- the bound ------------------------------------------------------------------------------------------------------------------

def scales(runs, designs, contrasts, groups):
    """The natural scales: per group for effect and variance, per run for the coefficients and for rho."""
    pl = glm._plan(runs, designs, contrasts, groups, 'scales', limits=False)
    ys = [np.asarray(r.cpu() if hasattr(r, 'cpu') else r, np.float32).astype(np.float64) for r in pl.runs]
    yy = [(y * y).sum(axis=0) for y in ys]
    se = [np.sqrt(tb.un2)[:, None] * np.sqrt(q)[None, :] for tb, q in zip(pl.tables, yy)]
    sv = [tb.un2[:, None] * q[None, :] / (tb.T - tb.rank) for tb, q in zip(pl.tables, yy)]
    sb = [np.linalg.norm(tb.B, axis=1)[:, None] * np.sqrt(q)[None, :] for tb, q in zip(pl.tables, yy)]
    sr = []
    for tb, y, q in zip(pl.tables, ys, yy):
        res = y - tb.Q @ (tb.Q.T @ y)
        sr.append(q / np.maximum((res * res).sum(axis=0), 1e-300))
    s_e = np.stack([sum(se[r] for r in m) / len(m) for m in pl.members])
    s_v = np.stack([sum(sv[r] for r in m) / len(m) ** 2 for m in pl.members])
    return s_e, s_v, sb, sr


def worst(got, ref, s, eps):
    """max over every element of |got - ref| / (2^-23 |ref| + eps s); with eps = 0 and no relative term: |got - ref| / s."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    if eps == 0:
        return float((np.abs(got - ref) / (s + 1e-300)).max())
    return float((np.abs(got - ref) / (EPS32 * np.abs(ref) + eps * s + 1e-300)).max())


def distances(res, ref, runs, designs, contrasts, groups, eps, live=None):
    """The five figures of ``worst`` of a result against the host's; vertices whose host variance is 0 are exempt from t (the
    device's t must be 0 there: asserted by the caller).  ``live``: the vertices of rho to hold (default all)."""
    s_e, s_v, s_b, s_r = scales(runs, designs, contrasts, groups)
    pos = ref.variance > 0
    v = np.where(pos, ref.variance, 1.0)
    s_t = np.where(pos, s_e / np.sqrt(v) + np.abs(ref.t) * s_v / (2.0 * v), 0.0)
    get = lambda x: np.asarray(x.cpu() if hasattr(x, 'cpu') else x)
    live = slice(None) if live is None else live
    return {'effect': worst(get(res.effect), ref.effect, s_e, eps), 'variance': worst(get(res.variance), ref.variance, s_v, eps),
            't': worst(np.where(pos, get(res.t), 0.0), np.where(pos, ref.t, 0.0), s_t, eps),
            'beta': max(worst(get(b), rb, s, eps) for b, rb, s in zip(res.betas, ref.betas, s_b)),
            'rho': max(worst(get(a)[live], b[live], s[live], eps) for a, b, s in zip(res.rho, ref.rho, s_r))}
