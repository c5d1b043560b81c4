"""First-level general linear model: task activation maps from the event designs the decoder is trained on.

``design_matrix`` turns the per-TR condition names ``match_events`` takes (or an ``(onset, duration, name)`` list) into a design:
one HRF-convolved regressor per condition, cosine drifts, confounds, intercept.  ``first_level`` regresses every vertex of every
staged run on its design on the device and returns, per subject, the effect, variance and t map of every contrast -- by default
one condition against the others, in the class order of ``EventWindows.classes`` and of the attribution maps, so that
``map_test(first_level(...).effect, A)`` and ``map_test(saliency maps, A)`` speak about the same subjects and classes.
``first_level_host`` restates it in float64 NumPy.

Condition regressors are in closed form.  With ``F_a`` the CDF of the unit-scale gamma distribution of shape ``a``, the response
to a unit step at time 0 of the double-gamma HRF ``h = (gamma_a1 - ratio gamma_a2) / (1 - ratio)`` (SPM: 6, 16, 1/6; unit area)
is ``G(s) = (F_a1(s) - ratio F_a2(s)) / (1 - ratio)`` for ``s >= 0`` and 0 below, so a block ``[on, off)`` contributes
``G(t - on) - G(t - off)`` at time t: no oversampling grid, plateau 1 for long blocks.

On the device a run's design enters as its thin SVD ``X = U S V^T`` of rank k (singular values above ``max(T, P) eps S_0``):
``Q = U[:, :k]``, ``B = V[:, :k] / S[:k]``.  One pass over the scan forms ``a = Q^T y`` and ``y.y`` (chebgcn_glm_project);
``rss = y.y - a.a``, ``b = B a`` (the minimum-norm solution), and for a contrast c ``effect = u.a`` with ``u = B^T c``,
``variance = rss / dof * u.u`` (chebgcn_glm_finish); the runs of a subject are combined as fixed effects
(chebgcn_glm_combine).  All of it float64 on the device, rounded once to float32: see include/chebgcn.h.

``noise='ar1'`` prewhitens: the noise of a run is a stationary AR(1) process, covariance ``sigma^2 rho^|i-j| / (1 - rho^2)``,
and the fit is exact generalised least squares (the first row scaled, Prais-Winsten, not dropped) -- the OLS t of a single run is
optimistic under the temporal autocorrelation of BOLD noise.  ``rho`` is estimated per (run, vertex) from the OLS residuals,
``sum r_t r_{t-1} / sum r_t^2`` clamped to ``+-RHO_MAX``, or given for every vertex (SPM's global AR(1)).  With
``K = (1 + rho^2) I - rho (Sh + Sh^T) - rho^2 (e_0 e_0^T + e_L e_L^T)`` (``Sh`` the one-row shift, ``L = T - 1``) everything is
linear or bilinear in y: the pass forms ``a = Q^T y``, ``h = Qs^T y`` (``Qs = Sh Q + Sh^T Q``), ``y.y`` and the lag sum
``sum y_t y_{t-1}`` (chebgcn_glm_project_ar1); per vertex ``rho = (S1 - a.h + a.D a / 2) / (y.y - a.a)``, ``D = Q^T Qs``, then the
``k x k`` system ``M = (1 + rho^2) I - rho D - rho^2 E`` (``E = q_0 q_0^T + q_L q_L^T``) is factored ``M = L L^T`` and
``z = L^-1 g``, ``w = L^-1 u`` give ``rss = y^T K y - z.z``, ``effect = w.z``, ``variance = rss / dof * w.w``, ``b = B L^-T z``
(chebgcn_glm_finish_ar1).  ``dof`` takes no correction for estimating rho (as nilearn and SPM).

Out of scope: bias correction of the estimated rho (the residual estimate is biased downward, the more so the more regressors),
AR orders above 1, rho smoothed across vertices, temporal derivatives of the HRF, precision-weighted fixed effects, and returning
residual series.

``trial_design`` / ``single_trial`` give one pattern per TRIAL for the searchlight and RSA chains: the beta series by "least
squares - separate", one GLM per trial ``[x_j | the other trials lumped per condition | nuisance]``.  The models of a run differ
by one column swap, so one set of projections of y serves all of them (chebgcn_glm_project over ``[Qn | Z_S]``, then
chebgcn_glm_trials, which finishes every trial where its projection was formed); ``single_trial_host`` restates it with one
explicit fit per trial.  See ``single_trial``.

The host-only parts need NumPy and SciPy only.
"""
import collections

import numpy as np

from . import runs as _runs

HRF_SPM = (6.0, 16.0, 1.0 / 6.0)
KMAX, CMAX, PMAX, RMAX = 64, 32, 64, 65535      # chebgcn_glm_query(2), (3), (7), (8)
ESTIMABLE_TOL = 1e-8
RHO_MAX = 0.99                                  # an estimated AR(1) coefficient is clamped to +- this (include/chebgcn.h)

Design = collections.namedtuple('Design', 'X columns conditions')
Design.__doc__ = """What ``design_matrix`` returns: ``X`` float64 [T, P]; ``columns`` the P column names (the conditions, then
``drift_1`` .., ``confound_0`` .., ``constant`` last); ``conditions`` the condition names, = the first columns, in class order."""

GLMResult = collections.namedtuple('GLMResult', 'effect variance t dof groups betas')
GLMResult.__doc__ = """What ``first_level`` returns.  ``effect``, ``variance``, ``t``: float32 [S, C, M], one map per group (subject)
and contrast (float64 from ``first_level_host``); ``dof`` int64 [S] the residual degrees of freedom (summed over the group's
runs); ``groups`` the S group keys in order of first appearance; ``betas`` None, or one float32 [P_r, M] per run."""

GLMResultAR1 = collections.namedtuple('GLMResultAR1', 'effect variance t dof groups betas rho')
GLMResultAR1.__doc__ = """What ``first_level(noise='ar1')`` returns: the fields of ``GLMResult``, then ``rho``: one float32 [M] array
per run (a tensor where the run came as a tensor; float64 from ``first_level_host``), the AR(1) coefficient of every vertex."""


# ---- designs --------------------------------------------------------------------------------------------------------------------

def _names(seq, what):
    a = np.asarray(seq)
    if isinstance(seq, str) or a.ndim != 1 or a.size == 0 or a.dtype.kind not in 'USO' \
            or (a.dtype.kind == 'O' and not all(isinstance(n, str) for n in a)):
        raise ValueError('design_matrix: %s must be a non-empty 1-d sequence of condition names (str), got %s %s'
                         % (what, a.dtype, a.shape))
    return a.astype(str)


def step_response(s, hrf=HRF_SPM):
    """``G(s)``: the response at time s (seconds, any shape) to a unit step at 0; the boxcar's own step for ``hrf=None``."""
    s = np.asarray(s, np.float64)
    if hrf is None:
        return (s >= 0).astype(np.float64)
    from scipy.stats import gamma
    a1, a2, ratio = hrf
    sp = np.maximum(s, 0.0)
    return np.where(s >= 0, (gamma.cdf(sp, a1) - ratio * gamma.cdf(sp, a2)) / (1.0 - ratio), 0.0)


def _design_args(names, events, T, tr, conditions, hrf, high_pass, confounds):
    """The arguments of ``design_matrix`` checked and parsed: ``(T, tr, hrf, blocks [(onset_s, offset_s, name)], conditions,
    drift order, confounds float64 [T, Qn] or None)``."""
    if (names is None) == (events is None):
        raise ValueError('design_matrix: give exactly one of names (per-TR condition names) and events ((onset, duration, name))')
    if isinstance(tr, (bool, np.bool_)) or not isinstance(tr, (int, float, np.integer, np.floating)) or not np.isfinite(tr) or tr <= 0:
        raise ValueError('design_matrix: tr must be a positive number of seconds, got %r' % (tr,))
    tr = float(tr)
    if T is not None and (isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)) or T < 1):
        raise ValueError('design_matrix: T must be an int >= 1, got %r' % (T,))
    if isinstance(hrf, str):
        if hrf != 'spm':
            raise ValueError("design_matrix: hrf must be 'spm', (a1, a2, ratio) or None, got %r" % (hrf,))
        hrf = HRF_SPM
    elif hrf is not None:
        try:
            hrf = tuple(float(v) for v in hrf)
        except (TypeError, ValueError):
            hrf = ()
        if len(hrf) != 3 or not all(np.isfinite(hrf)) or hrf[0] <= 0 or hrf[1] <= 0 or hrf[2] == 1.0:
            raise ValueError("design_matrix: hrf must be 'spm', (a1, a2, ratio) with shapes > 0 and ratio != 1, or None")
    blocks = []                                                 # (onset, offset, name), seconds
    if names is not None:
        names = _names(names, 'names')
        if T is not None and int(T) != names.size:
            raise ValueError('design_matrix: T = %d but names has %d entries' % (T, names.size))
        T = int(names.size)
        cuts = np.concatenate([[0], np.flatnonzero(names[1:] != names[:-1]) + 1, [T]])
        blocks = [(i * tr, i * tr + (j - i) * tr, str(names[i])) for i, j in zip(cuts[:-1], cuts[1:])]     # as (onset, duration) gives it
        seen = set(names.tolist())
    else:
        if T is None:
            raise ValueError('design_matrix: events need T, the number of rows of the run')
        T = int(T)
        if isinstance(events, (str, np.ndarray)) or not hasattr(events, '__len__') or len(events) == 0:
            raise ValueError('design_matrix: events must be a non-empty sequence of (onset_s, duration_s, name)')
        for i, ev in enumerate(events):
            try:
                on, dur, name = ev
                on, dur = float(on), float(dur)
            except (TypeError, ValueError):
                raise ValueError('design_matrix: event %d must be (onset_s, duration_s, name), got %r' % (i, ev)) from None
            if not isinstance(name, str) or not np.isfinite(on) or not np.isfinite(dur) or dur < 0:
                raise ValueError('design_matrix: event %d must be (onset_s, duration_s >= 0, name str), got %r' % (i, ev))
            blocks.append((on, on + dur, name))
        seen = set(b[2] for b in blocks)
    if conditions is None:
        conditions = sorted(seen - {'rest'})
    elif isinstance(conditions, str) or not hasattr(conditions, '__len__') or not all(isinstance(n, str) for n in conditions):
        raise ValueError('design_matrix: conditions must be a sequence of condition names (str), got %r' % (conditions,))
    conditions = [str(n) for n in conditions]
    if not conditions or len(set(conditions)) != len(conditions):
        raise ValueError('design_matrix: conditions must be non-empty and distinct, got %r' % (conditions,))
    order = 0
    if high_pass is not None:
        if isinstance(high_pass, (bool, np.bool_)) or not isinstance(high_pass, (int, float, np.integer, np.floating)) \
                or not np.isfinite(high_pass) or high_pass < 0:
            raise ValueError('design_matrix: high_pass must be a frequency >= 0 in Hz or None, got %r' % (high_pass,))
        order = int(np.floor(2.0 * T * tr * float(high_pass)))
    Qn = 0
    if confounds is not None:
        confounds = np.asarray(confounds)
        if confounds.ndim != 2 or confounds.shape[0] != T or confounds.dtype.kind not in 'fiu':
            raise ValueError('design_matrix: confounds must be numeric [T = %d, Q], got %s %r' % (T, confounds.dtype, confounds.shape))
        confounds = confounds.astype(np.float64)
        if not np.isfinite(confounds).all():
            raise ValueError('design_matrix: confounds hold non-finite values')
        Qn = confounds.shape[1]
    return T, tr, hrf, blocks, conditions, order, confounds


def _nuisance(T, order, confounds):
    """The columns of a design that are no conditions: ``(float64 [T, order + Qn + 1], their names)`` -- cosine drifts, the
    confounds as given, the intercept last."""
    Qn = 0 if confounds is None else confounds.shape[1]
    N = np.zeros((T, order + Qn + 1))
    k = np.arange(T, dtype=np.float64)
    for j in range(1, order + 1):
        N[:, j - 1] = np.cos(np.pi * (2.0 * k + 1.0) * j / (2.0 * T))
    if Qn:
        N[:, order:order + Qn] = confounds
    N[:, -1] = 1.0
    return N, ['drift_%d' % j for j in range(1, order + 1)] + ['confound_%d' % q for q in range(Qn)] + ['constant']


def design_matrix(names=None, events=None, T=None, tr=0.72, conditions=None, hrf='spm', high_pass=1.0 / 128, confounds=None):
    """The design of one run: a ``Design``.

    Exactly one of ``names`` -- per-TR condition names, the format ``match_events`` takes: a maximal stretch of equal names from
    TR i to TR j is a block ``[i tr, (j + 1) tr)`` -- and ``events`` -- a sequence of ``(onset_s, duration_s, name)``, which
    needs ``T``.  ``conditions`` defaults to the sorted set of names other than ``'rest'`` (the order of
    ``EventWindows.classes``); names outside ``conditions`` are left to the baseline.  ``tr``: seconds per row (0.72: HCP).
    ``hrf``: ``'spm'`` (shapes 6 and 16, ratio 1/6), a tuple ``(a1, a2, ratio)``, or None for the plain boxcar sampled at
    ``t_k = k tr``.  Regressors are ``x(t_k) = sum_blocks G(t_k - on) - G(t_k - off)`` in closed form (see the module).
    ``high_pass`` (Hz): drift columns ``cos(pi (2 k + 1) j / (2 T))``, ``j = 1 .. floor(2 T tr high_pass)``; None or an order of
    0 gives none.  ``confounds``: ``[T, Q]``, appended as given.  The intercept is the last column.  Every malformed argument
    is a ``ValueError``."""
    T, tr, hrf, blocks, conditions, order, confounds = _design_args(names, events, T, tr, conditions, hrf, high_pass, confounds)
    t = np.arange(T, dtype=np.float64) * tr
    N, nuisance = _nuisance(T, order, confounds)
    X = np.zeros((T, len(conditions) + N.shape[1]))
    for on, off, name in blocks:
        if name in conditions:
            X[:, conditions.index(name)] += step_response(t - on, hrf) - step_response(t - off, hrf)
    X[:, len(conditions):] = N
    return Design(X, conditions + nuisance, list(conditions))


def contrasts_one_vs_rest(design):
    """``[classes, P]``: +1 on a condition and ``-1 / (n - 1)`` on the others, in class order (one condition: +1 alone, the
    condition against the baseline).  The default of ``first_level``."""
    n, P = len(design.conditions), len(design.columns)
    if n < 1:
        raise ValueError('contrasts_one_vs_rest: the design has no conditions')
    c = np.zeros((n, P))
    c[:, :n] = -1.0 / (n - 1) if n > 1 else 0.0
    c[np.arange(n), np.arange(n)] = 1.0
    return c


# ---- arguments ------------------------------------------------------------------------------------------------------------------

_Run = collections.namedtuple('_Run', 'T X c rank Q B u un2')
_Plan = collections.namedtuple('_Plan', 'runs tables M C keys members tensors')


def _factor(X):
    """Thin SVD of a design: ``(rank, Q [T, k], B [P, k])`` -- ``b = B (Q^T y)`` is the minimum-norm least-squares solution."""
    U, S, Vt = np.linalg.svd(X, full_matrices=False)
    k = int((S > max(X.shape) * np.finfo(np.float64).eps * S[0]).sum()) if S.size and S[0] > 0 else 0
    return k, np.ascontiguousarray(U[:, :k]), np.ascontiguousarray(Vt[:k].T / S[:k])


def _plan(runs, designs, contrasts, groups, who, limits=True):
    """Everything that can be checked without the series' values; the per-run tables of the kernels."""
    runs, _, M, tensors = _runs.as_runs(runs, who)
    if isinstance(designs, Design):
        designs = [designs]
    designs = list(designs)
    if len(designs) != len(runs) or not all(isinstance(d, Design) for d in designs):
        raise ValueError('%s: designs must hold one Design per run (%d runs, %d designs)' % (who, len(runs), len(designs)))
    R = len(runs)
    _, keys, members = _runs.group_keys(groups, R, who)
    per_run = None
    if contrasts is not None:
        if isinstance(contrasts, (list, tuple)) and len(contrasts) == R and all(np.ndim(c) == 2 for c in contrasts):
            per_run = [np.asarray(c, np.float64) for c in contrasts]
        else:
            c = np.atleast_2d(np.asarray(contrasts, np.float64))
            if c.ndim != 2:
                raise ValueError('%s: contrasts must be [C, P] (or one such array per run), got shape %r' % (who, c.shape))
            per_run = [c] * R
    tables = []
    C = None
    for r, (y, d) in enumerate(zip(runs, designs)):
        X = np.asarray(d.X, np.float64)
        if X.ndim != 2 or X.shape[1] < 1 or not np.isfinite(X).all():
            raise ValueError('%s: the design of run %d must be a finite [T, P] matrix' % (who, r))
        T, P = int(y.shape[0]), int(X.shape[1])
        if X.shape[0] != T:
            raise ValueError('%s: the design of run %d has %d rows, the run %d' % (who, r, X.shape[0], T))
        c = contrasts_one_vs_rest(d) if per_run is None else per_run[r]
        if c.shape[1] != P or c.shape[0] < 1 or not np.isfinite(c).all():
            raise ValueError('%s: the contrasts of run %d must be finite [C, P = %d], got %r' % (who, r, P, c.shape))
        if C is None:
            C = int(c.shape[0])
        if c.shape[0] != C:
            raise ValueError('%s: run %d has %d contrasts, run 0 has %d' % (who, r, c.shape[0], C))
        if limits and (P > PMAX or C > CMAX):
            raise ValueError('%s: run %d has P = %d design columns and C = %d contrasts; served: P <= %d, C <= %d'
                             % (who, r, P, C, PMAX, CMAX))
        k, Q, B = _factor(X)
        if T <= k:
            raise ValueError('%s: run %d has T = %d rows and a design of rank %d: no residual degrees of freedom' % (who, r, T, k))
        if limits and k > KMAX:
            raise ValueError('%s: the design of run %d has rank %d; served: up to %d' % (who, r, k, KMAX))
        proj = Q.T @ X                                          # X^+ X c = V_k V_k^T c = B (Q^T X) c
        for i in range(C):
            miss = np.linalg.norm(c[i] - B @ (proj @ c[i]))
            if miss > ESTIMABLE_TOL * np.linalg.norm(c[i]) or not np.linalg.norm(c[i]) > 0:
                raise ValueError('%s: contrast %d is not estimable in run %d (its part outside the row space of the design: %.3g '
                                 'of its norm)' % (who, i, r, miss / max(np.linalg.norm(c[i]), 1e-300)))
        u = c @ B                                               # [C, k]
        tables.append(_Run(T, X, c, k, Q, B, u, (u * u).sum(axis=1)))
    return _Plan(runs, tables, M, C, keys, members, tensors)


# ---- the host restatement -------------------------------------------------------------------------------------------------------

def _noise_args(noise, rho, who):
    if noise not in ('ols', 'ar1'):
        raise ValueError("%s: noise must be 'ols' or 'ar1', got %r" % (who, noise))
    if rho is None:
        return None
    if noise == 'ols':
        raise ValueError("%s: rho is the coefficient of noise='ar1'; noise='ols' takes none" % who)
    if isinstance(rho, (bool, np.bool_)) or not isinstance(rho, (int, float, np.integer, np.floating)) or not abs(float(rho)) < 1.0:
        raise ValueError('%s: rho must be None (estimated per vertex) or a number inside (-1, 1), got %r' % (who, rho))
    return float(rho)


def _contrast_factor(c, X):
    """``c pinv(X^T X) c`` per contrast, formed as ``|pinv(X)^T c|^2`` from the SVD of X itself.  ``pinv(X^T X)`` with the
    squared cutoff takes the null eigenvalues of a rank-deficient design (which the product leaves at ``eps |X|^2``, far above
    ``(max(T, P) eps)^2 |X|^2``) for real ones and returns any number, negative ones included."""
    g = c @ np.linalg.pinv(X, rcond=max(X.shape) * np.finfo(np.float64).eps)
    return (g * g).sum(axis=1)


def _host_rho(res, y, T, rank):
    """``sum r_t r_{t-1} / sum r_t^2`` of OLS residuals [T, M], clamped to ``+-RHO_MAX``; 0 where the residuals are the round-off
    of a vertex the design explains exactly (``rss < 4 (T + rank) 2^-53 y.y``, the floor of the kernels)."""
    rss = (res * res).sum(axis=0)
    lag = (res[1:] * res[:-1]).sum(axis=0)
    live = rss >= 4.0 * (T + rank) * 2.0 ** -53 * (y * y).sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        raw = np.where(live & (rss > 0), lag / np.where(rss > 0, rss, 1.0), 0.0)
    return np.clip(raw, -RHO_MAX, RHO_MAX), raw


def _host_gls(tb, y, rho):
    """Explicit AR(1) GLS of one run, one coefficient per vertex: the ``T x T`` covariance ``rho^|i-j| / (1 - rho^2)``, its
    Cholesky factor, X and y whitened by it, ``lstsq``, residuals formed, ``pinv`` for the contrasts.
    ``(b [P, M], rss [M], factor [C, M])``."""
    from scipy.linalg import cholesky, solve_triangular
    T, P = tb.X.shape
    eps = max(tb.X.shape) * np.finfo(np.float64).eps
    b, rss, factor = np.empty((P, y.shape[1])), np.empty(y.shape[1]), np.empty((tb.c.shape[0], y.shape[1]))
    lags = np.abs(np.arange(T)[:, None] - np.arange(T)[None, :])
    for value in np.unique(rho):
        cols = np.flatnonzero(rho == value)
        Lc = cholesky(value ** lags / (1.0 - value * value), lower=True)
        Xw = solve_triangular(Lc, tb.X, lower=True)
        yw = solve_triangular(Lc, y[:, cols], lower=True)
        bw = np.linalg.lstsq(Xw, yw, rcond=eps)[0]
        res = yw - Xw @ bw
        b[:, cols] = bw
        rss[cols] = (res * res).sum(axis=0)
        factor[:, cols] = _contrast_factor(tb.c, Xw)[:, None]
    return b, rss, factor


def first_level_host(runs, designs, contrasts=None, groups=None, betas=False, noise='ols', rho=None):
    """``first_level`` restated in float64 NumPy (no device), without the projection trick of the kernels.  Per run:
    ``b = lstsq(X, y)`` (minimum norm), the residuals formed explicitly, ``rss = sum res^2``, ``dof = T - rank(X)``,
    ``sigma^2 = rss / dof``; per contrast ``effect = c.b``, ``variance = sigma^2 c pinv(X^T X) c``, ``t = effect / sqrt(variance)``
    (0 where the variance is 0).  The runs of a group are combined as fixed effects: ``effect = mean_r effect_r``,
    ``variance = sum_r variance_r / R_g^2``, ``dof = sum_r dof_r``.  The series are rounded to float32 first, as staging does.
    Returns a ``GLMResult`` of float64 maps (betas float64 as well).

    ``noise='ar1'`` uses none of the kernels' algebra either: the OLS fit above, ``rho = sum r_t r_{t-1} / sum r_t^2`` of its
    residuals clamped to ``+-RHO_MAX`` (or the given ``rho``), then per vertex the explicit ``T x T`` covariance, its Cholesky
    factor, X and y whitened by it, ``lstsq``, residuals and ``pinv`` again.  Slow: meant for the sizes of the tests.  Returns a
    ``GLMResultAR1`` (``rho`` float64 [M] per run)."""
    who = 'first_level_host'
    rho = _noise_args(noise, rho, who)
    pl = _plan(runs, designs, contrasts, groups, who, limits=False)
    eff, var, dof, bs, rhos = [], [], [], [], []
    for y, tb in zip(pl.runs, pl.tables):
        y = _runs.host_array(y, who).astype(np.float64)
        b = np.linalg.lstsq(tb.X, y, rcond=max(tb.X.shape) * np.finfo(np.float64).eps)[0]
        res = y - tb.X @ b
        rss = (res * res).sum(axis=0)
        d = tb.T - tb.rank
        factor = _contrast_factor(tb.c, tb.X)[:, None]
        if noise == 'ar1':
            rhos.append(np.full(pl.M, rho) if rho is not None else _host_rho(res, y, tb.T, tb.rank)[0])
            b, rss, factor = _host_gls(tb, y, rhos[-1])
        eff.append(tb.c @ b)
        var.append((rss / d)[None, :] * factor)
        dof.append(d)
        bs.append(b)
    S = len(pl.keys)
    effect = np.empty((S, pl.C, pl.M))
    variance = np.empty((S, pl.C, pl.M))
    gdof = np.empty(S, np.int64)
    for g, mem in enumerate(pl.members):
        se, sv = np.zeros((pl.C, pl.M)), np.zeros((pl.C, pl.M))
        for r in mem:
            se, sv = se + eff[r], sv + var[r]
        effect[g] = se / len(mem)
        variance[g] = sv / (float(len(mem)) * float(len(mem)))
        gdof[g] = sum(dof[r] for r in mem)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(variance > 0, effect / np.sqrt(variance), 0.0)
    if noise == 'ar1':
        return GLMResultAR1(effect, variance, t, gdof, list(pl.keys), bs if betas else None, rhos)
    return GLMResult(effect, variance, t, gdof, list(pl.keys), bs if betas else None)


# ---- the device -----------------------------------------------------------------------------------------------------------------

def _batch_tables(tabs, C):
    """The tables of one batch of runs, padded with zero columns to its common k (and zero rows to its common P)."""
    k = max(max(tb.rank for tb in tabs), 1)
    P = max(tb.X.shape[1] for tb in tabs)
    Q = np.zeros((sum(tb.T for tb in tabs), k))
    U = np.zeros((len(tabs), C, k))
    B = np.zeros((len(tabs), P, k))
    o = 0
    for i, tb in enumerate(tabs):
        Q[o:o + tb.T, :tb.rank] = tb.Q
        U[i, :, :tb.rank] = tb.u
        B[i, :tb.X.shape[1], :tb.rank] = tb.B
        o += tb.T
    return Q, U, np.stack([tb.un2 for tb in tabs]), B, np.array([tb.rank for tb in tabs], np.int32)


def _ar1_tables(tabs, k):
    """The tables of the AR(1) fit of one batch, padded like ``_batch_tables``: ``W = [Q | Qs]`` [T, 2k] with row t of ``Qs`` =
    ``Q[t - 1] + Q[t + 1]`` (zero beyond the ends of the run), ``D = Q^T Qs`` and ``E = q_0 q_0^T + q_L q_L^T`` [n, k, k]."""
    W = np.zeros((sum(tb.T for tb in tabs), 2 * k))
    D = np.zeros((len(tabs), k, k))
    E = np.zeros((len(tabs), k, k))
    o = 0
    for i, tb in enumerate(tabs):
        Q, kr = tb.Q, tb.rank
        Qs = np.zeros_like(Q)
        Qs[1:] += Q[:-1]
        Qs[:-1] += Q[1:]
        W[o:o + tb.T, :kr] = Q
        W[o:o + tb.T, k:k + kr] = Qs
        d = Q.T @ Qs
        D[i, :kr, :kr] = 0.5 * (d + d.T)
        E[i, :kr, :kr] = np.outer(Q[0], Q[0]) + np.outer(Q[-1], Q[-1])
        o += tb.T
    return W, D, E


def _batch_arg(batch_runs, who):
    if batch_runs is not None and (isinstance(batch_runs, (bool, np.bool_)) or not isinstance(batch_runs, (int, np.integer))
                                   or batch_runs < 1):
        raise ValueError('%s: batch_runs must be an int >= 1 or None, got %r' % (who, batch_runs))


def first_level(runs, designs, contrasts=None, groups=None, device=None, betas=False, batch_runs=None, noise='ols', rho=None):
    """Per-subject activation maps of a general linear model, on the device: a ``GLMResult``.

    ``runs``: one ``[T, M]`` array or a list (any lengths, same M; NumPy arrays, or torch tensors such as
    ``Parcellation.reduce`` returns, which are staged where they lie).  They are staged as ``[Ttot, plane_stride(M)]`` float32
    planes with a device table of run offsets (``runs.stage``, as for ``connectivity_graph``).  ``designs``: one ``Design`` per run.
    ``contrasts``: ``[C, P]`` for every run (or one such array per run, when designs differ in width); default
    ``contrasts_one_vs_rest`` of each design.  ``groups``: one hashable key per run -- the subject; default one group; the
    runs of a group are combined as fixed effects (``effect`` the mean, ``variance = sum / R_g^2``, ``dof`` the sum).
    ``batch_runs``: runs of one pass of the kernels, which bounds the float64 workspace of ``(k + 1) Mp`` values per run
    (``(2 k + 2) Mp`` with ``noise='ar1'``); default from the free device memory.  The result does not depend on it, bit for bit.
    ``noise``: ``'ols'``, or ``'ar1'`` for the prewhitened fit of the module's docstring, which returns a ``GLMResultAR1``:
    the same fields and ``rho``, one float32 ``[M]`` map per run.  ``rho``: None estimates the coefficient per (run, vertex)
    from the OLS residuals (clamped to ``+-RHO_MAX``; 0 at a vertex constant in time), a number inside (-1, 1) applies it to
    every vertex of every run.  ``dof`` is ``sum (T_r - k_r)`` either way.

    Returns ``effect``, ``variance``, ``t`` float32 ``[S, C, M]`` (NumPy; torch tensors on the device if every run came as a
    tensor), ``dof`` int64 ``[S]``, ``groups`` and, with ``betas``, one float32 ``[P_r, M]`` per run (the minimum-norm
    solution where a design is rank deficient).  ``t`` is 0 where the variance is 0 (a vertex constant in time), never NaN.

    ``ValueError`` before any launch: non-finite series, ``T_r <= rank``, a contrast that is not estimable in a run
    (``|c - X^+ X c| > 1e-8 |c|``), design rows != run rows, mixed M, P, C or rank beyond what the kernels serve.

    Out of scope: bias correction of the estimated rho, AR orders above 1, rho smoothed across vertices, temporal derivatives
    of the HRF, precision-weighted fixed effects, residual series."""
    who = 'first_level'
    rho = _noise_args(noise, rho, who)
    ar1 = noise == 'ar1'
    pl = _plan(runs, designs, contrasts, groups, who)
    _batch_arg(batch_runs, who)
    if len(pl.keys) > RMAX:
        raise ValueError('%s: %d groups; served: up to %d' % (who, len(pl.keys), RMAX))
    import torch
    from . import _lib, ops
    R, M, C = len(pl.runs), pl.M, pl.C
    Mp = _lib.plane_stride(M)
    dev, planes = _runs.stage(pl.runs, M, device, who)
    with torch.cuda.device(dev):
        kmax = max(tb.rank for tb in pl.tables)
        batch_runs = _runs.batch_size(batch_runs, R, RMAX, 8 * ((2 * kmax + 2) if ar1 else (kmax + 1)) * Mp, dev)
        e64 = torch.empty((R, C, Mp), dtype=torch.float64, device=dev)
        v64 = torch.empty((R, C, Mp), dtype=torch.float64, device=dev)
        beta_out, rho_out = [], []
        for r0, r1, rows, o in _runs.batches(planes, _runs.offsets(pl.runs), batch_runs):
            Q, U, un2, B, rank = (torch.as_tensor(a).to(dev) for a in _batch_tables(pl.tables[r0:r1], C))
            if ar1:
                W, D, E = (torch.as_tensor(a).to(dev) for a in _ar1_tables(pl.tables[r0:r1], int(Q.shape[1])))
                ah, s0, s1 = ops.glm_project_ar1(rows, o, M, W)
                beta, rmap = ops.glm_finish_ar1(ah, s0, s1, rows, W, o, rank, D, E, U, M, rho=rho, B=B if betas else None,
                                                out64=(e64[r0:r1], v64[r0:r1]))[3:]
                rho_out += [rmap[i, :M] for i in range(r1 - r0)]
            else:
                a, yy = ops.glm_project(rows, o, M, Q)
                beta = ops.glm_finish(a, yy, o, rows.shape[0], rank, U, un2, M, B=B if betas else None,
                                      out64=(e64[r0:r1], v64[r0:r1]))[3]
            if betas:
                beta_out += [beta[i, :tb.X.shape[1], :M] for i, tb in enumerate(pl.tables[r0:r1])]
        gptr = np.concatenate([[0], np.cumsum([len(m) for m in pl.members])]).astype(np.int32)
        gruns = np.concatenate([np.asarray(m, np.int32) for m in pl.members])
        effect, variance, t = ops.glm_combine(e64, v64, torch.as_tensor(gptr).to(dev), torch.as_tensor(gruns).to(dev), M)
        dof = np.array([sum(pl.tables[r].T - pl.tables[r].rank for r in m) for m in pl.members], np.int64)
        if pl.tensors:
            res = GLMResult(effect, variance, t, dof, list(pl.keys), [b.contiguous() for b in beta_out] if betas else None)
            return GLMResultAR1(*res, [x.contiguous() for x in rho_out]) if ar1 else res
        res = GLMResult(effect.cpu().numpy(), variance.cpu().numpy(), t.cpu().numpy(), dof, list(pl.keys),
                        [b.cpu().numpy() for b in beta_out] if betas else None)
        return GLMResultAR1(*res, [x.cpu().numpy() for x in rho_out]) if ar1 else res


# ---- single-trial patterns: least squares - separate ----------------------------------------------------------------------------

G1MAX, NMAX = 16, 4096                          # chebgcn_glm_trials_query(2), (4)

TrialDesign = collections.namedtuple('TrialDesign', 'X trials onsets nuisance columns conditions')
TrialDesign.__doc__ = """What ``trial_design`` returns: ``X`` float64 [T, n], one HRF regressor per trial in order of onset;
``trials`` int64 [n], the trial's condition as an index into ``conditions``; ``onsets`` float64 [n], seconds; ``nuisance`` float64
[T, q]: drifts, confounds, intercept last -- the non-condition columns of ``design_matrix``; ``columns`` the n + q column names
(``<condition>_<i>`` for the i-th trial of a condition, then the nuisance names); ``conditions`` the condition names in class
order."""


class TrialResult(collections.namedtuple('TrialResult', 'beta variance t labels run trial onset group dof classes')):
    """What ``single_trial`` returns.  ``beta``, ``variance``, ``t``: float32 [Ntrials, M] in run order then trial order (float64
    from ``single_trial_host``), None for what ``outputs`` does not name; per trial ``labels`` (the condition name), ``run``,
    ``trial`` (its index inside the run), ``onset`` (seconds), ``group`` (the run's key) and ``dof`` (int64, the residual degrees
    of freedom of the trial's model); ``classes`` the condition names in class order."""
    __slots__ = ()

    def folds(self, within=True):
        """One fold per trial, that of its run by ``searchlight.default_folds``: the run's position among the runs of its group
        (``within``), or its group's index in order of first appearance."""
        from .searchlight import default_folds
        first = np.flatnonzero(np.concatenate([[True], self.run[1:] != self.run[:-1]]))
        per_run = default_folds([self.group[i] for i in first], within)
        return per_run[np.searchsorted(self.run[first], self.run)]


def trial_design(names=None, events=None, T=None, tr=0.72, conditions=None, hrf='spm', high_pass=1.0 / 128, confounds=None):
    """The single-trial design of one run: a ``TrialDesign``.  The arguments and their checks are those of ``design_matrix``.
    Every block of a kept condition is one trial, in order of onset: with ``names`` a maximal stretch of equal names, with
    ``events`` one ``(onset, duration, name)`` tuple.  A trial's regressor is the closed-form response to its own block; the
    trial columns of a condition sum to ``design_matrix``'s column of that condition, and ``nuisance`` is its other columns."""
    try:
        T, tr, hrf, blocks, conditions, order, confounds = _design_args(names, events, T, tr, conditions, hrf, high_pass, confounds)
    except ValueError as e:
        raise ValueError(str(e).replace('design_matrix:', 'trial_design:', 1)) from None
    kept = sorted((b for b in blocks if b[2] in conditions), key=lambda b: b[0])       # (stable: ties keep the given order)
    t = np.arange(T, dtype=np.float64) * tr
    X = np.zeros((T, len(kept)))
    for i, (on, off, name) in enumerate(kept):
        X[:, i] = step_response(t - on, hrf) - step_response(t - off, hrf)
    codes = np.array([conditions.index(b[2]) for b in kept], np.int64)
    N, nuisance = _nuisance(T, order, confounds)
    seen = collections.Counter()
    cols = []
    for c in codes:
        cols.append('%s_%d' % (conditions[c], seen[c]))
        seen[c] += 1
    return TrialDesign(X, codes, np.array([b[0] for b in kept], np.float64), N, cols + nuisance, list(conditions))


_Trials = collections.namedtuple('_Trials', 'T n X N codes own q Qn ZX ZS keep rank w F onsets')
_TrialPlan = collections.namedtuple('_TrialPlan', 'runs tables M G classes groups outputs tensors')


def _others(tb, j, G):
    """The explicit ``others`` columns of trial j of a run: ``[T, G]``, column g the sum of the trials of group g other than j."""
    O = np.zeros((tb.T, G))
    for i in range(tb.n):
        if i != j:
            O[:, tb.own[i]] += tb.X[:, i]
    return O


def _trial_plan(runs, designs, others, outputs, groups, who, limits=True):
    """Everything of ``single_trial`` that can be checked without the series' values, and the per-run tables of the kernels."""
    runs, _, M, tensors = _runs.as_runs(runs, who)
    if isinstance(designs, TrialDesign):
        designs = [designs]
    designs = list(designs)
    R = len(runs)
    if len(designs) != R or not all(isinstance(d, TrialDesign) for d in designs):
        raise ValueError('%s: designs must hold one TrialDesign per run (%d runs, %d designs)' % (who, R, len(designs)))
    if others not in ('condition', 'pooled'):
        raise ValueError("%s: others must be 'condition' or 'pooled', got %r" % (who, others))
    if isinstance(outputs, str):
        outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or set(outputs) - {'beta', 'variance', 't'}:
        raise ValueError("%s: outputs must name some of 'beta', 'variance', 't', got %r" % (who, outputs))
    groups = _runs.group_keys(groups, R, who)[0]
    classes = list(designs[0].conditions)
    if any(list(d.conditions) != classes for d in designs):
        raise ValueError('%s: the designs differ in their conditions; build them with the same conditions=' % who)
    G = len(classes) if others == 'condition' else 1
    if limits and 1 + G > G1MAX:
        raise ValueError("%s: %d conditions; served: up to %d with others='condition' (others='pooled' takes any number)"
                         % (who, G, G1MAX - 1))
    eps = np.finfo(np.float64).eps
    tables = []
    for r, (y, d) in enumerate(zip(runs, designs)):
        X, N, codes = np.asarray(d.X, np.float64), np.asarray(d.nuisance, np.float64), np.asarray(d.trials)
        T = int(y.shape[0])
        if X.ndim != 2 or N.ndim != 2 or not np.isfinite(X).all() or not np.isfinite(N).all():
            raise ValueError('%s: the design of run %d must hold finite [T, n] trial and [T, q] nuisance columns' % (who, r))
        if X.shape[0] != T or N.shape[0] != T:
            raise ValueError('%s: the design of run %d has %d rows, the run %d' % (who, r, X.shape[0], T))
        n = int(X.shape[1])
        if n < 1:
            raise ValueError('%s: run %d has no trials' % (who, r))
        if codes.shape != (n,) or codes.dtype.kind not in 'iu' or (codes < 0).any() or (codes >= len(classes)).any():
            raise ValueError('%s: trials of run %d must be [n = %d] condition indices below %d' % (who, r, n, len(classes)))
        if limits and n > NMAX:
            raise ValueError('%s: run %d has %d trials; served: up to %d' % (who, r, n, NMAX))
        q, Qn = _factor(N)[:2] if N.shape[1] else (0, np.zeros((T, 0)))
        if limits and q + G > KMAX:
            raise ValueError('%s: run %d has nuisance rank %d and %d sums of other trials; served: q + G <= %d' % (who, r, q, G, KMAX))
        own = codes.astype(np.int64) if others == 'condition' else np.zeros(n, np.int64)
        ZX = X - Qn @ (Qn.T @ X)
        ZS = np.zeros((T, G))
        count = np.zeros(G, np.int64)
        for j in range(n):                                      # (so that a condition of one trial has that trial's very column)
            ZS[:, own[j]] += ZX[:, j]
            count[own[j]] += 1
        keep = np.zeros((n, 1 + G), bool)
        rank = np.zeros(n, np.int32)
        w = np.zeros((n, 1 + G))
        F = np.zeros((n, 1 + G, 1 + G))
        for j in range(n):
            A = np.concatenate([ZX[:, j:j + 1], ZS], axis=1)
            A[:, 1 + own[j]] -= ZX[:, j]
            keep[j, 0] = True
            keep[j, 1:] = count - (np.arange(G) == own[j]) > 0      # a column that is identically zero is dropped
            idx = np.flatnonzero(keep[j])
            A = A[:, idx]
            xn = np.linalg.norm(X[:, j])
            part = A[:, 0] - A[:, 1:] @ np.linalg.lstsq(A[:, 1:], A[:, 0], rcond=max(A.shape) * eps)[0] if idx.size > 1 else A[:, 0]
            if not xn > 0 or np.linalg.norm(part) <= ESTIMABLE_TOL * xn:
                raise ValueError('%s: trial %d of run %d is not estimable (the part of its regressor outside its other trials and '
                                 'the nuisance columns: %.3g of its norm)' % (who, j, r, np.linalg.norm(part) / max(xn, 1e-300)))
            S, Vt = np.linalg.svd(A, full_matrices=False)[1:]
            rj = int((S > max(A.shape) * eps * S[0]).sum())
            if T <= q + rj:
                raise ValueError('%s: run %d has T = %d rows and trial %d a model of rank %d: no residual degrees of freedom'
                                 % (who, r, T, j, q + rj))
            Fk = Vt[:rj] / S[:rj, None]
            F[j][:rj, idx] = Fk
            w[j, idx] = Fk[:, 0] @ Fk
            rank[j] = rj
        tables.append(_Trials(T, n, X, N, codes, own, q, Qn, ZX, ZS, keep, rank, w, F, np.asarray(d.onsets, np.float64)))
    return _TrialPlan(runs, tables, M, G, classes, groups, outputs, tensors)


def _trial_result(pl, maps, dof):
    tabs = pl.tables
    return TrialResult(maps.get('beta'), maps.get('variance'), maps.get('t'),
                       np.array([pl.classes[c] for tb in tabs for c in tb.codes]),
                       np.concatenate([np.full(tb.n, r, np.int64) for r, tb in enumerate(tabs)]),
                       np.concatenate([np.arange(tb.n, dtype=np.int64) for tb in tabs]),
                       np.concatenate([tb.onsets for tb in tabs]),
                       [pl.groups[r] for r, tb in enumerate(tabs) for _ in range(tb.n)], np.asarray(dof, np.int64), list(pl.classes))


def single_trial_host(runs, designs, others='condition', outputs=('beta', 't'), groups=None, device=None, batch_runs=None):
    """``single_trial`` restated in float64 NumPy (no device; ``device`` and ``batch_runs`` are accepted and ignored), with none
    of the kernels' algebra: per trial the explicit design ``[x_j | others | N]`` (an ``others`` column that is identically zero
    left out), ``lstsq``, the residuals formed, the rank by SVD, ``pinv(D^T D)[0, 0]`` for the variance factor.  The series are
    rounded to float32 first, as staging does.  Returns a ``TrialResult`` of float64 maps."""
    who = 'single_trial_host'
    pl = _trial_plan(runs, designs, others, outputs, groups, who, limits=False)
    beta, var, dof = [], [], []
    for y, tb in zip(pl.runs, pl.tables):
        y = _runs.host_array(y, who).astype(np.float64)
        for j in range(tb.n):
            O = _others(tb, j, pl.G)
            D = np.concatenate([tb.X[:, j:j + 1], O[:, tb.keep[j, 1:]], tb.N], axis=1)
            eps = max(D.shape) * np.finfo(np.float64).eps
            b = np.linalg.lstsq(D, y, rcond=eps)[0]
            res = y - D @ b
            d = tb.T - int(np.linalg.matrix_rank(D))
            f = np.linalg.pinv(D.T @ D, rcond=eps ** 2, hermitian=True)[0, 0]
            beta.append(b[0])
            var.append((res * res).sum(axis=0) / d * f)
            dof.append(d)
    beta, var = np.stack(beta), np.stack(var)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(var > 0, beta / np.sqrt(var), 0.0)
    maps = {k: v for k, v in (('beta', beta), ('variance', var), ('t', t)) if k in pl.outputs}
    return _trial_result(pl, maps, dof)


def _trial_tables(tabs, G):
    """The tables of one batch of runs: ``Q = [Qn | Z_S | 0]`` [Tb, k] for ``glm_project``, ``Z`` [Tb, nmax], the trial offsets,
    ``q_rank`` and the flat per-trial tables."""
    k = max(tb.q for tb in tabs) + G
    nmax = max(tb.n for tb in tabs)
    Tb = sum(tb.T for tb in tabs)
    Q, Z = np.zeros((Tb, k)), np.zeros((Tb, nmax))
    o = 0
    for tb in tabs:
        Q[o:o + tb.T, :tb.q] = tb.Qn
        Q[o:o + tb.T, tb.q:tb.q + G] = tb.ZS
        Z[o:o + tb.T, :tb.n] = tb.ZX
        o += tb.T
    toffs = np.concatenate([[0], np.cumsum([tb.n for tb in tabs])]).astype(np.int64)
    return (Q, Z, toffs, np.array([tb.q for tb in tabs], np.int32), np.concatenate([tb.own for tb in tabs]).astype(np.int32),
            np.concatenate([tb.rank for tb in tabs]).astype(np.int32), np.concatenate([tb.w for tb in tabs]),
            np.concatenate([tb.F for tb in tabs]))


def single_trial(runs, designs, others='condition', outputs=('beta', 't'), groups=None, device=None, batch_runs=None):
    """Single-trial patterns (a beta series) by "least squares - separate" (Mumford et al. 2012), on the device: a ``TrialResult``.

    One GLM per trial j of a run: ``[x_j | o_j1 .. o_jG | N]`` -- the trial's own HRF regressor, the other trials lumped into one
    regressor per condition (``others='condition'``: ``o_jg`` the sum of the trials of condition g without ``x_j``, G the number of
    conditions) or into one regressor overall (``'pooled'``, G = 1), and the nuisance columns.  The trial's pattern is the
    coefficient ``beta`` (or the ``t`` value) of ``x_j``: with short trials a few seconds apart the responses of neighbouring
    trials overlap, and a mean over the trial's rows (``searchlight_events``) mixes them and keeps drift and confounds.  An
    ``others`` column that is identically zero (a condition whose only trial is j) is dropped; the model's rank and dof follow.

    ``runs``, ``groups``, ``device``, ``batch_runs`` as ``first_level`` takes them (tensors are staged where they lie and the maps
    then stay on the device; the result does not depend on ``batch_runs``, bit for bit); ``designs``: one ``TrialDesign`` per run,
    all with the same conditions; ``outputs``: which of ``'beta'``, ``'variance'``, ``'t'`` to form, the rest are None.  Maps are
    float32 ``[Ntrials, M]`` in run order then trial order, so that
    ``searchlight(res.beta, res.labels, nb, res.folds(), groups=res.group)`` and ``crossnobis`` take them as they are.

    The models of a run differ by one column swap, so one pass serves them all.  With ``Qn`` an orthonormal basis of N (rank q),
    ``S`` the G sums of the trial columns and ``Z = (I - Qn Qn^T) [X | S]``: ``an = Qn^T y``, ``c = Z_S^T y`` and ``y.y`` come from
    chebgcn_glm_project over ``[Qn | Z_S]``, and chebgcn_glm_trials forms ``p_j = z_j^T y`` and finishes every trial where its
    projection lies: ``d = (p_j, c_g - [g = own_j] p_j)``, ``beta = w_j . d``, ``rss = y.y - an.an - |F_j d|^2``,
    ``variance = rss / (T - q - r_j) * w_j0`` with the vertex-independent ``H_j = D_j^T (I - Qn Qn^T) D_j``, ``w_j`` the first row
    of its pseudo-inverse, ``r_j`` its rank and ``F_j^T F_j = H_j^+``.  float64 on the device, rounded once: include/chebgcn.h.

    ``ValueError`` before any launch: non-finite series, design rows != run rows, a run without trials, a trial that is not
    estimable (the part of ``x_j`` outside the span of its others and the nuisance ``<= 1e-8 |x_j|``, e.g. an onset beyond the
    run), ``T <= rank``, more than 15 conditions with ``others='condition'``, ``q + G > 64``, more than 4096 trials in a run.

    Out of scope: LSA (all trials in one design; up to 64 columns that is ``first_level(betas=True)`` on ``[X | N]``), AR(1)
    noise, temporal derivatives of the HRF, and any change to ``searchlight_events`` / ``crossnobis_events``."""
    who = 'single_trial'
    pl = _trial_plan(runs, designs, others, outputs, groups, who)
    _batch_arg(batch_runs, who)
    import torch
    from . import _lib, ops
    R, M, G = len(pl.runs), pl.M, pl.G
    Mp = _lib.plane_stride(M)
    dev, planes = _runs.stage(pl.runs, M, device, who)
    with torch.cuda.device(dev):
        batch_runs = _runs.batch_size(batch_runs, R, RMAX, 8 * (max(tb.q for tb in pl.tables) + G + 1) * Mp, dev)
        parts = []
        for r0, r1, rows, o in _runs.batches(planes, _runs.offsets(pl.runs), batch_runs):
            Q, Z, toffs, qrank, own, rank, w, F = (torch.as_tensor(a).to(dev) for a in _trial_tables(pl.tables[r0:r1], G))
            a, yy = ops.glm_project(rows, o, M, Q)
            parts.append(ops.glm_trials(rows, o, M, Z, toffs, a, yy, qrank, own, rank, w, F, outputs=pl.outputs))
        maps = {}
        for i, name in enumerate(('beta', 'variance', 't')):
            if name in pl.outputs:
                full = torch.cat([p[i][:, :M] for p in parts]).contiguous()
                maps[name] = full if pl.tensors else full.cpu().numpy()
    dof = np.concatenate([tb.T - tb.q - tb.rank.astype(np.int64) for tb in pl.tables])
    return _trial_result(pl, maps, dof)
