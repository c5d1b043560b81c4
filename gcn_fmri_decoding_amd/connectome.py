"""Functional connectivity matrices per run, on the device: the shrunk covariance of a run's regions, its correlation, its
inverse (the precision) and the partial correlation -- what nilearn's ``ConnectivityMeasure`` gives on its default estimator,
scikit-learn's ``LedoitWolf`` -- from one staged copy of the scans, in float64, rounded once (chebgcn_connectome_*,
include/chebgcn.h).  The reference builds two of its three brain graphs from such matrices (model.py:93-134);
``graph.connectivity_graph(kind='partial correlation')`` sits on top of this module.

``connectome`` runs the kernels; ``connectome_host`` is the NumPy yardstick, which deliberately uses none of their algebra
(the centred product by ``@``, the inverse by ``numpy.linalg.inv``).

``tangent`` is nilearn's ``ConnectivityMeasure(kind='tangent')``: the geometric mean G of the runs' shrunk covariances and the
tangent matrices ``log(G^-1/2 Sigma_s G^-1/2)``, on a batched Jacobi eigensolver (chebgcn_sym_*); ``tangent_host``
is its yardstick on ``numpy.linalg.eigh``; ``eigh`` is the solver alone.

Host-only at import: NumPy and the constants of ``_lib`` (which loads the library only when asked); torch is imported by the
functions that need it.
"""
import collections
import numbers

import numpy as np

from . import _lib, runs as _runs

KINDS = _lib.CONNECTOME_KINDS          # 'covariance', 'correlation', 'precision', 'partial correlation'

Connectome = collections.namedtuple('Connectome', 'matrices mean shrinkage degenerate kind')
Connectome.__doc__ = """What ``connectome`` / ``connectome_host`` return.

``matrices``   float32 [S, R, R], one matrix per run, each symmetric bit for bit (a device tensor from ``connectome``, NumPy from
               ``connectome_host``); the identity for a degenerate run
``mean``       float32 [R, R]: the float64 sum of the float32 matrices of the runs that are not degenerate, in ascending run order,
               divided by their number and rounded once; zeros when every run is degenerate (tensor / NumPy as ``matrices``)
``shrinkage``  float64 [S] NumPy: the shrinkage of every run (the Ledoit-Wolf estimate, or the number given)
``degenerate`` bool [S] NumPy: runs whose shrunk covariance has no Cholesky factor (precision kinds only)
``kind``       the kind asked for"""


def _check(kind, shrinkage, who):
    """``kind`` and ``shrinkage`` checked -> (the index of the kind, the shrinkage as the C entry takes it: negative for 'auto')."""
    if kind not in KINDS:
        raise ValueError('%s: unknown kind %r (one of %s; tangent-space connectivity is connectome.tangent)' % (
            who, kind, ', '.join(repr(k) for k in KINDS)))
    if isinstance(shrinkage, str):
        if shrinkage != 'auto':
            raise ValueError("%s: shrinkage must be 'auto' or a number in [0, 1], got %r" % (who, shrinkage))
        return KINDS.index(kind), -1.0
    if isinstance(shrinkage, (bool, np.bool_)) or not isinstance(shrinkage, (numbers.Real, np.floating, np.integer)):
        raise ValueError("%s: shrinkage must be 'auto' or a number in [0, 1], got %r" % (who, shrinkage))
    s = float(shrinkage)
    if not 0.0 <= s <= 1.0:                                     # (NaN fails both)
        raise ValueError('%s: shrinkage %r lies outside [0, 1]' % (who, shrinkage))
    return KINDS.index(kind), s


def _as_runs(runs, who, limit):
    if (isinstance(runs, np.ndarray) or _runs.is_tensor(runs)) and runs.ndim == 3:
        runs = list(runs)                                       # (a stack [S, T, R] is taken as S runs)
    runs, _, R, _ = _runs.as_runs(runs, who, min_rows=2, min_cols=1, width='runs differ in the number of regions (or have none)',
                                  rows='a run needs at least two time points')
    if limit is not None and R > limit:
        raise ValueError('%s: %d regions; at most %d are served (vertex-level precision matrices are a different, sparse problem)'
                         % (who, R, limit))
    return runs, R


def mean_of(matrices, degenerate):
    """The mean as ``Connectome.mean`` defines it, restated: a float64 sum of the float32 matrices of the runs that are not
    flagged, in ascending run order, divided by their number, rounded once; zeros where there is none."""
    matrices = np.asarray(matrices, np.float32)
    acc = np.zeros(matrices.shape[1:], np.float64)
    n = 0
    for m, d in zip(matrices, degenerate):
        if not d:
            acc = acc + m.astype(np.float64)
            n += 1
    return (acc / n).astype(np.float32) if n else np.zeros(matrices.shape[1:], np.float32)


def pivot_floor(R):
    """A Cholesky pivot of column j at or below ``pivot_floor(R) * Sigma_jj`` is the round-off of its own chain of up to R
    products, each bounded by Sigma_jj: the run is degenerate (include/chebgcn.h)."""
    return 4.0 * R * 2.0 ** -53


def host_run(x, kind, shrinkage):
    """One run on the host -> (matrix float64 [R, R], shrinkage, degenerate)."""
    x = x.astype(np.float64)
    T, R = x.shape
    d = x - x.sum(axis=0) / T
    C = (d.T @ d) / T
    C = (C + C.T) / 2                                            # (a BLAS product is symmetric only to rounding)
    if shrinkage < 0:
        q = (d * d).sum(axis=1)
        beta_ = (q * q).sum()
        delta_ = (C * C).sum()
        tr = np.trace(C)
        mu = tr / R
        beta = (beta_ / T - delta_) / (R * T)
        delta = (delta_ - 2.0 * mu * tr + R * mu * mu) / R
        s = max(min(beta, delta), 0.0) / delta if delta > 0 else 0.0
        s = s + 0.0                                              # (never a negative zero)
    else:
        s = shrinkage
    mu = np.trace(C) / R
    sigma = (1.0 - s) * C
    sigma[np.diag_indices(R)] += s * mu
    if kind == 'covariance':
        return sigma, s, False
    if kind == 'correlation':
        dd = np.outer(np.diag(sigma), np.diag(sigma))
        with np.errstate(divide='ignore', invalid='ignore'):
            out = np.where(dd > 0, sigma / np.sqrt(np.where(dd > 0, dd, 1.0)), 0.0)
        out[np.diag_indices(R)] = 1.0
        return out, s, False
    degenerate = not np.isfinite(sigma).all()
    if not degenerate:
        try:
            piv = np.diag(np.linalg.cholesky(sigma)) ** 2
            degenerate = not bool((np.isfinite(piv) & (piv > pivot_floor(R) * np.diag(sigma))).all())
        except np.linalg.LinAlgError:
            degenerate = True
    if degenerate:
        return np.eye(R), s, True
    P = np.linalg.inv(sigma)
    P = (P + P.T) / 2
    if kind == 'precision':
        return P, s, False
    out = -P / np.sqrt(np.outer(np.diag(P), np.diag(P)))
    out[np.diag_indices(R)] = 1.0
    return out, s, False


def connectome_host(runs, kind='correlation', shrinkage='auto'):
    """``connectome`` on the host in NumPy float64, as the yardstick of the kernels: the same definitions (include/chebgcn.h),
    none of their algebra.  Returns a ``Connectome`` of NumPy arrays."""
    who = 'connectome_host'
    _, s = _check(kind, shrinkage, who)
    runs, R = _as_runs(runs, who, None)
    host = [_runs.host_array(r, who, any_dtype=True) for r in runs]
    out = [host_run(x, kind, s) for x in host]
    matrices = np.stack([m for m, _, _ in out]).astype(np.float32)
    degenerate = np.array([g for _, _, g in out], bool)
    return Connectome(matrices, mean_of(matrices, degenerate), np.array([v for _, v, _ in out], np.float64), degenerate, kind)


def connectome(runs, kind='correlation', shrinkage='auto', device=None, batch_runs=None):
    """One connectivity matrix per run, on the device.

    ``runs``       one ``[T, R]`` run or a list of runs (any lengths >= 2, one width R <= ``chebgcn_connectome_query(0)`` = 512;
                   NumPy arrays, or torch tensors such as ``Parcellation.reduce`` returns, which are staged where they lie)
    ``kind``       'covariance', 'correlation', 'precision' or 'partial correlation'
    ``shrinkage``  'auto' (Ledoit-Wolf, scikit-learn's ``LedoitWolf``) or a number in [0, 1]; 0 is the empirical covariance
    ``batch_runs`` runs per pass of the kernels (default: what fits a quarter of the free device memory)

    Per run: the biased covariance C of the centred series, the shrinkage s, ``Sigma = (1 - s) C + s mu I`` with mu the mean of
    the diagonal of C; the correlation ``Sigma_ij / sqrt(Sigma_ii Sigma_jj)`` (diagonal exactly 1; a zero diagonal entry gives a
    row and column of zeros beside it); the precision ``Sigma^-1`` by Cholesky without pivoting; the partial correlation
    ``-P_ij / sqrt(P_ii P_jj)`` (diagonal exactly 1).  A run whose factorisation meets a pivot that is not above its round-off
    (a run constant in time, T = 2, no shrinkage with T <= R or a constant region) is DEGENERATE for the two precision kinds:
    flagged, its matrix the identity, left out of the mean; nothing raises and no NaN comes out of finite input.

    Everything is float64 from the float32 samples to the one rounding of each output.  Results are bit-identical under any
    ``batch_runs``, for a run alone or among others, from call to call, and between NumPy and tensor input.  Bad arguments and
    non-finite host arrays raise ``ValueError`` before the device is touched.  Returns a ``Connectome``."""
    who = 'connectome'
    ikind, s = _check(kind, shrinkage, who)
    if batch_runs is not None and (isinstance(batch_runs, (bool, np.bool_)) or not isinstance(batch_runs, (int, np.integer))
                                   or batch_runs < 1):
        raise ValueError('%s: batch_runs must be an int >= 1, got %r' % (who, batch_runs))
    limit = int(_lib.lib().chebgcn_connectome_query(0))
    runs, R = _as_runs(runs, who, limit)
    dev, planes = _runs.stage(runs, R, device, who, any_dtype=True)
    import torch
    from . import ops
    S = len(runs)
    offs = _runs.offsets(runs)
    with torch.cuda.device(dev):
        run_bytes = int(_lib.lib().chebgcn_connectome_workspace(1, R))
        batch = _runs.batch_size(batch_runs, S, int(_lib.lib().chebgcn_connectome_query(1)), run_bytes, dev)
        matrices = torch.empty((S, R, R), dtype=torch.float32, device=dev)
        shrunk = torch.empty((S,), dtype=torch.float64, device=dev)
        flags = torch.empty((S,), dtype=torch.int32, device=dev)
        for r0, r1, rows, o in _runs.batches(planes, offs, batch):
            ws = ops.connectome_cov(rows, o, R)
            ops.connectome_finish(ws, o, int(rows.shape[0]), R, ikind, s, matrices[r0:r1], shrunk[r0:r1], flags[r0:r1])
        mean = ops.connectome_mean(matrices, flags)
        return Connectome(matrices, mean, shrunk.cpu().numpy(), flags.cpu().numpy() != 0, kind)


# ---- tangent space ----------------------------------------------------------------------------------------------------------------

Tangent = collections.namedtuple('Tangent', 'matrices mean whitening reference shrinkage degenerate iterations norms steps '
                                            'converged sweeps eig_converged')
Tangent.__doc__ = """What ``tangent`` / ``tangent_host`` return.

``matrices``      float32 [S, R, R]: ``log(W Sigma_s W)`` per run, symmetric bit for bit; zeros for a degenerate run (a device
                  tensor from ``tangent``, NumPy from ``tangent_host``, as ``mean`` and ``whitening``)
``mean``          float32 [R, R]: the geometric mean G of the usable runs' shrunk covariances (nilearn's ``mean_``)
``whitening``     float32 [R, R]: ``W = G^-1/2``
``reference``     float64 [R, R] NumPy: G before its rounding; ``tangent(other_runs, reference=...)`` maps onto it
``shrinkage``     float64 [S] NumPy
``degenerate``    bool [S] NumPy: runs whose Sigma has an eigenvalue that is not above ``4 R 2^-53`` of its largest (or not finite)
``iterations``    iterations of the geometric mean that ran (0 with ``reference=`` or without a usable run)
``norms``         float64 NumPy: ``||mean_s log B_s||_F / R^2`` of every iteration
``steps``         float64 NumPy: the step every iteration moved G with
``converged``     whether the last norm fell below ``tol`` (True with ``reference=``; False without a usable run)
``sweeps``        the most sweeps any eigendecomposition took (0 on the host)
``eig_converged`` whether every eigendecomposition ended before the cap of sweeps (True on the host)"""


def degenerate_floor(R):
    """A run is degenerate when the smallest eigenvalue of its Sigma is not above ``degenerate_floor(R)`` times the largest."""
    return 4.0 * R * 2.0 ** -53


def _check_tangent(shrinkage, max_iter, tol, batch_runs, who):
    _, s = _check('covariance', shrinkage, who)
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError('%s: max_iter must be an int >= 1, got %r' % (who, max_iter))
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (numbers.Real, np.floating, np.integer)) or not (
            0.0 <= float(tol) < np.inf):
        raise ValueError('%s: tol must be a finite number >= 0, got %r' % (who, tol))
    if batch_runs is not None and (isinstance(batch_runs, (bool, np.bool_)) or not isinstance(batch_runs, (int, np.integer))
                                   or batch_runs < 1):
        raise ValueError('%s: batch_runs must be an int >= 1, got %r' % (who, batch_runs))
    return s, int(max_iter), float(tol)


def _check_reference(reference, R, who):
    """``reference=`` as a float64 [R, R] array: symmetric, finite and positive definite, or ``ValueError``."""
    if reference is None:
        return None
    G = reference.detach().cpu().numpy() if _runs.is_tensor(reference) else np.asarray(reference)
    if G.dtype.kind not in 'fiu' or G.shape != (R, R):
        raise ValueError('%s: reference must be a real [%d, %d] matrix, got %s %r' % (who, R, R, G.dtype, G.shape))
    G = np.ascontiguousarray(G, np.float64)
    if not np.isfinite(G).all() or not np.array_equal(G, G.T):
        raise ValueError('%s: reference must be finite and symmetric' % who)
    try:
        np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        raise ValueError('%s: reference is not positive definite' % who) from None
    return G


def _sym_fun_host(A, f):
    """``V f(Lambda) V^T`` by ``numpy.linalg.eigh`` and ``@``, symmetrised."""
    w, V = np.linalg.eigh(A)
    out = (V * f(w)) @ V.T
    return (out + out.T) / 2


def _congruence_host(W, A):
    out = W @ A @ W
    return (out + out.T) / 2


def geometric_mean_host(sigmas, max_iter=30, tol=1e-7):
    """The geometric mean of SPD matrices by nilearn's rule (``_geometric_mean``), restated ->
    ``(G, iterations, norms / R^2, steps, converged)``."""
    R = sigmas[0].shape[0]
    G = np.zeros((R, R))
    for sig in sigmas:                                          # (ascending, as the device sums)
        G = G + sig
    G = G / len(sigmas)
    step, norm_old = 1.0, np.inf
    norms, steps, converged = [], [], False
    for _ in range(max_iter):
        W = _sym_fun_host(G, lambda w: 1.0 / np.sqrt(w))
        H = _sym_fun_host(G, np.sqrt)
        M = np.zeros((R, R))
        for sig in sigmas:
            M = M + _sym_fun_host(_congruence_host(W, sig), np.log)
        M = M / len(sigmas)
        norm = float(np.sqrt((M * M).sum()))
        norms.append(norm / R ** 2)
        steps.append(step)
        G = _congruence_host(H, _sym_fun_host(M, lambda w: np.exp(step * w)))
        if norm < norm_old:
            norm_old = norm
        elif norm > norm_old:
            step = step / 2.0
            norm = norm_old
        if norm / R ** 2 < tol:
            converged = True
            break
    return G, len(norms), np.array(norms), np.array(steps), converged


def tangent_host(runs, shrinkage='auto', max_iter=30, tol=1e-7, reference=None):
    """``tangent`` on the host in NumPy float64 with ``numpy.linalg.eigh`` and ``@``: the same definitions, none of the device's
    algebra.  Returns a ``Tangent`` of NumPy arrays."""
    who = 'tangent_host'
    s, max_iter, tol = _check_tangent(shrinkage, max_iter, tol, None, who)
    runs, R = _as_runs(runs, who, None)
    G = _check_reference(reference, R, who)
    host = [_runs.host_array(r, who, any_dtype=True) for r in runs]
    out = [host_run(x, 'covariance', s) for x in host]
    sigmas = [m for m, _, _ in out]
    degenerate = np.zeros(len(runs), bool)
    for r, sig in enumerate(sigmas):
        ev = np.linalg.eigvalsh(sig) if np.isfinite(sig).all() else np.array([np.nan])
        degenerate[r] = not (np.isfinite(ev).all() and ev.min() > degenerate_floor(R) * ev.max())
    usable = [sig for sig, d in zip(sigmas, degenerate) if not d]
    iterations, norms, steps, converged = 0, np.zeros(0), np.zeros(0), G is not None
    if G is None:
        if usable:
            G, iterations, norms, steps, converged = geometric_mean_host(usable, max_iter, tol)
        else:
            G = np.eye(R)
    W = _sym_fun_host(G, lambda w: 1.0 / np.sqrt(w))
    matrices = np.zeros((len(runs), R, R), np.float32)
    for r, sig in enumerate(sigmas):
        if not degenerate[r]:
            matrices[r] = _sym_fun_host(_congruence_host(W, sig), np.log).astype(np.float32)
    return Tangent(matrices, G.astype(np.float32), W.astype(np.float32), G, np.array([v for _, v, _ in out], np.float64), degenerate,
                   iterations, norms, steps, converged, 0, True)


def eigh(matrices, device=None):
    """Eigendecompositions of symmetric float64 matrices ``[S, R, R]`` (NumPy or a tensor; R <= 512) on the device, by the block
    Jacobi method of chebgcn_sym_eigh -> ``(w [S, R] ascending, V [S, R, R] with the eigenvectors in its columns, sweeps int32
    [S] NumPy)``, ``w`` and ``V`` device tensors.  The matrices must be symmetric bit for bit and finite (``ValueError``); a matrix
    still rotating after the cap of sweeps raises ``ChebgcnError``."""
    who = 'eigh'
    tensor = _runs.is_tensor(matrices)
    m = matrices if tensor else np.asarray(matrices)
    if m.ndim != 3 or m.shape[1] != m.shape[2] or m.shape[0] < 1 or m.shape[1] < 1 or str(m.dtype).split('.')[-1] != 'float64':
        raise ValueError('%s: matrices must be float64 [S, R, R], got %s %r' % (who, m.dtype, tuple(m.shape)))
    limit = int(_lib.lib().chebgcn_tangent_query(0))
    if m.shape[1] > limit:
        raise ValueError('%s: %d rows; at most %d are served' % (who, m.shape[1], limit))
    if not tensor and not (np.isfinite(m).all() and np.array_equal(m, m.transpose(0, 2, 1))):
        raise ValueError('%s: matrices must be finite and symmetric' % who)
    import torch
    from . import ops
    dev = _runs.cuda_device(device, m if tensor else None)
    m = (m.detach() if tensor else torch.as_tensor(np.ascontiguousarray(m))).to(dev).contiguous()
    with torch.cuda.device(dev):
        if tensor and not bool((torch.isfinite(m) & (m == m.transpose(1, 2))).all()):
            raise ValueError('%s: matrices must be finite and symmetric' % who)
        S, R = int(m.shape[0]), int(m.shape[1])
        step = int(_lib.lib().chebgcn_tangent_query(1))
        w = torch.empty((S, R), dtype=torch.float64, device=dev)
        V = torch.empty((S, R, R), dtype=torch.float64, device=dev)
        sweeps = np.zeros(S, np.int32)
        for s0 in range(0, S, step):
            ws, Vt, sw, ok = ops.sym_eigh(m[s0:s0 + step])
            if not bool(ok.all()):
                raise _lib.ChebgcnError('%s: a matrix is still rotating after %d sweeps' % (who, int(sw.max())))
            ws, order = torch.sort(ws, dim=1)
            w[s0:s0 + step] = ws
            V[s0:s0 + step] = torch.gather(Vt, 1, order[:, :, None].expand(-1, -1, R)).transpose(1, 2)
            sweeps[s0:s0 + step] = sw.cpu().numpy()
        return w, V, sweeps


def tangent(runs, shrinkage='auto', max_iter=30, tol=1e-7, reference=None, device=None, batch_runs=None):
    """Tangent-space connectivity on the device: nilearn's ``ConnectivityMeasure(kind='tangent')``.

    ``runs``       as ``connectome`` takes them (R <= 512)
    ``shrinkage``  'auto' (Ledoit-Wolf) or a number in [0, 1]
    ``max_iter``   iterations of the geometric mean at most (an int >= 1)
    ``tol``        the mean stops when ``||mean_s log B_s||_F / R^2 < tol`` (a finite number >= 0; 0 runs every iteration)
    ``reference``  a fitted mean G (``Tangent.reference``): no iteration, the runs are mapped onto it (nilearn's ``transform``)
    ``batch_runs`` runs per pass of the solver (default: what fits a quarter of the free device memory); the float64 Sigma of
                   ALL runs stays resident, ``8 S R^2`` bytes

    Per run ``Sigma_s`` is the shrunk covariance of ``connectome`` kept in float64.  G starts at the arithmetic mean and moves by
    nilearn's rule: ``W = G^-1/2``, ``M = mean_s log(W Sigma_s W)``, ``G <- G^1/2 exp(step M) G^1/2``, the step halved when the norm
    of M grows.  The outputs are ``W`` of the last G and ``log(W Sigma_s W)``.  A run whose Sigma is singular to round-off
    (constant in time; no shrinkage with T <= R) is DEGENERATE: flagged, its matrix zeros, left out of every mean; with no usable
    run ``mean`` and ``whitening`` are the identity.  Nothing raises and no NaN comes out of finite input.

    Everything is float64 up to the one rounding of each output; every sum has one order (include/chebgcn.h), the means run over
    the runs in ascending order.  So results are bit-identical under any ``batch_runs``, from call to call and between NumPy and
    tensor input; with ``reference=`` also for a run alone or among others, in any run order; without it a permuted run order
    gives the permuted result to rounding only.  Bad arguments and non-finite host arrays raise ``ValueError`` before the device
    is touched.  Returns a ``Tangent``."""
    who = 'tangent'
    s, max_iter, tol = _check_tangent(shrinkage, max_iter, tol, batch_runs, who)
    limit = int(_lib.lib().chebgcn_connectome_query(0))
    runs, R = _as_runs(runs, who, limit)
    Gref = _check_reference(reference, R, who)
    dev, planes = _runs.stage(runs, R, device, who, any_dtype=True)
    import torch
    from . import ops
    S = len(runs)
    offs = _runs.offsets(runs)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        run_bytes = int(lib.chebgcn_connectome_workspace(1, R)) + 6 * 8 * R * R
        batch = _runs.batch_size(batch_runs, S, min(int(lib.chebgcn_connectome_query(1)), int(lib.chebgcn_tangent_query(1))),
                                 run_bytes, dev)
        sigma = torch.empty((S, R, R), dtype=torch.float64, device=dev)
        shrunk = torch.empty((S,), dtype=torch.float64, device=dev)
        flags = torch.empty((S,), dtype=torch.int32, device=dev)
        spans, counts, oks = [], [], []

        def solve(m):
            w, Vt, sw, ok = ops.sym_eigh(m)
            counts.append(sw.max())
            oks.append(ok.min())
            return w, Vt

        floor = degenerate_floor(R)
        for r0, r1, rows, o in _runs.batches(planes, offs, batch):
            spans.append((r0, r1))
            ws = ops.connectome_cov(rows, o, R)
            ops.connectome_sigma(ws, o, int(rows.shape[0]), R, s, sigma[r0:r1], shrunk[r0:r1])
            w, _ = solve(sigma[r0:r1])
            good = torch.isfinite(w).all(dim=1) & (w.min(dim=1).values > floor * w.max(dim=1).values)
            flags[r0:r1] = (~good).to(torch.int32)
        degenerate = flags.cpu().numpy() != 0
        usable = int((~degenerate).sum())
        eye = torch.eye(R, dtype=torch.float64, device=dev)
        acc = torch.empty((R, R), dtype=torch.float64, device=dev)

        def mean_of_batches(make):
            """mean and norm of ``make(r0, r1)`` over the usable runs, the chain running through the batches in order."""
            for b, (r0, r1) in enumerate(spans):
                out = ops.sym_mean(make(r0, r1), flags[r0:r1], acc, first=b == 0, n_total=usable if b == len(spans) - 1 else 0)
            return out

        def logs(W, r0, r1, float32=False, out=None):
            w, Vt = solve(ops.sym_congruence(W, sigma[r0:r1]))
            return ops.sym_function(w, Vt, 'log', flags=flags[r0:r1].clone(), float32=float32, out=out)[0]

        def powers(G, *funcs):
            w, Vt = solve(G[None])
            return [ops.sym_function(w, Vt, func)[0][0] for func in funcs]

        norms, steps, converged = [], [], Gref is not None
        if Gref is not None:
            G = torch.as_tensor(Gref).to(dev)
        elif usable == 0:
            G = eye
        else:
            G = mean_of_batches(lambda r0, r1: sigma[r0:r1])[0]
            step, norm_old = 1.0, np.inf
            for _ in range(max_iter):
                W, H = powers(G, 'rsqrt', 'sqrt')
                M, norm = mean_of_batches(lambda r0, r1: logs(W, r0, r1))
                norm = float(norm.cpu()[0])                     # the one readback of an iteration: the rule below runs on the host
                norms.append(norm / R ** 2)
                steps.append(step)
                w, Vt = solve(M[None])
                G = ops.sym_congruence(H, ops.sym_function(w, Vt, 'exp', a=step)[0])[0]
                if norm < norm_old:
                    norm_old = norm
                elif norm > norm_old:
                    step = step / 2.0
                    norm = norm_old
                if norm / R ** 2 < tol:
                    converged = True
                    break
        W = eye if Gref is None and usable == 0 else powers(G, 'rsqrt')[0]
        matrices = torch.empty((S, R, R), dtype=torch.float32, device=dev)
        for r0, r1 in spans:
            logs(W, r0, r1, float32=True, out=matrices[r0:r1])
        return Tangent(matrices, G.to(torch.float32), W.to(torch.float32), G.cpu().numpy(), shrunk.cpu().numpy(), degenerate,
                       len(norms), np.array(norms, np.float64), np.array(steps, np.float64), converged,
                       int(torch.stack(counts).max()), bool(torch.stack(oks).min() != 0))
