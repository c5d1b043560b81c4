"""Functional connectivity matrices per run, on the device: the shrunk covariance of a run's regions, its correlation, its
inverse (the precision) and the partial correlation -- what nilearn's ``ConnectivityMeasure`` gives on its default estimator,
scikit-learn's ``LedoitWolf`` -- from one staged copy of the scans, in float64, rounded once (chebgcn_connectome_*,
include/chebgcn.h).  The reference builds two of its three brain graphs from such matrices (model.py:93-134);
``graph.connectivity_graph(kind='partial correlation')`` sits on top of this module.

``connectome`` runs the kernels; ``connectome_host`` is the NumPy yardstick, which deliberately uses none of their algebra
(the centred product by ``@``, the inverse by ``numpy.linalg.inv``).  ``kind='tangent'`` is out of scope: it needs symmetric
eigendecompositions of every matrix in every iteration of a geometric mean.

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
        raise ValueError('%s: unknown kind %r (one of %s; tangent-space connectivity is out of scope)' % (
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
