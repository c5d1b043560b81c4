"""Spatial filters on the brain graph: ``y = h(L) x`` for scalar functions ``h`` on the spectrum of a graph Laplacian -- heat-kernel
smoothing along the mesh, spectral graph wavelets, band decompositions -- applied to scans ``[T, M]`` or attribution maps
``[classes, M]`` on the device.

``h(L) x`` is approximated by ``sum_{k<K} c_k T_k(L~) x`` with the Chebyshev coefficients ``c_k`` of ``h`` on ``[0, lmax]`` and
``L~ = L * (2 / lmax) - I``: the recurrence of the conv layers with FIXED coefficients (``chebgcn_cheb_filter``).  Nothing is
learned and no eigendecomposition is taken.  ``cheb_order`` picks K from the tail of the coefficients, which is a bound on the
truncation error: ``|h(lambda) - sum_{k<K} c_k T_k| <= sum_{k>=K} |c_k|`` on the whole interval.

The host-only parts (coefficients, orders, ``GraphFilter.apply_host``) need NumPy and SciPy only.
"""
import numpy as np
import scipy.sparse as sp

from . import graph as _graph
from .runs import cuda_device, is_tensor

KMAX = 256                      # terms of a filter at most (chebgcn_cheb_filter)
JMAX = 8                        # filters of one launch; more are applied in groups
CHUNK_BYTES = 256 << 20         # a slice of host rows on the device, and the scratch of one launch, at most
ROWS_MAX = 65535                # rows of one launch of the layout kernels
ORDER_MIN = 1024                # relabel='auto': graphs above this many vertices are tried on the ordered kernels (as cgcnn does)


def heat(t):
    """``exp(-t lambda)``: the heat kernel, diffusion for time t (smoothing; larger t is smoother)."""
    t = float(t)

    def h(lam):
        return np.exp(-t * lam)
    h.__name__ = 'heat(%g)' % t
    return h


def mexican_hat(s):
    """``s lambda exp(-s lambda)``: the Mexican-hat wavelet at scale s (a band around ``lambda = 1 / s``)."""
    s = float(s)

    def h(lam):
        return s * lam * np.exp(-s * lam)
    h.__name__ = 'mexican_hat(%g)' % s
    return h


def _callables(h):
    single = callable(h)
    hs = [h] if single else list(h)
    if not hs or not all(callable(f) for f in hs):
        raise ValueError('h must be a callable or a non-empty list of callables')
    return hs, single


def cheb_coefficients(h, K, lmax=2.0):
    """The first K Chebyshev coefficients of ``h`` on ``[0, lmax]``, float64 ``[K]`` (``[J, K]`` for a list of J callables):
    ``h(lmax/2 (1 + t)) ~ sum_k c_k T_k(t)`` on ``t in [-1, 1]``, by Chebyshev-Gauss quadrature on ``max(4K, 256)`` nodes
    (``c_0`` halved).  ``h`` is called with a float64 array of eigenvalues and returns an array of the same shape."""
    hs, single = _callables(h)
    K = int(K)
    if K < 1:
        raise ValueError('K = %d: at least one term' % K)
    if not lmax > 0:
        raise ValueError('lmax = %r must be positive' % (lmax,))
    N = max(4 * K, 256)
    theta = np.pi * (np.arange(N) + 0.5) / N
    lam = 0.5 * float(lmax) * (1.0 + np.cos(theta))
    basis = np.cos(np.arange(K)[:, None] * theta[None, :])          # [K, N]
    out = np.empty((len(hs), K), np.float64)
    for j, f in enumerate(hs):
        v = np.broadcast_to(np.asarray(f(lam), np.float64), lam.shape)
        out[j] = (2.0 / N) * (basis @ v)
    out[:, 0] *= 0.5
    return out[0] if single else out


def cheb_order(h, tol, lmax=2.0, kmax=KMAX):
    """The smallest K whose coefficient tail ``sum_{k>=K} |c_k|``, taken over ``kmax`` coefficients, is at most ``tol`` (for a
    list of callables: for every one of them).  The tail bounds the truncation error of the filter on the whole spectrum.
    ``ValueError`` if even ``kmax - 1`` terms leave more than ``tol``."""
    hs, _ = _callables(h)
    kmax = int(kmax)
    if kmax < 2:
        raise ValueError('kmax = %d: at least 2' % kmax)
    c = np.abs(cheb_coefficients(hs, kmax, lmax))                  # [J, kmax]
    tail = np.concatenate([np.cumsum(c[:, ::-1], axis=1)[:, ::-1], np.zeros((len(hs), 1))], axis=1).max(axis=0)   # tail[K], K <= kmax
    ok = np.nonzero(tail[1:kmax] <= tol)[0]
    if ok.size == 0:
        raise ValueError('cheb_order: kmax = %d terms leave a tail of %.3g, above tol = %g' % (kmax, tail[kmax - 1], tol))
    return int(ok[0]) + 1


class GraphFilter:
    """``h(L)`` as a Chebyshev filter of K terms on the device.

    ``L``: symmetric SciPy Laplacian ``[M, M]`` with its spectrum in ``[0, lmax]`` (``graph.laplacian(W, normalized=True)`` with
    the default ``lmax = 2``; a combinatorial one with ``lmax = graph.lmax(L, normalized=False)``).  ``h``: one callable or a list
    of J callables (``heat``, ``mexican_hat``, anything that maps an array of eigenvalues to an array); K defaults to
    ``cheb_order(h, tol, lmax)``.  Or ``coeffs``: ``[K]`` / ``[J, K]`` Chebyshev coefficients on ``[0, lmax]`` given directly.
    ``relabel='auto'``: a graph in the range the library's ordered recurrence kernels serve is relabelled by
    ``graph.length_order`` internally; input and output stay in the caller's vertex order.  ``relabel=None``: never.

    Attributes: ``M``, ``K``, ``J``, ``single`` (one callable or a ``[K]`` vector: results have no filter axis), ``coeffs``
    (float64 ``[J, K]``), ``lmax``.  Bad arguments raise ``ValueError`` before the device is touched; the device graph is built by
    the first ``apply``."""

    def __init__(self, L, h=None, K=None, coeffs=None, tol=1e-6, lmax=2.0, relabel='auto', device=None):
        if not sp.issparse(L):
            L = sp.csr_matrix(np.asarray(L))
        if L.ndim != 2 or L.shape[0] != L.shape[1] or L.shape[0] < 1:
            raise ValueError('GraphFilter: L must be square, got shape %r' % (tuple(L.shape),))
        L = sp.csr_matrix(L)
        if not np.isfinite(L.data).all():
            raise ValueError('GraphFilter: L holds non-finite values')
        scale = float(np.abs(L.data).max()) if L.nnz else 0.0
        asym = abs(L - L.T)
        if asym.nnz and float(asym.max()) > 1e-6 * scale:
            raise ValueError('GraphFilter: L must be symmetric (max |L - L^T| = %.3g)' % float(asym.max()))
        if not lmax > 0:
            raise ValueError('GraphFilter: lmax = %r must be positive' % (lmax,))
        if relabel not in ('auto', None):
            raise ValueError("GraphFilter: relabel must be 'auto' or None, not %r" % (relabel,))
        if (h is None) == (coeffs is None):
            raise ValueError('GraphFilter: give either h or coeffs')
        self.M = int(L.shape[0])
        self.lmax = float(lmax)
        if coeffs is not None:
            c = np.asarray(coeffs, np.float64)
            if c.ndim not in (1, 2) or c.size == 0:
                raise ValueError('GraphFilter: coeffs must be [K] or [J, K], got shape %r' % (c.shape,))
            self.single = c.ndim == 1
            c = np.atleast_2d(c)
            if K is not None and int(K) != c.shape[1]:
                raise ValueError('GraphFilter: K = %d but coeffs hold %d terms' % (int(K), c.shape[1]))
            K = c.shape[1]
        else:
            hs, self.single = _callables(h)
            K = cheb_order(hs, tol, lmax) if K is None else int(K)
        if K < 1 or K > KMAX:
            raise ValueError('GraphFilter: K = %d terms, served: 1 .. %d' % (K, KMAX))
        if coeffs is None:
            c = cheb_coefficients(hs, K, lmax)
        if not np.isfinite(c).all():
            raise ValueError('GraphFilter: %s non-finite (NaN or infinite) values' %
                             ('coeffs hold' if coeffs is not None else 'the coefficients of h hold'))
        self.coeffs = c
        self.J, self.K = int(c.shape[0]), int(c.shape[1])
        self.relabel = relabel
        self.device = device
        # what ops.Graph rescales with lmax = 2, as always: L * (2 / lmax) has its spectrum in [0, 2]
        self._Ls = L if self.lmax == 2.0 else sp.csr_matrix(L * (2.0 / self.lmax))
        self._dev = None                # (graph, order table or None, coefficient table) once built

    # ---- the float64 restatement ---------------------------------------------------------------------------------------------------
    def _runs(self, series):
        single = (isinstance(series, np.ndarray) or is_tensor(series)) and series.ndim == 2
        runs = [series] if single else list(series)
        if not runs:
            raise ValueError('GraphFilter: series holds no runs')
        for r in runs:
            if not (isinstance(r, np.ndarray) or is_tensor(r)):
                raise ValueError('GraphFilter: series must be NumPy arrays or torch tensors, not %s' % type(r).__name__)
            if r.ndim != 2 or r.shape[1] != self.M:
                raise ValueError('GraphFilter: series must be [rows, %d] (M = L.shape[0]), got shape %r' % (self.M, tuple(r.shape)))
            if is_tensor(r):
                if str(r.dtype) == 'torch.float64':
                    raise ValueError('GraphFilter: series is a float64 tensor; the filter runs in float32 -- pass series.float()')
            elif not (np.issubdtype(r.dtype, np.number) or r.dtype == bool):
                raise ValueError('GraphFilter: series of dtype %s' % r.dtype)
        return runs, single

    def apply_host(self, series):
        """``apply`` restated in float64 on the host: SciPy sparse products with the float32-rounded entries of ``L~``
        (``graph.rescaled_laplacian_csr``) and the float32-rounded coefficients, on the float32-rounded input, summed in ascending
        k.  What the device computes, without its round-off.  float64 ``[R, M]`` (``[J, R, M]`` for a list of callables)."""
        runs, single = self._runs(series)
        indptr, indices, data = _graph.rescaled_laplacian_csr(self._Ls)
        Lt = sp.csr_matrix((data.astype(np.float64), indices, indptr), shape=(self.M, self.M))
        c = self.coeffs.astype(np.float32).astype(np.float64)
        out = []
        for r in runs:
            x = r.detach().cpu().numpy() if is_tensor(r) else np.asarray(r)
            prev, cur = None, x.astype(np.float32).astype(np.float64).T           # T_{k-2}, T_{k-1}: [M, R]
            y = c[:, 0, None, None] * cur[None]
            for k in range(1, self.K):
                prev, cur = cur, (Lt @ cur if k == 1 else 2.0 * (Lt @ cur) - prev)
                y = y + c[:, k, None, None] * cur[None]
            y = np.ascontiguousarray(y.transpose(0, 2, 1))
            out.append(y[0] if self.single else y)
        return out[0] if single else out

    # ---- the device -----------------------------------------------------------------------------------------------------------------
    def _tables(self, dev):
        import torch
        from . import ops
        if self._dev is None or self._dev[0].device != dev:
            g = order = None
            if self.relabel == 'auto' and self.M > ORDER_MIN:
                order = _graph.length_order(self._Ls)
                g = ops.Graph(self._Ls, dev, order=order)
                if not g.ordered:
                    g = order = None                                # no ordered kernel for this graph: nothing to gain
            if g is None:
                g = ops.Graph(self._Ls, dev)
            table = None if order is None else torch.as_tensor(order.astype(np.int32)).to(dev)
            coeff = torch.as_tensor(self.coeffs.astype(np.float32)).to(dev)
            self._dev = (g, table, coeff)
        return self._dev

    def apply(self, series, chunk_rows=None, arm=0, out=None):
        """One ``[R, M]`` NumPy array or device tensor (a scan, or ``[classes, M]`` maps), or a list of them -> contiguous float32
        device tensors ``[R, M]`` (``[J, R, M]`` for a list of callables), a list for a list.

        Rows go through the device ``chunk_rows`` at a time (default: as many as keep the launch's scratch and a slice of host
        rows inside 256 MiB each); a host run is uploaded slice by slice, so it never exists on the device as a whole.  ``arm``:
        0 automatic, 1 rolling, 2 stack (``chebgcn_cheb_filter``).  ``out``: for a single run, a float32 device tensor of the
        result's shape with contiguous rows (any row stride) to write into.  In the rolling arm the result of a row does not
        depend on ``chunk_rows`` or on the rows beside it: bit-identical."""
        runs, single = self._runs(series)
        if chunk_rows is not None and (int(chunk_rows) != chunk_rows or chunk_rows < 1):
            raise ValueError('GraphFilter: chunk_rows = %r' % (chunk_rows,))
        if arm not in (0, 1, 2):
            raise ValueError('GraphFilter: arm = %r (0 automatic, 1 rolling, 2 stack)' % (arm,))
        if out is not None and not single:
            raise ValueError('GraphFilter: out is for a single run')
        import torch
        from . import ops
        dev = cuda_device(self.device, next((r for r in runs if is_tensor(r) and r.is_cuda), None))
        res = []
        with torch.cuda.device(dev):
            g, order, coeff = self._tables(dev)
            Jg = min(self.J, JMAX)
            per_row = max(ops.cheb_filter_workspace(g, 1, self.K, Jg, arm), 4 * g.Mp * (1 + Jg))
            rows = int(chunk_rows) if chunk_rows is not None else max(1, CHUNK_BYTES // per_row)
            rows = min(rows, ROWS_MAX)
            for r in runs:
                R = int(r.shape[0])
                shape = (R, self.M) if self.single else (self.J, R, self.M)
                if out is None:
                    y = torch.empty(shape, dtype=torch.float32, device=dev)
                else:
                    y = out
                    if (not is_tensor(y) or not y.is_cuda or y.dtype != torch.float32 or tuple(y.shape) != shape
                            or (self.M > 1 and y.stride(-1) != 1)):
                        raise ValueError('GraphFilter: out must be a float32 device tensor %r with contiguous rows' % (shape,))
                yj = y[None] if self.single else y
                for r0 in range(0, R, rows):
                    piece = r[r0:r0 + rows]
                    if is_tensor(piece):
                        x = piece.to(torch.float32).contiguous().to(dev)
                    else:
                        x = torch.as_tensor(np.ascontiguousarray(piece, dtype=np.float32)).to(dev)
                    n = int(x.shape[0])
                    planes = ops.rows_to_planes(x, self.M, 1, order)                 # [n, 1, Mp], internal order
                    for j0 in range(0, self.J, JMAX):
                        f = ops.cheb_filter(g, planes, coeff[j0:j0 + JMAX], arm=arm)  # [Jg, n, 1, Mp]
                        for j in range(f.shape[0]):
                            ops.planes_to_rows(f[j], self.M, order, out=yj[j0 + j, r0:r0 + n])
                res.append(y)
        return res[0] if single else res


def smooth(series, L, t, tol=1e-6, **kw):
    """Heat-kernel smoothing along the graph: ``GraphFilter(L, heat(t), tol=tol).apply(series)``.  ``chunk_rows``, ``arm`` and
    ``out`` go to ``apply``, every other keyword to ``GraphFilter``."""
    how = {k: kw.pop(k) for k in ('chunk_rows', 'arm', 'out') if k in kw}
    return GraphFilter(L, heat(t), tol=tol, **kw).apply(series, **how)
