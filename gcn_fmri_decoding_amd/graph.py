"""Graph construction on the host: drop-in for the parts of ``lib_new/graph.py`` that
feed the Chebyshev hot path (reference citations are to that file).

These run once per model build on NumPy/SciPy, like the reference; the results (CSR
Laplacians) are uploaded to the GPU by ``ops.Graph``; ``fourier`` gives the dense basis
of the spectral filters (``cgcnn`` with ``filter='fourier'`` / ``'spline'``).  Out of scope
here and absent on purpose: ``plot_spectrum`` and the dense NumPy recurrence ``chebyshev``
(the GPU kernel replaces it).

The one stage that does run on the device is the neighbour search: ``knn_device`` and ``connectivity_graph`` (chebgcn_knn)
return the same ``[N, k]`` tables as ``distance_sklearn_metrics`` without the N x N matrix; ``adjacency`` (N k work) stays here.
``connectivity_graph(kind='partial correlation')`` takes its mean matrix from ``connectome`` (chebgcn_connectome_*) and its
neighbours from ``knn_from_similarity``.
"""
import numpy as np
import scipy.sparse as sp

from . import runs as _runs


def distance_sklearn_metrics(z, k=4, metric='euclidean'):
    """Exact k nearest neighbours from the full distance matrix (graph.py:9-17).

    Returns (d, idx): the k smallest non-self distances per row, ascending, and the
    matching column indices.
    """
    import sklearn.metrics
    d = sklearn.metrics.pairwise.pairwise_distances(z, metric=metric, n_jobs=-2)
    idx = np.argsort(d)[:, 1:k + 1]
    d.sort()
    return d[:, 1:k + 1], idx


def adjacency(dist, idx):
    """Gaussian-weighted, symmetrised kNN adjacency (graph.py:19-45).

    w_ij = exp(-d_ij^2 / sigma^2) with sigma = mean distance to the k-th neighbour;
    an undirected edge keeps the larger of the two directed weights.
    """
    M, k = dist.shape
    if idx.shape != (M, k):
        raise ValueError('dist and idx shapes differ')
    if dist.min() < 0:
        raise ValueError('negative distance')
    sigma2 = np.mean(dist[:, -1]) ** 2
    w = np.exp(-dist ** 2 / sigma2)
    rows = np.arange(0, M).repeat(k)
    W = sp.coo_matrix((w.reshape(M * k), (rows, idx.reshape(M * k))), shape=(M, M))
    W.setdiag(0)
    flip = W.T > W
    W = W - W.multiply(flip) + W.T.multiply(flip)
    return sp.csr_matrix(W)


KNN_METRICS = ('euclidean', 'cosine', 'correlation')
KNN_KMAX = 32


def _knn_check(N, k):
    if int(k) != k or not 1 <= k <= KNN_KMAX:
        raise ValueError('k = %r: 1 <= k <= %d neighbours are served on the device' % (k, KNN_KMAX))
    if k >= N:
        raise ValueError('k = %d neighbours need more than %d vertices' % (k, N))


def knn_device(z, k=4, metric='euclidean', device=None):
    """``distance_sklearn_metrics`` on the device (chebgcn_knn), without the N x N matrix: ``z`` [N, D] features, ``metric``
    'euclidean', 'cosine' or 'correlation'.  Returns (d float32 [N, k] ascending, idx int64 [N, k]) on the host, ready for
    ``adjacency``.  Distances are computed in float64 from the float32 features and rounded once.

    Differences from the reference function, both only where distances tie: vertex i itself is excluded by index (the reference
    drops column 0 of the sorted row, which among coincident points may be another vertex), and equal distances order by
    lower index.  A zero row under 'cosine' / a constant row under 'correlation' is at distance 1 from everything (sklearn
    gives such rows distance 1 and NaN).  Bad arguments raise ``ValueError`` before the device is touched."""
    if metric not in KNN_METRICS:
        raise ValueError('knn_device: unknown metric %r (one of %s)' % (metric, ', '.join(KNN_METRICS)))
    z = np.asarray(z)
    if z.ndim != 2:
        raise ValueError('knn_device: z must be [N, D], got shape %r' % (z.shape,))
    N, D = z.shape
    if D < 1:
        raise ValueError('knn_device: no features')
    _knn_check(N, k)
    z = np.ascontiguousarray(z, dtype=np.float32)
    if not np.isfinite(z).all():
        raise ValueError('knn_device: z holds non-finite values')
    import torch
    from . import _lib, ops
    dev = _runs.cuda_device(device)
    planes = np.zeros((D, _lib.plane_stride(N)), np.float32)
    planes[:, :N] = z.T
    with torch.cuda.device(dev):
        d, idx = ops.knn(torch.as_tensor(planes).to(dev), N, int(k), KNN_METRICS.index(metric))
        return d.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def knn_from_similarity(matrix, k):
    """The k most similar other vertices of every vertex from an explicit ``[N, N]`` similarity matrix: ``(values [N, k] in the
    matrix's dtype, descending, idx int64 [N, k])``.  The rules of ``knn_device``: vertex i itself is excluded by index, whatever
    the diagonal holds, and equal values order by lower index.  On the host (N k work on a matrix of atlas size, like
    ``adjacency``); ``1 - values`` are distances for ``adjacency``."""
    matrix = np.asarray(matrix)
    if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1]:
        raise ValueError('knn_from_similarity: matrix must be [N, N], got shape %r' % (matrix.shape,))
    N = matrix.shape[0]
    if int(k) != k or k < 1:
        raise ValueError('knn_from_similarity: k = %r neighbours' % (k,))
    if k >= N:
        raise ValueError('knn_from_similarity: k = %d neighbours need more than %d vertices' % (k, N))
    if not np.isfinite(matrix).all():
        raise ValueError('knn_from_similarity: matrix holds non-finite values')
    key = -matrix.astype(np.float64)
    key[np.diag_indices(N)] = np.inf                             # self: last, whatever the diagonal holds
    idx = np.argsort(key, axis=1, kind='stable')[:, :int(k)].astype(np.int64)
    return np.take_along_axis(matrix, idx, axis=1), idx


def connectivity_graph(series, k=8, device=None, return_sigma=False, kind='correlation', shrinkage='auto'):
    """Neighbours by functional connectivity, from the scans themselves: ``series`` is one ``[T, M]`` run or a list of runs
    (any lengths >= 2, same M; NumPy arrays, or torch tensors such as ``Parcellation.reduce`` returns, which are staged on the
    device without a host round trip and give the same result as their ``.cpu().numpy()``).
    The runs are staged as ``[Ttot, Mp]`` planes in the caller's order, every run is centred and
    scaled per vertex on the device (chebgcn_series_normalise), and the kNN kernels run on the Gram matrix of the result, which
    is the mean over runs of the per-run Pearson correlation matrices r (never formed; a vertex constant in a run has
    correlation 0 with everything in that run).  Returns (d, idx) with ``d = 1 - r`` float32 [M, k] ascending and idx int64,
    as ``knn_device``; with ``return_sigma`` also the mean of the whole matrix r (diagonal included), the reference's kernel
    width for its RSFC graph (model.py:126).

    ``kind='partial correlation'`` takes the neighbours from the mean over runs of the per-run partial correlation matrices of
    the ``shrinkage``-shrunk covariance ('auto': Ledoit-Wolf) instead, the reference's structural-covariance graph
    (model.py:93-106): ``connectome.connectome`` forms the matrices on the device (at most 512 regions; runs without a Cholesky
    factor are left out of the mean), ``knn_from_similarity`` picks the neighbours of the mean matrix on the host.  ``d = 1 -
    mean`` and the optional third value, the mean of the whole mean matrix, are as above.  The reference's ``tanh`` and
    ``exp(. / sigma)`` steps are the caller's.  ``shrinkage`` has no meaning for the default kind.  The tangent-space graph of the
    reference's ``RSFC`` setting is built from ``connectome.tangent(...).mean`` (INTEGRATION has the recipe)."""
    who = 'connectivity_graph'
    if kind not in ('correlation', 'partial correlation'):
        raise ValueError("%s: kind must be 'correlation' or 'partial correlation', got %r (the tangent-space graph is built "
                         'from connectome.tangent)' % (who, kind))
    if kind == 'partial correlation':
        return _partial_graph(series, k, device, return_sigma, shrinkage)
    if (isinstance(series, np.ndarray) or _runs.is_tensor(series)) and series.ndim != 2:
        series = list(series)                                   # (a stack [R, T, M] is taken as R runs)
    runs, _, M, _ = _runs.as_runs(series, who, min_rows=2, min_cols=0, width='runs differ in the number of vertices',
                                  rows='a run needs at least two time points')
    _knn_check(M, k)
    dev, planes = _runs.stage(runs, M, device, who, any_dtype=True)
    import torch
    from . import _lib, ops
    with torch.cuda.device(dev):
        zn = ops.series_normalise(planes, torch.as_tensor(_runs.offsets(runs)).to(dev), M, scale=1.0 / np.sqrt(len(runs)))
        d, idx = ops.knn(zn, M, int(k), _lib.KNN_DOT)
        out = (d.cpu().numpy(), idx.cpu().numpy().astype(np.int64))
        if return_sigma:
            col = zn[:, :M].sum(dim=1, dtype=torch.float64)       # sum_ij r_ij = sum_t (sum_m zn[t][m])^2
            out += (float((col * col).sum().item()) / (M * M),)
    return out


def _partial_graph(series, k, device, return_sigma, shrinkage):
    """``connectivity_graph(kind='partial correlation')``."""
    from . import connectome as _connectome
    who = 'connectivity_graph'
    _connectome._check('partial correlation', shrinkage, who)
    if (isinstance(series, np.ndarray) or _runs.is_tensor(series)) and series.ndim != 2:
        series = list(series)
    runs, _, M, _ = _runs.as_runs(series, who, min_rows=2, min_cols=0, width='runs differ in the number of vertices',
                                  rows='a run needs at least two time points')
    _knn_check(M, k)
    mean = _connectome.connectome(runs, 'partial correlation', shrinkage, device=device).mean.cpu().numpy()
    sim, idx = knn_from_similarity(mean, int(k))
    out = (np.float32(1) - sim, idx)
    if return_sigma:
        out += (float(mean.astype(np.float64).sum()) / (M * M),)
    return out


def replace_random_edges(A, noise_level):
    """Swap a fraction of the edges for uniformly random unit edges (graph.py:48-76).

    Consumes the global NumPy RNG in the reference's order (permutation, two randint
    draws, one uniform draw) so that a seeded call reproduces its graph.
    """
    M = A.shape[0]
    n = int(noise_level * A.nnz // 2)
    victims = np.random.permutation(A.nnz // 2)[:n]
    new_r = np.random.randint(0, M, n)
    new_c = np.random.randint(0, M, n)
    np.random.uniform(0, 1, n)            # drawn and unused by the reference as well
    upper = sp.triu(A, format='coo')
    if upper.nnz < n:
        raise ValueError('not enough edges to replace')
    A = A.tolil()
    for e, r, c in zip(victims, new_r, new_c):
        i, j = upper.row[e], upper.col[e]
        A[i, j] = 0
        A[j, i] = 0
        A[r, c] = 1
        A[c, r] = 1
    A.setdiag(0)
    A = A.tocsr()
    A.eliminate_zeros()
    return A


def laplacian(W, normalized=True):
    """Combinatorial (D - W) or normalised (I - D^-1/2 W D^-1/2) Laplacian, CSR, in the
    dtype of W (graph.py:79-98).  Degrees are column sums plus ``spacing(0)``."""
    W = sp.csr_matrix(W)
    d = np.asarray(W.sum(axis=0)).ravel()
    if not normalized:
        return sp.csr_matrix(sp.diags(d, 0) - W)
    d = d + np.spacing(np.array(0, W.dtype))
    s = sp.diags((1 / np.sqrt(d)).astype(W.dtype, copy=False), 0)
    eye = sp.identity(d.size, dtype=W.dtype)
    return sp.csr_matrix(eye - (s * W) * s)


def lmax(L, normalized=True):
    """Upper bound of the spectrum (graph.py:101-107)."""
    if normalized:
        return 2
    import scipy.sparse.linalg
    return scipy.sparse.linalg.eigsh(L, k=1, which='LM', return_eigenvectors=False)[0]


def rescale_L(L, lmax=2):
    """Map the spectrum to [-1, 1]: L / (lmax/2) - I (graph.py:146-152).

    Unlike the reference this does not mutate its argument (its only caller passes a
    private copy, models_gcn.py:590-591).  Entries that cancel exactly are dropped.
    """
    L = sp.csr_matrix(L, copy=True)
    L.data *= 1.0 / (lmax / 2)
    return sp.csr_matrix(L - sp.identity(L.shape[0], format='csr', dtype=L.dtype))


def fourier(L, algo='eigh', k=1):
    """The graph Fourier basis: eigenvalues ascending and the eigenvectors as columns (graph.py:110-128).

    ``'eigh'`` (what the spectral filters use) and ``'eig'`` take the dense matrix, in its own dtype (a float32
    Laplacian gives a float32 decomposition); ``'eigs'`` / ``'eigsh'`` the ``k`` smallest-magnitude pairs of the sparse one.
    """
    def ascending(lamb, U):
        idx = lamb.argsort()
        return lamb[idx], U[:, idx]

    dense = L.toarray() if sp.issparse(L) else np.asarray(L)
    if algo == 'eigh':
        return np.linalg.eigh(dense)
    if algo == 'eig':
        return ascending(*np.linalg.eig(dense))
    import scipy.sparse.linalg
    if algo == 'eigs':
        return ascending(*scipy.sparse.linalg.eigs(L, k=k, which='SM'))
    if algo == 'eigsh':
        return scipy.sparse.linalg.eigsh(L, k=k, which='SM')
    raise ValueError('fourier: unknown algo %r' % (algo,))


def rescaled_laplacian_csr(L):
    """What ``chebyshev5`` hands to its sparse matmul (models_gcn.py:590-596): the
    rescaled Laplacian as float32 CSR with row-major, ascending-column entries
    (``tf.sparse_reorder``).  Returns (indptr int32, indices int32, data float32)."""
    Lr = rescale_L(sp.csr_matrix(L), lmax=2).astype(np.float32)
    Lr.sort_indices()
    return (Lr.indptr.astype(np.int32), Lr.indices.astype(np.int32), Lr.data.astype(np.float32))


def length_order(L):
    """Vertex order in which the library's recurrence kernels are fastest: rows of the rescaled Laplacian sorted by
    DESCENDING length (number of neighbours), ties in the caller's order (stable), so isolated vertices -- the fake
    vertices the coarsening adds -- come last.  ``order[i]`` = the caller's index of internal vertex ``i``.

    With ``Lp = permute(L, order)`` a quad of four consecutive vertices is four rows of (nearly) equal length: a
    16-byte piece of an activation plane is then exactly the rows one thread of the recurrence kernel owns, and planes
    go from HBM to registers and back without a pass through LDS (csrc/recurrence_ord.hip).  The network is invariant
    under a relabelling of the vertices as long as everything per-vertex follows it (input columns, per-vertex biases,
    the rows of the first FC layer; pooling needs the tree order of ``coarsening.compute_perm`` and is not relabelled):
    ``models_gcn.cgcnn`` does that behind the reference's variable layout."""
    indptr, _, _ = rescaled_laplacian_csr(L)
    lengths = np.diff(indptr)
    return np.argsort(-lengths.astype(np.int64), kind='stable').astype(np.int64)


def bank_order(L, sweeps=4, stats=None):
    """``length_order(L)`` refined inside its classes of equal row length so that the LDS reads of the ordered recurrence
    kernels' gather spread over the banks (``chebgcn_bank_order``, csrc/graph.hip: pairwise label swaps inside the gather's
    lane sets, host only, deterministic).  Still sorted by descending row length: everything said of ``length_order`` holds.
    ``stats``: a list that receives [fullest-bank sum before, after, swaps]."""
    import ctypes as C
    from . import _lib
    order = length_order(L)
    indptr, indices, _ = rescaled_laplacian_csr(permute(L, order))
    M = int(L.shape[0])
    perm = np.empty(M, np.int32)
    st = np.zeros(3, np.int64)
    _lib.check(_lib.lib().chebgcn_bank_order(M, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p), int(sweeps),
                                             perm.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)), 'bank_order')
    if stats is not None:
        stats[:] = [int(v) for v in st]
    return order[perm.astype(np.int64)]


def permute(L, order):
    """``P L P^T``: row / column ``i`` of the result is row / column ``order[i]`` of ``L`` (CSR, sorted indices)."""
    L = sp.csr_matrix(L)
    Lp = sp.csr_matrix(L[order][:, order])
    Lp.sort_indices()
    return Lp


def hop_balls(A, hops):
    """The boolean CSR pattern of ``(I + A)^hops`` with sorted indices: row v lists the vertices within ``hops`` edges of v, itself
    included (``hops = 0``: the identity).  The pattern of ``A`` is its non-zero entries, taken as given: an edge stored in one
    direction only is walked in that direction only.  On the host; the neighbourhoods ``searchlight`` takes."""
    if isinstance(hops, (bool, np.bool_)) or not isinstance(hops, (int, np.integer)) or hops < 0:
        raise ValueError('hop_balls: hops must be an int >= 0, got %r' % (hops,))
    if not sp.issparse(A) or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError('hop_balls: A must be a square SciPy sparse matrix')
    n = A.shape[0]
    step = sp.csr_matrix(A != 0, dtype=np.int32) + sp.identity(n, dtype=np.int32, format='csr')
    step.data[:] = 1
    balls = sp.identity(n, dtype=np.int32, format='csr')
    for _ in range(int(hops)):
        balls = sp.csr_matrix(balls @ step)
        balls.data[:] = 1                                       # a pattern: path counts would overflow
    balls = balls.astype(bool)
    balls.sort_indices()
    return balls


def synthetic_graph(n_nodes=10000, k=8, levels=1, noise_level=0.01, seed=0, dtype=np.float32, knn='host'):
    """The seeded synthetic "brain" graph of the benchmark: kNN
    graph on uniform points in the unit cube, 1 % random edges, ``levels`` rounds of
    coarsening, one normalised Laplacian per level.  Returns (laplacians, perm, graphs).
    ``knn='device'`` finds the neighbours with ``knn_device`` instead of the full distance matrix.
    """
    from . import coarsening
    z = np.random.RandomState(seed).rand(n_nodes, 3).astype(np.float32)
    if knn == 'host':
        d, idx = distance_sklearn_metrics(z, k=k, metric='euclidean')
    elif knn == 'device':
        d, idx = knn_device(z, k=k, metric='euclidean')
    else:
        raise ValueError("synthetic_graph: knn must be 'host' or 'device', not %r" % (knn,))
    A = adjacency(d, idx).astype(dtype)
    np.random.seed(seed)
    A = replace_random_edges(A, noise_level)
    graphs, perm = coarsening.coarsen(A, levels=levels, self_connections=False, verbose=False)
    return [laplacian(G, normalized=True) for G in graphs], perm, graphs
