"""Permutation inference on maps: where does an effect hold across subjects, corrected for the number of vertices?

``map_test`` takes one map per subject (or fold, or run) -- attribution maps ``[S, classes, M]``, smoothed or not -- and tests the
group mean at every vertex with a sign-flip permutation test: under the null hypothesis a subject's map is as likely as its
negative, so every vector of S signs gives a map that is as likely as the observed one.  Family-wise error is controlled by the
maximum statistic: ``p[v]`` is the share of permutations whose LARGEST value anywhere reaches the observed value at ``v``.  The
statistic is the vertex-wise t (``'max'``), the extent of the vertex's cluster above a forming threshold (``'extent'``), or
threshold-free cluster enhancement (``'tfce'``, Smith & Nichols 2009) on the neighbourhood of the brain graph.

On the device (``chebgcn_signflip_t``, ``chebgcn_cluster_enhance``) the permutations run in batches; ``map_test_host`` restates
the same arithmetic with NumPy and SciPy, operation for operation: the two agree to the bit.  The stated arithmetic (see
include/chebgcn.h), per vertex and permutation in float64, every operation rounded on its own::

    s = sum_j sign_j x_j  (ascending j, from 0)      q = sum_j x_j x_j      m = s / S      d = q - s m
    t = float32(m / sqrt(d / (S (S - 1))))  where d > 0, else 0

A vertex is active at height h when ``t > float32(h)``.  TFCE: ``step`` defaults to the observed maximum / 100 and is the same
for every permutation; a map with maximum ``t_max`` has the heights ``h_i = i step``, ``i = 1 .. floor(t_max / step)``, and
``tfce[v] = sum_i extent_i(v)^E h_i^H step`` over the heights at which v is active, accumulated in float64 in DESCENDING i (the
kernels walk the heights downwards, where components only merge), each term ``ep[extent] * hw[i]`` a rounded product of the two
host-built tables ``ep[e] = e^E`` and ``hw[i] = h_i^H step``.  A cluster's id is its smallest vertex.

``design_test`` puts a general linear model across subjects under the same loop: one t contrast of a design ``[S, q]`` (two
groups, a covariate with nuisance regressors, paired conditions), the design permuted in the Freedman-Lane scheme (Winkler et
al. 2014).  Its t maps come from ``chebgcn_perm_glm_t``; ``perm_t_host`` restates that arithmetic and ``design_test_host`` the
whole test, bit for bit.

The host-only parts need NumPy and SciPy only.
"""
import collections

import numpy as np
import scipy.sparse as sp
from scipy.sparse import csgraph

from .runs import aug_draw, cuda_device, is_tensor

CHUNK_BYTES = 256 << 20         # the t maps and the labelling state of one batch of permutations on the device, at most
ARM = 0                         # chebgcn_cluster_enhance's arm: 0 automatic; 2 forces the streamed arm (measurements, tests)
HOST_CHUNK = 1 << 22            # (permutation, vertex) pairs of one slice of the host restatement
SMAX = 4096                     # subjects (chebgcn_signflip_t)
MMAX = 1 << 24                  # vertices
NHMAX = 1 << 16                 # heights of one map
PBMAX = 65535                   # permutations of one launch
STATS = ('max', 'extent', 'tfce')
_MODE = {'max': 0, 'extent': 1, 'tfce': 2}

MapTestResult = collections.namedtuple('MapTestResult', 't stat p null labels step n_perm exact seed')
MapTestResult.__doc__ = """What ``map_test`` returns.  ``t`` float32 [C, M] the observed t map (of the negated maps for
``tail=-1``); ``stat`` float64 [C, M] the observed statistic; ``p`` float64 [C, M] family-wise corrected p-values (>= 1 / n_perm);
``null`` float64 [C, P] every permutation's maximum; ``labels`` int32 [C, M] for ``'extent'`` (the cluster's smallest vertex, -1
below the threshold), else None; ``step`` the TFCE step per class (float64 [C], None for the other statistics); ``n_perm`` the
permutations actually run; ``exact`` whether they enumerate all sign vectors; ``seed``.  For ``[S, M]`` input the class axis is
dropped (``step`` a float)."""


def sign_flips(S, n_perm, seed):
    """The sign vectors ``map_test`` runs: ``(signs int8 [P, S] of +1 / -1, exact)``.  Row 0 is all +1 (the observed maps, which
    count as a permutation).  When ``2**S <= n_perm`` every sign vector is enumerated once: ``P = 2**S``, subject j of row q is
    negated where bit j of q is set, ``exact`` is True.  Otherwise ``P = n_perm`` and subject j of row q >= 1 is negated where the
    top bit of ``chebgcn_aug_draw(seed, refill=0, i=q, d=j)`` is set."""
    S, n_perm = int(S), int(n_perm)
    if S < 1 or n_perm < 1:
        raise ValueError('sign_flips: S = %d, n_perm = %d' % (S, n_perm))
    if S < 62 and (1 << S) <= n_perm:
        neg = (np.arange(1 << S, dtype=np.int64)[:, None] >> np.arange(S, dtype=np.int64)[None, :]) & 1
        return (1 - 2 * neg).astype(np.int8), True
    neg = aug_draw(seed, 0, np.arange(n_perm, dtype=np.uint64)[:, None], np.arange(S, dtype=np.uint64)[None, :]) >> np.uint64(31)
    neg = neg.astype(np.int64)
    neg[0] = 0
    return (1 - 2 * neg).astype(np.int8), False


def edges(A, M=None):
    """The neighbour lists ``map_test`` uses, from a SciPy sparse adjacency or Laplacian: the off-diagonal non-zeros, symmetrised
    by union, as CSR ``(ptr int32 [M + 1], idx int32 [nnz])`` with ascending neighbours."""
    if not sp.issparse(A):
        raise ValueError('map_test: A must be a SciPy sparse matrix, not %s' % type(A).__name__)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError('map_test: A must be square, got shape %r' % (tuple(A.shape),))
    if M is not None and A.shape[0] != M:
        raise ValueError('map_test: A is %d x %d but the maps have M = %d vertices' % (A.shape[0], A.shape[1], M))
    n = int(A.shape[0])
    if n > MMAX:
        raise ValueError('map_test: M = %d vertices, served: up to %d' % (n, MMAX))
    C = sp.coo_matrix(A)
    keep = (C.row != C.col) & (C.data != 0)
    r, c = C.row[keep].astype(np.int64), C.col[keep].astype(np.int64)
    G = sp.csr_matrix((np.ones(2 * r.size, np.int8), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n))
    G.sum_duplicates()
    G.sort_indices()
    if G.nnz >= 2 ** 31:
        raise ValueError('map_test: %d edges' % G.nnz)
    return G.indptr.astype(np.int32), G.indices.astype(np.int32)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------

_Plan = collections.namedtuple('_Plan', 'x single S C M ptr idx stat tail n_perm threshold step E H seed')


def _plan(maps, A, stat, n_perm, tail, threshold, step, E, H, seed):
    """Everything checked before any work (and before the device is touched); x: float32 host array [C, S, M], tail applied."""
    if is_tensor(maps):
        if str(maps.dtype) != 'torch.float32':
            raise ValueError('map_test: maps must be float32, not %s' % maps.dtype)
        x = maps.detach().cpu().numpy()
    else:
        x = np.asarray(maps)
        if not (np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.integer)):
            raise ValueError('map_test: maps of dtype %s' % x.dtype)
        x = x.astype(np.float32)
    if x.ndim not in (2, 3):
        raise ValueError('map_test: maps must be [S, M] or [S, C, M], got shape %r' % (tuple(x.shape),))
    single = x.ndim == 2
    if single:
        x = x[:, None, :]
    S, C, M = (int(v) for v in x.shape)
    if S < 2:
        raise ValueError('map_test: S = %d maps; a one-sample test needs at least 2' % S)
    if S > SMAX:
        raise ValueError('map_test: S = %d maps, served: up to %d' % (S, SMAX))
    if C < 1 or M < 1:
        raise ValueError('map_test: maps of shape %r' % (tuple(x.shape),))
    if not np.isfinite(x).all():
        raise ValueError('map_test: maps hold non-finite values')
    ptr, idx = edges(A, M)
    if stat not in STATS:
        raise ValueError('map_test: stat must be one of %r, not %r' % (STATS, stat))
    if tail not in (1, -1, 0):
        raise ValueError('map_test: tail must be 1, -1 or 0, not %r' % (tail,))
    if int(n_perm) != n_perm or n_perm < 1 or n_perm > 2 ** 31 - 1:
        raise ValueError('map_test: n_perm = %r' % (n_perm,))
    if stat == 'extent':
        if threshold is None or not np.isfinite(threshold):
            raise ValueError("map_test: stat='extent' needs a finite forming threshold, got %r" % (threshold,))
        threshold = float(threshold)
    if step is not None and not (np.isfinite(step) and step > 0):
        raise ValueError('map_test: step = %r must be positive and finite' % (step,))
    if not (np.isfinite(E) and np.isfinite(H)):
        raise ValueError('map_test: E = %r, H = %r must be finite' % (E, H))
    x = np.ascontiguousarray(x.transpose(1, 0, 2))
    if tail == -1:
        x = -x
    return _Plan(x, single, S, C, M, ptr, idx, stat, int(tail), int(n_perm), threshold, None if step is None else float(step),
                 float(E), float(H), int(seed))


def _tables(pl, step, NH):
    """``(hf float32 [NH + 1], hw float64 [NH + 1], ep float64 [M + 1])``: the heights, ``h^H step`` and ``e^E`` -- for 'extent'
    the threshold, 1 and e, so that the same sum gives the extent."""
    e = np.arange(pl.M + 1, dtype=np.float64)
    if pl.stat == 'extent':
        return np.array([0.0, pl.threshold], np.float32), np.array([0.0, 1.0]), e
    h = np.arange(NH + 1, dtype=np.float64) * step
    with np.errstate(divide='ignore', over='ignore'):
        hw = np.power(h, pl.H) * step
        ep = np.power(e, pl.E)
    hw[0] = 0.0
    if not (np.isfinite(hw[1:]).all() and np.isfinite(ep[1:]).all()):
        raise ValueError('map_test: E = %r, H = %r overflow float64 at this step and size' % (pl.E, pl.H))
    ep[0] = 0.0
    return h.astype(np.float32), hw, ep


def _default_step(pl, t_obs):
    """The TFCE step of one class: the observed maximum over the tested tail / 100 (1 where nothing is positive: no heights)."""
    if pl.step is not None:
        return pl.step
    top = float(np.abs(t_obs).max()) if pl.tail == 0 else float(t_obs.max())
    return top / 100.0 if top > 0 else 1.0


def _heights_needed(pl, step, top):
    """Heights of a map whose largest value is ``top`` (what the kernels compute per permutation)."""
    if pl.stat != 'tfce' or not top > 0:
        return 1
    n = np.floor(np.float64(top) / np.float64(step))
    if n > NHMAX:
        raise ValueError('map_test: step = %g gives %d heights, served: up to %d' % (step, int(n), NHMAX))
    return max(int(n), 1)


def _result(pl, t, stat, null, labels, steps, P, exact):
    p = np.empty_like(stat)
    for c in range(pl.C):
        srt = np.sort(null[c])
        p[c] = (P - np.searchsorted(srt, stat[c], side='left')) / float(P)
    if pl.stat != 'extent':
        labels = None
    steps = np.asarray(steps, np.float64) if pl.stat == 'tfce' else None
    if pl.single:
        return MapTestResult(t[0], stat[0], p[0], null[0], None if labels is None else labels[0],
                             None if steps is None else float(steps[0]), P, exact, pl.seed)
    return MapTestResult(t, stat, p, null, labels, steps, P, exact, pl.seed)


def _combine(t, pos, neg, lpos, lneg):
    """Two-sided: every vertex carries the value (and the cluster) of its own sign's part."""
    stat = np.where(t > 0, pos, np.where(t < 0, neg, 0.0))
    lab = None if lpos is None else np.where(t > 0, lpos, np.where(t < 0, lneg, -1)).astype(np.int32)
    return stat, lab


# ---- the host restatement -----------------------------------------------------------------------------------------------------------

def t_host(x, signs):
    """The stated t arithmetic: ``x`` float32 [S, M], ``signs`` [P, S] of +-1 -> float32 [P, M]."""
    S, M = x.shape
    xd = x.astype(np.float64)
    q = np.zeros(M)
    for j in range(S):
        q = q + xd[j] * xd[j]
    s = np.zeros((signs.shape[0], M))
    for j in range(S):
        s = s + signs[:, j, None].astype(np.float64) * xd[j][None, :]
    m = s / np.float64(S)
    d = q[None, :] - s * m
    with np.errstate(divide='ignore', invalid='ignore'):
        t = m / np.sqrt(d / np.float64(S * (S - 1)))
    return np.where(d > 0, t, 0.0).astype(np.float32)


def enhance_host(u, ptr, idx, mode, hf, hw, ep, step):
    """One map ``u`` float32 [M] -> ``(stat float64 [M], labels int32 [M])`` as ``chebgcn_cluster_enhance`` states it: SciPy's
    connected components of every supra-threshold subgraph, heights descending."""
    M = u.size
    if mode == 'max':
        return u.astype(np.float64), np.full(M, -1, np.int32)
    top = float(u.max())
    if mode == 'extent':
        n = 1
    else:
        n = int(np.floor(np.float64(top) / np.float64(step))) if top > 0 else 0
        if n > hf.size - 1:
            raise ValueError('map_test: %d heights, the tables hold %d' % (n, hf.size - 1))
    G = sp.csr_matrix((np.ones(idx.size, np.int8), idx, ptr), shape=(M, M))
    acc = np.zeros(M)
    labels = np.full(M, -1, np.int32)
    for i in range(n, 0, -1):
        act = np.nonzero(u > hf[i])[0]
        if act.size == 0:
            continue
        _, lab = csgraph.connected_components(G[act][:, act], directed=False)
        size = np.bincount(lab)
        acc[act] = acc[act] + ep[size[lab]] * hw[i]
        if i == 1:
            first = np.full(size.size, M, np.int64)
            np.minimum.at(first, lab, act)
            labels[act] = first[lab]
    return acc, labels


def _run_host(pl, P, exact, t_of):
    """The permutation loop of the host restatements.  ``t_of(c)`` gives class c's ``tmaps(p0, n)``: the float32 [n, M] t maps
    of permutations ``p0 .. p0 + n - 1`` (permutation 0 the observed one)."""
    sides = (1, -1) if pl.tail == 0 else (1,)
    t_all = np.empty((pl.C, pl.M), np.float32)
    stat_all = np.empty((pl.C, pl.M))
    null = np.empty((pl.C, P))
    labels = np.full((pl.C, pl.M), -1, np.int32)
    steps = []
    rows = max(1, HOST_CHUNK // pl.M)
    for c in range(pl.C):
        tmaps = t_of(c)
        t_obs = tmaps(0, 1)[0]
        st = _default_step(pl, t_obs)
        steps.append(st)
        tabs = None
        for p0 in range(0, P, rows):
            tb = tmaps(p0, min(rows, P - p0))
            NH = _heights_needed(pl, st, float(np.abs(tb).max()) if pl.tail == 0 else float(tb.max()))
            if tabs is None or tabs[0].size < NH + 1:
                tabs = _tables(pl, st, NH)
            for k in range(tb.shape[0]):
                parts = [enhance_host(tb[k] if sd > 0 else -tb[k], pl.ptr, pl.idx, pl.stat, tabs[0], tabs[1], tabs[2], st)
                         for sd in sides]
                null[c, p0 + k] = max(float(a.max()) for a, _ in parts)
                if p0 + k == 0:
                    t_all[c] = tb[k]
                    if pl.tail == 0:
                        stat_all[c], lab = _combine(tb[k], parts[0][0], parts[1][0], parts[0][1], parts[1][1])
                    else:
                        stat_all[c], lab = parts[0]
                    labels[c] = lab
    return _result(pl, t_all, stat_all, null, labels, steps, P, exact)


def map_test_host(maps, A, stat='tfce', n_perm=5000, tail=0, threshold=None, step=None, E=0.5, H=2.0, seed=0, device=None):
    """``map_test`` restated with NumPy and SciPy, operation for operation (no device; ``device`` is ignored): the same
    ``MapTestResult``, bit for bit.  One ``connected_components`` call per height and permutation: minutes at atlas size."""
    pl = _plan(maps, A, stat, n_perm, tail, threshold, step, E, H, seed)
    signs, exact = sign_flips(pl.S, pl.n_perm, pl.seed)
    return _run_host(pl, signs.shape[0], exact, lambda c: lambda p0, n: t_host(pl.x[c], signs[p0:p0 + n]))


# ---- the device ---------------------------------------------------------------------------------------------------------------------

def _run_device(pl, dev, P, exact, t_of):
    """The permutation loop on the device: per class the observed map, the TFCE step it sets, then the null in batches of
    permutations whose t maps and labelling state fit CHUNK_BYTES, the height tables grown when a batch needs more.
    ``t_of(c)`` gives class c's ``tmaps(p0, n)``: the float32 [n, M] device tensor of the t maps of permutations
    ``p0 .. p0 + n - 1`` (permutation 0 the observed one); it is called inside ``torch.cuda.device(dev)``."""
    import torch
    from . import _lib, ops
    mode = _MODE[pl.stat]
    sides = (False, True) if pl.tail == 0 else (False,)
    clustered = mode != _lib.CLUSTER_MAX
    t_all = np.empty((pl.C, pl.M), np.float32)
    stat_all = np.empty((pl.C, pl.M))
    null = np.empty((pl.C, P))
    labels = np.full((pl.C, pl.M), -1, np.int32)
    steps = []
    with torch.cuda.device(dev):
        ptr = idx = status = None
        if clustered:
            ptr = torch.as_tensor(pl.ptr).to(dev)
            idx = torch.as_tensor(pl.idx).to(dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
        per_perm = 4 * pl.M + ops.cluster_enhance_workspace(1, pl.M, mode, ARM) + 8
        Pb = int(max(1, min(PBMAX, P, CHUNK_BYTES // per_perm)))
        for c in range(pl.C):
            tmaps = t_of(c)
            t0 = tmaps(0, 1)
            t_obs = t0[0].cpu().numpy()
            st = _default_step(pl, t_obs)
            steps.append(st)
            tabs = None                 # (hf, hw, ep) on the device, grown when a batch needs more heights

            def tables(NH):
                nonlocal tabs
                if tabs is None or tabs[0].numel() < NH + 1:
                    tabs = tuple(torch.as_tensor(a).to(dev) for a in _tables(pl, st, NH))
                return tabs

            def enhance(tb, neg, obs):
                if not clustered:
                    return ops.cluster_enhance(tb, mode, negate=neg, want_out=obs)
                top = float(tb.abs().max()) if pl.tail == 0 else float(tb.max())
                NH = _heights_needed(pl, st, top)
                hf, hw, ep = tables(NH)
                return ops.cluster_enhance(tb, mode, ptr, idx, hf, hw, ep, step=st, NH=NH, negate=neg, want_out=obs,
                                           want_labels=obs and pl.stat == 'extent', arm=ARM, status=status)

            parts = [enhance(t0, neg, True) for neg in sides]
            if clustered:
                ops.cluster_check(status)
            outs = [o[0].cpu().numpy() for o, _, _ in parts]
            labs = [None if l is None else l[0].cpu().numpy() for _, l, _ in parts]
            t_all[c] = t_obs
            if pl.tail == 0:
                stat_all[c], lab = _combine(t_obs, outs[0], outs[1], labs[0], labs[1])
            else:
                stat_all[c], lab = outs[0], labs[0]
            if lab is not None:
                labels[c] = lab
            nul = torch.empty(P, dtype=torch.float64, device=dev)
            for p0 in range(0, P, Pb):
                n = min(Pb, P - p0)
                tb = tmaps(p0, n)
                mx = [enhance(tb, neg, False)[2] for neg in sides]
                nul[p0:p0 + n] = mx[0] if len(mx) == 1 else torch.maximum(mx[0], mx[1])
            if clustered:
                ops.cluster_check(status)
            null[c] = nul.cpu().numpy()
    return _result(pl, t_all, stat_all, null, labels, steps, P, exact)


def map_test(maps, A, stat='tfce', n_perm=5000, tail=0, threshold=None, step=None, E=0.5, H=2.0, seed=0, device=None):
    """Sign-flip permutation test of the group mean of ``maps`` at every vertex, family-wise corrected by the maximum statistic.

    ``maps``: float32 ``[S, M]`` or ``[S, C, M]`` (NumPy or a device tensor): one map per subject, fold or run, C classes; the
    classes are tested one after the other with the SAME sign flips; ``S >= 2``, finite values.  ``A``: SciPy sparse ``[M, M]``
    adjacency or Laplacian -- its off-diagonal non-zeros are the edges, symmetrised by union, so the ``L`` a model was built with
    is accepted as it is.  ``stat``: ``'max'`` (the vertex-wise t, no neighbourhood), ``'extent'`` (the size of the vertex's
    cluster above the forming ``threshold``, required) or ``'tfce'`` (``E``, ``H``; ``step`` defaults to the observed maximum /
    100).  ``tail``: 1 positive effects, -1 the maps are negated first, 0 two-sided (positive and negative parts are enhanced
    separately, each vertex carries the value of its own sign's part, the null takes the larger of the two maxima).

    Permutation 0 is the identity and is counted: ``p[v] = #{perm : null[perm] >= stat[v]} / P >= 1 / P``.  When
    ``2**S <= n_perm`` all sign vectors are enumerated (``exact``, ``P = 2**S``), else ``sign_flips`` draws them from ``seed``.
    The result is a pure function of the arguments: the same at any permutation batch size, from call to call, and bit for bit
    what ``map_test_host`` computes.  Bad arguments raise ``ValueError`` before the device is touched.  Returns a
    ``MapTestResult``."""
    pl = _plan(maps, A, stat, n_perm, tail, threshold, step, E, H, seed)
    import torch
    from . import ops
    dev = cuda_device(device, maps)
    exact = pl.S < 62 and (1 << pl.S) <= pl.n_perm
    P = (1 << pl.S) if exact else pl.n_perm
    bits = None

    def t_of(c):
        nonlocal bits
        if exact and bits is None:      # the enumeration as a table: bit j of word 0 of row q is bit j of q (S <= 31 here)
            bits = torch.arange(P, dtype=torch.int32, device=dev).reshape(P, 1).contiguous()
        x = torch.as_tensor(pl.x[c]).to(dev)
        xd = pl.x[c].astype(np.float64)
        q = np.zeros(pl.M)
        for j in range(pl.S):
            q = q + xd[j] * xd[j]
        q = torch.as_tensor(q).to(dev)
        return lambda p0, n: ops.signflip_t(x, q, p0, n, pl.seed, bits=None if bits is None else bits[p0:p0 + n])

    return _run_device(pl, dev, P, exact, t_of)


# ---- group designs ------------------------------------------------------------------------------------------------------------------

RMAX = 64                       # rank of a design (chebgcn_perm_glm_query(3))

DesignTestResult = collections.namedtuple('DesignTestResult', MapTestResult._fields + ('dof',))
DesignTestResult.__doc__ = """What ``design_test`` returns: the fields of ``MapTestResult`` (``t`` the observed t map of the
contrast, of the negated maps for ``tail=-1``), and ``dof = S - rank(design)``.  ``exact`` is always False: ``design_test`` never
enumerates the permutations of a design, it draws ``n_perm`` of them (the identity first)."""

_Design = collections.namedtuple('_Design', 'r dof Uf u unorm2 X Qz rows')


def _blocks(blocks, S):
    """The members of every block, ascending (one block of everybody for None)."""
    if blocks is None:
        return [np.arange(S, dtype=np.int64)]
    b = np.asarray(blocks)
    if b.shape != (S,) or not np.issubdtype(b.dtype, np.integer):
        raise ValueError('design_test: blocks must be %d integers, got %s %r' % (S, b.dtype, tuple(b.shape)))
    return [np.nonzero(b == v)[0].astype(np.int64) for v in np.unique(b)]


def permutations(S, n_perm, seed, blocks=None, flips=False):
    """The table ``design_test`` and ``design_test_host`` run: uint32 ``[P, S]``, ``P = n_perm``.  Entry ``[p, j]`` holds in its
    low 31 bits the row of the design (of its basis ``Uf``) that meets subject j in permutation p, in its top bit whether
    subject j's residual is negated.  Row 0 is the identity without flips.  For ``p >= 1`` every block (``blocks`` int [S]; None:
    one block) with ascending members ``m[0 .. n)`` is shuffled on its own, Fisher-Yates from the top: ``a = m``; for
    ``i = n - 1 .. 1``: ``k = (chebgcn_aug_draw(seed, refill=0, i=p, d=m[i]) * (i + 1)) >> 32``, swap ``a[i]`` and ``a[k]``;
    then entry ``[p, m[i]] = a[i]``.  With ``flips`` subject j is negated where the top bit of
    ``chebgcn_aug_draw(seed, refill=1, i=p, d=j)`` is set.  Row p depends on ``(seed, p)`` alone, not on ``n_perm``."""
    S, P = int(S), int(n_perm)
    if S < 1 or S > SMAX or P < 1:
        raise ValueError('permutations: S = %d, n_perm = %d' % (S, P))
    p = np.arange(P, dtype=np.uint64)
    ar = np.arange(P)
    rows = np.empty((P, S), np.uint32)
    for m in _blocks(blocks, S):
        a = np.tile(m, (P, 1))
        for i in range(m.size - 1, 0, -1):
            k = ((aug_draw(seed, 0, p, np.uint64(m[i])) * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)
            ai = a[:, i].copy()
            a[:, i] = a[ar, k]
            a[ar, k] = ai
        rows[:, m] = a
    if flips:
        neg = aug_draw(seed, 1, p[:, None], np.arange(S, dtype=np.uint64)[None, :]) >> np.uint64(31)
        rows |= (neg << np.uint64(31)).astype(np.uint32)
    rows[0] = np.arange(S, dtype=np.uint32)
    return rows


def _design(design, contrast, blocks, flips, S, n_perm, seed):
    """The host half of ``design_test``, float64, shared by the device path and the restatement: the thin SVD of the design,
    the contrast's vectors, the nuisance basis and the permutation table.  Every check on design, contrast and blocks."""
    D = np.asarray(design)
    if D.ndim != 2 or not (np.issubdtype(D.dtype, np.floating) or np.issubdtype(D.dtype, np.integer)):
        raise ValueError('design_test: design must be a float [S, q] array, got %s %r' % (D.dtype, tuple(D.shape)))
    D = D.astype(np.float64)
    if D.shape[0] != S or D.shape[1] < 1:
        raise ValueError('design_test: design is %r, the maps have S = %d subjects' % (tuple(D.shape), S))
    if not np.isfinite(D).all():
        raise ValueError('design_test: design holds non-finite values')
    c = np.asarray(contrast)
    if c.shape != (D.shape[1],) or not (np.issubdtype(c.dtype, np.floating) or np.issubdtype(c.dtype, np.integer)):
        raise ValueError('design_test: contrast must be %d numbers (one t contrast), got %r' % (D.shape[1], tuple(c.shape)))
    c = c.astype(np.float64)
    if not np.isfinite(c).all():
        raise ValueError('design_test: contrast holds non-finite values')
    U, sv, Vt = np.linalg.svd(D, full_matrices=False)
    r = int((sv > max(D.shape) * np.finfo(np.float64).eps * sv[0]).sum()) if sv.size and sv[0] > 0 else 0     # glm._factor's rule
    if r < 1 or r > RMAX:
        raise ValueError('design_test: the design has rank %d, served: 1 .. %d' % (r, RMAX))
    dof = S - r
    if dof < 1:
        raise ValueError('design_test: S = %d subjects, rank %d: no degrees of freedom left' % (S, r))
    Uf = np.ascontiguousarray(U[:, :r])
    V = Vt[:r].T
    cn = float(np.sqrt(c @ c))
    if not cn > 0 or float(np.sqrt(((c - V @ (V.T @ c)) ** 2).sum())) > 1e-8 * cn:
        raise ValueError('design_test: the contrast is zero or not estimable (it must lie in the row space of the design)')
    w = (V.T @ c) / sv[:r]
    pc = Uf @ w                                                     # pinv(D)^T c
    unorm2 = float(w @ w)                                           # c pinv(D^T D) c
    if not (unorm2 > 0 and np.isfinite(unorm2)):
        raise ValueError('design_test: c pinv(D^T D) c = %r must be positive' % unorm2)
    u = np.ascontiguousarray(Uf.T @ pc)
    X = pc / unorm2                                                 # D pinv(D^T D) c / (c pinv(D^T D) c): the effect regressor
    members = _blocks(blocks, S)
    if not flips:
        tol = 1e-10 * float(np.abs(X).max())
        if all(float(np.ptp(X[m])) <= tol for m in members):
            raise ValueError('design_test: the effect regressor is constant inside every block, so no permutation changes '
                             'anything; use flips=True (sign flips of the residuals)')
    g = Uf.T @ X
    N = np.linalg.svd(g[None, :], full_matrices=True)[2][1:].T     # [r, r - 1]: the null space of g^T
    Qz = np.ascontiguousarray(Uf @ N)                               # span(D) without X: the nuisance space
    return _Design(r, dof, Uf, u, unorm2, X, Qz, permutations(S, n_perm, seed, blocks, flips))


def _residuals(y, Qz):
    """``(e float32 [S, M], q float64 [M])`` of one class: the residual of the nuisance fit rounded once, and its squares summed
    in ascending subject."""
    yd = y.astype(np.float64)
    e = (yd - Qz @ (Qz.T @ yd)).astype(np.float32)
    ed = e.astype(np.float64)
    q = np.zeros(y.shape[1])
    for j in range(y.shape[0]):
        q = q + ed[j] * ed[j]
    return np.ascontiguousarray(e), q


def perm_t_host(e, q, Uf, u, unorm2, dof, rows):
    """The stated arithmetic of ``chebgcn_perm_glm_t`` (include/chebgcn.h) in float64 NumPy, one rounding per operation:
    ``e`` float32 [S, M], ``q`` [M], ``Uf`` [S, r], ``u`` [r], ``rows`` uint32 [P, S] -> float32 [P, M]."""
    S, M = e.shape
    r = Uf.shape[1]
    rows = np.asarray(rows).astype(np.uint32)
    P = rows.shape[0]
    row = np.minimum(rows & np.uint32(0x7FFFFFFF), np.uint32(S - 1)).astype(np.int64)
    neg = (rows >> np.uint32(31)).astype(bool)
    ed = e.astype(np.float64)
    a = np.zeros((r, P, M))
    for j in range(S):
        x = np.where(neg[:, j, None], -ed[j][None, :], ed[j][None, :])
        Uj = Uf[row[:, j]]                                          # [P, r]
        for k in range(r):
            a[k] = a[k] + Uj[:, k, None] * x
    ssq = np.zeros((P, M))
    num = np.zeros((P, M))
    for k in range(r):
        ssq = ssq + a[k] * a[k]
        num = num + np.float64(u[k]) * a[k]
    rss = q[None, :] - ssq
    rss = np.where(rss < (4.0 * np.float64(S + r) * 2.0 ** -53) * q[None, :], 0.0, rss)
    var = (rss / np.float64(dof)) * np.float64(unorm2)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = num / np.sqrt(var)
    return np.where(var > 0, t, 0.0).astype(np.float32)


def _design_doc(f):
    f.__doc__ = f.__doc__.replace('@ARGS@', _DESIGN_ARGS)
    return f


_DESIGN_ARGS = """``maps``, ``A``, ``stat``, ``tail``, ``threshold``, ``step``, ``E``, ``H`` and ``device`` are ``map_test``'s.  ``design``: float
    ``[S, q]``, finite, of rank ``1 <= r <= 64`` with ``S - r >= 1``; a rank-deficient design is accepted (thin SVD, the rank rule
    of ``first_level``).  ``contrast``: float ``[q]``, one t contrast; it must be non-zero and estimable (in the row space of
    the design to 1e-8 of its norm).  ``blocks``: int ``[S]`` or None: subjects are permuted only inside their block (paired
    and repeated-measures designs).  ``flips=True`` additionally negates each subject's residual with probability 1/2
    (independent symmetric errors); with a design of one column of ones it is ``map_test``'s test.  A design whose effect
    regressor is constant inside every block cannot be tested without ``flips``: ``ValueError``."""


@_design_doc
def design_test_host(maps, A, design, contrast, stat='tfce', n_perm=5000, tail=0, blocks=None, flips=False, threshold=None,
                     step=None, E=0.5, H=2.0, seed=0, device=None):
    """``design_test`` restated with NumPy and SciPy, operation for operation (no device; ``device`` is ignored): the same
    ``DesignTestResult``, bit for bit.

    @ARGS@"""
    pl = _plan(maps, A, stat, n_perm, tail, threshold, step, E, H, seed)
    ds = _design(design, contrast, blocks, flips, pl.S, pl.n_perm, pl.seed)

    def t_of(c):
        e, q = _residuals(pl.x[c], ds.Qz)
        return lambda p0, n: perm_t_host(e, q, ds.Uf, ds.u, ds.unorm2, ds.dof, ds.rows[p0:p0 + n])

    return DesignTestResult(*_run_host(pl, pl.n_perm, False, t_of), ds.dof)


@_design_doc
def design_test(maps, A, design, contrast, stat='tfce', n_perm=5000, tail=0, blocks=None, flips=False, threshold=None, step=None,
                E=0.5, H=2.0, seed=0, device=None):
    """Permutation test of one t contrast of a general linear model across subjects at every vertex (two groups, a covariate
    with nuisance regressors, paired conditions), family-wise corrected by the maximum statistic as in ``map_test``: FSL
    randomise / PALM in the Freedman-Lane scheme (Winkler et al. 2014).

    @ARGS@

    The model ``maps = design b + error`` is split into the effect regressor ``X = D Q c / (c Q c)``, ``Q = pinv(D^T D)``, and
    the nuisance space (the rest of the design's span).  The residuals ``e`` of the nuisance fit are permuted (table:
    ``permutations``), and the full model's t of the contrast is taken on every permuted ``e``: on the device by
    ``chebgcn_perm_glm_t``, which permutes the rows of the design's orthonormal basis instead (the same projections), in the
    float64 arithmetic include/chebgcn.h states and ``perm_t_host`` restates.  The t maps then go through ``map_test``'s loop:
    the statistic, the null of maxima, ``p[v] = #{perm : null[perm] >= stat[v]} / P`` with the identity counted.

    ``n_perm`` permutations are always drawn from ``seed``: nothing is enumerated, ``exact`` is always False (with few
    subjects per block the same permutation may be drawn more than once).  The result is a pure function of the arguments and
    bit for bit what ``design_test_host`` computes.  Bad arguments raise ``ValueError`` before the device is touched.  Returns a
    ``DesignTestResult`` (``MapTestResult``'s fields and ``dof``)."""
    pl = _plan(maps, A, stat, n_perm, tail, threshold, step, E, H, seed)
    ds = _design(design, contrast, blocks, flips, pl.S, pl.n_perm, pl.seed)
    import torch
    from . import ops
    dev = cuda_device(device, maps)
    shared = []

    def t_of(c):
        if not shared:
            shared.extend(torch.as_tensor(a).to(dev) for a in (ds.Uf, ds.u))
        Uf, u = shared
        e, q = (torch.as_tensor(a).to(dev) for a in _residuals(pl.x[c], ds.Qz))
        return lambda p0, n: ops.perm_glm_t(e, q, Uf, u, ds.unorm2, ds.dof,
                                            torch.as_tensor(ds.rows[p0:p0 + n].view(np.int32)).to(dev))

    return DesignTestResult(*_run_device(pl, dev, pl.n_perm, False, t_of), ds.dof)
