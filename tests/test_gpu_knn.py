"""kNN graphs on the MI355X: chebgcn_knn (both arms by name, whole and split), chebgcn_series_normalise, ``graph.knn_device``,
``graph.connectivity_graph`` and ``synthetic_graph(knn='device')`` against a float64 brute-force kNN written here in NumPy.

Check 1 (every row): the float64 distances of the returned neighbours, sorted, equal the float64 k smallest, and ``dist`` itself
equals float64 on the returned pairs -- 1e-5 relative on d for euclidean, 1e-5 absolute on the similarity for cosine /
correlation (the project's parity bound).  Check 2: index equality with float64 on every row whose float64 consecutive gaps
among the first k + 1 neighbours all exceed 1e-4 of d_k; rows below are excused in this check only, at most 5 % of them, and
the float64 reference alone is asserted to stay under that cap for the inputs used."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_golden, record_measured
from gcn_fmri_decoding_amd import _lib, graph, models_gcn, ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
METRICS = ('euclidean', 'cosine', 'correlation')
BOUND = 1e-5
GAP = 1e-4
CAP = 0.05


# ---------------------------------------------------------------------------------------------- float64 reference

def _prepared(z, metric):
    z = np.asarray(z, np.float64)
    if metric == 'euclidean':
        return z
    if metric == 'correlation':
        z = z - z.mean(axis=1, keepdims=True)
    n = np.sqrt((z * z).sum(axis=1))
    return z * np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)[:, None]       # zero-norm / constant rows: similarity 0


def pair_distance64(z, metric, rows, cols):
    """float64 distance of the pairs (rows[i], cols[i, j]): differences for euclidean, 1 - similarity otherwise."""
    zp = _prepared(z, metric)
    rows, cols = np.asarray(rows), np.asarray(cols)
    out = np.empty(cols.shape)
    step = max(1, (1 << 24) // max(1, cols.shape[1] * zp.shape[1]))        # row chunks of about 128 MB
    for s in range(0, len(rows), step):
        a, b = zp[rows[s:s + step]][:, None, :], zp[cols[s:s + step]]
        out[s:s + step] = np.sqrt(((a - b) ** 2).sum(axis=2)) if metric == 'euclidean' else 1.0 - (a * b).sum(axis=2)
    return out


def knn64(z, k, metric, block=1024):
    """Brute-force float64 kNN, self excluded by index, ties by lower index: (d [N, kk], idx [N, kk]), kk = min(k + 1, N - 1)
    (one neighbour more than asked for, for the gap rule).  Row blocks; the distances of the kept pairs are recomputed by
    differences, so the euclidean numbers never come from the Gram form."""
    zp = _prepared(z, metric)
    N = len(zp)
    kk = min(k + 1, N - 1)
    sq = (zp * zp).sum(axis=1)
    d_out, i_out = np.empty((N, kk)), np.empty((N, kk), np.int64)
    for r0 in range(0, N, block):
        r1 = min(N, r0 + block)
        g = zp[r0:r1] @ zp.T
        if metric == 'euclidean' and zp.shape[1] <= 16:
            d = np.zeros_like(g)
            for c in range(zp.shape[1]):
                d += (zp[r0:r1, None, c] - zp[None, :, c]) ** 2
        elif metric == 'euclidean':
            d = np.maximum(sq[r0:r1, None] + sq[None] - 2.0 * g, 0.0)
        else:
            d = 1.0 - g
        d[np.arange(r1 - r0), np.arange(r0, r1)] = np.inf
        # a few more than kk by the block's numbers, then exact distances and the final (distance, index) order
        kc = min(kk + 8, N - 1)
        cand = np.argpartition(d, kc - 1, axis=1)[:, :kc] if kc < N - 1 else np.argsort(d, axis=1)[:, :kc]
        cand.sort(axis=1)
        de = pair_distance64(z, metric, np.arange(r0, r1), cand)
        order = np.lexsort((cand, de), axis=1)[:, :kk]
        d_out[r0:r1], i_out[r0:r1] = np.take_along_axis(de, order, 1), np.take_along_axis(cand, order, 1)
    return d_out, i_out


def gap_rows(d64, k):
    """Rows on which index equality is required: every consecutive gap among the first k + 1 neighbours > GAP * d_k."""
    if d64.shape[1] < 2:
        return np.ones(len(d64), bool)
    kk = min(k + 1, d64.shape[1])
    return (np.diff(d64[:, :kk], axis=1) > GAP * d64[:, k - 1:k]).all(axis=1)


def check1(z, metric, k, d, idx, d64):
    got = pair_distance64(z, metric, np.arange(len(z)), idx)
    want = d64[:, :k]
    if metric == 'euclidean':
        tol = BOUND * np.maximum(want, 1e-30) + 1e-12
    else:
        tol = BOUND
    e_set = np.abs(np.sort(got, axis=1) - want)
    e_val = np.abs(d.astype(np.float64) - got)
    scale = np.maximum(want, 1e-30) if metric == 'euclidean' else 1.0
    worst_set, worst_val = float((e_set / scale).max()), float((e_val / scale).max())
    print('check1 %s N=%d D=%d k=%d: neighbour set %.3e, dist %.3e (bound %.0e)' % (metric, z.shape[0], z.shape[1], k, worst_set,
                                                                                     worst_val, BOUND))
    assert (np.diff(d, axis=1) >= 0).all(), 'dist not ascending'
    assert (idx != np.arange(len(z))[:, None]).all(), 'a vertex is its own neighbour'
    assert all(len(set(r)) == k for r in idx[:: max(1, len(idx) // 200)]), 'repeated neighbour'
    assert (e_set <= tol).all(), 'neighbour set: %.3e' % worst_set
    assert (e_val <= tol).all(), 'returned dist: %.3e' % worst_val
    return worst_set, worst_val


def check2(k, idx, d64, i64):
    need = gap_rows(d64, k)
    bad = int((idx[need] != i64[need, :k]).any(axis=1).sum())
    assert bad == 0, '%d of %d rows with clear gaps differ from float64' % (bad, int(need.sum()))
    return 1.0 - float(need.mean())


def features(N, D, seed, metric='euclidean', k=8, offset=0.3):
    """Seeded inputs of the grid, chosen so that the float64 reference itself excuses at most CAP of the rows in Check 2 (the
    share of rows with a near-tie among k + 1 neighbours grows like GAP * k^2 * the intrinsic dimension of the data):
      k < 32   uniform points in the unit cube for D <= 9; beyond, latent-factor features (40 factors, 15 % loadings, noise 0.7)
               for cosine / correlation and a 3-dimensional cube embedded linearly for euclidean (distances concentrate in the
               latent-factor features: 6 % of their rows are near-ties already at k = 8);
      k = 32   no random input stays under the cap (15 - 58 % measured), so designed ones: a geometric sequence x_i = r^i along
               one direction for euclidean (every neighbourhood is the same figure up to scale), and for cosine / correlation
               the same sequence as angles on a circle (N <= 300: beyond, float32 rounding of the coordinates moves the small
               angles by more than the gaps)."""
    rs = np.random.RandomState(seed)
    if k >= 32:
        return geometric_line(N, D, seed) if metric == 'euclidean' else geometric_circle(N, D, metric, seed)
    if D <= 9:
        return (rs.rand(N, D) - offset).astype(np.float32)
    if metric == 'euclidean':
        return (rs.rand(N, 3) @ rs.randn(3, D)).astype(np.float32)
    nf = 40
    load = rs.randn(N, nf) * (rs.rand(N, nf) < 0.15)
    return (load @ rs.randn(nf, D) + 0.7 * rs.randn(N, D)).astype(np.float32)


def geometric_line(N, D, seed):
    """x_i = r^i (up to 1e12) times a fixed direction in D dimensions."""
    r = min(1.1, 1e12 ** (1.0 / N))
    u = np.random.RandomState(seed).randn(1, D) if D > 1 else np.ones((1, 1))
    return ((r ** np.arange(N))[:, None] * u).astype(np.float32)


def geometric_circle(N, D, metric, seed, lo=3e-3, hi=3.0):
    """Angles lo (hi / lo)^(i / (N - 1)) on a unit circle in a random plane of D dimensions (for correlation: a plane
    orthogonal to the constant vector, plus an offset)."""
    assert N <= 300
    th = lo * (hi / lo) ** (np.arange(N) / max(N - 1, 1))
    rs = np.random.RandomState(seed)
    if metric == 'correlation':
        B = np.linalg.qr(np.concatenate([np.ones((D, 1)), rs.randn(D, 2)], axis=1))[0][:, 1:3]
        return (np.cos(th)[:, None] * B[:, 0] + np.sin(th)[:, None] * B[:, 1] + 0.7).astype(np.float32)
    B = np.linalg.qr(rs.randn(D, 2))[0]
    return (np.cos(th)[:, None] * B[:, 0] + np.sin(th)[:, None] * B[:, 1]).astype(np.float32)


def run_knn(z, k, metric):
    _lib.dispatch_log = log = []
    try:
        d, idx = graph.knn_device(z, k=k, metric=metric, device=DEV)
    finally:
        _lib.dispatch_log = None
    names = [n for w, n in log if w == 'knn']
    assert len(names) == 1
    return d, idx, names[0]


# ---------------------------------------------------------------------------------------------- the shape grid

GRID = [
    # N, D, k, metric, arm, split
    (2, 1, 1, 'euclidean', 'direct', 'whole'), (2, 9, 1, 'cosine', 'gram', 'whole'), (2, 64, 1, 'correlation', 'gram', 'whole'),
    (33, 3, 8, 'euclidean', 'direct', 'whole'), (33, 8, 1, 'cosine', 'direct', 'whole'), (33, 9, 32, 'euclidean', 'gram', 'whole'),
    (33, 64, 8, 'correlation', 'gram', 'whole'),
    (33, 63, 8, 'correlation', 'gram', 'whole'), (33, 1200, 1, 'cosine', 'gram', 'whole'),
    (1000, 1, 8, 'euclidean', 'direct', 'split'), (1000, 3, 32, 'euclidean', 'direct', 'split'),
    (1000, 3, 8, 'correlation', 'direct', 'split'),
    (1000, 8, 1, 'cosine', 'direct', 'split'), (1000, 9, 8, 'correlation', 'gram', 'split'),
    (1000, 63, 32, 'euclidean', 'gram', 'split'), (1000, 64, 8, 'cosine', 'gram', 'split'),
    (1000, 1200, 8, 'euclidean', 'gram', 'split'),
    (4097, 3, 8, 'cosine', 'direct', 'split'), (4097, 8, 8, 'euclidean', 'direct', 'split'), (4097, 9, 1, 'euclidean', 'gram', 'split'),
    (4097, 63, 8, 'cosine', 'gram', 'split'), (4097, 64, 8, 'correlation', 'gram', 'split'),
    (4097, 64, 32, 'euclidean', 'gram', 'split'), (4097, 1200, 8, 'correlation', 'gram', 'split'),
    (10000, 3, 8, 'euclidean', 'direct', 'split'), (10000, 8, 8, 'correlation', 'direct', 'split'),
    (10000, 8, 32, 'euclidean', 'direct', 'split'),
    (10000, 9, 8, 'cosine', 'gram', 'split'), (10000, 64, 8, 'euclidean', 'gram', 'split'),
    (10000, 1200, 8, 'cosine', 'gram', 'split'), (10000, 1200, 32, 'euclidean', 'gram', 'split'),
    # cosine / correlation at k = 32: the one input found that keeps the float64 reference under the cap (N = 300; at N = 33,
    # where k = 32 is every other vertex, none was found, and beyond 300 float32 rounding closes the designed gaps)
    (300, 2, 32, 'cosine', 'direct', 'split'), (300, 12, 32, 'cosine', 'gram', 'split'),
    (300, 3, 32, 'correlation', 'direct', 'split'), (300, 13, 32, 'correlation', 'gram', 'split'),
]


@pytest.mark.parametrize('N,D,k,metric,arm,split', GRID)
def test_knn_grid(N, D, k, metric, arm, split):
    z = features(N, D, seed=N * 7 + D, metric=metric, k=k)
    d64, i64 = knn64(z, k, metric)
    ref_excused = 1.0 - float(gap_rows(d64, k).mean())
    print('N=%d D=%d k=%d %s: float64 reference excuses %.2f %% of the rows' % (N, D, k, metric, 100 * ref_excused))
    assert ref_excused <= CAP, 'the reference alone excuses %.3f of the rows' % ref_excused
    d, idx, disp = run_knn(z, k, metric)
    assert disp == 'knn_prep_kernel + knn_%s_kernel<%s> + knn_merge_refine_kernel' % (arm, split), disp
    assert d.dtype == np.float32 and idx.dtype == np.int64 and d.shape == idx.shape == (N, k)
    assert np.isfinite(d).all() and idx.min() >= 0 and idx.max() < N
    ws, wv = check1(z, metric, k, d, idx, d64)
    excused = check2(k, idx, d64, i64)
    assert excused <= CAP
    record_measured('knn_grid', N=N, D=D, k=k, metric=metric, arm=arm, neighbour_set_err=ws, dist_err=wv, excused_share=excused)


# ---------------------------------------------------------------------------------------------- Check 2 with its cap

def _latent_series(T, M, seed):
    rs = np.random.RandomState(seed)
    load = rs.randn(M, 40) * (rs.rand(M, 40) < 0.15)
    return (rs.randn(T, 40) @ load.T + 0.7 * rs.randn(T, M)).astype(np.float32)      # [T, M]


@pytest.mark.parametrize('case', ['cube10000', 'cube3000', 'series_correlation', 'series_cosine'])
def test_index_equality_under_the_gap_rule(case):
    k = 8
    if case.startswith('cube'):
        N = int(case[4:])
        z, metric = np.random.RandomState(N).rand(N, 3).astype(np.float32), 'euclidean'
    else:
        z, metric = np.ascontiguousarray(_latent_series(1200, 3000, 17).T), case.split('_')[1]
    d64, i64 = knn64(z, k, metric)
    ref_excused = 1.0 - float(gap_rows(d64, k).mean())
    print('%s: float64 reference excuses %.2f %% of the rows' % (case, 100 * ref_excused))
    assert ref_excused <= CAP, 'the reference alone excuses %.3f of the rows' % ref_excused
    d, idx, disp = run_knn(z, k, metric)
    ws, wv = check1(z, metric, k, d, idx, d64)
    excused = check2(k, idx, d64, i64)
    assert excused <= CAP
    record_measured('knn_index_equality', case=case, dispatch=disp, excused_share=excused, neighbour_set_err=ws, dist_err=wv)


# ---------------------------------------------------------------------------------------------- edges

@pytest.mark.parametrize('D', [3, 12])
@pytest.mark.parametrize('metric', METRICS)
def test_duplicated_points_lower_index_first_self_excluded(D, metric):
    rs = np.random.RandomState(D)
    z = (rs.rand(300, D) + 0.2).astype(np.float32)
    group = [5, 40, 41, 170, 299]
    z[group] = z[5]
    z[[7, 250]] = z[100]
    d, idx, _ = run_knn(z, 4, metric)
    for g in group:
        others = [v for v in group if v != g]
        assert list(idx[g]) == others, (g, idx[g])
        assert (d[g] <= (0 if metric == 'euclidean' else 1e-6)).all()
    assert list(idx[100][:2]) == [7, 250] and list(idx[7][:2]) == [100, 250] and list(idx[250][:2]) == [7, 100]
    d64, i64 = knn64(z, 4, metric)
    check1(z, metric, 4, d, idx, d64)
    check2(4, idx, d64, i64)


@pytest.mark.parametrize('D', [4, 40])
def test_zero_norm_and_constant_rows_give_no_nan(D):
    rs = np.random.RandomState(D)
    z = rs.randn(200, D).astype(np.float32)
    z[3] = 0.0
    z[9] = 2.5
    for metric, rows in (('cosine', [3]), ('correlation', [3, 9])):
        d, idx, _ = run_knn(z, 5, metric)
        assert np.isfinite(d).all()
        for r in rows:
            assert (d[r] == 1.0).all(), d[r]
            assert list(idx[r]) == [v for v in range(6) if v != r][:5]          # all tied at 1: the lowest indices
        d64, i64 = knn64(z, 5, metric)
        check1(z, metric, 5, d, idx, d64)
    d, idx, _ = run_knn(z, 5, 'euclidean')
    assert np.isfinite(d).all()
    # a single feature: every row is constant under correlation
    d, idx, _ = run_knn(z[:, :1].copy(), 3, 'correlation')
    assert (d == 1.0).all() and list(idx[0]) == [1, 2, 3] and list(idx[2]) == [0, 1, 3]


@pytest.mark.parametrize('N,D,metric', [(4097, 3, 'euclidean'), (4097, 70, 'euclidean'), (1000, 33, 'correlation'), (33, 9, 'cosine')])
def test_repeat_calls_bit_identical(N, D, metric):
    z = features(N, D, seed=1)
    planes = np.zeros((D, ops.plane_stride(N)), np.float32)
    planes[:, :N] = z.T
    p = torch.as_tensor(planes).to(DEV)
    first = ops.knn(p, N, 8, graph.KNN_METRICS.index(metric))
    first = [t.clone() for t in first]
    for _ in range(2):
        again = ops.knn(p, N, 8, graph.KNN_METRICS.index(metric))
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_ops_knn_refuses_through_the_library():
    p = torch.zeros((3, ops.plane_stride(100)), device=DEV)
    with pytest.raises(_lib.ChebgcnError):
        ops.knn(p, 100, 33, 0)
    with pytest.raises(_lib.ChebgcnError):
        ops.knn(p, 100, 100, 0)
    with pytest.raises(_lib.ChebgcnError):
        ops.knn(p.cpu(), 100, 4, 0)


@pytest.mark.parametrize('name', ['cube', 'feat'])
@pytest.mark.parametrize('metric', METRICS)
def test_reference_fixture_through_knn_device(name, metric):
    """What the reference's own distance_sklearn_metrics + adjacency gave (tests/golden/knn_ref.npz), on the rows that pass the
    gap rule; where every row passes, the adjacency matrix as well."""
    g = load_golden('knn_ref')
    z, k = g['z_' + name], int(g['k'])
    key = '%s_%s' % (name, metric)
    d, idx, _ = run_knn(z, k, metric)
    d64, _ = knn64(z, k, metric)
    need = gap_rows(d64, k)
    assert need.mean() >= 1 - CAP
    assert np.array_equal(idx[need], g['idx_' + key][need])
    # looser than the 1e-5 parity bound on purpose: the fixture's d is sklearn's float32 output and carries the reference's own
    # Gram-form error; the parity bound itself is enforced against float64 by check1 in the grid
    np.testing.assert_allclose(d[need], g['d_' + key][need], rtol=2e-5, atol=2e-6)
    if need.all():
        A_ref = sp.csr_matrix((g['A_%s_data' % key], g['A_%s_indices' % key], g['A_%s_indptr' % key]),
                              shape=tuple(g['A_%s_shape' % key]))
        A = graph.adjacency(d, idx)
        assert abs(A - A_ref).max() <= 1e-4


# ---------------------------------------------------------------------------------------------- connectivity

def _mean_corr64(runs):
    acc = 0.0
    for r in runs:
        with np.errstate(invalid='ignore', divide='ignore'):
            c = np.corrcoef(r.astype(np.float64).T)
        acc = acc + np.nan_to_num(c, nan=0.0)          # a vertex constant in a run: correlation 0 with everything there
    return acc / len(runs)


def test_series_normalise_gram_is_the_mean_correlation():
    rs = np.random.RandomState(2)
    M = 70
    runs = [(rs.randn(T, M) * (1 + rs.rand(M)) + 3 * rs.randn(M)).astype(np.float32) for T in (31, 12, 50)]
    runs[1][:, 4] = 1.25
    Mp = ops.plane_stride(M)
    planes = np.zeros((93, Mp), np.float32)
    planes[:, :M] = np.concatenate(runs)
    offs = torch.as_tensor(np.array([0, 31, 43, 93], np.int64)).to(DEV)
    _lib.dispatch_log = log = []
    try:
        zn = ops.series_normalise(torch.as_tensor(planes).to(DEV), offs, M)
    finally:
        _lib.dispatch_log = None
    assert log == [('series_normalise', 'series_normalise_kernel')]
    zn = zn.cpu().numpy().astype(np.float64)
    assert (zn[:, M:] == 0).all() and (zn[31:43, 4] == 0).all()
    ref = _mean_corr64(runs)
    ref[4, 4] = 2.0 / 3.0
    err = np.abs(zn[:, :M].T @ zn[:, :M] / 3 - ref).max()
    record_measured('series_normalise_gram', err=err)
    assert err <= BOUND


def test_connectivity_graph_three_runs_of_unequal_length():
    M, k = 500, 8
    full = _latent_series(90 + 41 + 130, M, 23)
    full = (full + 1.5 * np.random.RandomState(5).randn(len(full), 1)).astype(np.float32) * 2.0 + 5.0      # a global signal: mean r well above 0
    runs = [full[:90].copy(), full[90:131].copy(), full[131:].copy()]
    runs[1][:, 17] = -3.0                                                  # constant in one run
    r = _mean_corr64(runs)
    dref = 1.0 - r
    np.fill_diagonal(dref, np.inf)
    i64 = np.argsort(dref, axis=1, kind='stable')[:, :k + 1]
    d64 = np.take_along_axis(dref, i64, 1)
    assert 1.0 - gap_rows(d64, k).mean() <= CAP
    _lib.dispatch_log = log = []
    try:
        d, idx, sigma = graph.connectivity_graph(runs, k=k, device=DEV, return_sigma=True)
    finally:
        _lib.dispatch_log = None
    assert [w for w, _ in log] == ['series_normalise', 'knn'] and 'knn_gram_kernel' in log[1][1]
    assert d.dtype == np.float32 and idx.dtype == np.int64 and d.shape == (M, k)
    got = np.take_along_axis(dref, idx, 1)
    e_set = np.abs(np.sort(got, axis=1) - d64[:, :k]).max()
    e_val = np.abs(d - got).max()
    record_measured('connectivity_graph', neighbour_set_err=e_set, dist_err=e_val, sigma_err=abs(sigma - r.mean()))
    assert e_set <= BOUND and e_val <= BOUND
    check2(k, idx, d64, i64)
    assert abs(sigma - r.mean()) <= BOUND
    d1, idx1 = graph.connectivity_graph(runs[0], k=k, device=DEV)         # one run, given as an array
    r0 = 1.0 - _mean_corr64(runs[:1])
    assert np.abs(d1 - np.take_along_axis(r0, idx1, 1)).max() <= BOUND
    # the reference's RSFC recipe continues on the host from the [N, k] tables
    w = np.exp((1.0 - d.astype(np.float64)) / sigma)
    w[w < 1] = 0
    A = graph.adjacency(w, idx)
    assert A.shape == (M, M) and abs(A - A.T).max() == 0


def test_connectivity_graph_of_at_most_eight_time_points_runs_the_direct_arm():
    """The DOT metric on the direct arm: runs of 3 + 2 + 3 time points."""
    M, k = 400, 4
    rs = np.random.RandomState(31)
    runs = [rs.randn(T, M).astype(np.float32) for T in (3, 2, 3)]
    dref = 1.0 - _mean_corr64(runs)
    np.fill_diagonal(dref, np.inf)
    d64 = np.sort(dref, axis=1)[:, :k]
    _lib.dispatch_log = log = []
    try:
        d, idx = graph.connectivity_graph(runs, k=k, device=DEV)
    finally:
        _lib.dispatch_log = None
    assert 'knn_direct_kernel' in log[1][1], log
    got = np.take_along_axis(dref, idx, 1)
    assert np.abs(np.sort(got, axis=1) - d64).max() <= BOUND and np.abs(d - got).max() <= BOUND
    assert (idx != np.arange(M)[:, None]).all()


def test_connectivity_graph_arrays_tensors_and_mixed_agree_to_the_bit():
    """Runs of 2, 3 and 9 rows at M = 33 (one vertex beyond a plane stride of 32), staged from arrays, from device tensors and
    from both."""
    M, k = 33, 4
    rs = np.random.RandomState(37)
    runs = [rs.randn(T, M).astype(np.float32) for T in (2, 3, 9)]
    on_device = [torch.as_tensor(r).to(DEV) for r in runs]
    d, idx = graph.connectivity_graph(runs, k=k, device=DEV)
    assert d.shape == (M, k) and np.isfinite(d).all() and (idx != np.arange(M)[:, None]).all()
    for given in (on_device, [runs[0], on_device[1], runs[2]]):
        d2, idx2 = graph.connectivity_graph(given, k=k, device=DEV)
        assert np.array_equal(d2, d) and np.array_equal(idx2, idx)


def test_series_normalise_refuses_mismatched_arguments():
    M = 70
    p = torch.zeros((10, ops.plane_stride(M)), device=DEV)
    offs = torch.as_tensor(np.array([0, 10], np.int64)).to(DEV)
    for bad in (lambda: ops.series_normalise(p, offs, 200), lambda: ops.series_normalise(p.double(), offs, M),
                lambda: ops.series_normalise(p.t(), offs, M), lambda: ops.series_normalise(p, offs.int(), M),
                lambda: ops.series_normalise(p, offs, M, out=torch.zeros((9, p.shape[1]), device=DEV)),
                lambda: ops.series_normalise(p, offs, M, out=p),
                lambda: ops.series_normalise(p, torch.as_tensor(np.array([0, 11], np.int64)).to(DEV), M)):
        with pytest.raises(_lib.ChebgcnError):
            bad()


# ---------------------------------------------------------------------------------------------- into the model

def test_adjacency_of_device_knn_and_a_training_step():
    z = np.random.RandomState(4).rand(2000, 3).astype(np.float32)
    A = graph.adjacency(*graph.knn_device(z, k=8, device=DEV))
    assert sp.isspmatrix_csr(A) and A.shape == (2000, 2000)
    assert abs(A - A.T).max() == 0 and A.diagonal().max() == 0 and A.nnz >= 2000 * 8
    N = 600
    Ls_dev, perm_dev, _ = graph.synthetic_graph(N, k=6, levels=0, seed=3, knn='device')
    Ls_host, perm_host, _ = graph.synthetic_graph(N, k=6, levels=0, seed=3)
    assert np.array_equal(np.asarray(perm_dev), np.asarray(perm_host))
    for a, b in zip(Ls_dev, Ls_host):
        a, b = sp.csr_matrix(a), sp.csr_matrix(b)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        np.testing.assert_allclose(a.data, b.data, rtol=1e-4, atol=1e-6)
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, [Ls_dev[0], Ls_dev[0]], [4, 6], [3, 3], [1, 1], [9, 5], channel=3, brelu='b1relu',
                           batch_size=8, verbose=False, dropout=1)
    rs = np.random.RandomState(0)
    x = torch.as_tensor(rs.randn(8, N, 3).astype(np.float32)).to(DEV)
    labels = torch.as_tensor(rs.randint(0, 5, 8)).to(DEV)
    _, loss = net.train_step(ops.plane_storage(x), labels)
    assert np.isfinite(float(loss))
