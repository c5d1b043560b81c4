"""``searchlight.crossnobis`` on the device (chebgcn_searchlight_fit with one model per cell, then chebgcn_searchlight_rdm per
bucket of row length and batch of centres) against its float64 host restatement ``searchlight.crossnobis_host``, which slices
every ball out, forms the residuals with NumPy, factorises with SciPy and takes the distance in the explicit double sum over
pairs of different cells.  Shapes come from ``ops.searchlight_rdm_geometry()``.

The bound, for EVERY distance:  ``|got - ref| <= B scale``,  ``scale = kappa (t_ab + q_ab) / (F (F - 1) P)`` from the reference,
``kappa`` the 2-norm condition number of that (group, centre)'s ``Sigma``: the magnitude a float64 evaluation may be off by.
``B = BOUND`` is set near 10x the worst ratio measured on an MI355X against the host restatement -- float64 round-off and
nothing else (the two sides sum the means and the covariance in different orders, factorise with different kernels and take the
distance by different formulas).  A covariance accumulated in float32 misses the bound on the P = 127, g = 0.01 rows at mean
1e4 / sd 50 (asserted on the CPU in the parity test).

``B = 1e-14``.  Measured on an MI355X (``record_measured`` keeps every case's figures), as fractions of ``scale``: worst 8.3e-16
(``shrinkage='auto'`` on rows sharing one strong factor at mean 1e4 / sd 50), 3.6e-16 on the tile-edge lists with ``'auto'``,
3.3e-16 on the edge rows at mean 0, 2.3e-16 at mean 1e4 / sd 50, 1.4e-16 with cells of 72 samples per class at mean / sd = 100,
3.1e-16 at 32 classes.  The float32 covariance is off by 8.9e-9 of ``scale``: it misses the bound by 8.9e5.  The shrinkage the
kernel reports agrees with ``lda_shrinkage_host`` to 1.6e-15 relative, and exactly where the rule clips.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, crossnobis, crossnobis_events, crossnobis_host, events, lda_shrinkage_host, searchlight as sl

pytestmark = pytest.mark.gpu

BOUND = 1e-14
EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128]                   # every bucket at its edges


@pytest.fixture(scope='module')
def geo():
    from gcn_fmri_decoding_amd import ops
    g = ops.searchlight_rdm_geometry()
    assert [g['buckets'][P] for P in EDGES] == [32, 32, 32, 64, 64, 64, 128, 128, 128] and g['max_P'] == sl.LDA_PMAX
    assert g['threads'] == 256 and g['tile'] == 32 and g['narrow'] == 8 and g['max_C'] == 32 and g['max_pairs'] == 496
    return g


def data(rng, S, M, C, mean=100.0, sd=1.0, parts=4, common=0.0):
    """Balanced classes whose means differ by 0.5 sd per vertex; every (partition, class) cell holds S / (parts C) samples.
    ``common``: the sd (in units of sd) of one noise all vertices share."""
    y = np.arange(S) % C
    part = np.arange(S) // C % parts
    X = (mean + sd * rng.randn(S, M) + common * sd * rng.randn(S, 1) + 0.5 * sd * rng.randn(C, M)[y]).astype(np.float32)
    return X, y, part


def rows_of(M, lengths, step=7):
    """Row i: ``lengths[i]`` consecutive vertices from ``step * i``."""
    r = sp.lil_matrix((len(lengths), M))
    for i, P in enumerate(lengths):
        assert step * i + P <= M
        r[i, step * i:step * i + P] = 1
    return r.tocsr()


def launches_of(nb, geo, batch=None):
    """The buckets of the launches one call makes, in order: the buckets ascending, each cut into batches of centres."""
    of_row = [geo['buckets'][int(n)] for n in np.diff(nb.indptr)]
    out = []
    for b in sorted(set(of_row)):
        n = of_row.count(b)
        out += [b] * (1 if batch is None else -(-n // min(batch, n)))
    return out


def run_device(args, kw, launches, head=(), fn=crossnobis):
    """``crossnobis`` (or ``crossnobis_events``) with the dispatch log checked: exactly the fit, then one ``searchlight_rdm`` per
    (bucket, batch) on the bucket's arm."""
    _lib.dispatch_log = log = []
    try:
        res = fn(*args, **kw)
    finally:
        _lib.dispatch_log = None
    assert [w for w, _ in log] == list(head) + ['searchlight_fit'] + ['searchlight_rdm'] * len(launches), log
    assert [d for w, d in log if w.startswith('searchlight')] == ['searchlight_fit_kernel'] + ['searchlight_rdm_kernel<%d>' % b for b in launches]
    return res


def against_host(name, args, kw, geo, batch=None):
    """Device against host the way the module's docstring states it; returns ``(device result, host result, scale)``."""
    ref, scale = crossnobis_host(*args, return_scale=True, **kw)
    nb = sp.csr_matrix(args[2])
    res = run_device(args, dict(kw, batch_centres=batch), launches_of(nb, geo, batch))
    assert isinstance(res.rdm, np.ndarray) and res.rdm.shape == ref.rdm.shape and res.rdm.dtype == np.float64 and np.isfinite(res.rdm).all()
    assert res.shrinkage.shape == ref.shrinkage.shape and res.shrinkage.dtype == np.float64
    assert res.groups == ref.groups and res.classes == ref.classes and np.array_equal(res.pairs, ref.pairs)
    assert np.array_equal(res.folds, ref.folds)
    assert np.array_equal(res.shrinkage == -1, ref.shrinkage == -1)
    frac = float((np.abs(res.rdm - ref.rdm) / (BOUND * scale + 1e-300)).max())
    record_measured(name, bound_used=frac, of_scale=frac * BOUND)
    print(name, 'distances at %.3g of the bound (%.3g of scale)' % (frac, frac * BOUND))
    assert frac <= 1.0, '%s: a distance is off by %.3f of its bound' % (name, frac)
    return res, ref, scale


def ball_rdm(A, y, part, g, acc):
    """The RDM of one ball with the covariance accumulated in ``acc`` precision; everything else float64."""
    parts, C, P = np.unique(part), int(y.max()) + 1, A.shape[1]
    F = len(parts)
    mu = np.stack([np.stack([A[(part == k) & (y == c)].mean(axis=0) for c in range(C)]) for k in parts])
    R = np.concatenate([A[(part == k) & (y == c)] - mu[i, c] for i, k in enumerate(parts) for c in range(C)]).astype(acc)
    S = (R.T @ R).astype(np.float64) / len(A)
    L = np.linalg.cholesky((1.0 - g) * S + g * np.trace(S) / P * np.eye(P))
    w = np.linalg.solve(L, (mu - A.mean(axis=0)).reshape(-1, P).T).T.reshape(F, C, P)
    out = []
    for a in range(C):
        for b in range(a + 1, C):
            d = w[:, a] - w[:, b]
            out.append(sum(d[k] @ d[l] for k in range(F) for l in range(F) if k != l) / (F * (F - 1) * P))
    return np.array(out)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mean,sd', [(100.0, 1.0), (1e4, 50.0), (0.0, 1.0)])
@pytest.mark.parametrize('g', [0.01, 0.1])
def test_parity_on_rows_at_the_bucket_edges(mean, sd, g, geo):
    """96 samples for up to 128 vertices: S is singular from P = 85 on, the normal case."""
    rng = np.random.RandomState(int(mean) + 1)
    X, y, part = data(rng, 96, 200, 3, mean, sd)
    nb = rows_of(200, EDGES)
    res, ref, scale = against_host('rsa_parity_mean%g_g%g' % (mean, g), (X, y, nb, part), dict(shrinkage=g), geo)
    assert res.rdm.shape == (1, 3, 9) and (res.shrinkage == g).all() and res.folds.tolist() == [4]
    if mean == 1e4 and g == 0.01:                               # the same covariance summed in float32 misses the bound
        u = EDGES.index(127)
        cols = np.arange(7 * u, 7 * u + 127)
        A = X.astype(np.float64)[:, cols]
        d64, d32 = ball_rdm(A, y, part, g, np.float64), ball_rdm(A, y, part, g, np.float32)
        assert (np.abs(d64 - ref.rdm[0, :, u]) <= BOUND * scale[0, :, u]).all()
        miss = float((np.abs(d32 - d64) / (BOUND * scale[0, :, u])).max())
        record_measured('rsa_float32_covariance', misses_by=miss)
        print('a float32 covariance misses the bound by %.3g' % miss)
        assert miss > 1.0, miss


def test_one_call_equals_one_call_per_row_and_any_batching(geo):
    import torch
    rng = np.random.RandomState(2)
    X, y, part = data(rng, 96, 200, 3, 1e4, 50.0)
    lengths = [128, 1, 64, 33, 31, 2, 3, 127, 32, 4, 5, 65, 63, 6, 7, 8, 9]        # eleven rows in bucket 32, three in the others
    nb = rows_of(200, lengths, step=4)
    kw = dict(shrinkage=0.01)
    whole = run_device((X, y, nb, part), kw, [32, 64, 128])
    for b, launches in ((1, [32] * 11 + [64] * 3 + [128] * 3), (7, [32, 32, 64, 128])):
        assert launches == launches_of(nb, geo, b)
        cut = run_device((X, y, nb, part), dict(kw, batch_centres=b), launches)
        assert np.array_equal(cut.rdm, whole.rdm) and np.array_equal(cut.shrinkage, whole.shrinkage), b
    for u, P in enumerate(lengths):
        if P in EDGES:
            alone = run_device((X, y, nb[u], part), kw, [geo['buckets'][P]])
            assert np.array_equal(alone.rdm[:, :, 0], whole.rdm[:, :, u]), P
    back = run_device((X, y, nb[::-1], part), kw, [32, 64, 128])                # the centres in another order
    assert np.array_equal(back.rdm[:, :, ::-1], whole.rdm)
    tens = run_device((torch.as_tensor(X).cuda(), y, nb, part), kw, [32, 64, 128])
    assert torch.is_tensor(tens.rdm) and tens.rdm.is_cuda and tens.rdm.dtype == torch.float64 and tens.shrinkage.is_cuda
    assert np.array_equal(tens.rdm.cpu().numpy(), whole.rdm) and np.array_equal(tens.shrinkage.cpu().numpy(), whole.shrinkage)
    sq = tens.square(0)
    assert torch.is_tensor(sq) and np.array_equal(sq.cpu().numpy(), whole.square(0))
    maps = tens.model_maps([[1.0, 0.0, 1.0]], 'cosine')
    assert torch.is_tensor(maps) and np.allclose(maps.cpu().numpy(), whole.model_maps([[1.0, 0.0, 1.0]], 'cosine'), rtol=1e-12, atol=0)


# ---- 2. classes, partitions, cells ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', ['2', '8', '9', 'Cmax'])
def test_class_counts_in_every_bucket(C, geo):
    """2 and 8 classes: the narrow class tables; 9 and 32 (496 pairs, two per thread): the wide ones, in each ball bucket."""
    C = geo['max_C'] if C == 'Cmax' else int(C)
    assert (C <= geo['narrow']) == (C in (2, 8)) and (C * (C - 1) // 2 > geo['threads']) == (C == 32)
    X, y, part = data(np.random.RandomState(C), 4 * C, 70, C, parts=2)
    res, _, _ = against_host('rsa_C%d' % C, (X, y, rows_of(70, [3, 40, 70], step=0), part), {}, geo)
    assert res.rdm.shape == (1, C * (C - 1) // 2, 3) and len(res.pairs) == C * (C - 1) // 2


def test_three_groups_of_2_3_and_5_partitions_in_one_call(geo):
    rng = np.random.RandomState(20)
    S, M = 180, 40
    X, y, part = data(rng, S, M, 3, mean=1000.0, sd=5.0, parts=5, common=1.0)
    groups = np.array(['s2', 's1', 's3'])[np.arange(S) // 15 % 3]          # (15 samples: one round of the 5 x 3 cells)
    part = np.where(groups == 's2', part % 2, np.where(groups == 's1', part % 3, part)) + 4
    balls = sp.vstack([rows_of(M, [5, 9, 33], step=2), rows_of(M, [40], step=0)]).tocsr()
    res, ref, _ = against_host('rsa_groups', (X, y, balls, part), dict(groups=groups), geo)
    assert res.groups == ['s2', 's1', 's3'] and res.folds.tolist() == [2, 3, 5] and res.rdm.shape == (3, 3, 4)
    for g, key in enumerate(res.groups):                        # a group alone: the same bits
        own = groups == key
        alone = run_device((X[own], y[own], balls, part[own]), {}, [32, 64])
        assert np.array_equal(alone.rdm[0], res.rdm[g]) and np.array_equal(alone.shrinkage[0], res.shrinkage[g])


def test_cells_of_one_sample_and_lists_across_the_tile_edge(geo):
    """Cell 0 holds one sample per class (zero residuals from that cell); the class lists of the other cells hold 31, 32 and 33
    samples: up to, at and across the 32-sample tile."""
    rng = np.random.RandomState(21)
    sizes = [(0, 1), (1, 31), (2, 32), (3, 33)]
    assert geo['tile'] == 32
    y = np.concatenate([np.repeat([0, 1], n) for _, n in sizes])
    part = np.concatenate([np.full(2 * n, k) for k, n in sizes])
    order = rng.permutation(y.size)
    y, part = y[order], part[order]
    M = 70
    X = (100.0 + rng.randn(y.size, M) + 0.5 * rng.randn(2, M)[y]).astype(np.float32)
    against_host('rsa_small_cells', (X, y, rows_of(M, [4, 40, 70], step=0), part), {}, geo)
    for g in (0.1, 'auto'):
        against_host('rsa_tile_edge_g%s' % g, (X[part > 0], y[part > 0], rows_of(M, [4, 40, 70], step=0), part[part > 0]),
                     dict(shrinkage=g), geo)


def test_cells_of_72_samples_per_class(geo):
    """576 samples at mean / sd = 100: the cell means -- a plain chain on the device, pairwise sums in NumPy -- differ most."""
    X, y, part = data(np.random.RandomState(22), 576, 70, 2, parts=4)
    against_host('rsa_large_cells', (X, y, rows_of(70, [3, 40, 70], step=0), part), dict(shrinkage=0.01), geo)


def test_nan_in_the_pad_of_the_patterns_stays_there(geo):
    import torch
    X, y, part = data(np.random.RandomState(14), 45, 33, 3, parts=3)
    balls = rows_of(33, [5, 33, 20], step=0)
    res = run_device((X, y, balls, part), {}, [32, 64])
    a = sl._check_rdm(X, y, balls, part, None, None, 0.1, None, 't')
    plan = sl._rdm_plan(a)
    dev = torch.device('cuda')
    Xt = sl._transposed(torch.as_tensor(X).to(dev), plan.order, dev)
    assert Xt.shape == (33, 64)
    Xt[:, 45:] = float('nan')
    rdm, gam = sl._run_rdm(a, plan, Xt, None)
    assert np.array_equal(rdm.cpu().numpy(), res.rdm) and np.array_equal(gam.cpu().numpy(), res.shrinkage)


# ---- 3. degenerate balls, 'auto' ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('g', [1e-6, 0.1, 1, 'auto'])
def test_all_zero_and_partly_zero_balls(g, geo):
    rng = np.random.RandomState(41)
    S, M = 48, 40
    X, y, part = data(rng, S, M, 3, parts=2)
    X[:, 20:] = 0.0
    nb = sp.vstack([rows_of(M, [6, 20], step=0), rows_of(M, [20], step=0)[:, ::-1], rows_of(M, [34], step=0)[:, ::-1]]).tocsr()
    res, ref, _ = against_host('rsa_zero_balls_g%s' % g, (X, y, nb, part), dict(shrinkage=g), geo)
    assert np.isfinite(res.rdm).all() and np.isfinite(res.shrinkage).all()
    assert (res.rdm[0, :, 2] == 0).all() and res.shrinkage[0, 2] == -1                  # the all-zero ball
    assert (res.shrinkage[0, [0, 1, 3]] > 0).all() and (res.rdm[0][:, [0, 1, 3]] != 0).all()


def test_ledoit_wolf_shrinkage(geo):
    """``shrinkage='auto'``: the distances against the host, and the shrinkage the kernel reports against ``lda_shrinkage_host``
    on the cell-centred residuals to 1e-14 relative: rows with a common factor and a row of 5 vertices on which one sample is a
    1000-sd outlier (g inside (0, 1)), the first 2 of those 5 vertices (the outlier's cell of 8 samples makes beta / delta about
    2 x 0.76 > 1: beta is cut to delta and g = 1) and a row of two vertices whose residuals are all +-(3, 5) exactly (beta = 0:
    g = 0, clipped to ``SHRINK_MIN``).  Where
    the rule clips, the device gives the limit exactly."""
    rng = np.random.RandomState(42)
    S, M, C = 96, 230, 3
    X, y, part = data(rng, S, M, C, 1e4, 50.0)
    X[:, :110] += (100.0 * rng.randn(S, 1)).astype(np.float32)                    # vertices 0 .. 109 share one strong noise
    X[0, 115:120] += 5e4                                        # sample 0: an outlier on vertices 115 .. 119
    sgn = np.where(np.arange(S) // 12 % 2 == 0, 1.0, -1.0)      # four of the 8 samples of every cell each way
    X[:, 120:122] = (100.0 + 10.0 * part + y)[:, None] + sgn[:, None] * np.array([3.0, 5.0])
    spans = [(0, 5), (0, 40), (0, 100), (115, 120), (115, 117), (120, 122)]
    nb = sp.csr_matrix(np.array([[float(lo <= v < hi) for v in range(M)] for lo, hi in spans]))
    res, _, _ = against_host('rsa_auto', (X, y, nb, part), dict(shrinkage='auto'), geo)
    X64 = X.astype(np.float64)
    worst, clipped = 0.0, set()
    for u in range(len(spans)):
        A = X64[:, nb[u].indices]
        R = np.concatenate([A[(part == k) & (y == c)] - A[(part == k) & (y == c)].mean(axis=0) for k in range(4) for c in range(C)])
        want = lda_shrinkage_host(R)
        worst = max(worst, abs(res.shrinkage[0, u] - want) / want)
        if want in (sl.SHRINK_MIN, 1.0):
            assert res.shrinkage[0, u] == want, (u, want, res.shrinkage[0, u])
            clipped.add((u, want))
        else:
            assert u < 4, (u, want)
    record_measured('rsa_gamma', rel=worst)
    print('shrinkage against lda_shrinkage_host: %.3g' % worst)
    assert worst <= 1e-14, worst
    assert clipped == {(4, 1.0), (5, sl.SHRINK_MIN)}, clipped


# ---- 4. the neighbours ----------------------------------------------------------------------------------------------------------

def test_lda_after_crossnobis_is_what_it_was(geo):
    rng = np.random.RandomState(50)
    X, y, fold = data(rng, 48, 40, 3, parts=2)
    nb = rows_of(40, [5, 33], step=0)

    def lda():
        _lib.dispatch_log = log = []
        try:
            res = sl.searchlight(X, y, nb, fold, classifier='lda', scores=True)
        finally:
            _lib.dispatch_log = None
        return res, log
    before, log0 = lda()
    run_device((X, y, nb, fold), {}, [32, 64])
    after, log1 = lda()
    assert log0 == log1 == [('searchlight_fit', 'searchlight_fit_kernel'), ('searchlight_lda', 'searchlight_lda_kernel<32>'),
                            ('searchlight_lda', 'searchlight_lda_kernel<64>')]
    assert np.array_equal(before.scores, after.scores) and np.array_equal(before.correct, after.correct)


def test_crossnobis_events_end_to_end(geo):
    import torch
    rng = np.random.RandomState(60)
    M, dura = 40, 4
    names = ['rest'] * 3 + ['a'] * 8 + ['rest'] * 2 + ['b'] * 9 + ['rest'] * 3 + ['a'] * 5 + ['rest'] + ['b'] * 8 + ['rest'] * 2
    T = len(names)
    subjects = ['s1', 's1', 's2', 's2', 's2']
    labels = [names, names[::-1], names, names[::-1], names]
    # vertices 10 .. 19 share a large noise; b moves the even ones against the odd ones
    sign = np.where(np.arange(M) % 2 == 0, 1.0, -1.0) * ((np.arange(M) >= 10) & (np.arange(M) < 20))
    runs = [(1000.0 + 0.5 * rng.randn(T, M) + 30.0 * rng.randn(T, 1) * (sign != 0) + 1.0 * sign * np.array([float(n == 'b') for n in run])[:, None]
             ).astype(np.float32) for run in labels]
    balls = rows_of(M, [5] * 8, step=5)
    ev = events.match_events(labels, ['a', 'b'], dura)
    want = np.concatenate([events.host_windows(runs[r], i, fold=dura)[:, :, 0] for r, i in zip(ev.kept, ev.index)])
    idx, lab, tg, tp, classes = sl._events_plan([T] * 5, labels, ['a', 'b'], dura, subjects, np.arange(5), True, {})
    assert sorted(set(tp.tolist())) == [0, 1, 2, 3, 4]
    res = run_device((runs, labels, ['a', 'b'], dura, balls), dict(groups=subjects, shrinkage=0.01), [32], head=['gather_windows_indexed'],
                     fn=crossnobis_events)
    direct = run_device((want, lab, balls, tp), dict(groups=tg, classes=classes, shrinkage=0.01), [32])
    assert res.groups == ['s1', 's2'] and res.classes == ['a', 'b'] and res.folds.tolist() == [2, 3] and isinstance(res.rdm, np.ndarray)
    assert np.array_equal(res.rdm, direct.rdm) and np.array_equal(res.shrinkage, direct.shrinkage)
    host, scale = crossnobis_host(want, lab, balls, tp, groups=tg, classes=classes, shrinkage=0.01, return_scale=True)
    assert (np.abs(res.rdm - host.rdm) <= BOUND * scale).all()
    # inside the patch: the shift of +-1 on 5 vertices, less its part along the shared noise, over the shrunk independent variance
    # 0.99 * 0.5^2 / 4 + 0.01 nu, nu about 30^2 / 4: (5 - 1 / 5) / 2.3 / 5 = 0.42 expected; half of that is asked
    inside = res.rdm[:, 0, 2:4]
    print('distance a-b inside the patch', inside)
    assert (inside > 0.2).all(), inside
    tens = run_device(([torch.as_tensor(r).cuda() for r in runs], labels, ['a', 'b'], dura, balls), dict(groups=subjects, shrinkage=0.01),
                      [32], head=['gather_windows_indexed'], fn=crossnobis_events)
    assert torch.is_tensor(tens.rdm) and np.array_equal(tens.rdm.cpu().numpy(), res.rdm)
