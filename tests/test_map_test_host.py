"""``stats.map_test_host`` and ``stats.sign_flips`` without a device: the draws against the project's generator, labels, extents and
TFCE against a breadth-first search written here, the properties of the exact test, and the power of TFCE on a planted blob."""
import numpy as np
import pytest
import scipy.sparse as sp

import map_test_cases as cases
from gcn_fmri_decoding_amd import stats


def test_sign_flips_restate_the_projects_generator():
    from gcn_fmri_decoding_amd import series
    S, P, seed = 37, 50, 1234
    signs, exact = stats.sign_flips(S, P, seed)
    assert signs.shape == (P, S) and signs.dtype == np.int8 and not exact
    assert (signs[0] == 1).all()
    u = series.aug_draw(seed, 0, np.arange(P, dtype=np.uint64)[:, None], np.arange(S, dtype=np.uint64)[None, :])
    want = np.where((u >> np.uint64(31)) & np.uint64(1), -1, 1)
    assert np.array_equal(signs[1:], want[1:])
    assert set(np.unique(signs)) == {-1, 1}
    assert 0.4 < (signs[1:] < 0).mean() < 0.6
    other, _ = stats.sign_flips(S, P, seed + 1)
    assert not np.array_equal(other[1:], signs[1:])


def test_sign_flips_enumerate_when_they_fit():
    signs, exact = stats.sign_flips(6, 64, 0)
    assert exact and signs.shape == (64, 6) and (signs[0] == 1).all()
    assert len({tuple(r) for r in signs.tolist()}) == 64
    q = np.arange(64)
    for j in range(6):
        assert np.array_equal(signs[:, j] < 0, ((q >> j) & 1) == 1)
    signs, exact = stats.sign_flips(6, 1000, 0)
    assert exact and signs.shape == (64, 6)
    signs, exact = stats.sign_flips(6, 63, 0)
    assert not exact and signs.shape == (63, 6)


GRAPHS = {
    'path': lambda: cases.path(33),
    'path_shuffled': lambda: cases.path(40, np.random.RandomState(5).permutation(40)),
    'ring': lambda: cases.ring(29),
    'star': lambda: cases.star(31, centre=17),
    'two_components_isolated': lambda: cases.two_components_with_isolated(40),
    'random': lambda: cases.random_graph(37, 3, 2),
    'single': lambda: cases.from_edges(1, []),
}


@pytest.mark.parametrize('name', sorted(GRAPHS))
@pytest.mark.parametrize('stat', ['tfce', 'extent'])
def test_labels_extents_and_tfce_against_breadth_first_search(name, stat):
    A = GRAPHS[name]()
    M = A.shape[0]
    S, P = 7, 9
    x = cases.smooth_maps(S, M, seed=len(name), A=A)
    kw = dict(stat=stat, n_perm=P, tail=1, seed=3)
    if stat == 'extent':
        kw['threshold'] = 0.7
    else:
        kw['step'] = 0.11
    res = stats.map_test_host(x, A, **kw)
    signs, _ = stats.sign_flips(S, P, 3)
    t = stats.t_host(x, signs)
    nb = cases.neighbours(A)
    assert np.array_equal(res.t, t[0])
    null = []
    for k in range(P):
        st, lab = cases.enhance_python(t[k], nb, stat, threshold=kw.get('threshold'), step=kw.get('step'))
        null.append(st.max())
        if k == 0:
            assert np.array_equal(res.stat, st)
            if stat == 'extent':
                assert np.array_equal(res.labels, np.array(lab, np.int32))
                assert (res.labels >= 0).any() or M == 1
                for v in range(M):              # an extent is the number of vertices that carry the cluster's id
                    assert res.stat[v] == (0 if lab[v] < 0 else lab.count(lab[v]))
            else:
                assert res.labels is None
    assert np.array_equal(res.null, np.array(null))
    assert np.array_equal(res.p, np.array([(np.array(null) >= s).sum() / P for s in res.stat]))


def test_two_sided_carries_each_signs_part():
    A = cases.ring(30)
    x = cases.smooth_maps(8, 30, seed=4, A=A)
    x[:, 15:25] -= 1.5
    res = stats.map_test_host(x, A, stat='tfce', n_perm=12, tail=0, step=0.2, seed=1)
    nb = cases.neighbours(A)
    pos, _ = cases.enhance_python(res.t, nb, 'tfce', step=0.2)
    neg, _ = cases.enhance_python(-res.t, nb, 'tfce', step=0.2)
    assert (res.t > 0).any() and (res.t < 0).any()
    assert np.array_equal(res.stat, np.where(res.t > 0, pos, np.where(res.t < 0, neg, 0.0)))
    assert res.null[0] == max(pos.max(), neg.max())


def test_exact_test_properties():
    A = cases.ring(24)
    x = cases.smooth_maps(6, 24, seed=9, A=A)
    for stat, kw in (('tfce', {'step': 0.25}), ('max', {}), ('extent', {'threshold': 1.0})):
        one = stats.map_test_host(x, A, stat=stat, n_perm=64, tail=1, **kw)
        assert one.exact and one.n_perm == 64 and one.null.shape == (64,)
        assert np.array_equal(one.p * 64, np.round(one.p * 64)) and one.p.min() >= 1 / 64 and one.p.max() <= 1
        flipped = stats.map_test_host(-x, A, stat=stat, n_perm=64, tail=-1, **kw)
        for a, b in zip(one, flipped):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        two = stats.map_test_host(x, A, stat=stat, n_perm=64, tail=0, **kw)
        neg = stats.map_test_host(-x, A, stat=stat, n_perm=64, tail=0, **kw)
        assert np.array_equal(two.t, -neg.t)
        assert np.array_equal(two.stat, neg.stat) and np.array_equal(two.p, neg.p)
        # (the null of an exact test is the same multiset whichever sign the data carries: the enumeration is closed under it)
        assert np.array_equal(np.sort(two.null), np.sort(neg.null))
        if stat == 'extent':
            assert np.array_equal(two.labels, neg.labels)


def test_classes_share_the_flips_and_the_class_axis_drops():
    A = cases.ring(20)
    x = np.stack([cases.smooth_maps(9, 20, seed=s, A=A) for s in range(3)], 1)         # [S, C, M]
    res = stats.map_test_host(x, A, n_perm=20, tail=1, seed=2)
    assert res.t.shape == (3, 20) and res.null.shape == (3, 20) and res.step.shape == (3,)
    for c in range(3):
        one = stats.map_test_host(x[:, c], A, n_perm=20, tail=1, seed=2)
        assert one.t.shape == (20,) and isinstance(one.step, float)
        assert np.array_equal(one.stat, res.stat[c]) and np.array_equal(one.null, res.null[c]) and np.array_equal(one.p, res.p[c])
        assert one.step == res.step[c] == float(one.t.max()) / 100


def test_laplacian_is_accepted_as_the_graph():
    from gcn_fmri_decoding_amd import graph
    A = cases.random_graph(30, 4, 1)
    W = sp.csr_matrix(A.maximum(A.T))
    W.setdiag(0)
    W.eliminate_zeros()
    x = cases.smooth_maps(6, 30, seed=0, A=A)
    a = stats.map_test_host(x, A, n_perm=10, tail=1)              # one direction of every edge only
    b = stats.map_test_host(x, graph.laplacian(W, normalized=True), n_perm=10, tail=1)
    assert np.array_equal(a.stat, b.stat) and np.array_equal(a.null, b.null)


def test_planted_blob_tfce_finds_what_max_t_misses():
    """19 x 19 grid, 12 subjects, unit noise plus 1.2 on a 5 x 5 block, 200 sign flips of the project's generator (seed 0).
    Measured: 'tfce' marks 21 of the 25 block vertices and none outside, 'max' marks 5."""
    n, S = 19, 12
    A = cases.grid(n)
    x = np.random.RandomState(0).randn(S, n, n)
    x[:, 3:8, 3:8] += 1.2
    x = x.reshape(S, n * n).astype(np.float32)
    block = np.zeros((n, n), bool)
    block[3:8, 3:8] = True
    grown = np.zeros((n, n), bool)
    grown[2:9, 3:8] = grown[3:8, 2:9] = True
    tfce = stats.map_test_host(x, A, stat='tfce', n_perm=200, tail=1)
    vmax = stats.map_test_host(x, A, stat='max', n_perm=200, tail=1)
    sig = (tfce.p < 0.05).reshape(n, n)
    print('tfce inside %d outside %d, max %d' % (sig[block].sum(), sig[~grown].sum(), (vmax.p < 0.05).sum()))
    assert not tfce.exact and tfce.n_perm == 200
    assert sig[block].sum() >= 13
    assert sig[~grown].sum() == 0
    assert sig.sum() > (vmax.p < 0.05).sum()


def test_argument_errors():
    A = cases.ring(10)
    x = cases.smooth_maps(5, 10, seed=0)
    bad = x.copy()
    bad[2, 3] = np.inf
    for fn in (stats.map_test_host, stats.map_test):            # the device entry refuses them before it touches the device
        with pytest.raises(ValueError):
            fn(x[:1], A)                                        # S = 1
        with pytest.raises(ValueError):
            fn(x, cases.ring(11))                               # wrong M
        with pytest.raises(ValueError):
            fn(bad, A)
        with pytest.raises(ValueError):
            fn(np.where(np.isinf(bad), np.nan, bad), A)
        with pytest.raises(ValueError):
            fn(x, A, stat='extent')                             # no threshold
        with pytest.raises(ValueError):
            fn(x, A, E=np.nan)
        with pytest.raises(ValueError):
            fn(x, A, H=np.inf)
        with pytest.raises(ValueError):
            fn(x, A, n_perm=0)
        with pytest.raises(ValueError):
            fn(x, A, stat='mass')
        with pytest.raises(ValueError):
            fn(x, A, tail=2)
        with pytest.raises(ValueError):
            fn(x, A, step=0.0)
        with pytest.raises(ValueError):
            fn(x, A.toarray())                                  # not sparse
        with pytest.raises(ValueError):
            fn(x[:, None, None, :], A)
