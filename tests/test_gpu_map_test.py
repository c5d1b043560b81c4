"""``stats.map_test`` on the device against its host restatement ``stats.map_test_host``: exact agreement in t, statistic, null
and p (and labels for 'extent') in both arms of ``chebgcn_cluster_enhance``, at the edges of the arms and on the graphs that are
hardest for a union-find.  Shapes come from ``ops.cluster_geometry()``."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import map_test_cases as cases
from gcn_fmri_decoding_amd import _lib, stats

pytestmark = pytest.mark.gpu

ONCHIP = 'cluster_onchip_kernel'
STREAMED = ('cluster_prep_kernel + cluster_hook_kernel + cluster_flatten_kernel + cluster_count_kernel + cluster_accum_kernel + '
            'cluster_final_kernel<state>')
PLAIN = 'cluster_final_kernel<plain>'


@pytest.fixture(scope='module')
def LIM():
    from gcn_fmri_decoding_amd import ops
    return ops.cluster_geometry()['onchip_M']


def assert_same(a, b):
    for name, u, v in zip(a._fields, a, b):
        if isinstance(u, np.ndarray):
            assert u.dtype == v.dtype and u.shape == v.shape, name
            assert np.array_equal(u, v), '%s differs at %d places' % (name, int((u != v).sum()))
        else:
            assert u == v, name


def both(x, A, arm, **kw):
    """Device result (twice: identical) against the host twin; the arm the last launch took."""
    _lib.dispatch_log = log = []
    try:
        dev = stats.map_test(x, A, **kw)
    finally:
        _lib.dispatch_log = None
    took = {d for what, d in log if what == 'cluster_enhance'}
    assert took == {arm}, took
    assert {d for what, d in log if what == 'signflip_t'} == {'signflip_t_kernel'}
    assert_same(dev, stats.map_test(x, A, **kw))
    host = stats.map_test_host(x.cpu().numpy() if hasattr(x, 'cpu') else x, A, **kw)
    assert_same(dev, host)
    return dev


def arm_of(M, LIM):
    return ONCHIP if M <= LIM else STREAMED


@pytest.mark.parametrize('M', [1, 63])
@pytest.mark.parametrize('stat,tail', [('tfce', 1), ('tfce', 0), ('tfce', -1), ('extent', 0), ('max', 0), ('max', 1)])
def test_small_maps_every_statistic_and_tail(M, stat, tail, LIM):
    A = cases.random_graph(M, 3, M) if M > 1 else cases.from_edges(1, [])
    x = cases.smooth_maps(9, M, seed=M, A=A)
    x[:, M // 2:] -= 0.5
    kw = {'threshold': 0.8} if stat == 'extent' else {}
    res = both(x, A, PLAIN if stat == 'max' else ONCHIP, stat=stat, tail=tail, n_perm=40, seed=5, **kw)
    assert res.n_perm == 40 and not res.exact and res.p.min() >= 1 / 40


@pytest.mark.parametrize('where', ['LIM-1', 'LIM', 'LIM+1', '3LIM+77'])
def test_edges_of_the_arms(where, LIM):
    M = {'LIM-1': LIM - 1, 'LIM': LIM, 'LIM+1': LIM + 1, '3LIM+77': 3 * LIM + 77}[where]
    A = cases.random_graph(M, 3, 1)
    x = cases.smooth_maps(8, M, seed=2, A=A)
    res = both(x, A, arm_of(M, LIM), stat='tfce', tail=1, n_perm=5, step=0.35, seed=1)
    assert res.stat.max() > 0
    both(x, A, arm_of(M, LIM), stat='extent', tail=0, n_perm=5, threshold=1.0, seed=1)


@pytest.mark.parametrize('extra', [0, 1])
def test_path_numbered_at_random(extra, LIM):
    """The deepest union-find trees: a path whose vertex numbers are a random permutation along it, all of it active."""
    M = LIM + extra
    A = cases.path(M, np.random.RandomState(7).permutation(M))
    x = cases.smooth_maps(6, M, seed=3, A=A)
    res = both(x, A, arm_of(M, LIM), stat='extent', tail=1, n_perm=4, threshold=-1e30, seed=0)
    assert (res.labels == 0).all() and (res.stat == M).all()
    both(x, A, arm_of(M, LIM), stat='tfce', tail=1, n_perm=4, step=0.4, seed=0)


@pytest.mark.parametrize('extra', [0, 1])
def test_star_hooks_everything_on_one_root(extra, LIM):
    M = LIM + extra
    A = cases.star(M, centre=M // 2)
    x = cases.smooth_maps(6, M, seed=4)
    x[:, M // 2] += 3.0                                             # the centre is active wherever a leaf is
    both(x, A, arm_of(M, LIM), stat='tfce', tail=1, n_perm=4, step=0.5, seed=0)
    res = both(x, A, arm_of(M, LIM), stat='extent', tail=1, n_perm=4, threshold=-1e30, seed=0)
    assert (res.labels == 0).all()


@pytest.mark.parametrize('extra', [0, 1])
def test_isolated_vertices_and_two_equal_components(extra, LIM):
    M = LIM + extra
    A = cases.two_components_with_isolated(M)
    x = cases.smooth_maps(7, M, seed=5, A=A, effect=0.3)
    res = both(x, A, arm_of(M, LIM), stat='extent', tail=1, n_perm=4, threshold=-1e30, seed=0)
    sizes = np.unique(res.stat, return_counts=True)
    assert sizes[0].tolist()[0] == 1.0 and len(sizes[0]) == 2 and sizes[1][1] == 2 * sizes[0][1]   # singletons, two equal paths
    both(x, A, arm_of(M, LIM), stat='tfce', tail=0, n_perm=4, step=0.4, seed=0)


@pytest.mark.parametrize('M', [200, 'LIM+1'])
def test_all_active_and_none_active(M, LIM):
    M = LIM + 1 if M == 'LIM+1' else M
    A = cases.random_graph(M, 4, 3)
    x = cases.smooth_maps(6, M, seed=6, A=A)
    res = both(x, A, arm_of(M, LIM), stat='extent', tail=1, n_perm=6, threshold=-1e30, seed=0)
    assert (res.labels >= 0).all() and res.stat.min() >= 1
    res = both(x, A, arm_of(M, LIM), stat='extent', tail=1, n_perm=6, threshold=1e30, seed=0)
    assert (res.stat == 0).all() and (res.p == 1).all() and (res.labels == -1).all()


@pytest.mark.parametrize('S', [2, 33])
def test_fewest_and_odd_subject_counts(S):
    M = 150
    A = cases.random_graph(M, 3, 8)
    x = cases.smooth_maps(S, M, seed=S, A=A)
    res = both(x, A, ONCHIP, stat='tfce', tail=0, n_perm=24, seed=9)
    assert res.exact == (S == 2) and res.n_perm == (4 if S == 2 else 24)


def test_exact_enumeration():
    M = 90
    A = cases.ring(M)
    x = cases.smooth_maps(5, M, seed=11, A=A)
    for stat, kw in (('tfce', {}), ('extent', {'threshold': 0.9}), ('max', {})):
        res = both(x, A, PLAIN if stat == 'max' else ONCHIP, stat=stat, tail=1, n_perm=32, **kw)
        assert res.exact and res.n_perm == 32
        assert np.array_equal(res.p * 32, np.round(res.p * 32)) and res.p.min() >= 1 / 32


@pytest.mark.parametrize('M', [63, 'LIM+1'])
def test_batches_do_not_change_the_result(M, LIM, monkeypatch):
    """n_perm no multiple of the batch; a budget that cuts one call into three batches gives what one batch gives."""
    from gcn_fmri_decoding_amd import ops
    M = LIM + 1 if M == 'LIM+1' else M
    A = cases.random_graph(M, 3, 4)
    x = cases.smooth_maps(8, M, seed=12, A=A)
    kw = dict(stat='tfce', tail=0, n_perm=19, step=0.3 if M > 63 else None, seed=3)
    one = stats.map_test(x, A, **kw)
    per_perm = 4 * M + ops.cluster_enhance_workspace(1, M, _lib.CLUSTER_TFCE) + 8
    monkeypatch.setattr(stats, 'CHUNK_BYTES', 7 * per_perm)         # batches of 7, 7 and 5
    calls = []
    real = ops.signflip_t
    monkeypatch.setattr(ops, 'signflip_t', lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    cut = both(x, A, arm_of(M, LIM), **kw)
    assert calls[:4] == [1, 7, 7, 5]                               # the observed map, then the three batches
    assert_same(one, cut)


def test_classes_and_device_input(LIM):
    import torch
    M = 300
    A = cases.random_graph(M, 4, 5)
    x = np.stack([cases.smooth_maps(10, M, seed=s, A=A) for s in (1, 2, 3)], 1)          # [S, C, M]
    res = both(x, A, ONCHIP, stat='tfce', tail=1, n_perm=30, seed=4)
    assert res.t.shape == (3, M) and res.null.shape == (3, 30)
    for c in range(3):
        one = stats.map_test(x[:, c], A, stat='tfce', tail=1, n_perm=30, seed=4)
        assert np.array_equal(one.stat, res.stat[c]) and np.array_equal(one.null, res.null[c]) and np.array_equal(one.p, res.p[c])
    on_dev = both(torch.as_tensor(x).cuda(), A, ONCHIP, stat='tfce', tail=1, n_perm=30, seed=4)
    assert_same(res, on_dev)


@pytest.mark.parametrize('arm', [_lib.CLUSTER_ONCHIP, _lib.CLUSTER_STREAMED])
def test_a_vertex_on_a_height_is_not_active_there(arm):
    """t values that are heights themselves (step 0.25: every height is a float32): active strictly above only."""
    import torch
    from gcn_fmri_decoding_amd import ops
    M, step, NH = 500, 0.25, 12
    A = cases.random_graph(M, 3, 6)
    ptr, idx = stats.edges(A)
    rs = np.random.RandomState(0)
    t = (rs.randint(-2, NH + 1, (3, M)) * step).astype(np.float32)          # every value ON a height
    t[:, ::7] += rs.rand(3, len(range(0, M, 7))).astype(np.float32) * 0.2   # ... but every seventh
    t[:, 5] = NH * step                                                     # the maximum as well: n = NH, nobody active there
    pl = stats._Plan(None, True, 0, 1, M, ptr, idx, 'tfce', 1, 1, None, step, 0.5, 2.0, 0)
    hf, hw, ep = stats._tables(pl, step, NH)
    dev = torch.device('cuda')
    out, _, pmax = ops.cluster_enhance(torch.as_tensor(t).to(dev), _lib.CLUSTER_TFCE, torch.as_tensor(ptr).to(dev),
                                       torch.as_tensor(idx).to(dev), torch.as_tensor(hf).to(dev), torch.as_tensor(hw).to(dev),
                                       torch.as_tensor(ep).to(dev), step=step, NH=NH, arm=arm)
    assert _lib.last_dispatch() == (ONCHIP if arm == _lib.CLUSTER_ONCHIP else STREAMED)
    for k in range(3):
        want, _ = stats.enhance_host(t[k], ptr, idx, 'tfce', hf, hw, ep, step)
        assert np.array_equal(out[k].cpu().numpy(), want)
        assert float(pmax[k]) == want.max()
        on = t[k] == np.float32(step)                                       # on height 1: not active anywhere
        assert on.any() and (want[on] == 0).all()


def test_packed_sign_table_of_more_than_one_word():
    """``chebgcn_signflip_t`` with a caller's table at S = 33 (two words a permutation) against the stated arithmetic."""
    import torch
    from gcn_fmri_decoding_amd import ops
    S, M, P = 33, 257, 11
    x = cases.smooth_maps(S, M, seed=1)
    x[:, 3] = 0.0                                                           # a vertex without signal: d = 0, t = 0
    signs = np.where(np.random.RandomState(2).rand(P, S) < 0.5, -1, 1).astype(np.int8)
    neg = (signs < 0).astype(np.uint64)
    words = np.zeros((P, 2), np.uint64)
    for j in range(S):
        words[:, j // 32] |= neg[:, j] << np.uint64(j % 32)
    bits = torch.as_tensor(words.astype(np.uint32).view(np.int32)).cuda()
    xd = x.astype(np.float64)
    q = np.zeros(M)
    for j in range(S):
        q = q + xd[j] * xd[j]
    t = ops.signflip_t(torch.as_tensor(x).cuda(), torch.as_tensor(q).cuda(), 0, P, 0, bits=bits).cpu().numpy()
    want = stats.t_host(x, signs)
    assert np.array_equal(t, want) and (want[:, 3] == 0).all()


def test_streamed_labels_on_a_knn_graph_against_scipy(LIM):
    """kNN graph (k = 8) on random coordinates, M = LIM + 1, 200 permutations picked at random: the labels of the streamed arm
    are SciPy's connected components of every supra-threshold subgraph, named by their smallest vertex."""
    import torch
    from gcn_fmri_decoding_amd import graph, ops
    M, S, thr = LIM + 1, 10, 0.9
    rs = np.random.RandomState(0)
    d, nn = graph.knn_device(rs.rand(M, 3).astype(np.float32), k=8)
    A = graph.adjacency(d, nn)
    ptr, idx = stats.edges(A)
    G = sp.csr_matrix((np.ones(idx.size, np.int8), idx, ptr), shape=(M, M))
    x = cases.smooth_maps(S, M, seed=1, A=A, effect=0.0)
    dev = torch.device('cuda')
    xd = x.astype(np.float64)
    q = torch.as_tensor((xd * xd).sum(0)).to(dev)                           # (any q: the labels are compared, not t)
    xt = torch.as_tensor(x).to(dev)
    perms = rs.randint(1, 2 ** 31 - 1, 200)
    t = torch.cat([ops.signflip_t(xt, q, int(p), 1, 77) for p in perms])
    pl = stats._Plan(None, True, 0, 1, M, ptr, idx, 'extent', 1, 1, thr, None, 0.5, 2.0, 0)
    hf, hw, ep = (torch.as_tensor(a).to(dev) for a in stats._tables(pl, 1.0, 1))
    out, labels, _ = ops.cluster_enhance(t, _lib.CLUSTER_EXTENT, torch.as_tensor(ptr).to(dev), torch.as_tensor(idx).to(dev), hf, hw,
                                         ep, NH=1, want_labels=True, arm=_lib.CLUSTER_STREAMED)
    assert _lib.last_dispatch() == STREAMED
    t, out, labels = t.cpu().numpy(), out.cpu().numpy(), labels.cpu().numpy()
    thr32 = np.float32(thr)
    nclusters = 0
    for k in range(200):
        act = np.nonzero(t[k] > thr32)[0]
        want = np.full(M, -1, np.int64)
        size = np.zeros(M)
        if act.size:
            nc, lab = csgraph.connected_components(G[act][:, act], directed=False)
            first = np.full(nc, M, np.int64)
            np.minimum.at(first, lab, act)
            want[act] = first[lab]
            size[act] = np.bincount(lab)[lab]
            nclusters += nc
        assert np.array_equal(labels[k], want), k
        assert np.array_equal(out[k], size), k
    assert nclusters > 200                                                   # (the threshold leaves clusters to label)


def test_sizes_beyond_the_limits_are_refused_before_any_launch(LIM):
    """By argument only: the entries answer CHEBGCN_EUNSUPPORTED (-4) and enqueue nothing."""
    import torch
    from gcn_fmri_decoding_amd import ops
    geo = ops.cluster_geometry()
    lib = _lib.lib()
    dev = torch.device('cuda')
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.chebgcn_signflip_t(p, p, None, p, geo['max_S'] + 1, 8, 0, 1, 0, stream) == -4
    assert lib.chebgcn_signflip_t(p, p, None, p, 4, geo['max_M'] + 1, 0, 1, 0, stream) == -4
    assert lib.chebgcn_signflip_t(p, p, None, p, 4, 8, 0, geo['max_perms'] + 1, 0, stream) == -4

    def enhance(Pb, M, NH, mode, arm):
        return lib.chebgcn_cluster_enhance(p, p, 0, p, 0, p, p, NH, p, 1.0, p, None, p, p, None, 0, Pb, M, mode, arm, stream)
    assert enhance(1, geo['max_M'] + 1, 1, _lib.CLUSTER_TFCE, 0) == -4
    assert enhance(geo['max_perms'] + 1, 8, 1, _lib.CLUSTER_TFCE, 0) == -4
    assert enhance(1, 8, geo['max_heights'] + 1, _lib.CLUSTER_TFCE, 0) == -4
    assert enhance(1, LIM + 1, 1, _lib.CLUSTER_TFCE, _lib.CLUSTER_ONCHIP) == -4
    assert b'on-chip arm' in lib.chebgcn_last_error()
    assert enhance(1, LIM + 1, 1, _lib.CLUSTER_TFCE, _lib.CLUSTER_STREAMED) == -1        # no workspace: refused as well
    assert ops.cluster_enhance_workspace(1, geo['max_M'] + 1, _lib.CLUSTER_TFCE) == 0
    assert ops.cluster_enhance_workspace(3, LIM, _lib.CLUSTER_TFCE) == 0
    assert ops.cluster_enhance_workspace(3, LIM + 1, _lib.CLUSTER_TFCE) == 3 * (LIM + 1) * geo['state_bytes']
    torch.cuda.synchronize()
    assert (buf == 0).all()
    x = cases.smooth_maps(4, 50, seed=0)
    with pytest.raises(ValueError):                                          # a step that asks for more heights than are served
        stats.map_test(x, cases.ring(50), stat='tfce', tail=1, n_perm=4, step=1e-9)
    with pytest.raises(ValueError):
        stats.map_test(np.zeros((geo['max_S'] + 1, 4), np.float32), cases.ring(4))
