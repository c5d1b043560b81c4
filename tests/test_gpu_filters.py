"""Graph filters on the MI355X: chebgcn_cheb_filter, both arms by name, at the edges of their launches, against the float64
restatement ``GraphFilter.apply_host`` (the device's float32-rounded operands, summed in float64), and ``GraphFilter.apply`` /
``smooth`` from host arrays, device tensors and lists of runs, relabelled or not, into ``Parcellation.reduce`` and out of
``saliency_maps``.

Bound: the project's standing ``max|device - host| <= 1e-5 * max|host|`` per filter.  Inputs carry NaN in every plane pad,
outputs are pre-filled with a sentinel, x is compared bit for bit after every call; every measured ratio is recorded."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import csr_from, load_golden, record_measured
from gcn_fmri_decoding_amd import GraphFilter, Parcellation, _lib, filters, graph, models_gcn, ops
from test_filters_host import knn_laplacian
from test_parcellation_host import bound as parcel_bound

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
REL = 1e-5
SENT = -77.0
STEP4, STEP1, MIX = 'cheb_filter_step_kernel<4>', 'cheb_filter_step_kernel<1>', 'cheb_filter_mix_kernel'
BANK = [filters.heat(2.0), filters.mexican_hat(4.0), filters.heat(8.0), filters.mexican_hat(1.0), filters.heat(30.0),
        filters.heat(0.5), filters.mexican_hat(8.0), filters.heat(15.0), filters.mexican_hat(2.0)]
_cache = {}


def _lap(M, k=8, seed=0):
    if M == 1:
        return sp.csr_matrix(np.full((1, 1), 0.5, np.float32))          # L~ = [[-0.5]]: one vertex, one entry
    return knn_laplacian(M, k=k, seed=seed)


def _graph(M, k=8, seed=0):
    """(Laplacian, device graph in the caller's vertex order), built once per shape."""
    key = (M, k, seed)
    if key not in _cache:
        L = _lap(M, k, seed)
        _cache[key] = (L, ops.Graph(L, DEV))
    return _cache[key]


def _big_graph():
    """M = 20 600, 4 neighbours (graph.knn_device): beyond every on-chip image."""
    if 'big' not in _cache:
        z = np.random.RandomState(7).standard_normal((20600, 3)).astype(np.float32)
        L = graph.laplacian(graph.adjacency(*graph.knn_device(z, k=4, device=DEV)), normalized=True)
        _cache['big'] = (L, ops.Graph(L, DEV))
    return _cache['big']


def _table(J, K):
    return np.atleast_2d(filters.cheb_coefficients(BANK[:J], K))


def _planes(x, Mp):
    p = torch.full((x.shape[0], Mp), float('nan'), device=DEV)
    p[:, :x.shape[1]] = torch.as_tensor(x).to(DEV)
    return p


def _bits(t):
    return t.contiguous().view(torch.int32)


def _filter(g, xp, c, arm):
    """One call on sentinel-filled output: ([J, n, Mp] tensor, dispatch).  x must come back bit for bit."""
    before = _bits(xp).clone()
    y = torch.full((c.shape[0],) + tuple(xp.shape), SENT, device=DEV)
    cd = torch.as_tensor(c.astype(np.float32)).to(DEV)
    ops.cheb_filter(g, xp, cd, arm=arm, out=y)
    names = _lib.last_dispatch()
    assert torch.equal(_bits(xp), before), 'x was written'
    return y, names


def _check(what, L, g, n, J, K, arm, seed=0):
    M = g.M
    x = np.random.default_rng(seed).standard_normal((n, M)).astype(np.float32)
    c = _table(J, K)
    y, names = _filter(g, _planes(x, g.Mp), c, arm)
    got = y[:, :, :M].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and not (got == SENT).any()
    want = GraphFilter(L, coeffs=c, relabel=None).apply_host(x)
    ratio = [float(np.abs(got[j] - want[j]).max() / np.abs(want[j]).max()) for j in range(J)]
    record_measured('cheb_filter_vs_float64', case=what, M=M, nplanes=n, J=J, K=K, dispatch=names, max_ratio=max(ratio), bound=REL)
    print('%s M=%d n=%d J=%d K=%d %s: max ratio %.3e' % (what, M, n, J, K, names, max(ratio)))
    assert max(ratio) <= REL, ratio
    return names, y, x


# ---- rolling arm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 4, 5, 9])
@pytest.mark.parametrize('M', [1, 255, 256, 257, 1000])
def test_rolling_workgroup_and_plane_group_edges(M, n):
    L, g = _graph(M)
    names, _, _ = _check('rolling_edges', L, g, n, J=2, K=5, arm=1, seed=M + n)
    assert names == (STEP4 if n >= 4 else STEP1)


@pytest.mark.parametrize('K', [1, 2, 3, 4, 7, 40])
def test_rolling_orders(K):
    L, g = _graph(257)
    names, _, _ = _check('rolling_orders', L, g, 5, J=2, K=K, arm=1, seed=K)
    assert set(names.split(' + ')) == {STEP4}
    names, _, _ = _check('rolling_orders', L, g, 2, J=2, K=K, arm=1, seed=K)
    assert set(names.split(' + ')) == {STEP1}


@pytest.mark.parametrize('J', [1, 8])
def test_rolling_filter_counts(J):
    L, g = _graph(257)
    _check('rolling_J', L, g, 5, J=J, K=12, arm=1)


def test_rolling_isolated_vertex_and_hub_row():
    M = 300
    W = sp.lil_matrix(graph.adjacency(*graph.distance_sklearn_metrics(
        np.random.RandomState(2).standard_normal((M, 3)).astype(np.float32), k=6)))
    W[7, :] = 0
    W[:, 7] = 0                                     # vertex 7: isolated
    hub = 11
    W[hub, :] = 0
    W[:, hub] = 0
    others = [v for v in range(M) if v not in (7, hub)][:140]
    for v in others:
        W[hub, v] = W[v, hub] = 0.5                 # row 11: exactly 140 entries
    L = graph.laplacian(sp.csr_matrix(W).astype(np.float32), normalized=True)
    g = ops.Graph(L, DEV)
    lengths = np.diff(graph.rescaled_laplacian_csr(L)[0])
    assert lengths[7] == 0 and lengths[hub] == 140 == lengths.max()
    _check('rolling_hub', L, g, 5, J=2, K=9, arm=1)
    _check('rolling_hub', L, g, 3, J=2, K=9, arm=1)


def test_rolling_more_plane_groups_than_grid_rows():
    L, g = _graph(20, k=4)
    n = 4 * 65536 + 5
    assert g.Mp == 32
    names, _, _ = _check('rolling_grid_y', L, g, n, J=1, K=3, arm=1)
    assert set(names.split(' + ')) == {STEP4}


def test_automatic_arm_without_an_image_is_the_step_kernel():
    L, g = _big_graph()
    assert not g.on_chip and not g.ordered
    assert ops.cheb_filter_workspace(g, 5, 6, 2, 0) == ops.cheb_filter_workspace(g, 5, 6, 2, 1) == 2 * 5 * g.Mp * 4
    names, _, _ = _check('auto_no_image', L, g, 5, J=2, K=6, arm=0)
    assert set(names.split(' + ')) == {STEP4}
    with pytest.raises(_lib.ChebgcnError, match='arm = 2'):
        _filter(g, _planes(np.zeros((2, g.M), np.float32), g.Mp), _table(1, 4), 2)


def test_rolling_plane_is_bit_identical_alone_among_others_and_again():
    L, g = _graph(1000)
    x = np.random.default_rng(3).standard_normal((9, 1000)).astype(np.float32)
    c = _table(3, 11)
    xp = _planes(x, g.Mp)
    full, _ = _filter(g, xp, c, 1)
    again, _ = _filter(g, xp, c, 1)
    assert torch.equal(full[:, :, :1000], again[:, :, :1000])
    for p in (0, 4, 8):
        alone, names = _filter(g, xp[p:p + 1].clone(), c, 1)
        assert names.startswith(STEP1)
        assert torch.equal(alone[:, 0, :1000], full[:, p, :1000])
    part, _ = _filter(g, xp[3:8].clone(), c, 1)      # other neighbours in the group
    assert torch.equal(part[:, :, :1000], full[:, 3:8, :1000])
    f = GraphFilter(L, coeffs=c, relabel=None)
    base = f.apply(x, arm=1)
    assert torch.equal(base, full[:, :, :1000])
    for rows in (1, 2, 4, 7):
        assert torch.equal(f.apply(x, arm=1, chunk_rows=rows), base)


# ---- stack arm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [2, 40])
@pytest.mark.parametrize('J', [1, 2, 8])
def test_stack_on_chip(J, K):
    L, g = _graph(100)
    assert g.on_chip and g.Mp == 128
    assert ops.cheb_filter_workspace(g, 3, K, J, 2) == ops.cheb_filter_workspace(g, 3, K, J, 0) == K * 3 * g.Mp * 4
    for n in (1, 3):                                 # slabs of 32 * 4 and 32 * 4 * 3 floats
        names, _, _ = _check('stack_on_chip', L, g, n, J=J, K=K, arm=2, seed=n)
        assert names.startswith('cheb_onchip_kernel') and names.endswith(' + ' + MIX)


def test_stack_slab_larger_than_one_grid_pass():
    L, g = _graph(100)
    n = 8192 * 256 * 4 // g.Mp + 37                  # more 16-byte pieces than threads of the largest mix grid
    names, _, _ = _check('stack_grid_loop', L, g, n, J=2, K=3, arm=0)
    assert names.endswith(' + ' + MIX)


def test_stack_one_term_mixes_x_directly():
    L, g = _graph(100)
    names, _, _ = _check('stack_K1', L, g, 3, J=2, K=1, arm=2)
    assert names == MIX


@pytest.fixture(scope='module')
def f1500():
    L = knn_laplacian(1500, k=8, seed=5)
    return L, GraphFilter(L, BANK[:2], K=20, device=DEV), GraphFilter(L, BANK[:2], K=20, relabel=None, device=DEV)


def _ratios(got, want):
    got = got.cpu().numpy().astype(np.float64)
    return max(float(np.abs(got[j] - want[j]).max() / np.abs(want[j]).max()) for j in range(len(want)))


def test_stack_ordered_and_both_arms_agree(f1500):
    L, f, fplain = f1500
    x = np.random.default_rng(8).standard_normal((6, 1500)).astype(np.float32)
    want = f.apply_host(x)
    _lib.dispatch_log = log = []
    try:
        stack = f.apply(x, arm=2)
        auto = f.apply(x)
    finally:
        _lib.dispatch_log = None
    g, order, _ = f._tables(DEV)
    assert g.ordered and order is not None
    names = [d for what, d in log if what == 'cheb_filter']
    assert len(names) == 2 and names[0] == names[1]
    assert names[0].startswith('cheb_ord') and names[0].endswith(' + ' + MIX), names
    rolling = f.apply(x, arm=1)
    plain = fplain.apply(x, arm=1)
    assert fplain._tables(DEV)[1] is None
    r = {'stack': _ratios(stack, want), 'rolling': _ratios(rolling, want), 'plain': _ratios(plain, want),
         'stack_vs_rolling': _ratios(stack, rolling.cpu().numpy().astype(np.float64)),
         'relabel_vs_plain': _ratios(rolling, plain.cpu().numpy().astype(np.float64))}
    record_measured('graph_filter_arms', M=1500, K=20, bound=REL, **r)
    print(r)
    assert max(r.values()) <= REL, r
    assert torch.equal(auto, stack)


# ---- the whole interface ------------------------------------------------------------------------------------------------------------
def test_apply_from_host_device_and_runs_is_the_same(f1500):
    L, f, _ = f1500
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal((5, 1500)).astype(np.float32), rng.standard_normal((3, 1500)).astype(np.float32)
    for arm in (1, 2):
        ya = f.apply(a, arm=arm)
        assert ya.is_cuda and ya.dtype == torch.float32 and ya.shape == (2, 5, 1500) and ya.is_contiguous()
        ad = torch.as_tensor(a).to(DEV)
        keep = ad.clone()
        assert torch.equal(f.apply(ad, arm=arm), ya)
        assert torch.equal(ad, keep)
        runs = f.apply([a, torch.as_tensor(b).to(DEV)], arm=arm)
        assert isinstance(runs, list) and len(runs) == 2 and torch.equal(runs[0], ya) and runs[1].shape == (2, 3, 1500)
        assert torch.equal(runs[1], f.apply(b, arm=arm))
    one = GraphFilter(L, BANK[0], K=20, device=DEV).apply(a, arm=1)
    assert one.shape == (5, 1500) and torch.equal(one, f.apply(a, arm=1)[0])


def test_out_with_a_row_stride_keeps_the_sentinel(f1500):
    L, f, _ = f1500
    x = np.random.default_rng(10).standard_normal((4, 1500)).astype(np.float32)
    big = torch.full((2, 4, 1500 + 7), SENT, device=DEV)
    out = big[:, :, 3:1503]
    got = f.apply(x, out=out)
    assert got is out and torch.equal(out, f.apply(x))
    assert (big[:, :, :3] == SENT).all() and (big[:, :, 1503:] == SENT).all()


def test_nine_filters_in_groups_of_eight():
    L, g = _graph(257)
    f = GraphFilter(L, BANK, K=16, device=DEV)
    assert f.J == 9
    x = np.random.default_rng(11).standard_normal((5, 257)).astype(np.float32)
    want = f.apply_host(x)
    for arm in (1, 2):
        got = f.apply(x, arm=arm)
        assert got.shape == (9, 5, 257)
        r = _ratios(got, want)
        record_measured('graph_filter_nine', arm=arm, max_ratio=r, bound=REL)
        assert r <= REL, r


def test_smooth_then_reduce():
    M, T, R = 1000, 12, 40
    L, _ = _graph(M)
    x = np.random.default_rng(12).standard_normal((T, M)).astype(np.float32)
    lab = np.random.RandomState(13).randint(0, R + 1, M)
    lab[:R] = np.arange(1, R + 1)
    P = Parcellation(lab)
    sm = filters.smooth(x, L, 2.0, device=DEV)
    f = GraphFilter(L, filters.heat(2.0), tol=1e-6)
    host = f.apply_host(x)
    r = float(np.abs(sm.cpu().numpy() - host).max() / np.abs(host).max())
    assert sm.shape == (T, M) and r <= REL
    got = P.reduce(sm).cpu().numpy().astype(np.float64)
    want = np.stack([host[:, P.idx[P.ptr[k]:P.ptr[k + 1]]].mean(axis=1) for k in range(P.R)], axis=1)
    assert np.array_equal(got, P.reduce_host(sm).astype(np.float64))
    # the filter's share: a mean of values each within REL * max|host|; the reduction's own: the derived bound of
    # tests/test_parcellation_host.py on the values it was given
    allowed = REL * np.abs(host).max() + parcel_bound(lab, sm.cpu().numpy())
    err = np.abs(got - want)
    record_measured('smooth_then_reduce', filter_ratio=r, max_err_over_allowed=float((err / allowed).max()))
    assert (err <= allowed).all()


def test_filtered_saliency_maps_keep_shape_and_order():
    z = load_golden('inference_pool_n212')
    Ls = [csr_from(z, 'L%d' % i) for i in range(int(z['nlevels']))]
    F, K, p, Mh = z['F'].tolist(), z['K'].tolist(), z['p'].tolist(), z['M'].tolist()
    net = models_gcn.cgcnn({'device': DEV}, Ls, F, K, p, Mh, channel=int(z['channel']), brelu=str(z['brelu']),
                           batch_size=int(z['x'].shape[0]), regularization=5e-4, dropout=1, verbose=False)
    for k in z.files:
        if k.startswith('param:'):
            net.set_variable(k[len('param:'):], z[k].copy())
    x = z['x']
    maps, _ = net.saliency_maps(x, np.arange(x.shape[0]) % Mh[-1])
    m = np.ascontiguousarray(maps[:, :, 0]).astype(np.float32)          # [classes, M]
    f = GraphFilter(Ls[0], filters.heat(1.0), tol=1e-6, device=DEV)
    got = f.apply(torch.as_tensor(m).to(DEV))
    want = f.apply_host(m)
    assert got.shape == m.shape
    r = float(np.abs(got.cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30))
    record_measured('filtered_saliency_maps', max_ratio=r, bound=REL)
    assert r <= REL
