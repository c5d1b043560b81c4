"""connectome on the MI355X: every kernel of chebgcn_connectome_* by name, at every entry, against ``connectome.host_run`` (NumPy
float64: the centred product by ``@``, the inverse by ``numpy.linalg.inv`` -- none of the kernels' algebra).

The bound, at EVERY entry of every matrix:  ``|dev - ref| <= 2^-23 |ref| + 1e-10 s``  -- the one float32 rounding of the output
plus 1e-10 of the quantity's natural scale s: ``sqrt(Sigma_ii Sigma_jj)`` for the covariance, 1 for the two correlations,
``sqrt(P_ii P_jj)`` for the precision; ``|s_dev - s_host| <= 1e-10`` for the shrinkage.  The form and the constant are those of
tests/test_gpu_glm.py.  Two float64 algorithms for the inverse (``inv``, and Cholesky plus a triangular inverse) differ by at most
1.3e-13 on partial correlations at condition numbers up to 5.6e3; every input drawn here is asserted on the host to have
``cond(Sigma) <= 1e5``, so the reference alone stays a thousand times inside the bound.  Degenerate flags must agree exactly.

The shapes straddle the kernels' own edges (``ops.connectome_geometry()``, pinned in tests/test_connectome_host.py): the 64-wide tile of the covariance and gram kernels,
the 16 rows of a tile's operands in LDS, the 16-column Cholesky panel, the 64 finished columns staged at once, the 8 row classes
of beta_.  A run is never cut along time, so there is no time-slice edge.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import record_measured
from guarded_buffers import FILLS, Guarded, bits
from gcn_fmri_decoding_amd import _lib, connectome as cn, graph, models_gcn
from test_connectome_host import latent

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
EPS32, FLOOR, COND = 2.0 ** -23, 1e-10, 1e5
INVERSE = ('precision', 'partial correlation')

COV_KERNELS = 'connectome_centre_kernel + connectome_rowsq_kernel + connectome_cov_kernel'
FINISH_KERNELS = {'covariance': 'connectome_finish_kernel<plain>', 'correlation': 'connectome_finish_kernel<plain>',
                  'precision': 'connectome_finish_kernel<inverse> + connectome_invert_kernel + connectome_gram_kernel',
                  'partial correlation': 'connectome_finish_kernel<inverse> + connectome_invert_kernel + connectome_gram_kernel'}

# (T, R, what the pair is there for)
PAIRS = [
    (2, 1, 'least'), (3, 1, 'one-region'), (64, 1, 'one-region'), (2, 2, 'two-points'), (31, 2, 'grid'), (600, 3, 'grid'),
    (3, 31, 'T<R'), (63, 31, 'grid'), (64, 32, 'grid'), (65, 33, 'grid'), (2, 33, 'two-points'), (127, 63, 'tile-1'),
    (128, 64, 'tile'), (129, 65, 'tile+1'), (31, 65, 'T<R,tile+1'), (284, 127, 'two-tiles-1'), (63, 128, 'T<R,two-tiles'),
    (129, 129, 'two-tiles+1'), (600, 129, 'grid'), (284, 360, 'atlas,T<R'), (600, 360, 'atlas'), (128, 360, 'atlas,T<R'),
    (284, 512, 'limit,T<R'), (600, 512, 'limit'), (3, 512, 'limit,three-points'), (65, 64, 'T=R+1'), (127, 3, 'grid'),
    (128, 31, 'grid'), (129, 32, 'grid'), (284, 33, 'grid'), (600, 63, 'grid'), (31, 32, 'T<R'), (2, 360, 'atlas,two-points'),
    # the kernels' own edges
    (15, 5, 'lds-rows-1'), (16, 5, 'lds-rows'), (17, 5, 'lds-rows+1'), (33, 5, 'lds-rows-x2+1'),
    (7, 4, 'classes-1'), (8, 4, 'classes'), (9, 4, 'classes+1'),
    (40, 15, 'panel-1'), (40, 16, 'panel'), (40, 17, 'panel+1'), (100, 47, 'panel-x3-1'), (100, 48, 'panel-x3'), (100, 49, 'panel-x3+1'),
    (200, 79, 'stage+panel-1'), (200, 80, 'stage+panel'), (200, 81, 'stage+panel+1'), (300, 191, 'three-tiles-1'),
    (300, 193, 'three-tiles+1'),
]


def ratio(got, ref, scale):
    """max over every entry of |got - ref| / (2^-23 |ref| + 1e-10 s): the bound holds iff <= 1."""
    got = np.asarray(got, np.float64)
    return float((np.abs(got - ref) / (EPS32 * np.abs(ref) + FLOOR * scale)).max())


def scale_of(kind, x, shrinkage):
    if kind == 'covariance':
        d = np.diag(cn.host_run(x, 'covariance', shrinkage)[0])
    elif kind == 'precision':
        d = np.diag(cn.host_run(x, 'precision', shrinkage)[0])
    else:
        return 1.0
    return np.sqrt(np.outer(d, d))


def check(x, kind, shrinkage, what):
    """One run, one kind: flags equal, shrinkage and every entry within the bound -> the ratio to the bound."""
    sh = -1.0 if shrinkage == 'auto' else float(shrinkage)
    ref, s_ref, flag = cn.host_run(x, kind, sh)
    if kind in INVERSE and not flag:
        c = np.linalg.cond(cn.host_run(x, 'covariance', sh)[0])
        assert c <= COND, '%s: cond(Sigma) = %.3g' % (what, c)
    _lib.dispatch_log = []
    try:
        got = cn.connectome(x, kind, shrinkage, device=DEV)
    finally:
        log, _lib.dispatch_log = _lib.dispatch_log, None
    assert [k for _, k in log] == [COV_KERNELS, FINISH_KERNELS[kind], 'connectome_mean_kernel'], log
    m = got.matrices.cpu().numpy()[0]
    assert m.dtype == np.float32 and np.isfinite(m).all() and np.array_equal(m, m.T), what
    assert bool(got.degenerate[0]) == flag, '%s: degenerate %r, reference %r' % (what, got.degenerate[0], flag)
    assert abs(got.shrinkage[0] - s_ref) <= 1e-10 and not np.signbit(got.shrinkage[0]), (what, got.shrinkage[0], s_ref)
    if kind in ('correlation', 'partial correlation'):
        assert (np.diag(m) == 1.0).all(), what
    if flag:
        assert np.array_equal(m, np.eye(x.shape[1], dtype=np.float32)) and not got.mean.cpu().numpy().any(), what
        return 0.0
    assert np.array_equal(got.mean.cpu().numpy(), m), what
    return ratio(m, ref, scale_of(kind, x, sh))


@pytest.mark.parametrize('T,R,why', PAIRS, ids=['T%d-R%d-%s' % p for p in PAIRS])
def test_every_kind_against_the_host(T, R, why):
    x = latent(T, R, seed=1000 * T + R, mix=0.3 if R == 512 else 1.0)      # (at 600 x 512 unit weights give cond 1.4e5 unshrunk)
    worst = {}
    for kind in cn.KINDS:
        for shrinkage in ('auto', 0.3) + ((0.0,) if T > R + 1 else ()):
            what = '%s shrinkage=%r T=%d R=%d' % (kind, shrinkage, T, R)
            r = check(x, kind, shrinkage, what)
            print('%s: %.3g of the bound' % (what, r))
            worst[kind] = max(worst.get(kind, 0.0), r)
            assert r <= 1.0, '%s: %.3g of the bound' % (what, r)
    record_measured('connectome[T%d-R%d-%s]' % (T, R, why), **{k.replace(' ', '_'): v for k, v in worst.items()})


def test_one_region():
    x = latent(64, 1, seed=5)
    var = float(cn.host_run(x, 'covariance', 0.0)[0][0, 0])
    for kind in ('correlation', 'partial correlation'):
        assert cn.connectome(x, kind, 0.0, device=DEV).matrices.cpu().numpy().tolist() == [[[1.0]]]
    p = float(cn.connectome(x, 'precision', 0.0, device=DEV).matrices.cpu().numpy()[0, 0, 0])
    assert abs(p - 1.0 / var) <= EPS32 / var + FLOOR / var


@pytest.fixture(scope='module')
def mixed():
    """Runs of mixed length, one of them degenerate for the precision kinds (T = 2)."""
    return [latent(T, 70, seed=T) for T in (90, 2, 284, 33, 129, 64)]


@pytest.mark.parametrize('kind', cn.KINDS)
def test_runs_of_mixed_length_in_one_call(mixed, kind):
    got = cn.connectome(mixed, kind, device=DEV)
    ref = cn.connectome_host(mixed, kind)
    assert got.degenerate.tolist() == ref.degenerate.tolist() == [False, kind in INVERSE, False, False, False, False]
    m = got.matrices.cpu().numpy()
    worst = 0.0
    for r, x in enumerate(mixed):
        if ref.degenerate[r]:
            assert np.array_equal(m[r], np.eye(70, dtype=np.float32))
            continue
        worst = max(worst, ratio(m[r], cn.host_run(x, kind, -1.0)[0], scale_of(kind, x, -1.0)))
    assert worst <= 1.0, worst
    assert np.abs(got.shrinkage - ref.shrinkage).max() <= 1e-10
    assert np.array_equal(got.mean.cpu().numpy(), cn.mean_of(m, got.degenerate))
    record_measured('connectome_mixed[%s]' % kind, ratio=worst)


def same(a, b):
    return (np.array_equal(bits(a.matrices.cpu().numpy()), bits(b.matrices.cpu().numpy())) and
            np.array_equal(bits(a.shrinkage), bits(b.shrinkage)) and np.array_equal(a.degenerate, b.degenerate))


@pytest.mark.parametrize('kind', ('covariance', 'partial correlation'))
def test_results_are_bit_identical(mixed, kind):
    base = cn.connectome(mixed, kind, device=DEV)
    mean = bits(base.mean.cpu().numpy())
    for batch in (1, 2, len(mixed)):
        got = cn.connectome(mixed, kind, device=DEV, batch_runs=batch)
        assert same(got, base) and np.array_equal(bits(got.mean.cpu().numpy()), mean), batch
    again = cn.connectome(mixed, kind, device=DEV)
    assert same(again, base) and np.array_equal(bits(again.mean.cpu().numpy()), mean)
    order = [4, 0, 5, 2, 1, 3]
    perm = cn.connectome([mixed[i] for i in order], kind, device=DEV, batch_runs=4)
    back = np.argsort(order)
    assert np.array_equal(bits(perm.matrices.cpu().numpy()[back]), bits(base.matrices.cpu().numpy()))
    assert np.array_equal(bits(perm.shrinkage[back]), bits(base.shrinkage)) and np.array_equal(perm.degenerate[back], base.degenerate)
    unpermuted = cn.mean_of(perm.matrices.cpu().numpy()[back], perm.degenerate[back])
    assert np.array_equal(bits(unpermuted), mean)
    for given in ([torch.as_tensor(x) for x in mixed], [torch.as_tensor(x).to(DEV) for x in mixed],
                  [mixed[0], torch.as_tensor(mixed[1]).to(DEV), torch.as_tensor(mixed[2])] + mixed[3:]):
        got = cn.connectome(given, kind, device=DEV)
        assert same(got, base) and np.array_equal(bits(got.mean.cpu().numpy()), mean)
    for r in (0, 2, 5):
        alone = cn.connectome(mixed[r], kind, device=DEV)
        assert np.array_equal(bits(alone.matrices.cpu().numpy()[0]), bits(base.matrices.cpu().numpy()[r]))
        assert bits(alone.shrinkage)[0] == bits(base.shrinkage)[r]


def test_bold_scaled_series():
    x = (1e4 + 50.0 * latent(284, 100, seed=11)).astype(np.float32)
    for kind in cn.KINDS:
        r = check(x, kind, 'auto', 'BOLD ' + kind)
        assert r <= 1.0, (kind, r)
        record_measured('connectome_bold[%s]' % kind, ratio=r)


def test_a_region_constant_in_time():
    x = latent(120, 40, seed=12)
    x[:, 7] = 3.25
    for kind in cn.KINDS:
        assert check(x, kind, 'auto', 'constant region, auto, ' + kind) <= 1.0
    c = cn.connectome(x, 'correlation', 0.0, device=DEV)
    m = c.matrices.cpu().numpy()[0]
    assert m[7, 7] == 1.0 and not np.delete(m[7], 7).any() and not np.delete(m[:, 7], 7).any() and not c.degenerate[0]
    assert ratio(m, cn.host_run(x, 'correlation', 0.0)[0], 1.0) <= 1.0
    for kind in INVERSE:
        got = cn.connectome(x, kind, 0.0, device=DEV)
        assert got.degenerate[0] and np.array_equal(got.matrices.cpu().numpy()[0], np.eye(40, dtype=np.float32))


def test_a_run_constant_everywhere():
    x = np.full((50, 33), 7.5, np.float32)
    for kind in cn.KINDS:
        got = cn.connectome([x, latent(50, 33, seed=13)], kind, device=DEV)
        m = got.matrices.cpu().numpy()
        assert np.isfinite(m).all() and got.shrinkage[0] == 0.0
        if kind in INVERSE:
            assert got.degenerate.tolist() == [True, False] and np.array_equal(m[0], np.eye(33, dtype=np.float32))
            assert np.array_equal(got.mean.cpu().numpy(), m[1])
        elif kind == 'covariance':
            assert not got.degenerate.any() and not m[0].any()
        else:
            assert not got.degenerate.any() and np.array_equal(m[0], np.eye(33, dtype=np.float32))


# ---------------------------------------------------------------------------------------------- the C entries directly

def entries(planes, offs, S, R, kind, shrinkage, fill, nan_pad):
    """cov, finish and mean on guarded, poisoned buffers -> (matrices, shrinkage, degenerate, mean) on the host; every guard
    band checked.  ``planes`` [Ttot, Rp] host float32, ``offs`` the offsets as given (int64 [S + 1])."""
    L = _lib.lib()
    Ttot, Rp = planes.shape
    if nan_pad:
        planes = planes.copy()
        planes[:, R:] = np.nan
    nbytes = int(L.chebgcn_connectome_workspace(S, R))
    gp = Guarded((Ttot, Rp), 'float32', fill, DEV, align=16, init=planes)
    go = Guarded((S + 1,), 'int64', fill, DEV, align=8, init=offs)
    ws = Guarded((nbytes // 8,), 'float64', fill, DEV, align=16)
    gm = Guarded((S, R, R), 'float32', fill, DEV, align=4)
    gs = Guarded((S,), 'float64', fill, DEV, align=8)
    gd = Guarded((S,), 'int32', fill, DEV, align=4)
    gmean = Guarded((R, R), 'float32', fill, DEV, align=4)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.chebgcn_connectome_cov(gp.ptr, Ttot, go.ptr, S, R, ws.ptr, nbytes, stream) == 0, L.chebgcn_last_error()
    assert _lib.last_dispatch() == COV_KERNELS
    assert L.chebgcn_connectome_finish(ws.ptr, nbytes, go.ptr, Ttot, S, R, cn.KINDS.index(kind), shrinkage, gm.ptr, gs.ptr, gd.ptr,
                                       stream) == 0, L.chebgcn_last_error()
    assert _lib.last_dispatch() == FINISH_KERNELS[kind]
    assert L.chebgcn_connectome_mean(gm.ptr, gd.ptr, S, R, gmean.ptr, stream) == 0, L.chebgcn_last_error()
    assert _lib.last_dispatch() == 'connectome_mean_kernel'
    torch.cuda.synchronize()
    for g, name in ((gp, 'planes'), (go, 'offsets'), (ws, 'workspace'), (gm, 'matrices'), (gs, 'shrinkage'), (gd, 'degenerate'),
                    (gmean, 'mean')):
        g.check('%s %s' % (kind, name))
    assert np.array_equal(bits(gp.host()), bits(planes)), 'the planes were written'
    return gm.host(), gs.host(), gd.host(), gmean.host()


def staged(runs, R):
    offs = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
    planes = np.zeros((int(offs[-1]), _lib.plane_stride(R)), np.float32)
    for r, o in zip(runs, offs):
        planes[o:o + len(r), :R] = r
    return planes, offs


@pytest.mark.parametrize('R', (33, 65, 130))
@pytest.mark.parametrize('kind', cn.KINDS)
def test_guard_bands_poisoned_buffers_and_nan_pads(kind, R):
    runs = [latent(T, R, seed=T + R) for T in (40, 2, 97)]
    planes, offs = staged(runs, R)
    ref = cn.connectome_host(runs, kind)
    out = [entries(planes, offs, 3, R, kind, -1.0, fill, nan_pad=True) for _, fill in FILLS]
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(bits(a), bits(b)), 'the result depends on memory nobody wrote'
    m, s, d, mean = out[0]
    assert np.isfinite(m).all() and np.isfinite(s).all() and (d != 0).tolist() == ref.degenerate.tolist()
    assert np.abs(s - ref.shrinkage).max() <= 1e-10
    for r, x in enumerate(runs):
        if ref.degenerate[r]:
            assert np.array_equal(m[r], np.eye(R, dtype=np.float32))
        else:
            assert ratio(m[r], cn.host_run(x, kind, -1.0)[0], scale_of(kind, x, -1.0)) <= 1.0
    assert np.array_equal(mean, cn.mean_of(m, d != 0))
    via = cn.connectome(runs, kind, device=DEV)                      # the Python path gives the same bits as the bare entries
    assert np.array_equal(bits(via.matrices.cpu().numpy()), bits(m)) and np.array_equal(bits(via.mean.cpu().numpy()), bits(mean))


def test_offsets_outside_the_planes_and_a_descending_pair():
    R = 37
    runs = [latent(30, R, seed=1), latent(50, R, seed=2)]
    planes, _ = staged(runs, R)                                       # 80 rows
    # run 0: [-5, 30) clamps to [0, 30); run 1: [30, 20) descends: empty; run 2: [20, 999) clamps to [20, 80)
    offs = np.array([-5, 30, 20, 999], np.int64)
    expect = [runs[0], None, np.concatenate([runs[0][20:], runs[1]])]
    for kind in ('covariance', 'partial correlation'):
        for _, fill in FILLS:
            m, s, d, _ = entries(planes, offs, 3, R, kind, -1.0, fill, nan_pad=True)
            assert np.isfinite(m).all() and np.isfinite(s).all()
            for r in (0, 2):
                assert not d[r] and ratio(m[r], cn.host_run(expect[r], kind, -1.0)[0], scale_of(kind, expect[r], -1.0)) <= 1.0
            assert s[1] == 0.0                                        # the empty run: zeros, or flagged with the identity
            if kind == 'covariance':
                assert not d[1] and not m[1].any()
            else:
                assert d[1] and np.array_equal(m[1], np.eye(R, dtype=np.float32))


# ---------------------------------------------------------------------------------------------- the graph on top

GAP, CAP = 1e-6, 0.05


def graph_runs(R):
    return [latent(T, R, seed=R + T, factors=6) for T in (284, 200, 284)]


@pytest.mark.parametrize('k', (1, 8))
@pytest.mark.parametrize('R', (33, 360))
def test_connectivity_graph_of_partial_correlations(R, k):
    runs = graph_runs(R)
    ref = cn.connectome_host(runs, 'partial correlation')
    assert not ref.degenerate.any()
    mean64 = np.mean([cn.host_run(x, 'partial correlation', -1.0)[0] for x in runs], axis=0)
    sim, idx_ref = graph.knn_from_similarity(mean64, k)
    off = mean64.copy()
    np.fill_diagonal(off, -np.inf)
    top = -np.sort(-off, axis=1)[:, :k + 1]
    excused = (top[:, k - 1] - top[:, k]) < GAP
    assert excused.mean() <= CAP, 'the reference alone excuses %.3f of the rows' % excused.mean()
    d, idx, sigma = graph.connectivity_graph(runs, k=k, device=DEV, return_sigma=True, kind='partial correlation')
    assert d.dtype == np.float32 and d.shape == (R, k) and idx.dtype == np.int64 and (np.diff(d, axis=1) >= 0).all()
    assert (idx != np.arange(R)[:, None]).all()
    assert np.array_equal(idx[~excused], idx_ref[~excused])
    pair = np.take_along_axis(mean64, idx, axis=1)
    assert (np.abs(d.astype(np.float64) - (1.0 - pair)) <= EPS32 * np.abs(1.0 - pair) + FLOOR).all()
    assert abs(sigma - mean64.mean()) <= EPS32 * np.abs(mean64).mean() + FLOOR
    d2, idx2 = graph.connectivity_graph([torch.as_tensor(x).to(DEV) for x in runs], k=k, kind='partial correlation')
    assert np.array_equal(d2, d) and np.array_equal(idx2, idx)


def test_into_adjacency_laplacian_and_a_forward_pass():
    R = 360
    d, idx = graph.connectivity_graph(graph_runs(R), k=8, device=DEV, kind='partial correlation')
    A = graph.adjacency(d, idx)
    assert sp.isspmatrix_csr(A) and A.shape == (R, R) and abs(A - A.T).max() == 0 and A.diagonal().max() == 0
    L = graph.laplacian(A.astype(np.float32), normalized=True)
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, [L, L], [4, 6], [3, 3], [1, 1], [9, 5], channel=3, brelu='b1relu', batch_size=8,
                           verbose=False, dropout=1)
    x = torch.as_tensor(np.random.RandomState(0).randn(8, R, 3).astype(np.float32)).to(DEV)
    with torch.no_grad():
        logits = net.inference(x, 1).cpu().numpy()
    assert logits.shape == (8, 5) and np.isfinite(logits).all()
