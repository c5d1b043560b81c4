"""Parcellation on the MI355X: chebgcn_parcellate, every arm by name, at the edges of its tile -- bit for bit against the float32
NumPy twin ``Parcellation.reduce_host``, within the derived bound of tests/test_parcellation_host.py of the float64 restatement
of the reference, and bit-identical from run to run; ``reduce`` under any row chunking and from host or device input; NaN
propagation; chebgcn_parcel_expand against NumPy indexing; and the way from raw runs to ``decode_series``, ``stage_windows`` and
``connectivity_graph``.  The shapes follow the kernel's constants (``ops.parcellate_geometry()``), not HCP's sizes."""
import numpy as np
import pytest
import torch

from gcn_fmri_decoding_amd import Parcellation, _lib, graph, models_gcn, ops
from test_parcellation_host import bound, make_labels, make_series, make_weights, ref64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
G = ops.parcellate_geometry() if torch.cuda.is_available() else dict(tile=4096, rows=4, wide_T=4096, regions_per_pass=512,
                                                                       max_grid=16384, expand_grid_rows=1024, expand_vec=4)
C1, C4 = G['tile'], G['tile'] // G['rows']          # vertices of a chunk: the one-row arm, the wide arm
PASS, WIDE, ROWS = G['regions_per_pass'], G['wide_T'], G['rows']

# (V, R, T): the one-row arm (T < WIDE) ...
NARROW = [
    (1, 1, 1), (63, 5, 3), (63, 63, 5),
    (C1 - 1, 64, ROWS - 1), (C1, 65, ROWS + 1), (C1 + 1, 1, 1),
    (3 * C1 + 1000, 360, 3),                        # more than 3 chunks and a remainder
    (2 * C1 + 5, 1000, 2), (C1 + 77, PASS + 1, 2),  # R beyond one pass: V is swept again
    (700, PASS, WIDE - 1),                          # the last T of this arm, exactly one pass
]
# ... and the wide arm (T >= WIDE): its own chunk, a last row tile that is not full, the grid loop
WIDE_CASES = [
    (C4 - 1, 63, WIDE), (C4, 64, WIDE + 1), (C4 + 1, 65, WIDE + ROWS - 1),
    (3 * C4 + 300, 40, WIDE + ROWS + 1),
    (63, 5, 70000), (PASS + 60, PASS + 1, WIDE + 2),
]


def _check(V, R, T, weighted, mode, strided):
    wide = T >= WIDE
    lab = make_labels(V, R, chunk=C4 if wide else C1)
    w = make_weights(lab) if weighted else None
    P = Parcellation(lab, weights=w)
    x = make_series(T, V)
    host = P.reduce_host(x, mode=mode)
    ptr, idx, _, wd = P._tables(DEV)
    if strided:                                     # ldx > V and ldo > R: columns of wider tensors, rows not 16-byte aligned
        big = torch.full((T, V + 3), float('nan'), device=DEV)
        big[:, 1:V + 1] = torch.as_tensor(x).to(DEV)
        xd = big[:, 1:V + 1]
        obig = torch.full((T, P.R + 5), -1.0, device=DEV)
        od = obig[:, 2:P.R + 2]
    else:
        xd = torch.as_tensor(x).to(DEV)
        obig = od = torch.full((T, P.R), float('nan'), device=DEV)
    m = ('mean', 'sum').index(mode)
    got = ops.parcellate(xd, ptr, idx, P.R, w=wd, mode=m, out=od)
    arm = 'parcellate_kernel<rows%d, %s>' % (ROWS if wide else 1, 'weighted' if weighted else 'plain')
    assert _lib.last_dispatch() == arm, _lib.last_dispatch()
    a = got.cpu().numpy()
    assert np.array_equal(a, host), 'device and float32 NumPy twin differ at %d of %d' % ((a != host).sum(), a.size)
    if strided:
        assert (obig[:, :2] == -1).all() and (obig[:, P.R + 2:] == -1).all()
    err, b = np.abs(a.astype(np.float64) - ref64(lab, x, w, mode)), bound(lab, x, w, mode)
    print('V=%d R=%d T=%d %s: max err / bound = %.3f' % (V, P.R, T, arm, (err / np.maximum(b, 1e-300)).max()))
    assert (err <= b).all()
    again = ops.parcellate(xd, ptr, idx, P.R, w=wd, mode=m)
    assert torch.equal(again, got)
    return P, x, host


@pytest.mark.parametrize('V,R,T', NARROW + WIDE_CASES)
def test_kernel_bits_bound_and_arm(V, R, T):
    _check(V, R, T, weighted=False, mode='mean', strided=False)


@pytest.mark.parametrize('V,R,T', [(63, 5, 3), (C1 + 1, 65, ROWS + 1), (3 * C1 + 1000, 360, 2), (C4 + 1, 65, WIDE + 1),
                                   (PASS + 60, PASS + 1, WIDE + 2)])
@pytest.mark.parametrize('weighted,mode,strided', [(True, 'mean', False), (True, 'sum', True), (False, 'sum', False),
                                                    (False, 'mean', True)])
def test_kernel_modes_weights_and_strides(V, R, T, weighted, mode, strided):
    _check(V, R, T, weighted, mode, strided)


def test_reduce_chunk_rows_host_and_device_input_same_bits():
    V, T = C1 + 333, 11
    lab = make_labels(V, 40, chunk=C1)
    x = make_series(T, V)
    for w in (None, make_weights(lab)):
        P = Parcellation(lab, weights=w)
        host = P.reduce_host(x)
        base = P.reduce(x)
        assert base.is_cuda and base.dtype == torch.float32 and base.shape == (T, 40)
        assert np.array_equal(base.cpu().numpy(), host)
        for cr in (1, 3, T, 10 ** 6):
            assert torch.equal(P.reduce(x, chunk_rows=cr), base), cr
        assert torch.equal(P.reduce(torch.as_tensor(x).to(DEV)), base)                 # a device tensor, reduced where it lies
        assert torch.equal(P.reduce(torch.as_tensor(x), chunk_rows=4), base)           # a host tensor
        assert torch.equal(P.reduce(x.astype(np.float64), chunk_rows=5), base)         # any numeric dtype
        outs = P.reduce([x[:4], torch.as_tensor(x[4:]).to(DEV)], mode='sum')
        assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(4, 40), (T - 4, 40)]
        assert np.array_equal(torch.cat(outs).cpu().numpy(), P.reduce_host(x, mode='sum'))


def test_a_nan_reaches_exactly_one_region_and_time_point():
    V, T = C1 + 50, 6
    lab = make_labels(V, 65, chunk=C1)
    P = Parcellation(lab)
    x = make_series(T, V)
    v = int(np.nonzero(lab > 0)[0][C1 // 2])
    x[4, v] = np.nan
    bg = int(np.nonzero(lab <= 0)[0][0])
    x[2, bg] = np.nan                                           # on the background: reaches nothing
    got = P.reduce(x).cpu().numpy()
    want = np.zeros((T, P.R), bool)
    want[4, P.region_of[v]] = True
    assert np.array_equal(np.isnan(got), want)
    assert np.array_equal(np.isnan(P.reduce_host(x)), want)


@pytest.mark.parametrize('V,B', [(1, 1), (63, 3), (4 * 256 + 2, 5), (4 * 256 * 3 + 1, 2), (37, G['expand_grid_rows'] + 3)])
def test_expand_bit_exact_against_numpy_indexing(V, B):
    lab = make_labels(V, min(V, 40), chunk=512)
    P = Parcellation(lab)
    maps = np.random.RandomState(V + B).randn(B, P.R).astype(np.float32)
    for fill in (0.0, -2.5):
        want = np.where(P.region_of[None, :] >= 0, maps[:, np.maximum(P.region_of, 0)], np.float32(fill))
        got = P.expand(torch.as_tensor(maps).to(DEV), fill=fill)
        assert _lib.last_dispatch() == 'parcel_expand_kernel'
        assert got.is_cuda and got.shape == (B, V) and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(P.expand(maps, fill=fill), want)
    one = P.expand(torch.as_tensor(maps[0]).to(DEV))
    assert one.shape == (V,) and np.array_equal(one.cpu().numpy(), P.expand(maps[0]))


def test_raw_runs_to_decode_series_stage_windows_and_connectivity_graph():
    M0, V, T, C = 40, 700, 60, 3
    L = graph.synthetic_graph(M0, k=6, levels=0, seed=3)[0]
    torch.manual_seed(0)
    net = models_gcn.cgcnn({'device': DEV}, L * 2, [8, 8], [3, 3], [1, 1], [12, 5], channel=C, batch_size=4, verbose=False)
    lab = make_labels(V, M0, chunk=512)
    P = Parcellation(lab)
    raw = [make_series(T, V, seed=1), make_series(T - 9, V, seed=2)]
    dev_runs, host_runs = P.reduce(raw), P.reduce_host(raw)
    assert all(r.is_cuda for r in dev_runs)
    a, b = net.decode_series(dev_runs), net.decode_series(host_runs)
    assert len(a) == 2 and all(np.array_equal(u, v) for u, v in zip(a, b))
    ws_dev, ws_host = net.stage_windows(dev_runs), net.stage_windows(host_runs)
    assert len(ws_dev) == (T - C + 1) + (T - 9 - C + 1) and torch.equal(ws_dev.planes, ws_host.planes)
    d1, i1 = graph.connectivity_graph(dev_runs, k=6)
    d2, i2 = graph.connectivity_graph([r.cpu().numpy() for r in dev_runs], k=6)
    assert np.array_equal(d1, d2) and np.array_equal(i1, i2)
    # attribution-shaped maps back on the surface
    maps = torch.randn(5, M0, device=DEV)
    surf = P.expand(maps)
    assert surf.shape == (5, V) and np.array_equal(surf.cpu().numpy(), P.expand(maps.cpu().numpy()))
