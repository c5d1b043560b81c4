"""The float64 restatements tests/test_gpu_head_kernels.py uses as truth for the head's FC and flatten kernels, against the
oracle's layers (oracle/layers_ref.py: fc_fwd, fc_bwd) on small random inputs, and the host-side figures that test relies on:
the exactness inequality of its exact leg, the census of the ReLU gate plants, the split counts and the vec condition of the
dispatch (against chebgcn_fc_fwd_workspace, which runs on the CPU), the case tables, and that "bit-equal" discriminates --
one term less in one reduction changes the exact leg's reference.  No GPU."""
import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import plane_stride
from oracle import layers_ref as R

import test_gpu_head_kernels as T


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('B,I,O', [(1, 1, 1), (5, 7, 3), (33, 40, 9)])
def test_restatement_is_the_oracle(B, I, O, relu):
    rs = np.random.RandomState(B + 10 * I + 100 * O)
    x, W, b, g = rs.randn(B, I), rs.randn(I, O) / np.sqrt(I), 0.1 * rs.randn(O), rs.randn(B, O)
    y = T.fc_ref(x, W, b, relu)
    y_o = R.fc_fwd(x, W, b, relu)
    eps = np.finfo(np.float64).eps
    assert np.abs(y - y_o).max() <= 4 * eps * np.abs(y_o).max()
    y_o[0, 0] = 0.0                                           # a closed gate at y == 0 whatever the draw
    r = T.fc_bwd_ref(x, W, g, y_o if relu else None)
    dx, dW, db = R.fc_bwd(g, x, W, y_o, relu)
    for got, ref in ((r['dx'], dx), (r['dW'], dW), (r['db'], db)):
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 4 * eps * max(np.abs(ref).max(), 1.0)
    if relu:
        assert r['gm'][0, 0] == 0 and np.array_equal(r['gm'] != 0, y_o > 0)
    else:
        assert r['gm'] is g or np.array_equal(r['gm'], g)
    # the bounds of the round-off leg dominate what fp32 inputs rounded from these would lose
    assert (T.fc_bounds(x, W, b) >= (I + 2) * T.U * np.abs(x @ W + b) - 1e-300).all()


def test_gate_is_a_select_on_written_out_values():
    y = np.array([[0.0, -0.0, -1.0, T.TINY, 2.0]], np.float32)
    g = np.array([[1e30, 1e30, 1e30, 3.0, -2.0]], np.float32)
    r = T.fc_bwd_ref(np.ones((1, 2)), np.ones((2, 5)) / 8, g, y)
    assert r['gm'].tolist() == [[0.0, 0.0, 0.0, 3.0, -2.0]] and r['db'].tolist() == [0.0, 0.0, 0.0, 3.0, -2.0]
    assert r['dx'].tolist() == [[0.125, 0.125]] and r['dW'].tolist() == [[0.0, 0.0, 0.0, 3.0, -2.0]] * 2
    assert T.gate_census(y) == dict(pzero=[0], nzero=[0], negative=[0], tiny=[0])
    with pytest.raises(AssertionError, match='no nzero entry'):
        T.assert_gate('x', [np.array([[0.0, -1.0, T.TINY]], np.float32)], 1)
    with pytest.raises(AssertionError, match='in the last row'):
        T.assert_gate('x', [np.concatenate([y, np.ones((1, 5), np.float32)])], 2)
    with pytest.raises(AssertionError, match='denormal'):
        T.gate_census(np.array([[T.TINY / 2]], np.float32))


def test_flatten_restatements_on_written_out_values():
    M, F = 3, 2
    planes = np.full((1, F, plane_stride(M)), np.nan)
    planes[0, 0, :M] = [10, 11, 12]
    planes[0, 1, :M] = [20, 21, 22]
    order = np.array([2, 0, 1], np.int32)                     # internal position v holds reference vertex order[v]
    rows = T.rows_ref(planes, order, M, F, M * F + 2, -7.0)
    assert rows.tolist() == [[11, 21, 12, 22, 10, 20, -7, -7]]
    assert T.rows_ref(planes, None, M, F, M * F, 0.0).tolist() == [[10, 20, 11, 21, 12, 22]]
    back = T.planes_ref(rows, order, M, F)
    assert np.array_equal(back[:, :, :M], planes[:, :, :M]) and np.all(back[:, :, M:] == 0)
    for c in T.FLAT_CASES[:4]:
        for permuted in (0, 1):
            p, r, o = T.flat_inputs(c, permuted)
            MF = c.M * c.F
            assert np.isnan(p[:, :, c.M:]).all() and (c.pad == 0 or np.isnan(r[:, MF:]).all())
            assert len(np.unique(p[:, :, :c.M])) == c.B * MF                                 # a misplaced element cannot hide
            rows = T.rows_ref(p, o, c.M, c.F, MF, 0.0)
            assert np.array_equal(T.planes_ref(rows, o, c.M, c.F)[:, :, :c.M], p[:, :, :c.M])
            assert (rows * r[:, :MF]).sum() == (p[:, :, :c.M].astype(np.float64) * T.planes_ref(r, o, c.M, c.F)[:, :, :c.M]).sum()


def test_exact_leg_is_exact_for_every_case():
    """32 n + 8 < 2^24 for every reduction of every case, and the float64 reference of the largest sums is an fp32 number."""
    assert T.exact_leg_is_exact(16416) and T.exact_leg_is_exact(2 ** 19 - 1) and not T.exact_leg_is_exact(2 ** 19)
    for c in T.FWD_CASES + [c for c, _, _ in T.FWD_REFUSED]:
        assert T.exact_leg_is_exact(c.I), c
    for c in T.BWD_CASES + [T.BWD_MISALIGNED]:
        assert all(T.exact_leg_is_exact(n) for n in (c.B, c.I, c.O)), c
    for c in (T._fwd(8, 5760, 12), T._fwd(4, 1027, 3)):
        x, W, b = T.fwd_inputs(c, True)
        assert np.isnan(x[:, c.I:]).sum() == (c.B - 1) * (c.ldx - c.I) and np.isinf(x[c.B // 2, c.I:]).all()
        assert np.abs(x[:, :c.I]).max() == 4 and np.abs(W).max() == 1 and np.array_equal(W * 8, np.round(W * 8))
        y = T.fc_ref(x[:, :c.I], W, b, False)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and np.array_equal(y * 8, np.round(y * 8))
        assert np.abs(y).max() <= 4 * c.I + 1
    c = T._bwd(1000, 8, 7)
    x, W, g, y = T.bwd_inputs(c, True, True)
    r = T.fc_bwd_ref(x, W, g, y)
    for k in ('dW', 'db', 'dx'):
        assert np.array_equal(r[k].astype(np.float32).astype(np.float64), r[k]) and np.abs(r[k]).max() <= 16 * c.B


@pytest.mark.parametrize('c', T.BWD_CASES + [T.BWD_MISALIGNED, T._bwd(8, 360, 9)], ids=T.case_id)
def test_gate_census_of_every_backward_case(c):
    """+0.0, -0.0, a negative number and the smallest positive normal in y: at all, in a row >= 32 where B allows, and in the
    last row; gated g is 1e30 in the exact leg and nowhere else; the gate at the smallest normal is open."""
    for exact in (True, False):
        ys = []
        for only in T.gate_variants(c):
            x, W, g, y = T.bwd_inputs(c, exact, True, only)
            assert x.shape == (c.B, c.ldx) and y.shape == g.shape == (c.B, c.O) and y.dtype == g.dtype == np.float32
            assert np.array_equal(g == T.GATE_LEAK, y <= 0) if exact else np.abs(g).max() < 10
            assert (g[y == T.TINY] != T.GATE_LEAK).all() and ((y > 0).any() or c.B * c.O < 4)
            assert c.ldx == c.I or np.isnan(x[:, c.I:]).sum() == (c.B - 1) * (c.ldx - c.I)
            r = T.fc_bwd_ref(x[:, :c.I], W, g, y)
            assert np.abs(r['gm']).max() < 1e3, 'a gated value reached the reference'
            ys.append(y)
        n = T.assert_gate(T.case_id(c), ys, c.B)
        if c.B * c.O >= 4:
            assert all(v >= len(T.plant_rows(c.B)) for v in n.values()) and len(T.plant_cells(c.B, c.O)) == 4 * len(T.plant_rows(c.B))
            assert len({(r, col) for r, col, _ in T.plant_cells(c.B, c.O)}) == 4 * len(T.plant_rows(c.B))
        else:
            assert len(ys) == 4
    assert T.bwd_inputs(c, True, False)[3] is None and np.abs(T.bwd_inputs(c, True, False)[2]).max() <= 4


def test_split_counts_and_vec_predictions():
    """The restated fc_splits against the library for the whole forward table and at its thresholds; the figures of the
    table: S == 1, 1 < S <= 16, S > 16, an empty last split; the vec condition of the backward."""
    lib = _lib.lib()

    def lib_splits(B, I, O):
        nws = lib.chebgcn_fc_fwd_workspace(B, I, O)
        assert nws % (4 * B * O) == 0
        return nws // (4 * B * O) if nws else 1

    shapes = [(c.B, c.I, c.O) for c in T.FWD_CASES] + [(64, 10466, 512), (128, 512, 256), (1, 512, 1), (1, 513, 1),
                                                         (32, 2 ** 20, 32), (33, 2 ** 20, 32), (8193, 1024, 32), (8192, 1024, 32)]
    for B, I, O in shapes:
        assert lib.chebgcn_fc_fwd_supported(B, I, O) == 1
        assert T.fc_splits(B, I, O) == lib_splits(B, I, O), (B, I, O)
    want = {(1, 1, 1): 1, (8, 37, 5): 1, (31, 16, 31): 1, (32, 32, 32): 1, (33, 33, 33): 1, (65, 255, 70): 1, (40, 512, 36): 1,
            (128, 512, 256): 1, (8, 5760, 12): 12, (4, 1027, 3): 3, (33, 10466, 40): 21, (128, 16416, 128): 32,
            (40, 513, 36): 2, (513, 513, 481): 1, (5, 360, 22): 1}
    got = {(c.B, c.I, c.O): lib_splits(c.B, c.I, c.O) for c in T.FWD_CASES}
    assert got == want
    S, n, cps = T.fc_chunks(128, 16416, 128)
    assert (S, n, cps) == (32, 513, 17) and (S - 1) * cps >= n                  # split 31 starts at chunk 527 of 513
    assert T.fc_chunks(33, 10466, 40) == (21, 328, 16) and T.fc_chunks(513, 513, 481) == (1, 17, 17)
    assert T.fwd_dispatch(128, 512, 256) == 'fc_fwd_kernel'
    assert T.fwd_dispatch(8, 5760, 12) == 'fc_fwd_kernel<split> + fc_fwd_reduce_kernel'
    # the backward: <true> needs O % 4 == 0 and aligned g, W, y
    assert T.bwd_dispatch(12, True, True) == 'fc_bwd_w_kernel + fc_bwd_x_kernel<true>'
    assert T.bwd_dispatch(12, True, True, aligned=False) == 'fc_bwd_w_kernel + fc_bwd_x_kernel<false>'
    assert T.bwd_dispatch(5, False, True) == ' + fc_bwd_x_kernel<false>' and T.bwd_dispatch(36, True, False) == 'fc_bwd_w_kernel'
    assert T.bwd_dispatch(8, False, False) == ''
    vec = {T.case_id(c): T.bwd_vec(c.O, True) for c in T.BWD_CASES}
    assert vec == {'1x1x1': False, '7x33x5': False, '8x37x12-ldx40-lddx40': True, '9x31x31': False, '64x32x32': True,
                   '65x40x33-lddx44': False, '129x70x36': True, '33x65x260': True, '33x65x257': False, '1000x8x7': False,
                   '8x5760x12': True}


def test_case_tables():
    reach = T.table_reach()
    assert set(reach) == set(T.ARMS) and all(reach[a] for a in T.ARMS)
    assert len(reach['fc_fwd_kernel']) == 10 and len(reach['fc_fwd_kernel<split> + fc_fwd_reduce_kernel']) == 5
    assert len(reach['fc_bwd_x_kernel<true>']) == 5 and len(reach['fc_bwd_x_kernel<false>']) == 7
    # the issue's lists, by shape
    assert [(c.B, c.I, c.O) for c in T.BWD_CASES] == [(1, 1, 1), (7, 33, 5), (8, 37, 12), (9, 31, 31), (64, 32, 32), (65, 40, 33),
                                                      (129, 70, 36), (33, 65, 260), (33, 65, 257), (1000, 8, 7), (8, 5760, 12)]
    assert {(c.B, c.I, c.O) for c in T.FWD_CASES} >= {(1, 1, 1), (8, 37, 5), (31, 16, 31), (32, 32, 32), (33, 33, 33), (65, 255, 70),
                                                      (40, 512, 36), (40, 513, 36), (128, 512, 256), (8, 5760, 12), (4, 1027, 3),
                                                      (33, 10466, 40), (128, 16416, 128)}
    assert [(c.B, c.M, c.F, c.pad) for c in T.FLAT_CASES] == [(1, 1, 1, 0), (2, 33, 1, 0), (3, 64, 32, 0), (3, 65, 33, 0),
                                                              (2, 100, 65, 0), (2, 360, 16, 0), (2, 360, 16, 12)]


SENSITIVITY = [T._bwd(7, 33, 5), T._bwd(65, 40, 33, 40, 44), T._bwd(33, 65, 260)]


@pytest.mark.parametrize('c', SENSITIVITY, ids=T.case_id)
def test_exact_leg_sees_one_missing_term(c):
    """One term less in one reduction -- the last i of the forward, the last b of dW and db, the last o of dx -- changes at least
    one element of the exact leg's reference: a dropped last chunk or an off-by-one mask cannot be bit-equal."""
    x, W, g, y = T.bwd_inputs(c, True, True)
    x = x[:, :c.I]
    full = T.fc_ref(x, W, None, False)
    assert (T.fc_ref(x[:, :-1], W[:-1], None, False) != full).any()
    r = T.fc_bwd_ref(x, W, g, y)
    less_b = T.fc_bwd_ref(x[:-1], W, g[:-1], y[:-1])
    assert (less_b['dW'] != r['dW']).any() and (less_b['db'] != r['db']).any()
    less_o = T.fc_bwd_ref(x, W[:, :-1], g[:, :-1], y[:, :-1])
    assert (less_o['dx'] != r['dx']).any()
    # ... and so does a term too many: a gated g that leaks
    leak = T.fc_bwd_ref(x, W, g, None)
    assert all((leak[k] != r[k]).any() for k in ('dW', 'db', 'dx'))
