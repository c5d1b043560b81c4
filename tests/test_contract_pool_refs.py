"""The float64 restatement tests/test_gpu_contract_pool_epilogue.py uses as truth for the contraction's pooling epilogue,
against the oracle's layers (oracle/layers_ref.py: brelu_fwd, mpool1_fwd, apool1_fwd, mpool1_bwd, brelu_bwd) on small random
and tie-heavy inputs at every pool size 1 ... 128, and the host-side figures that test relies on (the edge census, the
dispatch arithmetic, the case table).  No GPU."""
import numpy as np
import pytest

from oracle import layers_ref as R

import test_gpu_contract_pool_epilogue as T
from test_gpu_contract_pool_epilogue import AVG, MAX, F, N, V


def _oracle_layout(x):
    return np.ascontiguousarray(x.transpose(0, 2, 1))        # [B, F, M] -> the reference's [N, M, F]


def _inputs(rs, B, Fo, M, ties):
    if ties:                                                 # a handful of values: most windows hold their maximum twice
        y = rs.randint(-2, 3, (B, Fo, M)).astype(np.float64)
        return y, rs.randint(-1, 2, Fo).astype(np.float64), rs.randint(-1, 2, (Fo, M)).astype(np.float64)
    return rs.randn(B, Fo, M), 0.3 * rs.randn(Fo), 0.3 * rs.randn(Fo, M)


@pytest.mark.parametrize('ties', [False, True], ids=['random', 'ties'])
@pytest.mark.parametrize('pool', [1, 2, 4, 8, 16, 32, 64, 128])
def test_restatement_is_the_oracle(pool, ties):
    rs = np.random.RandomState(pool + 1000 * ties)
    B, Fo, Mo = 2, 3, 5
    M = Mo * pool
    y, bf, bv = _inputs(rs, B, Fo, M, ties)
    y[:, :, :pool] = -2.0                                    # nothing positive in the first window under either bias
    dout = rs.randn(B, Fo, Mo)
    x = _oracle_layout(y)
    seen = dict(tie=0, straddle=0, dead=0)
    for bias_kind, bias, b_o in ((N, None, np.zeros((1, 1, Fo))), (F, bf, bf.reshape(1, 1, Fo)), (V, bv, bv.T[None])):
        for relu in (0, 1):
            a_o = R.brelu_fwd(x, b_o) if relu else x + b_o
            for kind in (MAX, AVG):
                r = T.epilogue_ref(y, bias_kind, bias, relu, pool, kind)
                assert np.array_equal(_oracle_layout(r['a']), a_o)
                if kind == MAX:
                    out_o, arg_o = R.mpool1_fwd(a_o, pool)
                    assert np.array_equal(_oracle_layout(r['out']), out_o)
                    if pool > 1:
                        assert r['byte'].dtype == np.uint8 and np.array_equal(_oracle_layout(r['byte']), arg_o)
                        n = T.edge_census(r, relu, pool, kind)
                        for k in seen:
                            seen[k] += n[k]
                        if relu:                              # nothing positive: 0.0 and index 0
                            dead = r['a'].reshape(B, Fo, Mo, pool).max(axis=3) <= 0
                            assert np.all(r['out'][dead] == 0) and np.all(r['byte'][dead] == 0)
                    else:
                        assert r['byte'] is None and arg_o is None
                    d_a = R.mpool1_bwd(_oracle_layout(dout), None if pool == 1 else _oracle_layout(r['byte']).astype(np.int64),
                                       pool, M)
                else:
                    out_o = R.apool1_fwd(a_o, pool)
                    assert np.abs(_oracle_layout(r['out']) - out_o).max() <= 4 * np.finfo(np.float64).eps * np.abs(a_o).max()
                    if ties:
                        assert np.array_equal(_oracle_layout(r['out']), out_o)         # small integers: both means are exact
                    if 1 < pool <= 8:
                        w = a_o.reshape(B, Mo, pool, Fo)
                        for i in range(pool):
                            assert np.array_equal(_oracle_layout((r['byte'] >> i) & 1), (w[:, :, i, :] > 0).astype(np.uint8))
                        if pool < 8:
                            assert np.all(r['byte'] >> pool == 0)
                    else:
                        assert r['byte'] is None
                    d_a = np.repeat(_oracle_layout(dout) / pool, pool, axis=1)         # AvgPoolGrad: equal shares
                d_y = R.brelu_bwd(d_a, a_o, b_o.shape)[0] if relu else d_a
                g = T.epilogue_grad_ref(dout, r, relu, pool, kind)
                assert np.array_equal(_oracle_layout(g), d_y)
    if ties and pool >= 4:
        assert seen['tie'] > 0 and seen['dead'] > 0
        assert pool < 8 or seen['straddle'] > 0


def test_first_maximum_and_census_on_written_out_windows():
    """Four windows of eight written out by hand: what the byte and the census say about each."""
    w = np.array([[1, 3, 0, 3, 2, 2, 2, 2],                  # tie inside lane 0, first at 1
                  [0, 1, 5, 1, 1, 1, 5, 1],                  # tie across the lanes, first at 2
                  [7, 1, 1, 1, 1, 1, 1, 7],                  # tie across the lanes, but the first maximum is member 0
                  [-1, -2, -3, -1, -1, -5, -1, -2]], np.float64)
    y = w.reshape(1, 1, 32)
    r = T.epilogue_ref(y, N, None, 0, 8, MAX)
    assert r['byte'].tolist() == [[[1, 2, 0, 0]]] and r['out'].tolist() == [[[3, 5, 7, -1]]]
    assert T.edge_census(r, 0, 8, MAX) == dict(tie=2, straddle=1, dead=1)
    r = T.epilogue_ref(y, F, np.array([0.5]), 1, 8, MAX)
    assert r['byte'].tolist() == [[[1, 2, 0, 0]]] and r['out'].tolist() == [[[3.5, 5.5, 7.5, 0.0]]]
    assert T.edge_census(r, 1, 8, MAX) == dict(tie=2, straddle=1, dead=1)
    r = T.epilogue_ref(y, N, None, 1, 8, AVG)
    assert r['byte'].tolist() == [[[0b11111011, 0b11111110, 0xFF, 0]]] and r['out'].tolist() == [[[15 / 8, 15 / 8, 20 / 8, 0.0]]]
    r = T.epilogue_ref(y, N, None, 1, 4, AVG)
    assert r['byte'][0, 0].tolist() == [0b1011, 0b1111, 0b1110, 0b1111, 0b1111, 0b1111, 0, 0]
    with pytest.raises(AssertionError, match='no tie across a lane boundary'):
        T.assert_edges('x', T.epilogue_ref(y[:, :, :8], N, None, 0, 8, MAX), 0, 8, MAX)
    with pytest.raises(AssertionError, match='no window without a positive member'):
        T.assert_edges('x', T.epilogue_ref(y[:, :, :16], N, None, 1, 8, MAX), 1, 8, MAX)
    g = T.epilogue_grad_ref(np.array([[[10.0, 20.0, 30.0, 40.0]]]), T.epilogue_ref(y, N, None, 1, 8, MAX), 1, 8, MAX)
    assert np.flatnonzero(g).tolist() == [1, 10, 16] and g[0, 0, [1, 10, 16]].tolist() == [10, 20, 30]


def test_dispatch_arithmetic():
    """The restated rules on launches whose kernel tests/test_gpu_dispatch.py asserts on the device (CASES, SPLIT_CASES there),
    and at their thresholds."""
    assert T.fwd_arm(64, 10466, 160, 32, 1, V) == 'contract_fwd_ring_kernel'
    assert T.fwd_arm(64, 10466, 160, 32, 2, V) == 'contract_fwd_ring_kernel<pool>'
    assert T.fwd_arm(25, 10466, 800, 32, 1, V) == 'contract_fwd_kernel<1>'
    assert T.fwd_arm(3, 10466, 160, 32, 1, V) == 'contract_fwd_splitk_kernel'
    assert T.fwd_arm(3, 10466, 1600, 64, 1, V) == 'contract_fwd_kernel<2>'
    assert T.fwd_arm(511, 512, 4, 32, 2, N) == 'contract_fwd_splitk_kernel'
    assert T.fwd_arm(512, 512, 4, 32, 2, N) == 'contract_fwd_ring_kernel<pool>'
    assert T.fwd_arm(256, 513, 4, 33, 2, N) == 'contract_fwd_kernel<2>'
    assert T.fwd_arm(512, 512, 352, 32, 2, F) == 'contract_fwd_ring_kernel<pool>'
    assert T.fwd_arm(512, 512, 353, 32, 2, F) == 'contract_fwd_kernel<1>'
    assert T.fwd_arm(512, 512, 4, 3, 2, F) == 'contract_fwd_kernel<1>'
    assert T.fwd_arm(512, 512, 4, 3, 2, V) == 'contract_fwd_ring_kernel<pool>'
    assert T.fwd_arm(512, 512, 4, 4, 2, F) == 'contract_fwd_ring_kernel<pool>'
    assert T.bf16_arm(64, 3) == 'contract_fwd_bf16_kernel<3,4,tiles4>' and T.bf16_arm(65, 1) == 'contract_fwd_bf16_kernel<1,4,tiles2>'
    assert T.bf16_arm(128, 3) == 'contract_fwd_bf16_kernel<3,4,tiles2>' and T.bf16_arm(129, 3) == 'contract_fwd_bf16_kernel<3,4>'


def test_case_table():
    reach = T.table_reach()
    assert len(reach) == 10                                  # four fp32 kernels, three bf16 kernels in one and in three passes
    assert len({T.case_id(c) for c in T.CASES}) == len(T.CASES)
    for c in T.CASES + T.ROUND_TRIPS:
        # the exact leg's arithmetic: |sum| <= 4 * Fin*K (+ 1 of the bias) at a grain of 1/8 -- 14 bits; the average's sum 21
        assert (4 * c.Fin * c.K + 1) * 8 < 2 ** 14 and (4 * c.Fin * c.K + 1) * 8 * c.pool < 2 ** 24
