"""The float64 restatements tests/test_gpu_contract_grad_arms.py uses as truth for the fp32 pool-1 contraction and its gradients,
against the oracle's layers (oracle/layers_ref.py: chebyshev5_fwd / _bwd, brelu_fwd / _bwd), and the host-side figures that
test relies on: the exactness inequality, the plant census, the dispatch restatement against the library's CPU-callable
queries, the arm table -- and its discrimination: the exact leg passes on a NumPy stand-in of the entries and fails on each of
six planted faults.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import layers_ref as R

import test_gpu_contract_grad_arms as T
from test_gpu_contract_grad_arms import F, N, V, Case
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import plane_stride

EPS64 = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------------ the oracle

@pytest.mark.parametrize('B,M,Fin,K,Fout', [(3, 7, 2, 1, 3), (2, 9, 3, 4, 5), (4, 5, 1, 3, 1)])
def test_restatement_is_the_oracle(B, M, Fin, K, Fout):
    rs = np.random.RandomState(B + M + K)
    A = sp.random(M, M, 0.5, random_state=rs, format='csr')
    L = sp.csr_matrix(sp.diags(np.asarray((A + A.T).sum(axis=1)).ravel()) - (A + A.T))
    x = rs.randn(B, M, Fin)                                  # the reference's [N, M, F]
    W = rs.randn(Fin * K, Fout)
    bf, bv = 0.3 * rs.randn(Fout), 0.3 * rs.randn(Fout, M)
    dout = rs.randn(B, Fout, M)
    y_o, Tk = R.chebyshev5_fwd(x, L, W, K, return_stack=True)               # Tk [K, M, Fin, N]
    stack = np.ascontiguousarray(Tk.transpose(0, 3, 2, 1))                  # [K, B, Fin, M]
    S = T.rows_of(stack)
    sums = T.sums_ref(S, W, B, M)
    tol = 8 * EPS64 * np.abs(W).sum(axis=0).max() * np.abs(stack).max()
    assert np.abs(sums - y_o.transpose(0, 2, 1)).max() <= tol
    for kind, bias, b_o in ((F, bf, bf.reshape(1, 1, Fout)), (V, bv, bv.T[None])):
        pre = T.pre_ref(sums, kind, bias)
        a_o = R.brelu_fwd(y_o, b_o)
        out = T.out_ref(pre, 1)
        assert np.abs(out - a_o.transpose(0, 2, 1)).max() <= tol
        assert np.array_equal(T.out_ref(pre, 0), pre) and np.array_equal(T.pre_ref(sums, N, None), sums)
        gate = pre > 0
        assert np.array_equal(gate, a_o.transpose(0, 2, 1) > 0)
        assert np.allclose(T.mean_ref(out), a_o.mean(axis=2), rtol=0, atol=tol)
        # the mask byte: bit i of byte q is out[4q + i] > 0, the low nibble only, and back
        Mp = plane_stride(M)
        mask = T.pack_mask(gate, Mp)
        assert mask.shape == (B, Fout, Mp // 4) and (mask >> 4 == 0).all()
        for q in range(Mp // 4):
            for i in range(4):
                want = gate[:, :, 4 * q + i] if 4 * q + i < M else np.zeros((B, Fout), bool)
                assert np.array_equal((mask[:, :, q] >> i) & 1, want.astype(np.uint8))
        assert np.array_equal(T.unpack_mask(mask, M), gate)
        assert np.array_equal(T.gated_ref(sums, gate), sums * gate)
        # ReluGrad + the bias sums, then the two gradients of the contraction
        dy_o, db_o = R.brelu_bwd(np.ascontiguousarray(dout.transpose(0, 2, 1)), a_o, b_o.shape)
        dy = T.dy_ref(gate, dout)
        assert np.array_equal(dy, dy_o.transpose(0, 2, 1))
        db = T.dbias_ref(dy, kind)
        assert np.abs(db - (db_o[0, 0] if kind == F else db_o[0].T)).max() <= 8 * EPS64 * np.abs(dout).sum(axis=(0, 2)).max()
        dx_o, dW_o = R.chebyshev5_bwd(dy_o, L, W, K, Tk)
        assert np.abs(T.dW_ref(S, dy) - dW_o).max() <= 8 * EPS64 * B * M * np.abs(stack).max() * np.abs(dy).max()
        # gstack is the G of chebyshev5_bwd before its adjoint recurrence: run that recurrence on it (layers_ref.py:59-62)
        G = np.ascontiguousarray(T.gstack_ref(W, dy, Fin, K).transpose(0, 3, 2, 1)).reshape(K, M, Fin * B)
        Lt = sp.csr_matrix(R.rescaled_laplacian(L, G.dtype).T)
        for k in range(K - 1, 1, -1):
            G[k - 1] += 2 * Lt.dot(G[k])
            G[k - 2] -= G[k]
        if K > 1:
            G[0] += Lt.dot(G[1])
        dx = G[0].reshape(M, Fin, B).transpose(2, 0, 1)
        assert np.abs(dx - dx_o).max() <= 64 * EPS64 * max(np.abs(dx_o).max(), 1.0) * 4 ** K
        # the filter-mean form: every filter's gradient is the one plane
        gmean = rs.randn(B, M)
        assert np.array_equal(T.dy_mean_ref(gate, gmean), T.dy_ref(gate, np.repeat(gmean[:, None, :], Fout, axis=1)))


# ------------------------------------------------------------------------------------------------------------ host-side figures

def test_exactness_inequality_holds_for_every_case():
    assert max(c.B * c.M for c in T.CASES) == 262400
    for c in T.CASES:
        T.assert_exact_arithmetic(c)
    with pytest.raises(AssertionError):
        T.assert_exact_arithmetic(Case(2048, 513, 2, 2, 2, N))               # 16 B M = 2^24 + ...


@pytest.mark.parametrize('c', T.CASES, ids=T.case_id)
def test_plant_census_holds(c):
    inp = T.make_inputs(c, True)
    seen = T.census(c, inp)
    assert seen['zeros'] >= 1
    again = T.make_inputs(c, True)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(inp, again) if a is not None)      # the inputs are a function of the case
    data = inp.stack[..., :c.M]
    assert np.abs(data).max() <= 4 and np.array_equal(data, np.round(data))
    assert np.abs(inp.W).max() <= 1 and np.array_equal(inp.W * 8, np.round(inp.W * 8))


def test_census_notices_a_missing_plant():
    c = Case(3, 33, 3, 5, 2, F)
    inp = T.make_inputs(c, True)
    inp.stack[0, 2, 0, 32] = 0                               # the plant at vertex M - 1 of window B - 1
    with pytest.raises(AssertionError):
        T.census(c, inp)
    inp = T.make_inputs(c, True)
    inp.hand[0, 0, -1] = 0                                   # a pad byte of the hand-made mask
    with pytest.raises(AssertionError):
        T.census(c, inp)


def _shapes():
    rs = np.random.RandomState(7)
    yield from (c[:5] for c in T.CASES)
    # the thresholds: the small launch, the LDS, the reducers, the bias subsets, the row-tile groups
    yield from [(511, 512, 4, 8, 32), (512, 512, 4, 8, 32), (512, 512, 32, 11, 32), (512, 512, 353, 1, 32), (512, 512, 4, 8, 3),
                (512, 512, 4, 8, 4), (512, 512, 4, 8, 33), (256, 192, 4, 8, 32), (257, 192, 4, 8, 32), (64, 10466, 32, 5, 32),
                (25, 10466, 64, 25, 64), (128, 376, 32, 10, 32), (40, 1044, 32, 5, 24), (3, 8100, 4, 8, 32), (3, 8200, 4, 8, 32)]
    for _ in range(400):
        yield (int(rs.randint(1, 1200)), int(rs.randint(1, 3000)), int(rs.randint(1, 40)), int(rs.randint(1, 12)), int(rs.randint(1, 70)))


def test_dispatch_restatement_agrees_with_the_library():
    """chebgcn_contract_bwd_w_workspace, _bwd_w_relu_bias_merged, _fwd_mean_supported and _fwd_gated_supported need no device (without
    one the library assumes 256 CUs, as the restatement does)."""
    lib = _lib.lib()
    n = 0
    for B, M, Fin, K, Fout in _shapes():
        p = T.bwd_w_plan(B, M, Fin * K, Fout)
        assert lib.chebgcn_contract_bwd_w_workspace(B, M, Fin, K, Fout) == p.gx * p.gy * p.gz * p.rt * 16 * 64 * 4, (B, M, Fin, K, Fout, p)
        assert lib.chebgcn_contract_bwd_w_relu_bias_merged(B, M, Fin, K, Fout) == int(p.merged), (B, M, Fin, K, Fout, p)
        assert lib.chebgcn_contract_fwd_mean_supported(B, M, Fin, K, Fout) == int(T.mean_supported(B, M, Fin * K, Fout))
        assert lib.chebgcn_contract_fwd_gated_supported(B, M, Fin, K, Fout) == int(T.gated_supported(B, M, Fin * K, Fout))
        n += 1
    assert n > 400
    # and on launches whose kernels tests/test_gpu_dispatch.py asserts on the device
    assert T.fwd_arm(64, 10466, 160, 32, V) == 'contract_fwd_ring_kernel' and T.fwd_arm(25, 10466, 800, 32, V) == 'contract_fwd_kernel<1>'
    assert T.bwd_x_arm(64, 10466, 160, 32, True) == 'contract_bwd_x_lds_kernel<true>'
    assert T.bwd_x_arm(64, 10466, 75, 32, False) == 'contract_bwd_x_kernel<true,false,false>'
    assert T.bwd_x_arm(3, 10466, 1600, 64, True) == 'contract_bwd_x_kernel<false,true,true>'
    assert T.bwd_w_arm(64, 10466, 160, 32, True) == 'contract_bwd_w_kernel<5,true> + reduce_partials_wide'
    assert T.bwd_w_arm(25, 10466, 1600, 64, False) == 'contract_bwd_w_kernel<5,false> + reduce_partials_small'
    assert T.bwd_w_arm(64, 10466, 75, 32, True) == 'contract_bwd_w_kernel<3,true> + reduce_partials_wide'
    assert T.bwd_w_plan(25, 10466, 1600, 64)[:3] == (5, 10, 2) and T.bwd_w_plan(64, 10466, 300, 256)[:3] == (5, 2, 8)


def test_arm_table_reaches_every_arm():
    reach = T.table_reach()
    assert len(reach['fwd']) == 6 and len(reach['bwd_x']) == 10 and len(reach['bwd_w']) == 20
    assert len({T.case_id(c) for c in T.CASES}) == len(T.CASES) >= 19
    assert sum(T.mean_supported(c.B, c.M, c.Fin * c.K, c.Fout) for c in T.CASES) >= 3
    assert sum(not T.mean_supported(c.B, c.M, c.Fin * c.K, c.Fout) for c in T.CASES) >= 2
    assert sum(not T.gated_supported(c.B, c.M, c.Fin * c.K, c.Fout) for c in T.CASES) >= 2
    assert {c.bias for c in T.CASES if c.Fout <= 32} == {N, F, V}


# ------------------------------------------------------------------------------------------------------------ discrimination

FAULTS = ('drop_term', 'alias_rows', 'tail_ungated', 'pad_gate', 'drop_last_column', 'one_plane_stride')


class StandIn:
    """The entries in NumPy on the padded arrays (float64 sums stored as fp32, NaN left in every output pad), with one planted
    fault:
      drop_term         one term missing from one dW sum
      alias_rows        the rows beyond Fin*K of the last row-tile group written as copies of row 0 (not masked)
      tail_ungated      bwd_w sums the vertices >= M of the last chunk as well
      pad_gate          a gate bit of a pad vertex lets that vertex's dy into the sums of bwd_w and of the bias gradient
      drop_last_column  filter Fout - 1 of a ragged column tile takes no part in the gradients
      one_plane_stride  the one-plane forms step Fout*Mp from window to window"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def _pre(self, c, stack, W, bias_kind, bias):
        sums = T.sums_ref(T.rows_of(stack[..., :c.M]), W, c.B, c.M)
        return sums, T.pre_ref(sums, bias_kind, bias)

    def fwd(self, c, stack, W, bias_kind, bias, relu):
        Mp = plane_stride(c.M)
        pre = self._pre(c, stack, W, bias_kind, bias)[1]
        o, v = T.new_out((c.B, c.Fout, Mp))
        v[..., :c.M] = T.out_ref(pre, relu)
        if not relu:
            return o, None
        mo, mv = T.new_out((c.B, c.Fout, Mp // 4), np.uint8)
        mv[...] = T.pack_mask(pre > 0, Mp)
        return o, mo

    def fwd_mean(self, c, stack, W, bias_kind, bias):
        if not T.mean_supported(c.B, c.M, c.Fin * c.K, c.Fout):
            return T.EUNSUPPORTED, None, None
        Mp = plane_stride(c.M)
        pre = self._pre(c, stack, W, bias_kind, bias)[1]
        o, v = T.new_out((c.B, Mp))
        v[..., :c.M] = T.mean_ref(T.out_ref(pre, 1))
        mo, mv = T.new_out((c.B, c.Fout, Mp // 4), np.uint8)
        mv[...] = T.pack_mask(pre > 0, Mp)
        return 0, o, mo

    def fwd_gated(self, c, stack, W, gate):
        if not T.gated_supported(c.B, c.M, c.Fin * c.K, c.Fout):
            return T.EUNSUPPORTED, None
        o, v = T.new_out((c.B, c.Fout, plane_stride(c.M)))
        v[..., :c.M] = T.gated_ref(self._pre(c, stack, W, N, None)[0], T.unpack_mask(gate, c.M))
        return 0, o

    def _dy(self, c, src, mask, one_plane):
        """dy [B, Fout, n] float64 as the (faulty) gradient kernels see it: n = M, or Mp where a fault lets the pad in"""
        M, Mp = c.M, plane_stride(c.M)
        n = Mp if self.fault in ('tail_ungated', 'pad_gate') else M
        if one_plane:
            g = src
            if self.fault == 'one_plane_stride':
                flat = src.reshape(-1)
                g = np.stack([flat[(b * c.Fout * Mp + np.arange(Mp)) % flat.size] for b in range(c.B)])
            d = np.repeat(g[:, None, :n], c.Fout, axis=1).astype(np.float64)
        else:
            d = src[..., :n].astype(np.float64)
        if mask is not None:
            d = np.where(T.unpack_mask(mask, n), d, 0.0)
        if self.fault == 'pad_gate' and mask is None:
            d[..., M:] = 0.0
        if self.fault == 'drop_last_column' and c.Fout % 32:
            d[:, -1] = 0.0
        return d

    def bwd_x(self, c, dy, mask, W, one_plane):
        o, v = T.new_out((c.K, c.B, c.Fin, plane_stride(c.M)))
        v[..., :c.M] = T.gstack_ref(W, self._dy(c, dy, mask, one_plane)[..., :c.M], c.Fin, c.K)
        return (o,)

    def _dW(self, c, stack, dy, mask, one_plane):
        d = self._dy(c, dy, mask, one_plane)
        st = stack[..., :d.shape[2]].copy()
        if self.fault == 'pad_gate':
            st[..., c.M:] = 0
        S = T.rows_of(st)
        dW = T.dW_ref(S, d)
        if self.fault == 'drop_term':
            col = (c.B - 1) * d.shape[2] + c.M - 1                       # vertex M - 1 of window B - 1
            terms = np.outer(S[:, col], d[c.B - 1, :, c.M - 1])
            r, o = np.argwhere(terms != 0)[0]
            dW[r, o] -= terms[r, o]
        return dW

    def bwd_w(self, c, stack, dy, mask, one_plane):
        FinK = c.Fin * c.K
        o, v = T.new_out((FinK, c.Fout))
        v[...] = self._dW(c, stack, dy, mask, one_plane)
        if self.fault == 'alias_rows':
            extra = ((FinK + 31) // 32 * 32 - FinK) * c.Fout
            beyond = o.whole[T.GUARD + v.size:][:extra]
            beyond[:] = np.resize(v[0], beyond.size)
        return (o,)

    def bias_grad(self, c, dout, mask, kind, one_plane=False):
        d = self._dy(c, dout, mask, one_plane)
        o, v = T.new_out((c.Fout, plane_stride(c.M)) if kind == V else (c.Fout,))
        if kind == V:
            v[:, :c.M] = T.dbias_ref(d[..., :c.M], V)
        else:
            v[...] = T.dbias_ref(d, F)
        return (o,)

    def bwd_w_bias(self, c, stack, dout, mask):
        if not T.bwd_w_plan(c.B, c.M, c.Fin * c.K, c.Fout).merged:
            return T.EUNSUPPORTED, None, None
        return 0, self.bwd_w(c, stack, dout, mask, False)[0], self.bias_grad(c, dout, mask, V)[0]

    def relu_grad_mean(self, c, gmean, mask, kind):
        o, v = T.new_out((c.B, c.Fout, plane_stride(c.M)))
        v[..., :c.M] = self._dy(c, gmean, mask, True)[..., :c.M]
        return o, self.bias_grad(c, gmean, mask, kind, True)[0]


SMALL = Case(3, 33, 3, 5, 2, F)      # a ragged row tile (15 rows), a ragged column tile, Mp = 64 > M, B and Fout coprime


@pytest.mark.parametrize('c', [Case(1, 1, 1, 1, 1, V), SMALL, Case(2, 129, 7, 5, 31, N), Case(2, 100, 11, 17, 40, N),
                               Case(1, 64, 33, 10, 7, F), Case(512, 33, 4, 8, 32, N), Case(512, 12, 2, 2, 5, V)], ids=T.case_id)
def test_exact_leg_passes_on_the_stand_in(c):
    """(two big launches among them: the filter mean and the gated forward are served there)"""
    T.run_exact(StandIn(), c)


@pytest.mark.parametrize('fault', FAULTS)
def test_exact_leg_fails_on_a_planted_fault(fault):
    assert plane_stride(SMALL.M) > SMALL.M and (SMALL.Fin * SMALL.K) % 32 and SMALL.Fout % 32
    with pytest.raises(AssertionError):
        T.run_exact(StandIn(fault), SMALL)


def test_roundoff_leg_on_the_stand_in():
    """float64 sums rounded once to fp32: every figure within one rounding of its bound's scale, and reported."""
    m = T.run_roundoff(StandIn(), SMALL)
    assert {'fwd', 'bwd_x relu', 'bwd_w relu', 'bwd_x plain', 'bwd_w plain', 'bwd_x relu_mean', 'bwd_w relu_mean', 'bias grad v',
            'bias grad f'} <= set(m)
    for name, (err, bound, ew) in m.items():
        assert err <= T.EPS32 and bound in (T.REL, T.GREL) and ew <= 1.0, (name, err, ew)


def test_sentinels_are_checked():
    o, v = T.new_out((3, 4))
    v[...] = 1.0
    assert np.array_equal(T.inside(o, 'x'), np.ones((3, 4), np.float32))
    o.whole[T.GUARD + 12] = 0.0
    with pytest.raises(AssertionError, match='a store left the buffer'):
        T.inside(o, 'x')
