"""The float64 restatements tests/test_gpu_contract_bf16_arms.py uses as truth for the bf16 contraction at pool 1 and its gradients,
against the oracle's layers (oracle/layers_ref.py: chebyshev5_fwd / _bwd, brelu_fwd / _bwd), and the host-side figures that test
relies on: the exactness inequality, the plant and low-part census, the dispatch restatement against the library's CPU-callable
queries (the gx knobs set and unset), the arm table -- and its discrimination: both legs pass on a NumPy stand-in of the entries
that implements the hi/lo arithmetic, and fail on each planted fault; two faults of one-pass arithmetic pass the old comparison
(1e-2 of the tensor's max) at a size where one term of a weight-gradient sum is small beside the max.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import layers_ref as R

import test_gpu_contract_grad_arms as T
import test_gpu_contract_bf16_arms as A
from test_gpu_contract_bf16_arms import V, Case, Inputs, _f, _w, _x
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import plane_stride

EPS64 = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------------ the oracle

@pytest.mark.parametrize('B,M,Fin,K,Fout', [(3, 7, 2, 1, 3), (2, 9, 3, 4, 5), (4, 5, 11, 3, 2)])
def test_restatement_is_the_oracle(B, M, Fin, K, Fout):
    """The emulated arithmetic is the oracle's layer up to the operands' rounding: 2^-8 per operand in one pass; in three passes
    the residues of the two splits (2^-17 each) and, beyond ``lolo``, the product of two low parts (2^-18).  On bf16-exact
    operands it is the oracle's layer to float64 round-off, whatever the passes."""
    rs = np.random.RandomState(B + M + K)
    Am = sp.random(M, M, 0.5, random_state=rs, format='csr')
    L = sp.csr_matrix(sp.diags(np.asarray((Am + Am.T).sum(axis=1)).ravel()) - (Am + Am.T))
    x = rs.randn(B, M, Fin)
    W = rs.randn(Fin * K, Fout).astype(np.float32)
    bv = (0.3 * rs.randn(Fout, M)).astype(np.float32)
    dout = rs.randn(B, Fout, M).astype(np.float32)
    y_oracle, Tk = R.chebyshev5_fwd(x, L, W.astype(np.float64), K, return_stack=True)   # Tk [K, M, Fin, N]
    for exact in (False, True):
        stack = np.ascontiguousarray(Tk.transpose(0, 3, 2, 1)).astype(np.float32)       # [K, B, Fin, M]: the kernels' fp32 operands
        Wc, dy = W, dout
        if exact:
            stack, Wc, dy = np.round(4 * np.tanh(stack)), np.round(8 * np.tanh(W)) / 8, np.round(4 * np.tanh(dout))
            stack, Wc, dy = stack.astype(np.float32), Wc.astype(np.float32), dy.astype(np.float32)
        # the oracle's contraction (of its own float64 stack; on the rounded operands of the exact pass: the contraction of
        # layers_ref.py chebyshev5_fwd from that stack on) and its bias + ReLU
        Tk32 = np.ascontiguousarray(stack.transpose(0, 3, 2, 1)).astype(np.float64)
        y_o = (Tk32.transpose(3, 1, 2, 0).reshape(B * M, Fin * K) @ Wc.astype(np.float64)).reshape(B, M, Fout)
        S = T.rows_of(stack)
        assert np.abs(T.sums_ref(S, Wc, B, M) - y_o.transpose(0, 2, 1)).max() <= 64 * EPS64 * np.abs(y_o).max()
        if not exact:
            assert np.abs(y_o - y_oracle).max() <= 2.0 ** -22 * np.abs(S).max() * np.abs(Wc).sum(axis=0).max()    # the stack in fp32
            y_o = y_oracle
        a_o = R.brelu_fwd(y_o, bv.T[None].astype(np.float64))
        mag = T.sums_ref(np.abs(S), np.abs(Wc), B, M)
        dy_o, _ = R.brelu_bwd(np.ascontiguousarray(dy.transpose(0, 2, 1)).astype(np.float64), a_o, (1, M, Fout))
        gate = a_o.transpose(0, 2, 1) > 0
        dyg = np.where(gate, dy, np.float32(0))
        assert np.array_equal(dyg, dy_o.transpose(0, 2, 1))
        _, dW_o = R.chebyshev5_bwd(dy_o, L, Wc.astype(np.float64), K, Tk32)
        c = Case('f', B, M, Fin, K, Fout, V, None)
        inp = Inputs(stack, Wc, bv, dyg, None)
        for passes in (1, 3):
            tol = 0.0 if exact else (2.0 ** -7 if passes == 1 else 2.0 ** -15)
            pre = A.pre_emu(c, inp, passes)
            assert np.abs(np.maximum(pre, 0) - a_o.transpose(0, 2, 1)).max() <= tol * mag.max() + 64 * EPS64 * (mag.max() + 1)
            dW = A.dW_emu(c, inp, passes)
            wmag = T.dW_ref(np.abs(S), np.abs(dyg))
            assert np.abs(dW - dW_o).max() <= tol * wmag.max() + 64 * EPS64 * wmag.max()
            # gstack against the restatement tests/test_contract_grad_refs.py runs through the oracle's adjoint recurrence
            gs = A.gstack_emu(c, inp, passes)
            gmag = T.gstack_ref(np.abs(Wc), np.abs(dyg), Fin, K)
            assert np.abs(gs - T.gstack_ref(Wc, dyg, Fin, K)).max() <= tol * gmag.max() + 64 * EPS64 * gmag.max()
            if exact:
                assert np.array_equal(pre, A.plain(c, inp)) and np.array_equal(dW, A.plain(c._replace(kind='w'), inp))
        # what chebgcn_relu_grad_bf16 writes: the oracle's gated gradient, rounded once
        d16 = A.bits_f32(A.bf16_bits(dyg))
        assert np.abs(d16 - dyg).max() <= 2.0 ** -8 * np.abs(dyg).max() and np.array_equal(d16 == 0, dyg == 0)


def test_the_split_is_the_kernels():
    """hi = RNE bf16, lo = bf16(x - hi); x - hi - lo is at most 2^-17 |x|; ties go to even"""
    x = np.random.RandomState(1).standard_normal(4096).astype(np.float32)
    hi, lo = A.split(x)
    assert np.abs(x - hi).max() <= 2.0 ** -8 * np.abs(x).max() and (np.abs(x - hi - lo) <= 2.0 ** -17 * np.abs(x)).all()
    assert np.array_equal(A.bits_f32(A.bf16_bits(x)).astype(np.float64), hi)
    t = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)], np.float32)      # ties
    assert np.array_equal(A.split(t)[0], [1.0, 1 + 2.0 ** -6, -1.0]) and np.array_equal(A.split(t)[1], [2.0 ** -8, -2.0 ** -8, -2.0 ** -8])


# ------------------------------------------------------------------------------------------------------------ host-side figures

def test_exactness_inequality_holds_for_every_case():
    for c in A.CASES:
        A.assert_exact_arithmetic(c)
    assert {A.grid_bits(c, leg) for c in A.CASES for leg, _ in A.legs_of(c) if leg in 'bc'} == {8, 9, 10}
    with pytest.raises(AssertionError):
        A.assert_exact_arithmetic(_w(64, 97, 7, 23, 65))                    # 6208 terms of up to 8.02: no nine-bit grid fits
    with pytest.raises(AssertionError):
        A.assert_exact_arithmetic(_w(2048, 513, 2, 2, 2))                   # leg a: 16 B M > 2^23


@pytest.mark.parametrize('c', A.CASES, ids=A.case_id)
def test_plant_and_low_part_census_hold(c):
    for leg, _ in A.legs_of(c):
        for pad in A.PADS[leg]:
            inp = A.make_inputs(c, leg, pad)
            seen = A.census(c, leg, inp, pad)
            again = A.make_inputs(c, leg, pad)
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(inp, again) if a is not None)
            first = inp.dy if c.kind == 'x' else inp.stack
            second = inp.dy if c.kind == 'w' else inp.W
            data = lambda a: a if a is inp.W else a[..., :c.M]              # noqa: E731
            if leg in 'bd':
                assert seen['first_lo'] == data(first).size                 # every element carries a low part
            if leg in 'cd':
                assert seen['second_lo'] == data(second).size
            if leg == 'a':
                assert np.abs(data(first)).max() <= 4 and np.array_equal(data(first), np.round(data(first)))
                assert c.kind == 'w' or (np.abs(inp.W).max() <= 1 and np.array_equal(inp.W * 8, np.round(inp.W * 8)))


def test_census_notices_a_missing_plant():
    c = _w(3, 33, 3, 5, 33)
    inp = A.make_inputs(c, 'a')
    inp.stack[14 % 5, 2, 14 // 5, 32] = 0                    # row Fin*K - 1 at vertex M - 1 of window B - 1
    with pytest.raises(AssertionError):
        A.census(c, 'a', inp)
    inp = A.make_inputs(c, 'b')
    inp.stack[0, 0, 0, 0] = 1.0                              # a planted corner without a low part
    with pytest.raises(AssertionError):
        A.census(c, 'b', inp)
    inp = A.make_inputs(c, 'c', 'big')
    inp.dy[0, 0, 40] = 0.0                                   # a pad
    with pytest.raises(AssertionError):
        A.census(c, 'c', inp, 'big')
    with pytest.raises(AssertionError):                      # a grid on which a quarter of the values carry low parts
        A.low_census('x', (np.arange(-512, 513) / 256.0).astype(np.float32))


def _shapes():
    rs = np.random.RandomState(11)
    yield from (c[1:6] for c in A.CASES)
    # the thresholds of wide / tiled, of the row-tile groups and of the grid, and the BASELINE layers
    yield from [(3, 97, 160, 1, 65), (3, 97, 161, 1, 64), (3, 97, 161, 1, 65), (3, 97, 320, 1, 256), (3, 97, 321, 1, 257),
                (64, 10466, 60, 5, 256), (16, 10466, 64, 25, 64), (32, 10466, 32, 10, 64), (700, 64, 1, 33, 1000),
                (600, 40, 8, 5, 33), (40, 3000, 8, 5, 600), (1, 1, 1, 1, 1)]
    for _ in range(300):
        yield (int(rs.randint(1, 300)), int(rs.randint(1, 3000)), int(rs.randint(1, 80)), int(rs.randint(1, 26)), int(rs.randint(1, 600)))


def test_dispatch_restatement_agrees_with_the_library(monkeypatch):
    """chebgcn_contract_bwd_w_bf16_workspace (gx, gy, gz and the tile of a partial), _bwd_x_bf16_workspace (the wave count),
    _fwd_bf16_workspace and chebgcn_bf16_dy16_supported need no device (without one the library assumes 256 CUs, as the
    restatement does); the gx knobs are read on every call."""
    lib = _lib.lib()
    n = 0
    for tiled, wide in ((None, None), (7, None), (None, 9), (300, 2), (1, 257), (0, -3)):
        for k, v in ((A.KNOB_TILED, tiled), (A.KNOB_WIDE, wide)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
        for B, M, Fin, K, Fout in _shapes():
            p = A.bwb_plan(B, M, Fin * K, Fout, tiled, wide)
            assert lib.chebgcn_contract_bwd_w_bf16_workspace(B, M, Fin, K, Fout) == A.bwb_workspace(p), (B, M, Fin, K, Fout, p, tiled, wide)
            assert lib.chebgcn_bf16_dy16_supported(B, M, Fin, K, Fout) == int(p.wide)
            assert 1 <= p.gx <= p.total and sum(A.chunk_ranges(p)) == p.total
            if tiled is None and wide is None:
                assert lib.chebgcn_contract_bwd_x_bf16_workspace(Fin, K, Fout) == A.bwd_x_workspace(Fin * K, Fout)
                assert lib.chebgcn_contract_fwd_bf16_workspace(Fin, K, Fout) == A.fwd_workspace(Fin * K, Fout)
            n += 1
    assert n > 1800
    # and on launches whose kernels tests/test_gpu_dispatch.py asserts on the device
    assert A.bwd_w_arm(A.bwb_plan(16, 10466, 1600, 64), 3).startswith('contract_bwd_w_bf16_kernel<5,2,3> + ')
    assert A.bwd_w_arm(A.bwb_plan(32, 10466, 300, 256), 3).startswith('contract_bwd_w_bf16_wide_kernel<3> + ')
    assert A.bwd_w_arm(A.bwb_plan(3, 77, 165, 65), 1, dy16=True).startswith('contract_bwd_w_bf16_wide_kernel<1,dy16> + ')
    assert A.fwd_arm(64, 3).endswith('<3,4,tiles4>') and A.fwd_arm(128, 3).endswith('<3,4,tiles2>') and A.fwd_arm(256, 1).endswith('<1,4>')
    assert A.bwd_x_arm(300, 3).endswith('<3,5>') and A.bwd_x_arm(1600, 3).endswith('<3,5>') and A.bwd_x_arm(600, 1, True).endswith('<1,5,x16>')
    assert A.bwd_x_arm(165, 1, True).endswith('<1,4,x16>')
    assert A.lolo(3, 32) and not A.lolo(3, 33) and not A.lolo(1, 4)


def test_arm_table_reaches_every_arm():
    reach = A.table_reach()
    assert len(reach['tiled']) == 20 and len(reach['wide']) == 9 and len(reach['bwd_x']) == 6 and len(reach['fwd']) == 6
    assert len({A.case_id(c) for c in A.CASES}) == len(A.CASES)
    # every kernel family runs the production plan, and the knob cases set the other kernel's knob to a value that must be ignored
    w = [c for c in A.CASES if c.kind == 'w']
    for wide in (False, True):
        assert sum(c.gx is None for c in w if A.plan_of(c).wide == wide) >= 5 and any(c.gx for c in w if A.plan_of(c).wide == wide)
    assert all(len(set(A.knobs_of(c).values())) == 2 for c in w if c.gx)
    broken = set()                                           # removing a case that alone carries an arm breaks the reach
    for c in A.CASES:
        try:
            A.table_reach([d for d in A.TABLE if d is not c])
        except AssertionError:
            broken.add(A.case_id(c))
    assert len(broken) >= 30 and broken >= {
        'w-B1-M1-1x1-F1', 'w-B3-M32-3x23-F32', 'w-B3-M63-5x32-F17', 'w-B2-M96-32x4-F5', 'w-B2-M65-1x17-F64', 'w-B3-M95-7x13-F40',
        'w-B22-M129-11x3-F1000', 'w-B13-M305-7x23-F65-gx257', 'w-B2-M40-3x107-F65', 'w-B3-M97-7x23-F65-gx2', 'x-B1-M160-171x3-F16',
        'x-B3-M129-12x25-F65', 'f-B3-M4-4x8-F64-f', 'f-B33-M900-2x2-F129-v', 'x-B300-M5-13x5-F17'}, sorted(broken)


# ------------------------------------------------------------------------------------------------------------ discrimination

FAULTS = ('tail_vertex', 'chunk_twice', 'pad_column', 'placeholder_row', 'lo_first', 'lo_second', 'lolo_extra', 'scatter_plane',
          'mask_bit')
SCATTER_K = 3


class StandIn:
    """The entries in NumPy on the padded arrays: float64 sums of the hi/lo arithmetic stored as fp32, NaN left in every output
    pad -- with one planted fault:
      tail_vertex      bwd_w drops the last vertex of one tail chunk (vertex M - 1 of window B - 1, M no multiple of the chunk)
      chunk_twice      bwd_w counts the last chunk of window B - 1 twice
      pad_column       bwd_w sums vertex M of the pad as well
      placeholder_row  the rows beyond Fin*K of the last row tile (kk = 0: copies of row 0) written behind dW
      lo_first         the low part of the stack (bwd_x: of dy) zeroed
      lo_second        the low part of W (bwd_w: of dy) zeroed
      lolo_extra       lo*lo added where it must not be (bwd_x and the forward beyond ``lolo``)
      scatter_plane    the out_K scatter of bwd_x off by one plane for K = 3
      mask_bit         the forward's mask bit of vertex M - 1 flipped (window B - 1, filter Fout - 1)"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def _arith(self, swapped):
        z = (self.fault == 'lo_first', self.fault == 'lo_second')
        return dict(zero_lo=z[::-1] if swapped else z, lolo_extra=self.fault == 'lolo_extra')

    def dy16_supported(self, c):
        return A.plan_of(c).wide

    def bwd_w(self, c, stack, dy, passes):
        p, M, FinK = A.plan_of(c), c.M, c.Fin * c.K
        n = M + 1 if self.fault == 'pad_column' and plane_stride(M) > M else M
        S = T.rows_of(stack[..., :n]).reshape(FinK, c.B, n).copy()
        D = T._flat(dy[..., :n]).reshape(c.Fout, c.B, n).copy()
        if self.fault == 'tail_vertex' and M % p.chunk:
            S[:, c.B - 1, M - 1] = 0
        S2, D2 = S.reshape(FinK, -1), D.reshape(c.Fout, -1)
        if self.fault == 'chunk_twice':
            m0 = (M - 1) // p.chunk * p.chunk
            S2, D2 = np.hstack([S2, S[:, c.B - 1, m0:M]]), np.hstack([D2, D[:, c.B - 1, m0:M]])
        arith = self._arith(False)
        arith['lolo_extra'] = False                           # (the weight gradient's kernels have no such branch)
        o, v = T.new_out((FinK, c.Fout))
        with np.errstate(all='ignore'):
            v[...] = A.emu(S2, np.ascontiguousarray(D2.T), passes, **arith)
        if self.fault == 'placeholder_row':
            beyond = o.whole[T.GUARD + v.size:][:((FinK + 31) // 32 * 32 - FinK) * c.Fout]
            beyond[:] = np.resize(v[0], beyond.size)
        return o

    def bwd_w_dy16(self, c, stack, d16):
        if not A.plan_of(c).wide:
            return -1, None, 'contract_bwd_w_bf16_dy16: only for wide layers (Fin*K > 160 and Fout > 64)'
        return 0, self.bwd_w(c, stack, A.bits_f32(d16), 1), ''

    def bwd_x(self, c, dy, W, passes):
        gs = A.gstack_emu(c, Inputs(None, W, None, dy, None), passes, **self._arith(True))
        if self.fault == 'scatter_plane' and c.K == SCATTER_K:
            gs = np.roll(gs, 1, axis=0)
        o, v = T.new_out((c.K, c.B, c.Fin, plane_stride(c.M)))
        v[..., :c.M] = gs
        return o

    def bwd_x_dy16(self, c, d16, W):
        return self.bwd_x(c, A.bits_f32(d16), W, 1)

    def fwd(self, c, stack, W, bias, relu, passes):
        Mp = plane_stride(c.M)
        pre = A.pre_emu(c, Inputs(stack, W, bias, None, None), passes, **self._arith(True))
        o, v = T.new_out((c.B, c.Fout, Mp))
        v[..., :c.M] = T.out_ref(pre, relu)
        if not relu:
            return o, None
        mo, mv = T.new_out((c.B, c.Fout, Mp // 4), np.uint8)
        mv[...] = T.pack_mask(pre.astype(np.float32) > 0, Mp)
        if self.fault == 'mask_bit':
            mv[c.B - 1, c.Fout - 1, (c.M - 1) // 4] ^= 1 << ((c.M - 1) % 4)
        return o, mo

    def relu_grad16(self, c, dout, mask):
        o, v = T.new_out((c.B, c.Fout, plane_stride(c.M)), np.uint16)
        v[..., :c.M] = A.bf16_bits(np.where(T.unpack_mask(mask, c.M), dout[..., :c.M], np.float32(0)))
        return o


# a tail chunk, a pad (Mp = 64 > M), a ragged row tile (15 / 161 rows); K = 3 and 33 reduction rows: the twin of lolo
SMALL = {'tiled': _w(3, 33, 3, 5, 33), 'wide': _w(2, 33, 7, 23, 65), 'x': _x(2, 5, 11, 3, 33), 'f': _f(2, 5, 11, 3, 33, V)}
CAUGHT_BY = {'tiled': FAULTS[:6], 'wide': FAULTS[:6], 'x': ('lo_first', 'lo_second', 'lolo_extra', 'scatter_plane'),
             'f': ('lo_first', 'lo_second', 'lolo_extra', 'mask_bit')}
# A full-size launch of the weight gradient's sums: B M = 266240 terms, a tail chunk of one vertex
BIG = _w(4096, 65, 2, 4, 8)


@pytest.mark.parametrize('c', [c for c in A.CASES if c.B * c.M * max(c.Fout, c.Fin * c.K) < 2e6] + list(SMALL.values()), ids=A.case_id)
def test_both_legs_pass_on_the_stand_in(c):
    A.run_exact(StandIn(), c)
    m = A.run_roundoff(StandIn(), c)
    A.assert_roundoff(c, m)
    for name, (err, bound, perr, pbound) in m.items():       # float64 sums rounded once to fp32
        assert err <= T.EPS32 and bound in (A.REL, A.GREL) and pbound == (A.BF16_REL if 'P1' in name else A.SPLIT_REL), (name, err)


def test_every_fault_is_planted_somewhere():
    assert set(FAULTS) == {f for fs in CAUGHT_BY.values() for f in fs}
    for c in SMALL.values():
        assert plane_stride(c.M) > c.M and (c.Fin * c.K) % 32
    assert SMALL['x'].K == SCATTER_K and A.reduction(SMALL['x']) == A.reduction(SMALL['f']) == 33
    assert all(c.M % A.plan_of(c).chunk for c in (SMALL['tiled'], SMALL['wide'], BIG))


@pytest.mark.parametrize('where,fault', [(w, f) for w in sorted(CAUGHT_BY) for f in CAUGHT_BY[w]])
def test_exact_leg_fails_on_a_planted_fault(where, fault):
    with pytest.raises(AssertionError):
        A.run_exact(StandIn(fault), SMALL[where])


@pytest.mark.parametrize('where,fault', [(w, f) for w in sorted(CAUGHT_BY) for f in CAUGHT_BY[w]])
def test_roundoff_leg_fails_on_a_planted_fault(where, fault):
    """All but one: lo*lo is at most 2^-18 of a product, so adding it where it must not be moves a sum by less than the 1e-5 /
    2e-5 the leg holds fp32 accumulation to (the kernel's own figures: 0.80e-5 with it against 1.07e-5 without, of the plain
    product).  Only the exact leg's twin of lolo sees that fault; here the leg is asserted to pass, so that the gap is on record."""
    c = SMALL[where]
    if fault == 'lolo_extra':
        m = A.run_roundoff(StandIn(fault), c)
        A.assert_roundoff(c, m)
        assert max(v[0] for v in m.values()) > T.EPS32       # (it did change the sums)
        return
    with pytest.raises(AssertionError):
        A.assert_roundoff(c, A.run_roundoff(StandIn(fault), c))


@pytest.mark.parametrize('fault', ['tail_vertex', 'chunk_twice'])
def test_the_old_comparison_is_blind_to_a_fault_of_one_pass_arithmetic(fault):
    """One term dropped from, or added to, every sum of 266240 terms of the one-pass weight gradient: within 1e-2 of the tensor's
    max of the plain product (the only bound the one-pass arms had), far above 2e-5 of the emulated arithmetic."""
    m = A.run_roundoff(StandIn(fault), BIG)
    err, bound, perr, pbound = m['bwd_w P1']
    assert pbound == A.BF16_REL and perr <= pbound, perr
    assert bound == A.GREL and err > 10 * bound, err
    clean = A.run_roundoff(StandIn(), BIG)['bwd_w P1']
    assert clean[0] <= T.EPS32 and clean[2] <= pbound


def test_sentinels_are_checked_for_dy16():
    o, v = T.new_out((3, 4), np.uint16)
    v[...] = 7
    assert np.array_equal(T.inside(o, 'x'), np.full((3, 4), 7, np.uint16))
    o.whole[T.GUARD + 12] = 0
    with pytest.raises(AssertionError, match='a store left the buffer'):
        T.inside(o, 'x')
