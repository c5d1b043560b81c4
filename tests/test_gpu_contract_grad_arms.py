"""Every arm of the fp32 pool-1 contraction and of its gradients (csrc/contract.hip, csrc/bias_grad_body.h) at the edges of its
tiles, against float64 NumPy restatements of models_gcn.py:611-629 and its autodiff (:297-303).  Needs an MI355X: ``-m gpu``.

The C entries are called directly: chebgcn_contract_fwd (pool 1), _fwd_mean, _fwd_gated; chebgcn_contract_bwd_x, _bwd_x_relu,
_bwd_x_relu_mean; chebgcn_contract_bwd_w, _bwd_w_relu, _bwd_w_relu_mean, _bwd_w_relu_bias; chebgcn_brelu_pool_bwd (pool 1, the
mask, dy = NULL) and chebgcn_relu_grad_mean.  ``small_launch`` / ``fwd_arm`` / ``bwd_x_arm`` / ``bwd_w_plan`` restate the
dispatch arithmetic for 256 CUs; every call asserts that ``_lib.last_dispatch()`` is exactly the predicted string, and
``test_tables_reach_every_arm`` asserts from the restatement alone that the case table reaches

    contract_fwd_kernel<1>, <2>, contract_fwd_ring_kernel, contract_fwd_splitk_kernel, contract_fwd_ring_kernel<mean>, <gated>;
    the eight contract_bwd_x_kernel<HOLD,MASK,SPLIT> and both contract_bwd_x_lds_kernel<MASK>, the one-plane (filter mean)
    strides on a small, an LDS and a non-LDS arm;
    contract_bwd_w_kernel<RT,MASK> for RT = 1 ... 5 and both MASK, each ending in reduce_partials_small and in
    reduce_partials_wide; reduce_partials_small_bias_kernel at several RT; a ragged last row-tile group (gy > 1), a ragged
    column tile (gz > 1), gx = 1 and gx = 2.

Each case runs two legs through ``run_exact`` / ``run_roundoff``, which take the entries as an object: ``Device`` here, a NumPy
stand-in (with planted faults) in tests/test_contract_grad_refs.py.

Exact leg.  Stack, dout and gmean are integers in [-4, 4], W and the biases multiples of 1/8 in [-1, 1].  Every forward sum is
a multiple of 1/8 of magnitude <= 4 Fin K + 1, every gstack sum a multiple of 1/8 of magnitude <= 4 Fout, every dW sum an
integer of magnitude <= 16 B M, every bias sum an integer <= 4 B M: all below 2^24 units (``assert_exact_arithmetic``), so
exact in fp32 in any order, and out, the mask's low nibbles, gstack, dW, dbias and the gated output over the data columns
[0, M) equal the restatement bit for bit.  The filter mean is bit for bit where Fout is a power of two and goes to the
round-off leg elsewhere.  ``plant`` puts both gate values at vertex 0, at vertex M - 1 and at the first vertex of the last
32-group, 64-chunk and 128-tile for filters 0 and Fout - 1 and windows 0 and B - 1, a pre-activation of exactly zero, and
nonzero weights and operands at the corners; ``census`` asserts that on the host before a case is trusted (a case of one
output -- 1,1,1,1,1 -- holds one gate value: the closed gate at exactly zero; the hand-made mask opens it).  A planted column of
the stack is zero but for reduction row 0, so those vertices reach rows > 0 of dW only in the windows between 0 and B - 1 and
in the round-off leg.  Each launch runs twice into freshly poisoned buffers and the two runs are bit-identical; the entries with
the ReLU gate folded in equal the plain entries on the pre-gated dy, and the merged bias entry the two separate calls, bit for
bit.

Round-off leg.  Standard-normal operands scaled as in test_contraction_arm_vs_float64, against float64 sums of the same fp32
operands, relative to the reference tensor's max: REL = 1e-5 forward, GREL = 2e-5 gradients (test_gpu_dispatch.py).  The
gates of the gradients are the bits the device's own forward wrote (they must equal ``out > 0`` of its output).  The measured
errors and the elementwise figure (error in eps of the element's own term magnitudes, not asserted) go to ``record_measured``.
Measured on an MI355X over the table, worst error / bound: forward 0.075 (7.5e-07, fwd on B512-M100-48x8-F3-f), gradients 0.36
(7.2e-06, the per-filter bias gradient of B1030-M3-2x1-F1-f: ONE sum of 3090 terms that largely cancel; its elementwise figure
is below 1 eps); of the contraction's own gradients bwd_x 0.015 (3.1e-07, B3-M200-32x5-F65-v) and bwd_w 0.021 (4.1e-07,
B1030-M3-2x1-F1-f).  The worst elementwise figures: 2.9 eps forward and bwd_x, 0.9 eps bwd_w, 1.0 eps the bias gradient.

Pad and bounds contract (include/chebgcn.h: the pad [M, Mp) is scratch and never read as data).  Every input pad is NaN --
stack planes, dout / gmean, per-vertex bias rows -- with and without the mask.  The gradients run with the forward's own mask
(round trip) and with a hand-made one whose pad bits -- the pad vertices of the last live byte and every pad byte -- are ones in
the low nibble (the high nibble is unspecified and stays zero).  Nothing is asserted about the values of output pads.  Every
output buffer (gstack [K][B][Fin][Mp], dW, dbias, out, mask, mean, dy) sits between sentinels that must stay intact; the
workspace is exactly chebgcn_contract_bwd_w_workspace() bytes and followed by a sentinel; dW and the data columns of every
float output must be finite.
"""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import BIAS_FILTER, BIAS_NONE, BIAS_VERTEX, plane_stride

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
REL = 1e-5                # forward (test_gpu_dispatch.py REL)
GREL = 2e-5               # gradients (test_gpu_dispatch.py GREL)
EPS32 = float(np.finfo(np.float32).eps)
EUNSUPPORTED = -4         # CHEBGCN_EUNSUPPORTED
CUS = 256                 # the CU count the dispatch restatement assumes
ASSUMES = 'the dispatch restatement assumes %d CUs' % CUS
N, F, V = BIAS_NONE, BIAS_FILTER, BIAS_VERTEX


# ------------------------------------------------------------------------------------------------------------ restatement
# Host layout: stack [K, B, Fin, M], W [Fin*K, Fout] (row r = fin*K + k), bias [Fout] or [Fout, M], dout [B, Fout, M],
# gmean [B, M] -- data columns only, float64 arithmetic.

def rows_of(stack):
    """[K, B, Fin, M] -> S [Fin*K, B*M] float64: row r = fin*K + k is plane stack[r % K, :, r // K, :]."""
    K, B, Fin, M = stack.shape
    return np.ascontiguousarray(stack.transpose(2, 0, 1, 3), dtype=np.float64).reshape(Fin * K, B * M)


def _flat(t):
    """[B, Fout, M] -> [Fout, B*M] float64"""
    B, Fo, M = t.shape
    return np.ascontiguousarray(t.transpose(1, 0, 2), dtype=np.float64).reshape(Fo, B * M)


def sums_ref(S, W, B, M):
    """sum_r W[r, o] stack[r % K, b, r // K, m]: [B, Fout, M]"""
    return (np.asarray(W, np.float64).T @ S).reshape(W.shape[1], B, M).transpose(1, 0, 2)


def pre_ref(sums, bias_kind, bias):
    if bias_kind == BIAS_FILTER:
        return sums + np.asarray(bias, np.float64)[None, :, None]
    if bias_kind == BIAS_VERTEX:
        return sums + np.asarray(bias, np.float64)[None, :, :sums.shape[2]]
    return sums


def out_ref(pre, relu):
    return np.maximum(pre, 0.0) if relu else pre


def mean_ref(out):
    return out.sum(axis=1) / out.shape[1]


def gated_ref(sums, gate):
    """chebgcn_contract_fwd_gated: gate bit ? sum : 0, no bias"""
    return np.where(gate, sums, 0.0)


def pack_mask(gate, Mp):
    """bool [B, Fout, M] -> bytes [B, Fout, Mp / 4]: bit i of byte q is gate[4q + i], low nibble only, pad bits zero"""
    B, Fo, M = gate.shape
    g = np.zeros((B, Fo, Mp), np.uint8)
    g[..., :M] = gate
    g = g.reshape(B, Fo, Mp // 4, 4)
    return (g[..., 0] | g[..., 1] << 1 | g[..., 2] << 2 | g[..., 3] << 3).astype(np.uint8)


def unpack_mask(mask, M):
    """bytes [B, Fout, Mq] -> bool [B, Fout, M] (the low nibbles' bits of the data vertices)"""
    B, Fo, Mq = mask.shape
    return ((mask[..., None] >> np.arange(4, dtype=np.uint8)) & 1).reshape(B, Fo, 4 * Mq)[..., :M].astype(bool)


def dy_ref(gate, dout):
    return np.where(gate, np.asarray(dout, np.float64), 0.0)


def dy_mean_ref(gate, gmean):
    """the _mean entries: every filter's gradient is the one plane gmean[b]"""
    return np.where(gate, np.asarray(gmean, np.float64)[:, None, :], 0.0)


def dW_ref(S, dy):
    """dW[r, o] = sum_{b, m} stack_r[b, m] dy[b, o, m]"""
    return S @ _flat(dy).T


def gstack_ref(W, dy, Fin, K):
    """gstack[k, b, fin, m] = sum_o W[fin*K + k, o] dy[b, o, m]"""
    B, Fo, M = dy.shape
    return (np.asarray(W, np.float64) @ _flat(dy)).reshape(Fin, K, B, M).transpose(1, 2, 0, 3)


def dbias_ref(dy, bias_kind):
    return dy.sum(axis=0) if bias_kind == BIAS_VERTEX else dy.sum(axis=(0, 2))


# ------------------------------------------------------------------------------------------------------------ dispatch restatement

def small_launch(B, M):
    return (M + 511) // 512 * B < 2 * CUS


def ring_rows(FinK):
    return (FinK + 15) // 16 * 16


def ring_fits(FinK):
    return ring_rows(FinK) * 136 <= 48 * 1024


def fwd_arm(B, M, FinK, Fout, bias_kind):
    """The kernel chebgcn_contract_fwd launches at pool 1."""
    if Fout > 32:
        return 'contract_fwd_kernel<2>'
    if small_launch(B, M):
        return 'contract_fwd_splitk_kernel'
    if ring_fits(FinK) and (bias_kind != BIAS_FILTER or Fout >= 4):
        return 'contract_fwd_ring_kernel'
    return 'contract_fwd_kernel<1>'


def mean_supported(B, M, FinK, Fout):
    return 4 <= Fout <= 32 and not small_launch(B, M) and ring_fits(FinK)


def gated_supported(B, M, FinK, Fout):
    return Fout <= 32 and not small_launch(B, M) and ring_fits(FinK)


def bwd_x_arm(B, M, FinK, Fout, mask):
    mk, hold = 'true' if mask else 'false', 'true' if Fout <= 32 else 'false'
    if small_launch(B, M):
        return 'contract_bwd_x_kernel<%s,%s,true>' % (hold, mk)
    if Fout <= 32 and FinK % 32 == 0 and (FinK + 31) // 32 * 32 * 136 <= 48 * 1024:
        return 'contract_bwd_x_lds_kernel<%s>' % mk
    return 'contract_bwd_x_kernel<%s,%s,false>' % (hold, mk)


def bw_rt(ntiles):
    return min(ntiles, 5)


def bw_grid_x(B, M, groups):
    """Workgroups per row-tile group and column tile: two per CU over the launch in multiples of 64, at least a quarter of the CUs,
    at most one per CG_BWW_MINCHUNK = 3 chunks of 64 vertices."""
    gx = (2 * CUS // max(groups, 1) + 63) // 64 * 64
    gx = max(gx, CUS // 4)
    total = B * ((M + 63) // 64)
    return max(1, min(gx, (total + 2) // 3))


def bias_grad_blocks(M, Fo):
    """(workgroups along the vertices, batch subsets per workgroup) of bias_grad_relu_kernel"""
    Mq = plane_stride(M) // 4
    fine = (Mq + 63) // 64 * Fo < 512
    return ((Mq + 15) // 16, 16) if fine else ((Mq + 63) // 64, 4)


Plan = collections.namedtuple('Plan', 'rt gy gz gx tail merged')


def bwd_w_plan(B, M, FinK, Fout):
    """Row tiles per workgroup, grid (gx, gy, gz), the reducer of chebgcn_contract_bwd_w* and whether
    chebgcn_contract_bwd_w_relu_bias serves the launch."""
    ntiles = (FinK + 31) // 32
    rt = bw_rt(ntiles)
    gy, gz = (ntiles + rt - 1) // rt, (Fout + 31) // 32
    gx = bw_grid_x(B, M, gy * gz)
    return Plan(rt, gy, gz, gx, 'reduce_partials_small' if gx <= 256 else 'reduce_partials_wide',
                gx <= 256 and bias_grad_blocks(M, Fout)[1] == 16)


def bwd_w_arm(B, M, FinK, Fout, mask, merged=False):
    p = bwd_w_plan(B, M, FinK, Fout)
    return 'contract_bwd_w_kernel<%d,%s> + %s' % (p.rt, 'true' if mask else 'false',
                                                  'reduce_partials_small_bias_kernel' if merged else p.tail)


def bias_grad_arm(M, Fo, bias_kind, mean=False):
    name = 'bias_grad_relu_kernel<%s,%d>%s' % ({F: 'CHEBGCN_BIAS_FILTER', V: 'CHEBGCN_BIAS_VERTEX'}[bias_kind],
                                               bias_grad_blocks(M, Fo)[1], '<mean>' if mean else '')
    return name + (' + bias_filter_reduce_kernel' if bias_kind == F else '')


# ------------------------------------------------------------------------------------------------------------ the case table

Case = collections.namedtuple('Case', 'B M Fin K Fout bias')
# what the issue's table says of each row: forward arm, bwd_x arm (MASK left open), (rt, gy, gz, gx), reducer
Expect = collections.namedtuple('Expect', 'fwd bwd_x grid tail')
_SPLITK, _RING, _F1, _F2 = 'contract_fwd_splitk_kernel', 'contract_fwd_ring_kernel', 'contract_fwd_kernel<1>', 'contract_fwd_kernel<2>'
_BX, _LDS = 'contract_bwd_x_kernel<%s,*,%s>', 'contract_bwd_x_lds_kernel<*>'
_S, _W = 'reduce_partials_small', 'reduce_partials_wide'

TABLE = [
    # B, M, Fin, K, Fout, bias kind of the forward
    (Case(1, 1, 1, 1, 1, V), Expect(_SPLITK, _BX % ('true', 'true'), (1, 1, 1, 1), _S)),         # one output
    (Case(3, 33, 3, 5, 2, F), Expect(_SPLITK, _BX % ('true', 'true'), (1, 1, 1, 1), _S)),
    (Case(2, 129, 7, 5, 31, N), Expect(_SPLITK, _BX % ('true', 'true'), (2, 1, 1, 2), _S)),      # Mp = 160: half of the last 64-chunk outside the plane
    (Case(5, 127, 13, 5, 32, V), Expect(_SPLITK, _BX % ('true', 'true'), (3, 1, 1, 4), _S)),
    (Case(2, 513, 32, 4, 33, F), Expect(_F2, _BX % ('false', 'true'), (4, 1, 2, 6), _S)),        # gz = 2, the second tile holds one column
    (Case(3, 200, 32, 5, 65, V), Expect(_F2, _BX % ('false', 'true'), (5, 1, 3, 4), _S)),        # gz = 3 ragged
    (Case(2, 100, 11, 17, 40, N), Expect(_F2, _BX % ('false', 'true'), (5, 2, 2, 2), _S)),       # six row tiles: the last group holds one
    (Case(1, 64, 33, 10, 7, F), Expect(_SPLITK, _BX % ('true', 'true'), (5, 3, 1, 1), _S)),      # eleven row tiles, gx = 1
    (Case(512, 33, 4, 8, 32, N), Expect(_RING, _LDS, (1, 1, 1, 171), _S)),
    (Case(520, 31, 32, 11, 5, V), Expect(_RING, _LDS, (5, 3, 1, 174), _S)),                      # 352 rows: the most the LDS holds
    (Case(512, 129, 3, 5, 4, F), Expect(_RING, _BX % ('true', 'false'), (1, 1, 1, 512), _W)),    # a per-filter bias at Fout = 4
    (Case(512, 100, 48, 8, 3, F), Expect(_F1, _BX % ('true', 'false'), (5, 3, 1, 192), _S)),     # 384 rows: beyond the LDS, and Fout < 4
    (Case(600, 40, 8, 5, 33, V), Expect(_F2, _BX % ('false', 'false'), (2, 1, 2, 200), _S)),
    (Case(771, 33, 13, 5, 32, N), Expect(_RING, _BX % ('true', 'false'), (3, 1, 1, 257), _W)),   # one over the reducers' threshold
    (Case(257, 130, 16, 4, 17, V), Expect(_SPLITK, _BX % ('true', 'true'), (2, 1, 1, 257), _W)),
    (Case(300, 513, 16, 8, 32, F), Expect(_RING, _LDS, (4, 1, 1, 512), _W)),                     # the second workgroup of a window: one live wave
    (Case(800, 64, 32, 5, 32, N), Expect(_RING, _LDS, (5, 1, 1, 267), _W)),
    (Case(1030, 3, 2, 1, 1, F), Expect(_F1, _BX % ('true', 'false'), (1, 1, 1, 344), _W)),       # K = 1; one filter with a per-filter bias
    (Case(1030, 3, 2, 1, 1, V), Expect(_RING, _BX % ('true', 'false'), (1, 1, 1, 344), _W)),     # (an added row: the ring kernel on that shape)
    (Case(256, 1025, 5, 7, 24, V), Expect(_RING, _BX % ('true', 'false'), (2, 1, 1, 512), _W)),  # Mp = 1056: 32 of the last 128 inside
]
CASES = [c for c, _ in TABLE]


def case_id(c):
    return 'B%d-M%d-%dx%d-F%d-%s' % (c.B, c.M, c.Fin, c.K, c.Fout, 'nfv'[c.bias])


def table_reach():
    """What the table reaches by the dispatch restatement (no device): asserts the list in the module docstring."""
    fwd, bwx, one_plane, bww, merged_rt = set(), set(), set(), set(), set()
    ragged_y = ragged_z = False
    gxs = set()
    for c, e in TABLE:
        FinK = c.Fin * c.K
        p = bwd_w_plan(c.B, c.M, FinK, c.Fout)
        assert fwd_arm(c.B, c.M, FinK, c.Fout, c.bias) == e.fwd, (c, fwd_arm(c.B, c.M, FinK, c.Fout, c.bias))
        for mk in (True, False):
            assert bwd_x_arm(c.B, c.M, FinK, c.Fout, mk) == e.bwd_x.replace('*', 'true' if mk else 'false'), (c, mk)
        assert (p.rt, p.gy, p.gz, p.gx) == e.grid and p.tail == e.tail, (c, p)
        fwd.add(e.fwd)
        if mean_supported(c.B, c.M, FinK, c.Fout):
            fwd.add('contract_fwd_ring_kernel<mean>')
        if gated_supported(c.B, c.M, FinK, c.Fout):
            fwd.add('contract_fwd_ring_kernel<gated>')
        for mk in (True, False):
            bwx.add(bwd_x_arm(c.B, c.M, FinK, c.Fout, mk))
            bww.add(bwd_w_arm(c.B, c.M, FinK, c.Fout, mk))
        one_plane.add(bwd_x_arm(c.B, c.M, FinK, c.Fout, True))           # the _mean gradients run on every row
        if p.merged:
            merged_rt.add(p.rt)
        ntiles = (FinK + 31) // 32
        ragged_y |= p.gy > 1 and ntiles % p.rt != 0
        ragged_z |= p.gz > 1 and c.Fout % 32 != 0
        gxs.add(p.gx)
    tf = ('true', 'false')
    assert fwd == {_F1, _F2, _RING, _SPLITK, 'contract_fwd_ring_kernel<mean>', 'contract_fwd_ring_kernel<gated>'}, sorted(fwd)
    assert bwx == {'contract_bwd_x_kernel<%s,%s,%s>' % (h, m, s) for h in tf for m in tf for s in tf} | \
        {'contract_bwd_x_lds_kernel<%s>' % m for m in tf}, sorted(bwx)
    assert any(a.endswith(',true>') for a in one_plane) and any('lds' in a for a in one_plane) and \
        any(a.endswith(',false>') for a in one_plane), sorted(one_plane)
    assert bww == {'contract_bwd_w_kernel<%d,%s> + %s' % (rt, m, t) for rt in range(1, 6) for m in tf for t in (_S, _W)}, sorted(bww)
    assert len(merged_rt) >= 2, sorted(merged_rt)
    assert ragged_y and ragged_z and {1, 2} <= gxs
    assert any(p.tail == _W and not p.merged for p in (bwd_w_plan(c.B, c.M, c.Fin * c.K, c.Fout) for c in CASES))
    return dict(fwd=sorted(fwd), bwd_x=sorted(bwx), one_plane=sorted(one_plane), bwd_w=sorted(bww), merged_rt=sorted(merged_rt),
                gx=sorted(gxs))


def assert_exact_arithmetic(c):
    """Every sum of the exact leg stays below 2^24 units of its grain (1/8 or 1): exact in fp32 in any order."""
    FinK = c.Fin * c.K
    assert (4 * FinK + 1) * 8 < 2 ** 24, c                   # forward: |stack| <= 4, |W| <= 1, |bias| <= 1, grain 1/8
    assert (4 * FinK + 1) * 8 * c.Fout < 2 ** 24, c          # the sum over the filters of the mean
    assert 4 * c.Fout * 8 < 2 ** 24, c                       # gstack: |W| <= 1, |dy| <= 4, grain 1/8
    assert 16 * c.B * c.M < 2 ** 24, c                       # dW: |stack| <= 4, |dy| <= 4, integers
    assert 4 * c.B * c.M < 2 ** 24, c                        # dbias


# ------------------------------------------------------------------------------------------------------------ inputs

Inputs = collections.namedtuple('Inputs', 'stack W bias dout gmean hand')


def special_vertices(M):
    """vertex 0, vertex M - 1 (the last vertex of the last 32-group, 64-chunk and 128-tile) and the first vertex of each of those"""
    last = M - 1
    return sorted({0, last, last // 32 * 32, last // 64 * 64, last // 128 * 128})


def zero_vertex(M):
    """where ``plant`` puts a pre-activation of exactly zero (window 0, filter 0)"""
    return 1 if M >= 3 else 0


def plant(c, stack, W, bias, dout, gmean):
    """Filters 0 and Fout - 1 see reduction row 0 with weights +1 and -1; the planted columns of the stack hold +-2 or +-4 in row 0
    and zero elsewhere, so the two filters' gates are opposite and alternate from one special vertex and window to the next."""
    B, M, Fin, K, Fout = c[:5]
    FinK, lf = Fin * K, Fout - 1
    W[0, 0] = 1.0
    if Fout > 1:
        W[0, lf] = -1.0
    if FinK > 1:
        W[FinK - 1, 0] = W[FinK - 1, 0] or 0.5
        W[FinK - 1, lf] = W[FinK - 1, lf] or -0.5
    for bi, b in enumerate(sorted({0, B - 1})):
        for vi, v in enumerate(special_vertices(M)):
            stack[:, b, :, v] = 0
            stack[0, b, 0, v] = (1 if (bi + vi) % 2 == 0 else -1) * (2 + 2 * (vi % 2))
            for f in (0, lf):
                dout[b, f, v] = dout[b, f, v] or 3
            gmean[b, v] = gmean[b, v] or -3
    z = zero_vertex(M)
    stack[:, 0, :, z] = 0
    if c.bias != BIAS_NONE:                                  # 1 * 1 + (-1) = 0
        stack[0, 0, 0, z] = 1
        if c.bias == BIAS_FILTER:
            bias[0] = -1.0
        else:
            bias[0, z] = -1.0
    dout[B - 1, :, M - 1] = np.where(dout[B - 1, :, M - 1] == 0, 3, dout[B - 1, :, M - 1])


def _seed(c, exact):
    return (zlib.crc32(case_id(c).encode()) + (0 if exact else 1)) % (2 ** 31)


def make_inputs(c, exact):
    """Padded fp32 arrays, every pad NaN: stack [K, B, Fin, Mp], W, bias (None / [Fout] / [Fout, Mp]), dout [B, Fout, Mp],
    gmean [B, Mp], and the hand-made mask [B, Fout, Mp / 4] (random low nibbles, the bits of pad vertices ones)."""
    B, M, Fin, K, Fout = c[:5]
    Mp, FinK = plane_stride(M), Fin * K
    rs = np.random.RandomState(_seed(c, exact))
    bshape = {N: None, F: (Fout,), V: (Fout, Mp)}[c.bias]
    if exact:
        def draw(shape, lo, hi, scale=1.0):
            return (rs.randint(lo, hi + 1, shape).astype(np.float32) * np.float32(scale))
        stack, dout, gmean = draw((K, B, Fin, Mp), -4, 4), draw((B, Fout, Mp), -4, 4), draw((B, Mp), -4, 4)
        W = draw((FinK, Fout), -8, 8, 0.125)
        bias = draw(bshape, -8, 8, 0.125) if bshape else None
        plant(c, stack, W, bias, dout, gmean)
    else:
        def draw(shape, scale=1.0):
            return (rs.standard_normal(shape) * scale).astype(np.float32)
        stack, dout, gmean = draw((K, B, Fin, Mp)), draw((B, Fout, Mp)), draw((B, Mp))
        W = draw((FinK, Fout), 0.5 / np.sqrt(FinK))
        bias = draw(bshape, 0.3) if bshape else None
    hand = rs.randint(0, 16, (B, Fout, Mp // 4)).astype(np.uint8)
    vert = np.arange(Mp).reshape(Mp // 4, 4)
    hand |= ((vert >= M) << np.arange(4)).sum(axis=1).astype(np.uint8)[None, None, :]
    for a in (stack, dout, gmean) + ((bias,) if c.bias == BIAS_VERTEX else ()):
        a[..., M:] = np.nan
    return Inputs(stack, W, bias, dout, gmean, hand)


def census(c, inp):
    """The plants hold (host arithmetic on windows 0 and B - 1 only)."""
    B, M, Fin, K, Fout = c[:5]
    what = case_id(c)
    bs, fs, vs = sorted({0, B - 1}), sorted({0, Fout - 1}), special_vertices(M)
    sub = inp.stack[:, bs][..., :M]
    pre = pre_ref(sums_ref(rows_of(sub), inp.W, len(bs), M), c.bias, inp.bias)
    gate = pre > 0
    pos = [(bi, f, v) for bi in range(len(bs)) for f in fs for v in vs if not (bi == 0 and v == zero_vertex(M))]
    for axis, keys in ((0, range(len(bs))), (1, fs), (2, vs)):
        for k in keys:
            here = [gate[p] for p in pos if p[axis] == k]
            assert len(here) < 2 or set(here) == {False, True}, '%s: one gate value only at %s %d' % (what, 'bfv'[axis], k)
    assert len(pos) < 2 or {gate[p] for p in pos} == {False, True}, what
    assert pre[0, 0, zero_vertex(M)] == 0 and not gate[0, 0, zero_vertex(M)], what + ': no closed gate at exactly zero'
    W = inp.W
    assert W[0].any() and W[-1].any() and W[:, 0].any() and W[:, -1].any(), what + ': a zero edge of W'
    assert inp.stack[:, B - 1, :, M - 1].any() and inp.dout[B - 1, :, M - 1].all() and inp.gmean[B - 1, M - 1] != 0, what
    assert np.isnan(inp.stack[..., M:]).all() and np.isnan(inp.dout[..., M:]).all() and np.isnan(inp.gmean[..., M:]).all()
    if c.bias == BIAS_VERTEX:
        assert np.isnan(inp.bias[:, M:]).all()
    # the hand-made mask: pad bits ones in the low nibble, the high nibble zero
    assert (inp.hand >> 4 == 0).all() and unpack_mask(inp.hand, plane_stride(M))[..., M:].all(), what
    return dict(open=int(gate.sum()), zeros=int((pre == 0).sum()))


# ------------------------------------------------------------------------------------------------------------ guarded buffers

GUARD = 4096                                                 # elements on either side of every output
SENT = {np.dtype(np.float32): -12345.0, np.dtype(np.uint8): 0xA5}
POISON = {np.dtype(np.float32): np.nan, np.dtype(np.uint8): 0x5A}
Out = collections.namedtuple('Out', 'whole shape')           # a flat host array, guards included, and the shape of its inside


def new_out(shape, dtype=np.float32):
    """(Out, inside view) on the host: poison inside, sentinels around."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, POISON[np.dtype(dtype)], dtype)
    whole[:GUARD] = SENT[np.dtype(dtype)]
    whole[GUARD + n:] = SENT[np.dtype(dtype)]
    return Out(whole, tuple(shape)), whole[GUARD:GUARD + n].reshape(shape)


def inside(o, what):
    """The inside of an output after asserting that its sentinels are intact."""
    s = SENT[o.whole.dtype]
    n = o.whole.size - 2 * GUARD
    assert (o.whole[:GUARD] == s).all() and (o.whole[GUARD + n:] == s).all(), what + ': a store left the buffer (sentinels changed)'
    return o.whole[GUARD:GUARD + n].reshape(o.shape)


# ------------------------------------------------------------------------------------------------------------ the two legs

def _bits_equal(what, got, ref64):
    """fp32 ``got`` equals the float64 reference bit for bit (the reference must be exact in fp32; its zeros are +0)."""
    ref32 = ref64.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref64), what + ': the reference is not exact in fp32'
    assert np.isfinite(got).all(), what + ': a value that is not finite'
    bad = np.ascontiguousarray(got).view(np.uint32) != (ref32 + np.float32(0)).view(np.uint32)
    assert not bad.any(), '%s: %d of %d values differ from the restatement, first at %s: %r against %r' % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref32[bad][0])


def _twice(what, call, ncols):
    """``call()`` twice into fresh buffers: the first run's outputs (insides, sentinels checked) after asserting that the data
    columns of both runs are bit-identical.  ncols: per output the number of leading data columns, None = all."""
    first, second = call(), call()
    res = []
    for i, (a, b, n) in enumerate(zip(first, second, ncols)):
        if a is None:
            res.append(None)
            continue
        x, y = inside(a, what)[..., :n], inside(b, what)[..., :n]
        if x.dtype == np.uint8:
            x, y = x & 15, y & 15
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), \
            '%s: two runs differ (output %d)' % (what, i)
        res.append(inside(a, what))
    return res


def _served(what, res):
    """(rc, outputs ...) of an entry that may refuse a shape -> the outputs, after asserting that it did not"""
    assert res[0] == 0, '%s: refused (%d)' % (what, res[0])
    return res[1:]


def _bias_kinds(c):
    """bias gradients asked of a case: per vertex always (what the merged entry must equal), per filter with a per-filter layer"""
    return (V, F) if c.bias == F else (V,)


def run_exact(E, c, inp=None):
    """The exact leg of case ``c`` on the entries ``E``: every comparison bit for bit.  Returns the census."""
    what = case_id(c)
    B, M, Fin, K, Fout = c[:5]
    Mp, FinK, Mq = plane_stride(M), Fin * K, (M + 3) // 4
    assert_exact_arithmetic(c)
    inp = inp or make_inputs(c, True)
    seen = census(c, inp)
    plan = bwd_w_plan(B, M, FinK, Fout)
    S = rows_of(inp.stack[..., :M])
    sums = sums_ref(S, inp.W, B, M)
    pre = pre_ref(sums, c.bias, inp.bias)
    gate = pre > 0

    # ---- forward: with ReLU and the mask (twice), without ReLU
    out, mask = _twice(what + ' fwd', lambda: E.fwd(c, inp.stack, inp.W, c.bias, inp.bias, 1), (M, Mq))
    _bits_equal(what + ' fwd out', out[..., :M], out_ref(pre, 1))
    assert np.array_equal(unpack_mask(mask, M), gate), what + ': the mask is not out > 0'
    out0, _ = E.fwd(c, inp.stack, inp.W, c.bias, inp.bias, 0)
    _bits_equal(what + ' fwd out without ReLU', inside(out0, what)[..., :M], pre)
    if mean_supported(B, M, FinK, Fout):
        mean, mmask = _twice(what + ' fwd_mean', lambda: _served(what, E.fwd_mean(c, inp.stack, inp.W, c.bias, inp.bias)), (M, Mq))
        assert np.array_equal(unpack_mask(mmask, M), gate), what + ': the mask of fwd_mean is not out > 0'
        if Fout & (Fout - 1) == 0:
            _bits_equal(what + ' mean', mean[..., :M], mean_ref(out_ref(pre, 1)))
        else:                                                # an inexact division: one rounding of an exact sum
            err = np.abs(mean[..., :M] - mean_ref(out_ref(pre, 1))).max() / np.abs(pre).max()
            assert err <= REL, '%s mean: %.3e' % (what, err)
    else:
        assert E.fwd_mean(c, inp.stack, inp.W, c.bias, inp.bias)[0] == EUNSUPPORTED, what + ': fwd_mean served an unsupported shape'
    hand_gate = unpack_mask(inp.hand, M)
    if gated_supported(B, M, FinK, Fout):
        gout, = _twice(what + ' fwd_gated', lambda: _served(what, E.fwd_gated(c, inp.stack, inp.W, inp.hand)), (M,))
        _bits_equal(what + ' gated out', gout[..., :M], gated_ref(sums, hand_gate))
    else:
        assert E.fwd_gated(c, inp.stack, inp.W, inp.hand)[0] == EUNSUPPORTED, what + ': fwd_gated served an unsupported shape'

    # ---- gradients.  The forward's own mask as the device left it (round trip), and the hand-made one with its pad bits set.
    pregated = np.where(np.isnan(inp.dout), inp.dout, 0).astype(np.float32)       # gate * dout on the data, the pad stays NaN
    pregated[..., :M] = dy_ref(gate, inp.dout[..., :M])
    for tag, mk, g in (('own mask', np.ascontiguousarray(mask), gate), ('hand mask', inp.hand, hand_gate)):
        w = '%s %s' % (what, tag)
        dy = dy_ref(g, inp.dout[..., :M])
        gs, = _twice(w + ' bwd_x_relu', lambda: E.bwd_x(c, inp.dout, mk, inp.W, False), (M,))
        _bits_equal(w + ' bwd_x_relu', gs[..., :M], gstack_ref(inp.W, dy, Fin, K))
        dW, = _twice(w + ' bwd_w_relu', lambda: E.bwd_w(c, inp.stack, inp.dout, mk, False), (None,))
        _bits_equal(w + ' bwd_w_relu', dW, dW_ref(S, dy))
        for kind in _bias_kinds(c):
            db, = _twice(w + ' bias grad', lambda: E.bias_grad(c, inp.dout, mk, kind), (M if kind == V else None,))
            _bits_equal(w + ' bias grad %d' % kind, db[..., :M] if kind == V else db, dbias_ref(dy, kind))
        if plan.merged:
            rc, dWm, dbm = E.bwd_w_bias(c, inp.stack, inp.dout, mk)
            assert rc == 0, (w, rc)
            assert np.array_equal(inside(dWm, w).view(np.uint32), dW.view(np.uint32)), w + ': the merged entry\'s dW differs'
            dbv = inside(E.bias_grad(c, inp.dout, mk, V)[0], w)
            assert np.array_equal(inside(dbm, w)[:, :M].view(np.uint32), np.ascontiguousarray(dbv[:, :M]).view(np.uint32)), \
                w + ': the merged entry\'s dbias differs'
        elif plan.tail == _W:
            assert E.bwd_w_bias(c, inp.stack, inp.dout, mk)[0] == EUNSUPPORTED, w + ': the merged entry served a wide reduction'
        if tag == 'own mask':                                # the plain entries on the pre-gated dy: the same bits
            gp, = _twice(w + ' bwd_x', lambda: E.bwd_x(c, pregated, None, inp.W, False), (M,))
            assert np.array_equal(gp[..., :M].view(np.uint32), gs[..., :M].view(np.uint32)), w + ': bwd_x_relu is not bwd_x on the gated dy'
            dWp, = _twice(w + ' bwd_w', lambda: E.bwd_w(c, inp.stack, pregated, None, False), (None,))
            assert np.array_equal(dWp.view(np.uint32), dW.view(np.uint32)), w + ': bwd_w_relu is not bwd_w on the gated dy'
            del gp
        del gs
    # the plain entries on the ungated dout (every gate open)
    gs, = _twice(what + ' bwd_x', lambda: E.bwd_x(c, inp.dout, None, inp.W, False), (M,))
    _bits_equal(what + ' bwd_x', gs[..., :M], gstack_ref(inp.W, inp.dout[..., :M], Fin, K))
    dW, = _twice(what + ' bwd_w', lambda: E.bwd_w(c, inp.stack, inp.dout, None, False), (None,))
    _bits_equal(what + ' bwd_w', dW, dW_ref(S, inp.dout[..., :M].astype(np.float64)))
    # the filter-mean forms: one plane of gradient per window
    for tag, mk, g in (('own mask', np.ascontiguousarray(mask), gate), ('hand mask', inp.hand, hand_gate)):
        w = '%s %s, one plane' % (what, tag)
        dy = dy_mean_ref(g, inp.gmean[..., :M])
        gs, = _twice(w + ' bwd_x_relu_mean', lambda: E.bwd_x(c, inp.gmean, mk, inp.W, True), (M,))
        _bits_equal(w + ' bwd_x_relu_mean', gs[..., :M], gstack_ref(inp.W, dy, Fin, K))
        dW, = _twice(w + ' bwd_w_relu_mean', lambda: E.bwd_w(c, inp.stack, inp.gmean, mk, True), (None,))
        _bits_equal(w + ' bwd_w_relu_mean', dW, dW_ref(S, dy))
        kind = F if c.bias == F else V
        dyg, db = _twice(w + ' relu_grad_mean', lambda: E.relu_grad_mean(c, inp.gmean, mk, kind), (M, M if kind == V else None))
        _bits_equal(w + ' relu_grad_mean dy', dyg[..., :M], dy)
        _bits_equal(w + ' relu_grad_mean dbias', db[..., :M] if kind == V else db, dbias_ref(dy, kind))
    return seen


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _elementwise(got, ref, mag):
    """max over the elements of |got - ref| / (eps32 * the sum of the magnitudes of the element's own terms)"""
    return float((np.abs(got - ref) / (EPS32 * np.maximum(mag, 1e-30))).max())


def run_roundoff(E, c):
    """The round-off leg: {name: (relative error, bound, elementwise eps)}, the bounds asserted after every figure is taken."""
    what = case_id(c)
    B, M, Fin, K, Fout = c[:5]
    FinK = Fin * K
    inp = make_inputs(c, False)
    S = rows_of(inp.stack[..., :M])
    W64, aW = inp.W.astype(np.float64), np.abs(inp.W.astype(np.float64))
    sums = sums_ref(S, inp.W, B, M)
    pre = pre_ref(sums, c.bias, inp.bias)
    mag = sums_ref(np.abs(S), aW, B, M) + np.abs(pre - sums)
    scale = np.abs(pre).max()
    m = {}

    def fwd_fig(name, got, ref, mg):
        m[name] = (float(np.abs(got - ref).max() / scale), REL, _elementwise(got, ref, mg))

    out, mask = E.fwd(c, inp.stack, inp.W, c.bias, inp.bias, 1)
    out, mask = inside(out, what)[..., :M].astype(np.float64), np.ascontiguousarray(inside(mask, what))
    fwd_fig('fwd', out, out_ref(pre, 1), mag)
    gate = unpack_mask(mask, M)
    assert np.array_equal(gate, out > 0), what + ': the mask is not out > 0 of the device\'s own output'
    if mean_supported(B, M, FinK, Fout):
        rc, mean, mmask = E.fwd_mean(c, inp.stack, inp.W, c.bias, inp.bias)
        assert rc == 0, (what, rc)
        assert np.array_equal(inside(mmask, what)[..., :(M + 3) // 4] & 15, mask[..., :(M + 3) // 4] & 15), what + ': fwd_mean\'s mask'
        fwd_fig('fwd_mean', inside(mean, what)[..., :M].astype(np.float64), mean_ref(out_ref(pre, 1)), mag.sum(axis=1) / Fout)
    hand_gate = unpack_mask(inp.hand, M)
    if gated_supported(B, M, FinK, Fout):
        rc, gout = E.fwd_gated(c, inp.stack, inp.W, inp.hand)
        assert rc == 0, (what, rc)
        got, ref = inside(gout, what)[..., :M].astype(np.float64), gated_ref(sums, hand_gate)
        m['fwd_gated'] = (float(np.abs(got - ref).max() / np.abs(sums).max()), REL, _elementwise(got, ref, mag))
    del mag

    def grads(tag, src, mk, dy, one_plane):
        ady = np.abs(dy)
        ref = gstack_ref(W64, dy, Fin, K)
        got = inside(E.bwd_x(c, src, mk, inp.W, one_plane)[0], what)[..., :M].astype(np.float64)
        assert np.isfinite(got).all(), '%s bwd_x %s: a value that is not finite' % (what, tag)
        m['bwd_x ' + tag] = (_rel(got, ref), GREL, _elementwise(got, ref, gstack_ref(aW, ady, Fin, K)))
        del got, ref
        ref = dW_ref(S, dy)
        got = inside(E.bwd_w(c, inp.stack, src, mk, one_plane)[0], what).astype(np.float64)
        assert np.isfinite(got).all(), '%s bwd_w %s: a value that is not finite' % (what, tag)
        m['bwd_w ' + tag] = (_rel(got, ref), GREL, _elementwise(got, ref, dW_ref(np.abs(S), ady)))

    dy = dy_ref(gate, inp.dout[..., :M])
    grads('relu', inp.dout, mask, dy, False)
    for kind in _bias_kinds(c):
        got = inside(E.bias_grad(c, inp.dout, mask, kind)[0], what).astype(np.float64)
        got, ref = (got[:, :M] if kind == V else got), dbias_ref(dy, kind)
        m['bias grad %s' % 'nfv'[kind]] = (_rel(got, ref), GREL, _elementwise(got, ref, dbias_ref(np.abs(dy), kind)))
    grads('plain', inp.dout, None, inp.dout[..., :M].astype(np.float64), False)
    grads('relu_mean', inp.gmean, mask, dy_mean_ref(gate, inp.gmean[..., :M]), True)
    for name, (err, bound, ew) in sorted(m.items()):
        print('%s %s: %.3e (bound %.0e, %.2f of it), elementwise %.2f eps' % (what, name, err, bound, err / bound, ew))
    return m


# ------------------------------------------------------------------------------------------------------------ the device's entries

def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Device:
    """The C entries on padded host arrays: uploads (cached per array), guarded device outputs, the dispatch assertion, and the
    outputs back on the host, guards included."""

    def __init__(self, lib):
        self.lib = lib
        self.held = {}

    def up(self, a):
        if a is None:
            return None
        if id(a) not in self.held:
            self.held[id(a)] = (a, torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
        return self.held[id(a)][1]

    @staticmethod
    def buf(shape, dtype=np.float32):
        n = int(np.prod(shape))
        td = torch.float32 if dtype == np.float32 else torch.uint8
        whole = torch.full((n + 2 * GUARD,), POISON[np.dtype(dtype)], dtype=td, device=DEV)
        whole[:GUARD] = SENT[np.dtype(dtype)]
        whole[GUARD + n:] = SENT[np.dtype(dtype)]
        return whole, whole[GUARD:GUARD + n], tuple(shape)

    @staticmethod
    def down(b):
        return Out(b[0].cpu().numpy(), b[2])

    def ran(self, c, rc, entry, want):
        _lib.check(rc, entry)
        got = _lib.last_dispatch()
        assert got == want, '%s %s: launched %r, predicted %r (%s)' % (case_id(c), entry, got, want, ASSUMES)
        torch.cuda.synchronize()

    def fwd(self, c, stack, W, bias_kind, bias, relu):
        Mp = plane_stride(c.M)
        out = self.buf((c.B, c.Fout, Mp))
        mask = self.buf((c.B, c.Fout, Mp // 4), np.uint8) if relu else None
        rc = self.lib.chebgcn_contract_fwd(_P(self.up(stack)), _P(self.up(W)), _P(self.up(bias)), bias_kind, _P(out[1]),
                                           _P(mask[1]) if relu else None, c.B, c.M, c.Fin, c.K, c.Fout, 1, 0, relu, _stream())
        self.ran(c, rc, 'contract_fwd', fwd_arm(c.B, c.M, c.Fin * c.K, c.Fout, bias_kind))
        return self.down(out), self.down(mask) if relu else None

    def fwd_mean(self, c, stack, W, bias_kind, bias):
        Mp = plane_stride(c.M)
        mean, mask = self.buf((c.B, Mp)), self.buf((c.B, c.Fout, Mp // 4), np.uint8)
        rc = self.lib.chebgcn_contract_fwd_mean(_P(self.up(stack)), _P(self.up(W)), _P(self.up(bias)), bias_kind, _P(mean[1]),
                                                _P(mask[1]), c.B, c.M, c.Fin, c.K, c.Fout, _stream())
        if rc == 0:
            self.ran(c, rc, 'contract_fwd_mean', 'contract_fwd_ring_kernel<mean>')
        return rc, self.down(mean), self.down(mask)

    def fwd_gated(self, c, stack, W, gate):
        out = self.buf((c.B, c.Fout, plane_stride(c.M)))
        rc = self.lib.chebgcn_contract_fwd_gated(_P(self.up(stack)), _P(self.up(W)), _P(self.up(gate)), _P(out[1]), c.B, c.M, c.Fin,
                                                 c.K, c.Fout, _stream())
        if rc == 0:
            self.ran(c, rc, 'contract_fwd_gated', 'contract_fwd_ring_kernel<gated>')
        return rc, self.down(out)

    def bwd_x(self, c, dy, mask, W, one_plane):
        gs = self.buf((c.K, c.B, c.Fin, plane_stride(c.M)))
        shape = (c.B, c.M, c.Fin, c.K, c.Fout, _stream())
        if mask is None:
            assert not one_plane
            rc, entry = self.lib.chebgcn_contract_bwd_x(_P(self.up(dy)), _P(self.up(W)), _P(gs[1]), *shape), 'contract_bwd_x'
        else:
            entry = 'contract_bwd_x_relu_mean' if one_plane else 'contract_bwd_x_relu'
            rc = getattr(self.lib, 'chebgcn_' + entry)(_P(self.up(dy)), _P(self.up(mask)), _P(self.up(W)), _P(gs[1]), *shape)
        self.ran(c, rc, entry, bwd_x_arm(c.B, c.M, c.Fin * c.K, c.Fout, mask is not None))
        return (self.down(gs),)

    def workspace(self, c):
        """exactly chebgcn_contract_bwd_w_workspace() bytes between sentinels"""
        n = self.lib.chebgcn_contract_bwd_w_workspace(c.B, c.M, c.Fin, c.K, c.Fout)
        p = bwd_w_plan(c.B, c.M, c.Fin * c.K, c.Fout)
        assert n == p.gx * p.gy * p.gz * p.rt * 16 * 64 * 4, (case_id(c), n, p, ASSUMES)
        return self.buf((n,), np.uint8), n

    def ws_intact(self, c, ws):
        s = SENT[np.dtype(np.uint8)]
        assert bool((ws[0][:GUARD] == s).all()) and bool((ws[0][-GUARD:] == s).all()), case_id(c) + ': a store left the workspace'

    def bwd_w(self, c, stack, dy, mask, one_plane):
        dW = self.buf((c.Fin * c.K, c.Fout))
        ws, n = self.workspace(c)
        shape = (c.B, c.M, c.Fin, c.K, c.Fout, _stream())
        if mask is None:
            assert not one_plane
            rc, entry = self.lib.chebgcn_contract_bwd_w(_P(self.up(stack)), _P(self.up(dy)), _P(dW[1]), _P(ws[1]), n, *shape), 'contract_bwd_w'
        else:
            entry = 'contract_bwd_w_relu_mean' if one_plane else 'contract_bwd_w_relu'
            rc = getattr(self.lib, 'chebgcn_' + entry)(_P(self.up(stack)), _P(self.up(dy)), _P(self.up(mask)), _P(dW[1]), _P(ws[1]), n,
                                                       *shape)
        self.ran(c, rc, entry, bwd_w_arm(c.B, c.M, c.Fin * c.K, c.Fout, mask is not None))
        self.ws_intact(c, ws)
        return (self.down(dW),)

    def bwd_w_bias(self, c, stack, dout, mask):
        dW, db = self.buf((c.Fin * c.K, c.Fout)), self.buf((c.Fout, plane_stride(c.M)))
        ws, n = self.workspace(c)
        before = _lib.last_dispatch()
        rc = self.lib.chebgcn_contract_bwd_w_relu_bias(_P(self.up(stack)), _P(self.up(dout)), _P(self.up(mask)), _P(dW[1]), _P(db[1]),
                                                       _P(ws[1]), n, c.B, c.M, c.Fin, c.K, c.Fout, _stream())
        if rc == 0:
            self.ran(c, rc, 'contract_bwd_w_relu_bias', bwd_w_arm(c.B, c.M, c.Fin * c.K, c.Fout, True, merged=True))
            self.ws_intact(c, ws)
        else:
            assert _lib.last_dispatch() == before, case_id(c) + ': a refused call enqueued ' + _lib.last_dispatch()
        return rc, self.down(dW), self.down(db)

    def _bias_ws(self, c, kind):
        n = self.lib.chebgcn_brelu_pool_bwd_workspace(c.B, c.M, c.Fout, 1, kind)
        return (torch.empty(n, dtype=torch.uint8, device=DEV), n) if n else (None, 0)

    def bias_grad(self, c, dout, mask, kind):
        db = self.buf((c.Fout, plane_stride(c.M)) if kind == V else (c.Fout,))
        ws, n = self._bias_ws(c, kind)
        rc = self.lib.chebgcn_brelu_pool_bwd(_P(self.up(dout)), None, _P(self.up(mask)), None, _P(db[1]), kind, c.B, c.M, c.Fout, 1, 0, 1,
                                             _P(ws), n, _stream())
        self.ran(c, rc, 'brelu_pool_bwd', bias_grad_arm(c.M, c.Fout, kind))
        return (self.down(db),)

    def relu_grad_mean(self, c, gmean, mask, kind):
        Mp = plane_stride(c.M)
        dy, db = self.buf((c.B, c.Fout, Mp)), self.buf((c.Fout, Mp) if kind == V else (c.Fout,))
        ws, n = self._bias_ws(c, kind)
        rc = self.lib.chebgcn_relu_grad_mean(_P(self.up(gmean)), _P(self.up(mask)), _P(dy[1]), _P(db[1]), kind, c.B, c.M, c.Fout, _P(ws),
                                             n, _stream())
        self.ran(c, rc, 'relu_grad_mean', bias_grad_arm(c.M, c.Fout, kind, mean=True))
        return self.down(dy), self.down(db)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, ASSUMES
    return _lib.lib()


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_exact_leg(lib, c):
    """Integer-grained operands: every output of every entry bit for bit, twice (``run_exact``)."""
    seen = run_exact(Device(lib), c)
    record_measured('contract_grad_arms_exact[%s]' % case_id(c), **seen)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_roundoff_leg(lib, c):
    """Standard-normal operands: 1e-5 of max forward, 2e-5 of max for the gradients (``run_roundoff``)."""
    m = run_roundoff(Device(lib), c)
    record_measured('contract_grad_arms_roundoff[%s]' % case_id(c),
                    **{k.replace(' ', '_'): v[0] for k, v in m.items()},
                    **{k.replace(' ', '_') + '_elementwise_eps': v[2] for k, v in m.items()},
                    worst_ratio=max(v[0] / v[1] for v in m.values()))
    for name, (err, bound, _) in sorted(m.items()):
        assert err <= bound, '%s %s: %.3e above %.0e' % (case_id(c), name, err, bound)


def test_tables_reach_every_arm():
    """The case table reaches every arm named in the module docstring, by the dispatch restatement (which every launch checks
    against chebgcn_last_dispatch())."""
    reach = table_reach()
    record_measured('contract_grad_arms_tables', cases=len(CASES), **reach)
