"""The spectral filter kernels (csrc/spectral.hip) called directly -- chebgcn_spectral_transform, chebgcn_spectral_mix_fwd,
chebgcn_spectral_mix_bwd_x, chebgcn_spectral_mix_bwd_w, chebgcn_spectral_spline_expand, chebgcn_spectral_spline_expand_bwd --
against float64 NumPy restatements at the edges of their tiles, loops and masks.  Needs an MI355X: ``-m gpu``.
tests/test_spectral_kernel_refs.py checks the restatements, the exactness inequality, the launch geometry restated here and
that the exact leg's inputs tell the restatements from their near misses, without a GPU.

``transform_geometry`` / ``mix_geometry`` / ``bwd_w_geometry`` restate the launch arithmetic of the entry points; every launch
asserts that ``_lib.last_dispatch()`` names the kernel expected, and ``table_reach`` asserts that the tables reach

    spectral_transform_kernel<false>, spectral_transform_kernel<true>, spectral_mix_kernel<false>, spectral_mix_kernel<true>,
    spectral_mix_bwd_w_kernel, spectral_spline_expand_kernel, spectral_spline_expand_bwd_kernel

and, read off the kernels, every arm listed there.

Every case runs two legs, each launch twice into freshly poisoned outputs (the two runs are bit-identical).

Exact leg: every operand (the basis and the spline basis too: a kernel test needs no orthonormal basis) is a non-zero integer in
[-4, 4].  Every product and every partial sum is then an integer of magnitude <= 16 n (n: the length of the reduction): exact
in fp32 in ANY summation order, the matrix instruction's included, while 16 n + 1 < 2^24 (``exact_leg_is_exact``, asserted per
case).  So the result equals the float64 restatement -- no tolerance (the sign of a zero aside: both sides are compared after
``+ 0.0``).  No operand is 0, so one term less or one term more in any reduction changes that element.

Round-off leg: standard-normal operands, one side scaled by 1/sqrt(n) (the spline basis: models_gcn.bspline_basis, a partition
of unity, unscaled); componentwise
    |got - ref| <= (n + 2) 2^-24 (|a| . |b|) + 2^-24 |ref|
(the any-order summation bound; |a| . |b| is the same contraction on absolute values; n = M for the transform and for
spline_expand_bwd, Ni for the mixes, B for bwd_w, K for spline_expand).  No denormal operand (``_normal``).  The largest measured
|err| / bound of every case goes to ``record_measured`` (largest over the tables on an MI355X: 0.23 for the transform, whose
matrix instruction keeps the bound of an fmaf chain, 0.32 for the mixes, 0.36 for bwd_w, 0.27 and 0.03 for the spline pair).

Poison: the pad [M, Mp) of every input plane is NaN, +Inf in the middle plane; the basis is [Mp][Mp] with a zero pad
(ops.spectral_basis' layout); every output lies between guard rows of a sentinel, which must be intact afterwards; the pad of
every plane the transform and the two mixes write is exactly 0.
"""
import collections
import os
import re
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT, record_measured
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import plane_stride
from test_gpu_head_kernels import DEV, SENTINEL, Guarded, _dev, _P, _stream, assert_exact, assert_same_bits, roundoff_ratio
from test_gpu_head_kernels import U as UNIT                 # unit round-off of fp32

pytestmark = pytest.mark.gpu
TINY = np.finfo(np.float32).tiny


# ------------------------------------------------------------------------------------------------------------ restatements

def transform_ref(x, U, transpose):
    """out[r][j] = sum_m x[r][m] U[m][j] (analysis) or sum_m x[r][m] U[j][m] (synthesis); x [R, M], U [M, M]."""
    return np.einsum('rm,jm->rj' if transpose else 'rm,mj->rj', np.asarray(x, np.float64), np.asarray(U, np.float64))


def mix_fwd_ref(W, xh):
    """yh[b][o][m] = sum_f W[m][o][f] xh[b][f][m]; W [M, Fout, Fin], xh [B, Fin, M]."""
    return np.einsum('mof,bfm->bom', np.asarray(W, np.float64), np.asarray(xh, np.float64))


def mix_bwd_x_ref(W, dyh):
    """dxh[b][f][m] = sum_o W[m][o][f] dyh[b][o][m]; dyh [B, Fout, M]."""
    return np.einsum('mof,bom->bfm', np.asarray(W, np.float64), np.asarray(dyh, np.float64))


def mix_bwd_w_ref(dyh, xh):
    """dW[m][o][f] = sum_b dyh[b][o][m] xh[b][f][m]."""
    return np.einsum('bom,bfm->mof', np.asarray(dyh, np.float64), np.asarray(xh, np.float64))


def spline_ref(Bs, Wk):
    """W = Bs Wk; Bs [M, K], Wk [K, C]."""
    return np.asarray(Bs, np.float64) @ np.asarray(Wk, np.float64)


def spline_bwd_ref(Bs, dW):
    """dWk = Bs^T dW; dW [M, C]."""
    return np.asarray(Bs, np.float64).T @ np.asarray(dW, np.float64)


def exact_leg_is_exact(n):
    """Sums of n products of integers in [-4, 4] are exact in fp32 in any order."""
    return 16 * n + 1 < 2 ** 24


# ------------------------------------------------------------------------------------------------------------ launch geometry

TR_ROWS, TR_COLS, TR_WAVES = 32, 64, 4                       # spectral_transform_kernel: four tiles per workgroup
MIX_NB, MIX_OT, MIX_WAVES = 4, 8, 4                          # spectral_mix_kernel: 4 waves x MIX_NB windows per workgroup
WG_OT, WG_IT, WG_WAVES = 8, 4, 4                             # spectral_mix_bwd_w_kernel


def _ceil(a, b):
    return (a + b - 1) // b


def transform_geometry(R, M):
    """chebgcn_spectral_transform's launch: ``two_last`` -- the last column tile has its second 32-column block; ``idle`` --
    waves of the last workgroup that return early; ``clamped`` -- rows past R that the last row tile loads and must not store."""
    Mp = plane_stride(M)
    ntc = _ceil(Mp, TR_COLS)
    row_tiles = _ceil(R, TR_ROWS)
    tiles = row_tiles * ntc
    groups = _ceil(tiles, TR_WAVES)
    return dict(Mp=Mp, ntc=ntc, tiles=tiles, groups=groups, idle=groups * TR_WAVES - tiles,
                two_last=(ntc - 1) * TR_COLS + 32 < Mp, clamped=row_tiles * TR_ROWS - R, turns=Mp // 32)


def mix_geometry(B, M, No):
    """The grid of spectral_mix_kernel: (frequency blocks of 64, blocks of 16 windows, blocks of MIX_OT outputs)."""
    return (_ceil(plane_stride(M), 64), _ceil(B, MIX_WAVES * MIX_NB), _ceil(No, MIX_OT))


def bwd_w_geometry(B, M, Fin, Fout):
    """The grid of spectral_mix_bwd_w_kernel and the window range [bb, be) of each of its four waves."""
    nb = (B + 3) // 4
    ranges = [(min(w * nb, B), min(min(w * nb, B) + nb, B)) for w in range(WG_WAVES)]
    return dict(grid=(_ceil(M, 64), _ceil(Fout, WG_OT), _ceil(Fin, WG_IT)), nb=nb, ranges=ranges)


def require_status():
    """(name, value) of the status a failed CG_REQUIRE returns: the macro of csrc/status.h (which common.h includes), the value
    from include/chebgcn.h."""
    csrc = os.path.join(ROOT, 'gcn_fmri_decoding_amd', 'csrc')
    assert re.search(r'#include\s+"status\.h"', open(os.path.join(csrc, 'common.h')).read())
    macro = re.search(r'#define\s+CG_REQUIRE\(cond, \.\.\.\)(.*?)while \(0\)', open(os.path.join(csrc, 'status.h')).read(), re.S)
    name = re.search(r'return\s+chebgcn::fail\((\w+),', macro.group(1)).group(1)
    value = re.search(r'\b%s\s*=\s*(-?\d+)' % name, open(os.path.join(ROOT, 'include', 'chebgcn.h')).read())
    return name, int(value.group(1))


# ------------------------------------------------------------------------------------------------------------ case tables

Tr = collections.namedtuple('Tr', 'R M')                      # transform, both directions
Mix = collections.namedtuple('Mix', 'B Fin Fout M')           # mix forward and bwd_x
Bww = collections.namedtuple('Bww', 'B Fin Fout M')           # mix bwd_w
Spl = collections.namedtuple('Spl', 'M K C')                  # spline expand and its gradient

TR_CASES = [
    Tr(1, 1),          # Mp = 32: ntc = 1, no second block; one tile, three waves return
    Tr(31, 3),
    Tr(32, 31),
    Tr(129, 32),       # five tiles: a second workgroup with one live wave
    Tr(64, 33),        # Mp = 64: both blocks, ntc = 1
    Tr(65, 61),
    Tr(33, 64),
    Tr(33, 65),        # Mp = 96: ntc = 2, the last column tile has no second block; four tiles
    Tr(1, 95),
    Tr(65, 97),        # Mp = 128
    Tr(31, 100),
    Tr(32, 126),       # M % 8 = 6
    Tr(129, 130),      # Mp = 160: ntc = 3, fifteen tiles
]
MIX_CASES = [
    Mix(1, 1, 1, 1),
    Mix(4, 3, 10, 63),
    Mix(5, 8, 9, 64),
    Mix(16, 9, 8, 65),
    Mix(17, 17, 33, 100),
    Mix(5, 32, 32, 65),                                       # the network's own 32-to-32 layer
    Mix(17, 32, 32, 1),
    Mix(1, 3, 10, 100),
]
BWW_CASES = [
    Bww(1, 1, 1, 1),
    Bww(2, 3, 7, 63),
    Bww(3, 4, 8, 64),
    Bww(4, 5, 9, 65),
    Bww(5, 9, 17, 130),
    Bww(8, 3, 9, 65),
    Bww(9, 5, 7, 130),
    Bww(33, 9, 8, 63),
]
SPL_CASES = [
    Spl(1, 1, 1),
    Spl(2, 4, 255),
    Spl(100, 7, 256),
    Spl(2, 20, 257),
    Spl(100, 7, 480),
    Spl(1, 4, 1024),
    Spl(100, 20, 1),
    Spl(100, 1, 257),
]
ALL_CASES = TR_CASES + MIX_CASES + BWW_CASES + SPL_CASES


def case_id(c):
    if isinstance(c, Tr):
        return 'R%d-M%d' % c
    if isinstance(c, Spl):
        return 'M%d-K%d-C%d' % c
    return 'B%d-%dto%d-M%d' % c


def _seed(c, exact, salt=0):
    return (zlib.crc32((type(c).__name__ + case_id(c)).encode()) + 2 * salt + (0 if exact else 1)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------ inputs (host)

NONZERO = np.array([-4, -3, -2, -1, 1, 2, 3, 4], np.float32)


def _ints(rs, *shape):
    return rs.choice(NONZERO, shape)


def _normal(a):
    """fp32, and no denormal in it."""
    a = np.asarray(a, np.float32)
    assert not ((a != 0) & (np.abs(a) < TINY)).any(), 'a denormal operand'
    return a


def _unsymmetric(A):
    """A [..., n, n] of the exact leg with every matrix unsymmetric (n > 1): where A[0][1] == A[1][0], A[0][1] moves to the next
    non-zero integer of [-4, 4]."""
    if A.shape[-1] > 1:
        same = A[..., 0, 1] == A[..., 1, 0]
        nxt = np.where(A[..., 0, 1] == 4, -4, np.where(A[..., 0, 1] == -1, 1, A[..., 0, 1] + 1))
        A[..., 0, 1] = np.where(same, nxt, A[..., 0, 1])
    return A


def transform_data(c, exact):
    """(x [R, M], U [M, M]) in fp32; the exact leg's U is not symmetric (M > 1)."""
    rs = np.random.RandomState(_seed(c, exact))
    if exact:
        return _ints(rs, c.R, c.M), _unsymmetric(_ints(rs, c.M, c.M))
    return _normal(rs.randn(c.R, c.M)), _normal(rs.randn(c.M, c.M) / np.sqrt(c.M))


def mix_data(c, exact, transpose):
    """(W [M, Fout, Fin], planes [B, Ni, M]) in fp32, Ni = Fout for bwd_x (``transpose``) and Fin for the forward; the exact
    leg's W[m] is not symmetric where Fin == Fout > 1."""
    rs = np.random.RandomState(_seed(c, exact, 1 + transpose))
    Ni = c.Fout if transpose else c.Fin
    if exact:
        W = _ints(rs, c.M, c.Fout, c.Fin)
        return (_unsymmetric(W) if c.Fin == c.Fout else W), _ints(rs, c.B, Ni, c.M)
    return _normal(rs.randn(c.M, c.Fout, c.Fin) / np.sqrt(Ni)), _normal(rs.randn(c.B, Ni, c.M))


def bwd_w_data(c, exact):
    """(dyh [B, Fout, M], xh [B, Fin, M]) in fp32."""
    rs = np.random.RandomState(_seed(c, exact))
    if exact:
        return _ints(rs, c.B, c.Fout, c.M), _ints(rs, c.B, c.Fin, c.M)
    return _normal(rs.randn(c.B, c.Fout, c.M)), _normal(rs.randn(c.B, c.Fin, c.M) / np.sqrt(c.B))


def spline_data(c, exact, bwd):
    """(Bs [M, K], Wk [K, C]) or, ``bwd``, (Bs, dW [M, C]) in fp32.  Round-off leg: Bs = models_gcn.bspline_basis at M sorted
    uniform points, cubic where K allows (degree K - 1 below four control points)."""
    rs = np.random.RandomState(_seed(c, exact, 1 + bwd))
    rows = c.M if bwd else c.K
    if exact:
        return _ints(rs, c.M, c.K), _ints(rs, rows, c.C)
    from gcn_fmri_decoding_amd import models_gcn
    lamb = np.sort(rs.rand(c.M)).astype(np.float32)
    Bs = np.asarray(models_gcn.bspline_basis(c.K, lamb, degree=min(3, c.K - 1)), np.float64)
    assert Bs.shape == (c.M, c.K)
    return _normal(Bs), _normal(rs.randn(rows, c.C) / (np.sqrt(c.M) if bwd else 1.0))


def pad_planes(a):
    """[..., M] -> [..., Mp] fp32: NaN over the pad [M, Mp), +Inf there in the middle plane."""
    M = a.shape[-1]
    out = np.full(a.shape[:-1] + (plane_stride(M),), np.nan, np.float32)
    out[..., :M] = a
    flat = out.reshape(-1, out.shape[-1])
    flat[flat.shape[0] // 2, M:] = np.inf
    return out


def pad_basis(U):
    """[M, M] -> [Mp, Mp] with a zero pad (ops.spectral_basis' layout, on the host)."""
    M = U.shape[0]
    out = np.zeros((plane_stride(M),) * 2, np.float32)
    out[:M, :M] = U
    return out


# One launch: the entry point, the kernel it must name, the two inputs as the device sees them, the integer arguments, the output
# [rows, cols] of which the columns [0, data) hold data (the rest is a plane's pad), the float64 reference [rows, data], the same
# contraction on absolute values, and the length of the reduction.
Job = collections.namedtuple('Job', 'entry expect ins args rows cols data ref absdot n')


def transform_job(c, exact, transpose):
    x, U = transform_data(c, exact)
    Mp = plane_stride(c.M)
    return Job('chebgcn_spectral_transform', 'spectral_transform_kernel<%s>' % ('true' if transpose else 'false'),
               [pad_planes(x), pad_basis(U)], (c.R, c.M, int(transpose)), c.R, Mp, c.M, transform_ref(x, U, transpose),
               transform_ref(np.abs(x), np.abs(U), transpose), c.M)


def mix_job(c, exact, transpose):
    W, p = mix_data(c, exact, transpose)
    ref = mix_bwd_x_ref if transpose else mix_fwd_ref
    No = c.Fin if transpose else c.Fout
    return Job('chebgcn_spectral_mix_bwd_x' if transpose else 'chebgcn_spectral_mix_fwd',
               'spectral_mix_kernel<%s>' % ('true' if transpose else 'false'), [pad_planes(p), W], (c.B, c.M, c.Fin, c.Fout),
               c.B * No, plane_stride(c.M), c.M, ref(W, p).reshape(c.B * No, c.M),
               ref(np.abs(W), np.abs(p)).reshape(c.B * No, c.M), c.Fout if transpose else c.Fin)


def bwd_w_job(c, exact):
    dyh, xh = bwd_w_data(c, exact)
    FF = c.Fout * c.Fin
    return Job('chebgcn_spectral_mix_bwd_w', 'spectral_mix_bwd_w_kernel', [pad_planes(dyh), pad_planes(xh)],
               (c.B, c.M, c.Fin, c.Fout), c.M, FF, FF, mix_bwd_w_ref(dyh, xh).reshape(c.M, FF),
               mix_bwd_w_ref(np.abs(dyh), np.abs(xh)).reshape(c.M, FF), c.B)


def spline_job(c, exact, bwd):
    Bs, V = spline_data(c, exact, bwd)
    ref = spline_bwd_ref if bwd else spline_ref
    return Job('chebgcn_spectral_spline_expand_bwd' if bwd else 'chebgcn_spectral_spline_expand',
               'spectral_spline_expand_bwd_kernel' if bwd else 'spectral_spline_expand_kernel', [Bs, V], (c.M, c.K, c.C),
               c.K if bwd else c.M, c.C, c.C, ref(Bs, V), ref(np.abs(Bs), np.abs(V)), c.M if bwd else c.K)


# ------------------------------------------------------------------------------------------------------------ table coverage

ARMS = ('spectral_transform_kernel<false>', 'spectral_transform_kernel<true>', 'spectral_mix_kernel<false>',
        'spectral_mix_kernel<true>', 'spectral_mix_bwd_w_kernel', 'spectral_spline_expand_kernel',
        'spectral_spline_expand_bwd_kernel')


def table_reach():
    """arm -> ids of its cases, after asserting that the tables hold the shapes asked for and reach, by the launch geometry
    restated above, every arm of csrc/spectral.hip that one shape per kernel left unreached.  Host arithmetic only."""
    reach = collections.defaultdict(list)
    assert len({(type(c).__name__, case_id(c)) for c in ALL_CASES}) == len(ALL_CASES)
    # transform
    for c in TR_CASES:
        reach['spectral_transform_kernel<false>'].append(case_id(c))
        reach['spectral_transform_kernel<true>'].append(case_id(c))
    by_Mp = collections.defaultdict(set)
    for c in TR_CASES:
        by_Mp[plane_stride(c.M)].add(c.M)
    assert by_Mp[32] >= {1, 3, 31, 32} and by_Mp[64] >= {33, 61, 64} and by_Mp[96] >= {65, 95}
    assert by_Mp[128] >= {97, 100} and by_Mp[160] >= {130}
    assert {c.M % 8 for c in TR_CASES} == set(range(8)), 'the kb + s < M mask: every M % 8, both lane halves'
    assert {c.R for c in TR_CASES} >= {1, 31, 32, 33, 64, 65, 129}
    g = [transform_geometry(c.R, c.M) for c in TR_CASES]
    assert any(t['ntc'] == 1 and not t['two_last'] for t in g), 'Mp = 32: the second block absent'
    assert any(t['ntc'] == 1 and t['two_last'] for t in g), 'Mp = 64'
    assert any(t['ntc'] == 2 and not t['two_last'] for t in g) and any(t['ntc'] == 2 and t['two_last'] for t in g)
    assert any(t['ntc'] == 3 for t in g) and any(t['turns'] > 4 for t in g)
    assert any(t['tiles'] == 1 and t['idle'] == 3 for t in g), 'one tile: three waves return early'
    assert any(t['tiles'] % 4 == 0 for t in g) and any(t['tiles'] > 1 and t['tiles'] % 4 == 1 for t in g)
    assert any(c.R < 32 for c in TR_CASES) and any(c.R == 32 for c in TR_CASES) and any(c.R > 32 and c.R % 32 == 0 for c in TR_CASES)
    assert any(t['clamped'] == 31 for t in g) and any(t['clamped'] == 1 for t in g) and any(t['clamped'] == 0 for t in g)
    assert any(t['clamped'] and t['groups'] > 1 for t in g), 'clamped rows in a tile past the first workgroup'
    # mix forward and bwd_x
    for c in MIX_CASES:
        reach['spectral_mix_kernel<false>'].append(case_id(c))
        reach['spectral_mix_kernel<true>'].append(case_id(c))
    assert {c.B for c in MIX_CASES} >= {1, 4, 5, 16, 17} and {c.M for c in MIX_CASES} >= {1, 63, 64, 65, 100}
    assert {(c.Fin, c.Fout) for c in MIX_CASES} >= {(1, 1), (3, 10), (8, 9), (9, 8), (17, 33), (32, 32)}
    for tr in (False, True):
        gm = [(c, mix_geometry(c.B, c.M, c.Fin if tr else c.Fout)) for c in MIX_CASES]
        assert any(z > 1 for _, (_, _, z) in gm) and any(z > 2 for _, (_, _, z) in gm), 'blockIdx.z > 0 (TR = %s)' % tr
        assert any(z == 1 for _, (_, _, z) in gm) and any(y > 1 for _, (_, y, _) in gm) and any(x > 1 for _, (x, _, _) in gm)
        assert any(z > 1 and (c.Fin if tr else c.Fout) % MIX_OT for c, (_, _, z) in gm), 'a partial last output tile'
        assert any(z > 1 and c.Fin == c.Fout == 32 for c, (_, _, z) in gm), 'the 32-to-32 layer'
    assert any(c.Fin > 8 for c in MIX_CASES) and any(c.Fin > 16 for c in MIX_CASES), 'bwd_x: ii * Fin + o past one output tile'
    assert any(c.B % MIX_NB for c in MIX_CASES) and any(c.B == MIX_WAVES * MIX_NB for c in MIX_CASES)
    assert any(c.B < MIX_NB for c in MIX_CASES), 'three waves return at b0 >= B'
    assert any(c.M < 64 for c in MIX_CASES) and any(c.M > 64 and c.M % 64 for c in MIX_CASES)
    # bwd_w
    for c in BWW_CASES:
        reach['spectral_mix_bwd_w_kernel'].append(case_id(c))
    assert {c.B for c in BWW_CASES} >= {1, 2, 3, 4, 5, 8, 9, 33} and {c.Fin for c in BWW_CASES} >= {1, 3, 4, 5, 9}
    assert {c.Fout for c in BWW_CASES} >= {1, 7, 8, 9, 17} and {c.M for c in BWW_CASES} >= {1, 63, 64, 65, 130}
    gw = [(c, bwd_w_geometry(c.B, c.M, c.Fin, c.Fout)) for c in BWW_CASES]
    assert any(t['grid'][2] > 1 for _, t in gw) and any(t['grid'][2] > 2 for _, t in gw), 'Fin > WG_IT: blockIdx.z > 0'
    assert any(t['grid'][1] > 1 for _, t in gw) and any(t['grid'][0] > 2 for _, t in gw)
    for B in (1, 2, 3):
        t = bwd_w_geometry(B, 1, 1, 1)
        assert t['nb'] == 1 and sum(b == e for b, e in t['ranges']) == 4 - B and t['ranges'][3] == (B, B)
    assert any(t['ranges'][3][0] == c.B and c.B > 4 for c, t in gw), 'bb = min(wave * nb, B) clamps'
    assert any(c.B % 4 == 0 and c.B > 4 for c in BWW_CASES) and any(t['nb'] > 2 for _, t in gw)
    for c, t in gw:
        assert [w for b, e in t['ranges'] for w in range(b, e)] == list(range(c.B)), 'every window once, in order'
    assert any(c.M > 64 and c.M % 64 and (c.Fin > WG_IT or c.Fout > WG_OT) for c in BWW_CASES), 'e -> (ml, t, u) at a partial tile'
    assert any(c.M < 64 for c in BWW_CASES) and any(c.M % 64 == 0 for c in BWW_CASES)
    # spline
    for c in SPL_CASES:
        reach['spectral_spline_expand_kernel'].append(case_id(c))
        reach['spectral_spline_expand_bwd_kernel'].append(case_id(c))
    assert {c.M for c in SPL_CASES} >= {1, 2, 100} and {c.K for c in SPL_CASES} >= {1, 4, 7, 20}
    assert {c.C for c in SPL_CASES} >= {1, 255, 256, 257, 480, 1024}
    assert any(c.C < 256 for c in SPL_CASES) and any(c.C > 256 and c.C % 256 == 0 for c in SPL_CASES)
    assert any(c.K == 1 and c.M > 1 for c in SPL_CASES) and any(c.M == 1 and c.K > 1 for c in SPL_CASES)
    assert set(reach) == set(ARMS), sorted(reach)
    return dict(reach)


# ------------------------------------------------------------------------------------------------------------ device plumbing

@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.lib()


def _run(lib, job, ins, what):
    """One launch into a fresh guarded output (NaN all over): the [rows, cols] result on the device."""
    out = Guarded(job.rows, job.cols)
    _lib.check(getattr(lib, job.entry)(_P(ins[0]), _P(ins[1]), _P(out.t), *job.args, _stream()), job.entry)
    assert _lib.last_dispatch() == job.expect, (what, _lib.last_dispatch())
    torch.cuda.synchronize()
    out.check(what)
    return out.t


def _legs(lib, name, c, make):
    """Both legs of one case of one kernel; returns the round-off leg's |err| / bound."""
    ratio = None
    for exact in (True, False):
        job = make(c, exact)
        assert exact_leg_is_exact(job.n)
        what = '%s %s %s' % (name, case_id(c), 'exact' if exact else 'round-off')
        ins = [_dev(a) for a in job.ins]
        got = _run(lib, job, ins, what)
        assert_same_bits(what, got, _run(lib, job, ins, what))
        if job.data < job.cols:
            assert bool((got[:, job.data:] == 0).all()), what + ': the pad of an output plane is not 0'
        if exact:
            assert_exact(what, got[:, :job.data], job.ref)
        else:
            ratio = roundoff_ratio(what, got[:, :job.data], job.ref, (job.n + 2) * UNIT * job.absdot)
    record_measured('%s_vs_float64[%s]' % (name, case_id(c)), arm=job.expect, n=job.n, ratio=ratio)
    return ratio


# ------------------------------------------------------------------------------------------------------------ the kernels

@pytest.mark.parametrize('transpose', [False, True], ids=['analysis', 'synthesis'])
@pytest.mark.parametrize('c', TR_CASES, ids=case_id)
def test_transform_vs_float64(lib, c, transpose):
    _legs(lib, 'spectral_synthesis' if transpose else 'spectral_analysis', c, lambda c, e: transform_job(c, e, transpose))


@pytest.mark.parametrize('transpose', [False, True], ids=['fwd', 'bwd_x'])
@pytest.mark.parametrize('c', MIX_CASES, ids=case_id)
def test_mix_vs_float64(lib, c, transpose):
    _legs(lib, 'spectral_mix_bwd_x' if transpose else 'spectral_mix_fwd', c, lambda c, e: mix_job(c, e, transpose))


@pytest.mark.parametrize('c', BWW_CASES, ids=case_id)
def test_mix_bwd_w_vs_float64(lib, c):
    _legs(lib, 'spectral_mix_bwd_w', c, bwd_w_job)


@pytest.mark.parametrize('bwd', [False, True], ids=['expand', 'expand_bwd'])
@pytest.mark.parametrize('c', SPL_CASES, ids=case_id)
def test_spline_vs_float64(lib, c, bwd):
    _legs(lib, 'spectral_spline_expand_bwd' if bwd else 'spectral_spline_expand', c, lambda c, e: spline_job(c, e, bwd))


# ------------------------------------------------------------------------------------------------------------ refusals

BIG_M, BIG_GRID = 32768 + 1, 65535 + 1
# entry point -> (its valid integer arguments, [(what, argument index, value)] that it must refuse)
REFUSED_SHAPES = {
    'chebgcn_spectral_transform': ((2, 3, 0), [('R = 0', 0, 0), ('R < 0', 0, -1), ('M > 32768', 1, BIG_M)]),
    'chebgcn_spectral_mix_fwd': ((2, 3, 2, 2), [('M > 32768', 1, BIG_M)]),
    'chebgcn_spectral_mix_bwd_x': ((2, 3, 2, 2), [('M > 32768', 1, BIG_M)]),
    'chebgcn_spectral_mix_bwd_w': ((2, 3, 2, 2), [('M > 32768', 1, BIG_M)]),
    'chebgcn_spectral_spline_expand': ((3, 2, 4), [('M > 65535', 0, BIG_GRID)]),
    'chebgcn_spectral_spline_expand_bwd': ((3, 2, 4), [('K > 65535', 1, BIG_GRID)]),
}
IN_PLACE_REFUSED = ('chebgcn_spectral_transform', 'chebgcn_spectral_mix_fwd', 'chebgcn_spectral_mix_bwd_x')


def refused_calls():
    """(entry, what, which of the three pointers are NULL, in == out, integer arguments) of every call that must be refused."""
    calls = []
    for entry, (args, bad) in REFUSED_SHAPES.items():
        for k in range(3):
            calls.append((entry, 'NULL argument %d' % k, k, False, args))
        if entry in IN_PLACE_REFUSED:
            calls.append((entry, 'in == out', None, True, args))
        for what, idx, value in bad:
            calls.append((entry, what, None, False, args[:idx] + (value,) + args[idx + 1:]))
    return calls


@pytest.mark.parametrize('entry,what,null,in_place,args', refused_calls(),
                         ids=['%s-%s' % (r[0].replace('chebgcn_spectral_', ''), r[1].replace(' ', '_')) for r in refused_calls()])
def test_bad_arguments_are_refused(lib, entry, what, null, in_place, args):
    """The status of a failed CG_REQUIRE, nothing enqueued, and a sentinel-filled output untouched after a synchronize."""
    name, status = require_status()
    a, b = (torch.ones(4096, device=DEV) for _ in range(2))
    out = Guarded(64, 64, poison=SENTINEL)
    ptrs = [_P(out.t) if in_place else _P(a), _P(b), _P(out.t)]
    if null is not None:
        ptrs[null] = None
    torch.cuda.synchronize()
    before = _lib.last_dispatch()
    rc = getattr(lib, entry)(*ptrs, *args, _stream())
    assert rc == status, '%s %s: status %d, not %s = %d' % (entry, what, rc, name, status)
    assert _lib.last_dispatch() == before, 'a refused call enqueued %s' % _lib.last_dispatch()
    torch.cuda.synchronize()
    assert out.untouched(), '%s %s: a refused call wrote its output' % (entry, what)


# ------------------------------------------------------------------------------------------------------------ wrappers

def _planes_dev(a):
    return torch.from_numpy(pad_planes(a)).to(DEV)


def _conv_operands(filt):
    """x, gy (planes with poisoned pads), W, basis, Bs on the device at M = 33, B = 5, Fin = 3, Fout = 9."""
    from gcn_fmri_decoding_amd import models_gcn, ops
    M, B, Fin, Fout, K = 33, 5, 3, 9, 7
    rs = np.random.RandomState(33 + (filt == 'spline'))
    basis = ops.spectral_basis(_normal(rs.randn(M, M) / np.sqrt(M)), DEV)
    x, gy = _planes_dev(_normal(rs.randn(B, Fin, M))), _planes_dev(_normal(rs.randn(B, Fout, M)))
    if filt == 'spline':
        Bs = torch.from_numpy(_normal(models_gcn.bspline_basis(K, np.sort(rs.rand(M)).astype(np.float32)))).to(DEV)
        W = torch.from_numpy(_normal(rs.randn(K, Fout * Fin))).to(DEV)
    else:
        Bs, W = None, torch.from_numpy(_normal(rs.randn(M, Fout, Fin) / np.sqrt(Fin))).to(DEV)
    return M, Fin, Fout, x, gy, W, basis, Bs


@pytest.mark.parametrize('filt', ['fourier', 'spline'])
def test_spectral_conv_is_the_chained_kernels(lib, filt):
    """ops.SpectralConv for each requires_grad combination of (x, W): the output and each gradient carry the bits of the
    individual wrappers chained by hand; an operand that needs no gradient gets None, and its kernel is not launched."""
    from gcn_fmri_decoding_amd import ops
    M, Fin, Fout, x, gy, W, basis, Bs = _conv_operands(filt)
    Wf = (ops.spline_expand(Bs, W) if Bs is not None else W).view(M, Fout, Fin)
    xh = ops.spectral_transform(x, basis, M, False)
    y0 = ops.spectral_transform(ops.spectral_mix(xh, Wf, M), basis, M, True)
    dyh = ops.spectral_transform(gy, basis, M, False)
    dW0 = ops.spectral_mix_bwd_w(dyh, xh, M)
    if Bs is not None:
        dW0 = ops.spline_expand(Bs, dW0.view(M, -1), transpose=True)
    dx0 = ops.spectral_transform(ops.spectral_mix(dyh, Wf, M, transpose=True), basis, M, True)
    assert bool((y0[:, :, M:] == 0).all()) and bool((dx0[:, :, M:] == 0).all()) and dW0.shape == W.shape
    for need_x in (False, True):
        for need_w in (False, True):
            what = 'SpectralConv %s x:%d W:%d' % (filt, need_x, need_w)
            xv, Wv = x.clone().requires_grad_(need_x), W.clone().requires_grad_(need_w)
            saved, _lib.dispatch_log = _lib.dispatch_log, []
            try:
                y = ops.SpectralConv.apply(xv, Wv, basis, Bs, M, Fout)
                if need_x or need_w:
                    y.backward(gy)
                log = [k for _, k in _lib.dispatch_log]
            finally:
                _lib.dispatch_log = saved
            assert y.requires_grad == (need_x or need_w)
            assert_same_bits(what + ' y', y.detach(), y0)
            assert (xv.grad is None) == (not need_x) and (Wv.grad is None) == (not need_w), what
            assert ('spectral_mix_kernel<true>' in log) == need_x, (what, log)
            assert ('spectral_mix_bwd_w_kernel' in log) == need_w, (what, log)
            assert ('spectral_spline_expand_bwd_kernel' in log) == (need_w and Bs is not None), (what, log)
            if need_x:
                assert_same_bits(what + ' dx', xv.grad, dx0)
            if need_w:
                assert_same_bits(what + ' dW', Wv.grad, dW0)


def test_wrappers_copy_a_view(lib):
    """A non-contiguous view of either operand gives the bits of its contiguous copy (it used to be read as if it were dense)."""
    from gcn_fmri_decoding_amd import ops
    c = Mix(5, 3, 9, 33)
    rs = np.random.RandomState(5)
    xh2, dyh2 = _planes_dev(_ints(rs, c.B, 2 * c.Fin, c.M)), _planes_dev(_ints(rs, c.B, 2 * c.Fout, c.M))
    xh, dyh = xh2[:, ::2], dyh2[:, 1::2]
    W = torch.from_numpy(_ints(rs, c.M, c.Fin, c.Fout)).to(DEV).transpose(1, 2)          # [M, Fout, Fin], strides swapped
    Bs = torch.from_numpy(_ints(rs, 7, c.M)).to(DEV).t()                                     # [M, 7]
    Wk = torch.from_numpy(_ints(rs, 7, 2 * c.Fin * c.Fout)).to(DEV)[:, ::2]
    dW = torch.from_numpy(_ints(rs, c.M, 2 * c.Fin * c.Fout)).to(DEV)[:, 1::2]
    for t in (xh, dyh, W, Bs, Wk, dW):
        assert not t.is_contiguous()
    k = torch.Tensor.contiguous
    assert_same_bits('spectral_mix', ops.spectral_mix(xh, W, c.M), ops.spectral_mix(k(xh), k(W), c.M))
    assert_exact('spectral_mix', ops.spectral_mix(xh, W, c.M)[:, :, :c.M],
                 mix_fwd_ref(W.cpu().numpy(), xh[:, :, :c.M].cpu().numpy()))
    assert_same_bits('spectral_mix^T', ops.spectral_mix(dyh, W, c.M, transpose=True), ops.spectral_mix(k(dyh), k(W), c.M, transpose=True))
    assert_same_bits('spectral_mix_bwd_w', ops.spectral_mix_bwd_w(dyh, xh, c.M), ops.spectral_mix_bwd_w(k(dyh), k(xh), c.M))
    assert_same_bits('spline_expand', ops.spline_expand(Bs, Wk), ops.spline_expand(k(Bs), k(Wk)))
    assert_exact('spline_expand', ops.spline_expand(Bs, Wk), spline_ref(Bs.cpu().numpy(), Wk.cpu().numpy()))
    assert_same_bits('spline_expand^T', ops.spline_expand(Bs, dW, transpose=True), ops.spline_expand(k(Bs), k(dW), transpose=True))


def test_wrappers_refuse_mismatched_shapes(lib):
    """ValueError where the shapes of the operands do not agree; ChebgcnError for a host tensor."""
    from gcn_fmri_decoding_amd import ops
    M, Mp, B, Fin, Fout, K = 33, 64, 2, 3, 5, 4

    def z(*shape):
        return torch.zeros(shape, device=DEV)
    bad = {
        'mix: xh has Fout planes': lambda: ops.spectral_mix(z(B, Fout, Mp), z(M, Fout, Fin), M),
        'mix^T: dyh has Fin planes': lambda: ops.spectral_mix(z(B, Fin, Mp), z(M, Fout, Fin), M, transpose=True),
        'mix: Mp is not the stride of M': lambda: ops.spectral_mix(z(B, Fin, Mp + 32), z(M, Fout, Fin), M),
        'mix: dense planes': lambda: ops.spectral_mix(z(B, Fin, M), z(M, Fout, Fin), M),
        'mix: W of M - 1 frequencies': lambda: ops.spectral_mix(z(B, Fin, Mp), z(M - 1, Fout, Fin), M),
        'mix: W of Mp frequencies': lambda: ops.spectral_mix(z(B, Fin, Mp), z(Mp, Fout, Fin), M),
        'mix: 2-D W': lambda: ops.spectral_mix(z(B, Fin, Mp), z(M, Fout * Fin), M),
        'bwd_w: B differs': lambda: ops.spectral_mix_bwd_w(z(B, Fout, Mp), z(B + 1, Fin, Mp), M),
        'bwd_w: Mp differs': lambda: ops.spectral_mix_bwd_w(z(B, Fout, Mp), z(B, Fin, Mp + 32), M),
        'bwd_w: Mp is not the stride of M': lambda: ops.spectral_mix_bwd_w(z(B, Fout, Mp), z(B, Fin, Mp), M + 32),
        'spline: Wk of K + 1 rows': lambda: ops.spline_expand(z(M, K), z(K + 1, 6)),
        'spline: Wk of M rows': lambda: ops.spline_expand(z(M, K), z(M, 6)),
        'spline^T: dW of K rows': lambda: ops.spline_expand(z(M, K), z(K, 6), transpose=True),
        'spline: 3-D Wk': lambda: ops.spline_expand(z(M, K), z(K, 2, 3)),
        'spline: float64': lambda: ops.spline_expand(z(M, K).double(), z(K, 6)),
    }
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + ': accepted')
    host = torch.zeros(B, Fin, Mp)
    for call in (lambda: ops.spectral_mix(host, z(M, Fout, Fin), M), lambda: ops.spectral_mix(z(B, Fin, Mp), z(M, Fout, Fin).cpu(), M),
                 lambda: ops.spectral_mix_bwd_w(z(B, Fout, Mp), host, M), lambda: ops.spline_expand(z(M, K).cpu(), z(K, 6)),
                 lambda: ops.spline_expand(z(M, K), z(K, 6).cpu())):
        with pytest.raises(_lib.ChebgcnError):
            call()
    assert ops.spectral_mix(z(B, Fin, Mp), z(M, Fout, Fin), M).shape == (B, Fout, Mp)
    assert ops.spectral_mix_bwd_w(z(B, Fout, Mp), z(B, Fin, Mp), M).shape == (M, Fout, Fin)
    assert ops.spline_expand(z(M, K), z(K, 6)).shape == (M, 6) and ops.spline_expand(z(M, K), z(M, 6), transpose=True).shape == (K, 6)


def test_tables_reach_every_arm():
    """The tables reach every kernel and arm of csrc/spectral.hip (``table_reach``, by the geometry restated above; every launch
    above checks the kernel's name against chebgcn_last_dispatch())."""
    record_measured('spectral_kernel_tables', arms=table_reach())
