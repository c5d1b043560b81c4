"""The head's hand-written kernels (csrc/head.hip) called directly -- chebgcn_fc_fwd, chebgcn_fc_bwd, chebgcn_planes_to_rows,
chebgcn_rows_to_planes -- against float64 NumPy restatements at the edges of their tiles, loops and masks.  Needs an
MI355X: ``-m gpu``.  tests/test_head_kernel_refs.py holds the restatements to the oracle and checks the host-side figures
used here (the exactness inequality, the gate census, the dispatch arithmetic, the case tables) without a GPU.

``fc_splits`` / ``fwd_dispatch`` / ``bwd_dispatch`` restate the dispatch arithmetic; every call asserts that
``_lib.last_dispatch()`` names the kernels the restatement predicts, and ``table_reach`` asserts that the tables reach

    fc_fwd_kernel, fc_fwd_kernel<split> + fc_fwd_reduce_kernel, fc_bwd_w_kernel, fc_bwd_x_kernel<true>,
    fc_bwd_x_kernel<false>, planes_rows_kernel<to_rows>, planes_rows_kernel<to_planes>

(softmax_xent_kernel: test_softmax_xent_vs_float64).

Every FC case runs two legs.

Exact leg: x and g are integers in [-4, 4], W and the bias multiples of 1/8 in [-1, 1].  Every product and every partial sum
is then a multiple of 1/8 of magnitude <= 4 n + 1 (n: the length of the reduction; 16 n for dW, whose factors are both
integers): exact in fp32 in ANY summation order while 32 n + 8 < 2^24 (``exact_leg_is_exact``, asserted per case).  So the
result equals the float64 restatement -- no tolerance (the sign of a zero aside: an exact sum that cancels is +0 or -0 by the
order of its terms, in float64 as in fp32; both sides are compared after ``+ 0.0``).  Each launch runs twice into freshly
poisoned outputs; the two runs are bit-identical.  g at the gated positions (y <= 0) is 1e30: finite, so a term that leaks
through the gate destroys the exactness instead of hiding in a NaN rule.

Round-off leg: standard-normal x and g, W scaled by 1/sqrt(I), the bias by 0.1; componentwise
    |got - ref| <= (n + 2) 2^-24 (|x| @ |W| + |b|) + 2^-24 |ref|
(the any-order summation bound; |x|.T @ |gm|, sum_b |gm|, |gm| @ |W|.T for the three gradients).  Deliberately loose: the
exact leg discriminates.  The largest measured |err| / bound of every case goes to ``record_measured``.  y of the backward is
the float64 forward rounded to fp32, so the gate of the kernel and of the restatement see the same number.

Poison: the columns [I, ldx) of every x row are NaN (+Inf in one row) wherever ldx > I; every output and the workspace lie
between guard rows of a sentinel, which must be intact afterwards; the columns [I, lddx) of dx and [M*F, ldr) of the flatten's
rows hold the sentinel before and after; with dW == NULL the db buffer keeps its sentinel.

ReLU gate: ``plant_cells`` puts +0.0, -0.0, a negative number and the smallest positive normal (gate open) into y in the
first row, a middle row, row 32 (where B > 32) and the last row; ``assert_gate`` checks that census on the host before a
case is trusted.  A case with fewer than four entries of y (1 x 1 x 1) runs once per planted value instead.  No denormal y.
"""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import plane_stride

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
U = 2.0 ** -24                                               # unit round-off of fp32
TINY = np.finfo(np.float32).tiny                             # smallest positive normal
GATE_LEAK = np.float32(1e30)
EUNSUPPORTED = -4                                            # CHEBGCN_EUNSUPPORTED (include/chebgcn.h)
SENTINEL = -12345.0


# ------------------------------------------------------------------------------------------------------------ restatements

def fc_ref(x, W, b, relu):
    """y = act(x @ W + b) in float64; x [B, I] (no row tail), b [O] or None."""
    y = np.asarray(x, np.float64) @ np.asarray(W, np.float64)
    if b is not None:
        y = y + np.asarray(b, np.float64)
    return np.maximum(y, 0.0) if relu else y


def fc_bwd_ref(x, W, g, y):
    """The layer's gradients in float64: gm = g where y > 0 else 0 (a select: TF's ReluGrad), gm = g for y None."""
    x, W, g = (np.asarray(a, np.float64) for a in (x, W, g))
    gm = g if y is None else np.where(np.asarray(y, np.float64) > 0, g, 0.0)
    return dict(gm=gm, dW=x.T @ gm, db=gm.sum(axis=0), dx=gm @ W.T)


def fc_bounds(x, W, b):
    """Componentwise any-order bound of the forward sums (without the final rounding)."""
    x, W = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(W, np.float64))
    return (x.shape[1] + 2) * U * (x @ W + (0.0 if b is None else np.abs(np.asarray(b, np.float64))))


def fc_bwd_bounds(x, W, gm):
    x, W, gm = (np.abs(np.asarray(a, np.float64)) for a in (x, W, gm))
    B, O = gm.shape
    return dict(dW=(B + 2) * U * (x.T @ gm), db=(B + 2) * U * gm.sum(axis=0), dx=(O + 2) * U * (gm @ W.T))


def _order(order, M):
    return np.arange(M) if order is None else np.asarray(order, np.int64)


def rows_ref(planes, order, M, F, ldr, fill):
    """rows[b, order[v] * F + f] = planes[b, f, v] for v < M; the columns [M*F, ldr) hold ``fill``."""
    planes = np.asarray(planes, np.float64)
    B = planes.shape[0]
    r3 = np.empty((B, M, F))
    r3[:, _order(order, M), :] = planes[:, :, :M].transpose(0, 2, 1)
    rows = np.full((B, ldr), fill, np.float64)
    rows[:, :M * F] = r3.reshape(B, M * F)
    return rows


def planes_ref(rows, order, M, F):
    """The adjoint: planes[b, f, v] = rows[b, order[v] * F + f] for v < M, zero over [M, Mp)."""
    rows = np.asarray(rows, np.float64)
    B = rows.shape[0]
    planes = np.zeros((B, F, plane_stride(M)))
    planes[:, :, :M] = rows[:, :M * F].reshape(B, M, F)[:, _order(order, M), :].transpose(0, 2, 1)
    return planes


def exact_leg_is_exact(n):
    """Sums of n products of the exact leg's values are exact in fp32 in any order."""
    return 32 * n + 8 < 2 ** 24


# ------------------------------------------------------------------------------------------------------------ dispatch restatement

def fc_splits(B, I, O):
    tiles = ((O + 31) // 32) * ((B + 31) // 32)
    return max(1, min(512 // tiles, (I + 511) // 512))


def fc_chunks(B, I, O):
    """(S, chunks of 32 input features, chunks per split)."""
    S = fc_splits(B, I, O)
    n = (I + 31) // 32
    return S, n, (n + S - 1) // S


def fwd_dispatch(B, I, O):
    return 'fc_fwd_kernel<split> + fc_fwd_reduce_kernel' if fc_splits(B, I, O) > 1 else 'fc_fwd_kernel'


def bwd_vec(O, aligned):
    """fc_bwd_x_kernel<true>: 16-byte loads along o -- O a multiple of 4 and g, W, y (where given) 16-byte aligned."""
    return O % 4 == 0 and bool(aligned)


def bwd_dispatch(O, has_dW, has_dx, aligned=True):
    names = ['fc_bwd_w_kernel' if has_dW else '']
    if has_dx:
        names.append('fc_bwd_x_kernel<%s>' % ('true' if bwd_vec(O, aligned) else 'false'))
    return ' + '.join(names)


# ------------------------------------------------------------------------------------------------------------ case tables

Fwd = collections.namedtuple('Fwd', 'B I O ldx')
Bwd = collections.namedtuple('Bwd', 'B I O ldx lddx')
Flat = collections.namedtuple('Flat', 'B M F pad')              # ldr = M*F + pad


def _up4(n):
    return (n + 3) & ~3


def _fwd(B, I, O, ldx=None):
    return Fwd(B, I, O, ldx or _up4(I))


def _bwd(B, I, O, ldx=None, lddx=None):
    return Bwd(B, I, O, ldx or I, lddx or I)


FWD_CASES = [
    # one launch (no workspace)
    _fwd(1, 1, 1),
    _fwd(8, 37, 5, 64),                                      # a [B, 37] view of a [B, plane_stride(37)] buffer
    _fwd(31, 16, 31),
    _fwd(32, 32, 32),
    _fwd(33, 33, 33),
    _fwd(65, 255, 70),
    _fwd(40, 512, 36),
    _fwd(128, 512, 256),                                     # the shape the kernel's header comment names
    _fwd(5, 360, 22, 384),                                   # a [B, 360] view of a [B, plane_stride(360)] buffer
    # I > 512 is split unless the launch has more than 256 tiles: 17 x 16 tiles, 17 chunks -- the second trip of the wave loop
    # with the reduction in one workgroup
    _fwd(513, 513, 481),
    # split across workgroups
    _fwd(40, 513, 36),                                       # S = 2 (the library's figure: 513 features are two lengths of 512)
    _fwd(8, 5760, 12),                                       # S = 12, FlatFC's shape
    _fwd(4, 1027, 3),                                        # S = 3, I % 4 = 3
    _fwd(33, 10466, 40),                                     # S = 21: the reduce kernel's second batch of sixteen
    _fwd(128, 16416, 128),                                   # S = 32, 17 chunks per split, split 31 empty
]
FWD_SPLITS = {(40, 513, 36): 2, (8, 5760, 12): 12, (4, 1027, 3): 3, (33, 10466, 40): 21, (128, 16416, 128): 32}
FWD_COMBOS = [(bias, relu) for bias in (1, 0) for relu in (1, 0)]            # every case runs all four
FWD_REFUSED = [(_fwd(4, 37, 5, 38), 0, 'ldx % 4 != 0'), (_fwd(4, 37, 5, 40), 1, 'x offset by 4 bytes')]

BWD_CASES = [
    _bwd(1, 1, 1),
    _bwd(7, 33, 5),                                          # <false>: O is odd
    _bwd(8, 37, 12, 40, 40),
    _bwd(9, 31, 31),
    _bwd(64, 32, 32),
    _bwd(65, 40, 33, 40, 44),
    _bwd(129, 70, 36),                                       # second wave trip of bwd_w; <true> with O % 8 = 4
    _bwd(33, 65, 260),                                       # <true>, second trip of bwd_x
    _bwd(33, 65, 257),                                       # <false>, second trip
    _bwd(1000, 8, 7),
    _bwd(8, 5760, 12),                                       # FlatFC's shape
]
BWD_MISALIGNED = _bwd(16, 40, 12)                            # <false> by a pointer off by one float: g, then W, then y
BWD_FORMS = {'full': ('dW', 'db', 'dx'), 'no_dW': ('db', 'dx'), 'no_dx': ('dW', 'db'), 'no_db': ('dW', 'dx')}

FLAT_CASES = [Flat(1, 1, 1, 0), Flat(2, 33, 1, 0), Flat(3, 64, 32, 0), Flat(3, 65, 33, 0), Flat(2, 100, 65, 0),
              Flat(2, 360, 16, 0), Flat(2, 360, 16, 12)]


def case_id(c):
    if isinstance(c, Flat):
        return 'B%d-M%d-F%d%s' % (c.B, c.M, c.F, '-ldr+%d' % c.pad if c.pad else '')
    s = '%dx%dx%d' % (c.B, c.I, c.O)
    if c.ldx != (_up4(c.I) if isinstance(c, Fwd) else c.I):
        s += '-ldx%d' % c.ldx
    if isinstance(c, Bwd) and c.lddx != c.I:
        s += '-lddx%d' % c.lddx
    return s


def _seed(c, exact):
    return (zlib.crc32((type(c).__name__ + case_id(c)).encode()) + (0 if exact else 1)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------ inputs (host)

def _x_rows(rs, B, I, ldx, exact):
    """[B, ldx] fp32: data over [0, I), NaN over [I, ldx), +Inf there in row B // 2."""
    x = np.full((B, ldx), np.nan, np.float32)
    x[:, :I] = rs.randint(-4, 5, (B, I)) if exact else rs.randn(B, I)
    if ldx > I:
        x[B // 2, I:] = np.inf
    return x


def _weights(rs, I, O, exact):
    if exact:
        return (rs.randint(-8, 9, (I, O)) / 8.0).astype(np.float32), (rs.randint(-8, 9, O) / 8.0).astype(np.float32)
    return (rs.randn(I, O) / np.sqrt(I)).astype(np.float32), (0.1 * rs.randn(O)).astype(np.float32)


def fwd_inputs(c, exact):
    """(x [B, ldx], W [I, O], b [O]) in fp32 on the host."""
    rs = np.random.RandomState(_seed(c, exact))
    x = _x_rows(rs, c.B, c.I, c.ldx, exact)
    W, b = _weights(rs, c.I, c.O, exact)
    return x, W, b


PLANTS = (np.float32(0.0), np.float32(-0.0), np.float32(-1.0), TINY)
PLANT_NAMES = ('pzero', 'nzero', 'negative', 'tiny')


def gate_variants(c):
    """The runs of a backward case with y: one with all four plants, or -- fewer than four entries -- one per plant."""
    return [None] if c.B * c.O >= 4 else [0, 1, 2, 3]


def plant_rows(B):
    return sorted({0, B // 2, B - 1} | ({32} if B > 32 else set()))


def plant_cells(B, O, only=None):
    """(row, column, kind) of the planted entries of y: the four kinds in every row of plant_rows, in the columns 0, O/3, 2O/3
    and O - 1, rotated from row to row."""
    if only is not None:
        return [(0, 0, only)]
    assert O >= 4
    cols = [0, O // 3, 2 * O // 3, O - 1]
    return [(r, cols[(k + j) % 4], k) for j, r in enumerate(plant_rows(B)) for k in range(4)]


def gate_census(y):
    """kind -> sorted rows of y that hold an entry of that kind."""
    y = np.asarray(y, np.float32)
    sign = np.signbit(y)
    kinds = dict(pzero=(y == 0) & ~sign, nzero=(y == 0) & sign, negative=y < 0, tiny=y == TINY)
    assert not ((y > 0) & (y < TINY)).any(), 'denormal y'
    return {k: sorted(set(np.nonzero(m)[0].tolist())) for k, m in kinds.items()}


def assert_gate(what, ys, B):
    """Every kind occurs over the runs ``ys`` of a case, in a row >= 32 where B > 32, and in the last row."""
    rows = {k: set() for k in PLANT_NAMES}
    for y in ys:
        for k, r in gate_census(y).items():
            rows[k] |= set(r)
    for k in PLANT_NAMES:
        assert rows[k], '%s: y holds no %s entry' % (what, k)
        assert B - 1 in rows[k], '%s: no %s entry in the last row' % (what, k)
        if B > 32:
            assert any(r >= 32 for r in rows[k]), '%s: no %s entry in a row >= 32' % (what, k)
    return {k: len(v) for k, v in rows.items()}


def bwd_inputs(c, exact, with_y, only=None):
    """(x [B, ldx], W [I, O], g [B, O], y [B, O] or None) in fp32 on the host.  y: the float64 forward (ReLU, no bias) rounded
    to fp32, then the plants; exact leg: g = 1e30 wherever the gate is closed."""
    rs = np.random.RandomState(_seed(c, exact))
    x = _x_rows(rs, c.B, c.I, c.ldx, exact)
    W, _ = _weights(rs, c.I, c.O, exact)
    g = (rs.randint(-4, 5, (c.B, c.O)) if exact else rs.randn(c.B, c.O)).astype(np.float32)
    if not with_y:
        return x, W, g, None
    y = fc_ref(x[:, :c.I], W, None, True).astype(np.float32)
    for r, col, k in plant_cells(c.B, c.O, only):
        y[r, col] = PLANTS[k]
    if exact:
        g[y <= 0] = GATE_LEAK
    return x, W, g, y


def flat_inputs(c, permuted):
    """(planes [B, F, Mp] distinct integers with a NaN pad, r [B, ldr] integers in [-4, 4] with a NaN tail, order or None)."""
    rs = np.random.RandomState(_seed(c, True) + permuted)
    Mp, ldr = plane_stride(c.M), c.M * c.F + c.pad
    planes = np.full((c.B, c.F, Mp), np.nan, np.float32)
    planes[:, :, :c.M] = 1 + rs.permutation(c.B * c.F * c.M).reshape(c.B, c.F, c.M)
    r = np.full((c.B, ldr), np.nan, np.float32)
    r[:, :c.M * c.F] = rs.randint(-4, 5, (c.B, c.M * c.F))
    return planes, r, rs.permutation(c.M).astype(np.int32) if permuted else None


# ------------------------------------------------------------------------------------------------------------ table coverage

ARMS = ('fc_fwd_kernel', 'fc_fwd_kernel<split> + fc_fwd_reduce_kernel', 'fc_bwd_w_kernel', 'fc_bwd_x_kernel<true>',
        'fc_bwd_x_kernel<false>', 'planes_rows_kernel<to_rows>', 'planes_rows_kernel<to_planes>')


def table_reach():
    """arm -> ids of its cases, after asserting that the tables reach every kernel of csrc/head.hip but the softmax and, read off
    the kernels, every loop trip, tile edge and mask listed below.  Host arithmetic only."""
    reach = collections.defaultdict(list)
    assert len({case_id(c) for c in FWD_CASES}) == len(FWD_CASES) and len({case_id(c) for c in BWD_CASES}) == len(BWD_CASES)
    fw = [(c,) + fc_chunks(c.B, c.I, c.O) for c in FWD_CASES]
    for c, S, n, cps in fw:
        assert c.ldx >= c.I and c.ldx % 4 == 0 and exact_leg_is_exact(c.I), c
        assert S == FWD_SPLITS.get((c.B, c.I, c.O), 1), (c, S)
        reach[fwd_dispatch(c.B, c.I, c.O)].append(case_id(c))
    one = [t for t in fw if t[1] == 1]
    split = [t for t in fw if t[1] > 1]
    assert any(1 < S <= 16 for _, S, _, _ in split) and any(S > 16 for _, S, _, _ in split)
    assert any((S - 1) * cps >= n for _, S, n, cps in split), 'no empty last split'
    assert any(cps > 16 for _, _, _, cps in split) and any(n > 16 for _, _, n, _ in one), 'no second trip of the wave loop'
    assert any(n < 8 for _, _, n, _ in one), 'no idle wave'
    for group in (one, split):
        cs = [t[0] for t in group]
        assert any(c.I % 4 and c.ldx > c.I for c in cs) and any(c.I % 32 == 0 for c in cs)
        assert any(c.B > 32 and c.B % 32 for c in cs) and any(c.O > 32 and c.O % 32 for c in cs)
    cs = [t[0] for t in one]
    assert any(c.I % 16 == 0 and c.I % 32 for c in cs) and any(c.ldx >= c.I + 16 for c in cs)      # a whole NaN half-chunk is loaded
    assert any(c.O > 32 and c.O % 2 for c in FWD_CASES)
    assert any(c.ldx == plane_stride(c.I) and c.I == 360 for c in cs) and any(c.ldx == plane_stride(c.I) and c.I == 37 for c in cs)
    assert len(FWD_COMBOS) == 4 and len(set(FWD_COMBOS)) == 4                    # NULL bias with ReLU on and off on every case
    for c, off, _ in FWD_REFUSED:
        assert (c.ldx % 4 != 0) != (off != 0) and c.ldx >= c.I
    for c in BWD_CASES + [BWD_MISALIGNED]:
        assert c.ldx >= c.I and c.lddx >= c.I and all(exact_leg_is_exact(n) for n in (c.B, c.I, c.O)), c
        reach['fc_bwd_w_kernel'].append(case_id(c))
        reach['fc_bwd_x_kernel<%s>' % ('true' if bwd_vec(c.O, c is not BWD_MISALIGNED) else 'false')].append(case_id(c))
    bw = BWD_CASES
    assert any(c.B % 8 for c in bw) and any(128 < c.B <= 256 for c in bw) and any(c.B > 256 for c in bw)
    assert any(c.I > 32 and c.O > 32 for c in bw), 'db from the first row of workgroups only'
    assert any(c.lddx > c.I for c in bw) and any(c.ldx > c.I for c in bw)
    vec = [c for c in bw if bwd_vec(c.O, True)]
    sca = [c for c in bw if not bwd_vec(c.O, True)]
    assert any(c.O > 256 for c in vec) and any(c.O > 256 for c in sca) and any(c.O % 8 == 4 for c in vec)
    assert any(c.O % 2 for c in sca) and BWD_MISALIGNED.O % 4 == 0
    assert any(c.B * c.O < 4 for c in bw) and any(c.B > 32 for c in bw)
    for c in FLAT_CASES:
        reach['planes_rows_kernel<to_rows>'].append(case_id(c))
        reach['planes_rows_kernel<to_planes>'].append(case_id(c))
    assert {c.F for c in FLAT_CASES} >= {1, 33, 65} and {c.M for c in FLAT_CASES} >= {1, 64, 65}
    assert any(c.pad for c in FLAT_CASES) and any(c.M > 128 for c in FLAT_CASES)
    assert set(reach) == set(ARMS), sorted(reach)
    return dict(reach)


# ------------------------------------------------------------------------------------------------------------ device plumbing

@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.lib()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, offset=0):
    """``a`` (fp32) on the device, ``offset`` floats past a 16-byte boundary."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 4, device=DEV)
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * offset
    return v


class Guarded:
    """A [rows, cols] output between guard rows of the sentinel; the columns [0, written) are poisoned (NaN, or the sentinel
    for a buffer that must stay untouched), the columns [written, cols) hold the sentinel."""

    def __init__(self, rows, cols, written=None, poison=float('nan')):
        self.n, self.written = rows * cols, cols if written is None else written
        self.g = (max(256, 2 * cols) + 63) // 64 * 64
        self.whole = torch.full((2 * self.g + self.n,), SENTINEL, device=DEV)
        self.t = self.whole[self.g:self.g + self.n].view(rows, cols)
        self.t[:, :self.written] = poison

    def check(self, what):
        assert bool((self.whole[:self.g] == SENTINEL).all()) and bool((self.whole[self.g + self.n:] == SENTINEL).all()), \
            what + ': a store left the buffer (guard rows changed)'
        assert bool((self.t[:, self.written:] == SENTINEL).all()), what + ': the columns past the data were written'

    def untouched(self):
        return bool((self.whole == SENTINEL).all())


def _bits(a):
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)


def assert_exact(what, got, ref64):
    """``got`` (device or host fp32) equals the float64 reference, which is itself exact in fp32."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref32 = np.asarray(ref64).astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref64), what + ': the reference is not exact in fp32'
    assert got.shape == ref32.shape, (what, got.shape, ref32.shape)
    bad = _bits(got) != _bits(ref32)
    assert not bad.any(), '%s: %d of %d values differ from the restatement, first at %s: %r against %r' % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref32[bad][0])


def assert_same_bits(what, a, b):
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what + ': two runs differ'


def roundoff_ratio(what, got, ref64, bound):
    """max |got - ref| / (bound + 2^-24 |ref|), asserted <= 1."""
    got = got.cpu().numpy().astype(np.float64)
    full = bound + U * np.abs(ref64)
    err = np.abs(got - ref64)
    assert np.isfinite(got).all(), what + ': not finite'
    ratio = float((err[full > 0] / full[full > 0]).max()) if (full > 0).any() else 0.0
    print('%s: |err| / bound = %.3f' % (what, ratio))
    assert (err <= full).all(), '%s: |err| / bound = %.3f (worst |err| %.3e)' % (what, ratio, err.max())
    return ratio


# ------------------------------------------------------------------------------------------------------------ forward

def _fc_fwd(lib, c, x, W, b, relu, what):
    """One launch into fresh guarded buffers: y [B, O] on the device."""
    y = Guarded(c.B, c.O)
    nws = lib.chebgcn_fc_fwd_workspace(c.B, c.I, c.O)
    S = fc_splits(c.B, c.I, c.O)
    assert nws == (S * c.B * c.O * 4 if S > 1 else 0), (what, nws, S)
    ws = Guarded(1, nws // 4) if nws else None
    _lib.check(lib.chebgcn_fc_fwd(_P(x), c.ldx, _P(W), _P(b), _P(y.t), _P(ws.t) if ws else None, nws, c.B, c.I, c.O, relu,
                                  _stream()), 'fc_fwd')
    assert _lib.last_dispatch() == fwd_dispatch(c.B, c.I, c.O), (what, _lib.last_dispatch())
    torch.cuda.synchronize()
    y.check(what + ' y')
    if ws:
        ws.check(what + ' workspace')
    return y.t


@pytest.mark.parametrize('c', FWD_CASES, ids=case_id)
def test_fc_forward_vs_float64(lib, c):
    """Exact leg: bit for bit, twice, for every bias / ReLU combination.  Round-off leg: the any-order bound."""
    assert exact_leg_is_exact(c.I)
    ratios = {}
    for exact in (True, False):
        x, W, b = fwd_inputs(c, exact)
        pre = fc_ref(x[:, :c.I], W, None, False)             # one float64 product per leg, shared by the combinations
        xd, Wd, bd = _dev(x), _dev(W), _dev(b)
        bound = None if exact else fc_bounds(x[:, :c.I], W, None)
        for bias, relu in FWD_COMBOS:
            what = 'fc_fwd %s %s%s%s' % (case_id(c), 'exact' if exact else 'round-off', ' bias' if bias else '', ' relu' if relu else '')
            ref = pre + b.astype(np.float64) if bias else pre
            ref = np.maximum(ref, 0.0) if relu else ref
            got = _fc_fwd(lib, c, xd, Wd, bd if bias else None, relu, what)
            if exact:
                assert_exact(what, got, ref)
                assert_same_bits(what, got, _fc_fwd(lib, c, xd, Wd, bd if bias else None, relu, what))
            else:
                full = bound + (c.I + 2) * U * np.abs(b.astype(np.float64)) if bias else bound      # fc_bounds(x, W, b)
                ratios['bias%d_relu%d' % (bias, relu)] = roundoff_ratio(what, got, ref, full)
    record_measured('fc_forward_vs_float64[%s]' % case_id(c), arm=fwd_dispatch(c.B, c.I, c.O), splits=fc_splits(c.B, c.I, c.O),
                    **ratios)


@pytest.mark.parametrize('c,offset,why', FWD_REFUSED, ids=['ldx', 'pointer'])
def test_fc_forward_refuses_unaligned_rows(lib, c, offset, why):
    """A row stride that is no multiple of 4 floats, an x that is not 16-byte aligned: CHEBGCN_EUNSUPPORTED, y untouched."""
    x, W, b = fwd_inputs(c, True)
    xd, Wd, bd = _dev(x, offset), _dev(W), _dev(b)
    y = Guarded(c.B, c.O, poison=SENTINEL)
    torch.cuda.synchronize()
    before = _lib.last_dispatch()
    rc = lib.chebgcn_fc_fwd(_P(xd), c.ldx, _P(Wd), _P(bd), _P(y.t), None, 0, c.B, c.I, c.O, 1, _stream())
    assert rc == EUNSUPPORTED, (why, rc)
    assert _lib.last_dispatch() == before, 'a refused call enqueued %s' % _lib.last_dispatch()
    torch.cuda.synchronize()
    assert y.untouched(), why + ': a refused call wrote y'


# ------------------------------------------------------------------------------------------------------------ backward

def _fc_bwd(lib, c, d, form, what, aligned=True):
    """One launch of chebgcn_fc_bwd into fresh guarded buffers.  d: x, W, g, y on the device (y may be None).  Returns the
    outputs of ``form`` by name; with dW == NULL the db buffer must keep its sentinel."""
    want = BWD_FORMS[form]
    dW = Guarded(c.I, c.O) if 'dW' in want else None
    db = Guarded(1, c.O, poison=float('nan') if dW else SENTINEL) if 'db' in want else None
    dx = Guarded(c.B, c.lddx, written=c.I) if 'dx' in want else None
    _lib.check(lib.chebgcn_fc_bwd(_P(d['x']), c.ldx, _P(d['W']), _P(d['g']), _P(d['y']), _P(dW.t) if dW else None,
                                  _P(db.t) if db else None, _P(dx.t) if dx else None, c.lddx, c.B, c.I, c.O, _stream()), 'fc_bwd')
    assert _lib.last_dispatch() == bwd_dispatch(c.O, dW is not None, dx is not None, aligned), (what, _lib.last_dispatch())
    torch.cuda.synchronize()
    out = {}
    for name, buf in (('dW', dW), ('db', db), ('dx', dx)):
        if buf is not None:
            buf.check('%s %s' % (what, name))
            out[name] = buf.t
    if db is not None and dW is None:
        assert db.untouched(), what + ': db was written although dW is NULL'
        del out['db']
    if dx is not None:
        out['dx'] = dx.t[:, :c.I]
    if db is not None and dW is not None:
        out['db'] = db.t[0]
    return out


def _bwd_device(x, W, g, y, off=()):
    return dict(x=_dev(x), W=_dev(W, 'W' in off), g=_dev(g, 'g' in off), y=_dev(y, 'y' in off))


def _bwd_exact(lib, c, with_y, only, off=()):
    what = 'fc_bwd %s exact%s%s' % (case_id(c), ' y' if with_y else '', ' off:' + ','.join(off) if off else '')
    x, W, g, y = bwd_inputs(c, True, with_y, only)
    r = fc_bwd_ref(x[:, :c.I], W, g, y)
    d = _bwd_device(x, W, g, y, off)
    for form in BWD_FORMS:
        got = _fc_bwd(lib, c, d, form, '%s %s' % (what, form), aligned=not off)
        for name, t in got.items():
            assert_exact('%s %s %s' % (what, form, name), t, r[name])
        if form == 'full':
            again = _fc_bwd(lib, c, d, form, what, aligned=not off)
            for name, t in got.items():
                assert_same_bits('%s %s' % (what, name), t, again[name])
    return y


@pytest.mark.parametrize('c', BWD_CASES, ids=case_id)
def test_fc_backward_vs_float64(lib, c):
    """With y and with y NULL; all three gradients, then dW, dx and db NULL in turn.  Exact leg bit for bit, the full form
    twice; round-off leg within the any-order bounds."""
    assert all(exact_leg_is_exact(n) for n in (c.B, c.I, c.O))
    ys = [_bwd_exact(lib, c, True, only) for only in gate_variants(c)]
    census = assert_gate(case_id(c), ys, c.B)
    _bwd_exact(lib, c, False, None)
    ratios = {}
    for with_y in (True, False):
        for only in (gate_variants(c) if with_y else [None]):
            x, W, g, y = bwd_inputs(c, False, with_y, only)
            r = fc_bwd_ref(x[:, :c.I], W, g, y)
            bounds = fc_bwd_bounds(x[:, :c.I], W, r['gm'])
            what = 'fc_bwd %s round-off%s' % (case_id(c), ' y' if with_y else '')
            got = _fc_bwd(lib, c, _bwd_device(x, W, g, y), 'full', what)
            for name, t in got.items():
                key = '%s_%s' % (name, 'y' if with_y else 'noy')
                ratios[key] = max(ratios.get(key, 0.0), roundoff_ratio('%s %s' % (what, name), t, r[name], bounds[name]))
    record_measured('fc_backward_vs_float64[%s]' % case_id(c), arm=bwd_dispatch(c.O, True, True), plants=census, **ratios)


@pytest.mark.parametrize('which', ['g', 'W', 'y'])
def test_fc_backward_misaligned_pointer_takes_scalar_loads(lib, which):
    """O % 4 == 0, but g, W or y starts one float past a 16-byte boundary: fc_bwd_x_kernel<false> (asserted in _fc_bwd), exact."""
    c = BWD_MISALIGNED
    assert c.O % 4 == 0 and bwd_dispatch(c.O, True, True, False).endswith('fc_bwd_x_kernel<false>')
    y = _bwd_exact(lib, c, True, None, off=(which,))
    assert_gate(case_id(c), [y], c.B)


# ------------------------------------------------------------------------------------------------------------ flatten

def _flatten(lib, to_rows, c, src, order, what, dst_rows=None):
    Mp, ldr = plane_stride(c.M), c.M * c.F + c.pad
    dst = Guarded(c.B, ldr, written=c.M * c.F) if to_rows else Guarded(c.B * c.F, Mp)
    fn = lib.chebgcn_planes_to_rows if to_rows else lib.chebgcn_rows_to_planes
    _lib.check(fn(_P(src), _P(dst.t), _P(order), c.B, c.M, c.F, ldr, _stream()), what)
    assert _lib.last_dispatch() == 'planes_rows_kernel<%s>' % ('to_rows' if to_rows else 'to_planes'), (what, _lib.last_dispatch())
    torch.cuda.synchronize()
    dst.check(what)
    return dst.t if to_rows else dst.t.view(c.B, c.F, Mp)


@pytest.mark.parametrize('permuted', [1, 0], ids=['order', 'identity'])
@pytest.mark.parametrize('c', FLAT_CASES, ids=case_id)
def test_flatten_vs_restatement(lib, c, permuted):
    """planes_to_rows and rows_to_planes bit for bit (pure copies), twice; NaN source pads; the columns [M*F, ldr) keep the
    sentinel; exact zeros over the pad of the planes; the round trip; the adjoint identity on integers."""
    what = 'flatten %s %s' % (case_id(c), 'order' if permuted else 'identity')
    M, F, MF = c.M, c.F, c.M * c.F
    planes, r, order = flat_inputs(c, permuted)
    pd, rd = _dev(planes), _dev(r)
    od = torch.as_tensor(order).to(DEV) if permuted else None
    rows = _flatten(lib, True, c, pd, od, what + ' to_rows')
    assert_exact(what + ' to_rows', rows[:, :MF], rows_ref(planes, order, M, F, MF, 0.0))
    assert_same_bits(what + ' to_rows', rows[:, :MF], _flatten(lib, True, c, pd, od, what + ' to_rows')[:, :MF])
    back = _flatten(lib, False, c, rd, od, what + ' to_planes')
    want = planes_ref(r, order, M, F)
    assert_exact(what + ' to_planes', back, want)
    assert bool((back[:, :, M:].contiguous().view(torch.int32) == 0).all()), what + ': the pad of the planes is not +0.0'
    assert_same_bits(what + ' to_planes', back, _flatten(lib, False, c, rd, od, what + ' to_planes'))
    # the round trip reads the rows exactly as the gather left them (sentinel columns included)
    trip = _flatten(lib, False, c, rows, od, what + ' round trip')
    assert_exact(what + ' round trip', trip[:, :, :M], planes[:, :, :M].astype(np.float64))
    assert bool((trip[:, :, M:] == 0).all())
    lhs = (rows[:, :MF].cpu().numpy().astype(np.float64) * r[:, :MF]).sum()
    rhs = (planes[:, :, :M].astype(np.float64) * back[:, :, :M].cpu().numpy()).sum()
    assert lhs == rhs, '%s: <to_rows(p), r> = %r, <p, to_planes(r)> = %r' % (what, lhs, rhs)


# ------------------------------------------------------------------------------------------------------------ wrappers

def test_ops_fc_forward_declines_and_serves(lib):
    from gcn_fmri_decoding_amd import ops
    c = _fwd(5, 37, 6, 38)
    x, W, b = fwd_inputs(c, True)
    Wd, bd = _dev(W), _dev(b)
    assert ops.fc_forward(_dev(x)[:, :c.I], Wd, bd, True) is None, 'a row stride of 38 floats'
    c = _fwd(5, 37, 6, 40)
    x, _, _ = fwd_inputs(c, True)
    assert ops.fc_forward(_dev(x, 1)[:, :c.I], Wd, bd, True) is None, 'x one float past a 16-byte boundary'
    c = _fwd(6, 360, 9, plane_stride(360))
    x, W, b = fwd_inputs(c, True)
    y = ops.fc_forward(_dev(x)[:, :c.I], _dev(W), _dev(b), True)
    assert y is not None and _lib.last_dispatch() == 'fc_fwd_kernel'
    assert_exact('ops.fc_forward', y, fc_ref(x[:, :c.I], W, b, True))


def test_ops_fc_backward_writes_given_buffers(lib):
    from gcn_fmri_decoding_amd import ops
    c = _bwd(8, 360, 9)
    x, W, g, y = bwd_inputs(c, True, True)
    assert_gate('ops.fc_backward', [y], c.B)
    r = fc_bwd_ref(x, W, g, y)
    dW, db = Guarded(c.I, c.O), Guarded(1, c.O)
    res = ops.fc_backward(_dev(x), _dev(W), _dev(g), _dev(y), dW.t, db.t[0], True)
    assert res is not None and _lib.last_dispatch() == bwd_dispatch(c.O, True, True)
    torch.cuda.synchronize()
    dW.check('ops.fc_backward dW')
    db.check('ops.fc_backward db')
    assert_exact('ops.fc_backward dW', dW.t, r['dW'])
    assert_exact('ops.fc_backward db', db.t[0], r['db'])
    assert_exact('ops.fc_backward dx', res[0], r['dx'])
    assert ops.fc_backward(_dev(x), _dev(W), _dev(g), _dev(y), dW.t, db.t[0], False) == (None,)


def test_ops_fc_input_grad_copies_odd_rows(lib):
    """A dense [5, 37] x (row stride 37) goes through ops._fc_rows' copy; forward and input gradient are the library's
    kernels, no weight gradient is launched."""
    from gcn_fmri_decoding_amd import ops
    c = _bwd(5, 37, 6)
    x, W, g, _ = bwd_inputs(c, True, False)
    b = (np.arange(c.O) - 3).astype(np.float32) / 8
    y_ref = fc_ref(x, W, b, True)
    g[y_ref <= 0] = GATE_LEAK
    r = fc_bwd_ref(x, W, g, y_ref)
    xd = _dev(x).requires_grad_(True)
    assert xd.stride(0) == 37 and ops._fc_rows(xd.detach()).data_ptr() != xd.data_ptr()
    saved, _lib.dispatch_log = _lib.dispatch_log, []
    try:
        y = ops.FCInputGrad.apply(xd, _dev(W), _dev(b), True)
        y.backward(_dev(g))
        log = list(_lib.dispatch_log)
    finally:
        _lib.dispatch_log = saved
    assert log == [('fc_fwd', 'fc_fwd_kernel'), ('fc_bwd_x', bwd_dispatch(c.O, False, True))], log
    assert 'fc_bwd_x_kernel' in log[1][1] and not any('bwd_w' in k for _, k in log)
    assert_exact('FCInputGrad y', y.detach(), y_ref)
    assert_exact('FCInputGrad dx', xd.grad, r['dx'])


def test_tables_reach_every_arm():
    """The tables reach every kernel and arm of csrc/head.hip but the softmax (``table_reach``, by the dispatch restatement,
    which every launch above checks against chebgcn_last_dispatch())."""
    reach = table_reach()
    record_measured('head_kernel_tables', arms=reach)
