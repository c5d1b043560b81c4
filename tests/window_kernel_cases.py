"""What tests/test_gpu_window_kernels.py (on the device) and tests/test_window_kernel_refs.py (on the host) share: the case tables
of the window gathers and window statistics of csrc/series.hip and csrc/augment.hip -- ``chebgcn_gather_windows``, ``_mix``,
``_indexed``, ``_reflect``, ``chebgcn_window_drop``, ``chebgcn_window_stats`` and ``chebgcn_window_stats_indexed`` -- with their
references, the kernels' constants read from the sources, their dispatch arithmetic restated, and the comparisons both modules
use.  Plain helpers, built on the host without a GPU.

Inputs are seeded per case (crc32 of its id).  Lanes the header says are never read as data (the pad [M, Mp) of the series and
of the tables) hold NaN.  ``B``, or the number of windows of a launch, is at most 9 unless the edge is the window count itself.

References
  * Gathers and drop: the contract of include/chebgcn.h in float32 NumPy -- sources added in ascending order, one correctly
    rounded division per level (and only where its count is above 1), the tables as a rounded product then a rounded sum, the
    pad zero; every row, count, shift, source and (indexed) sample outside its range reads what the clamped value reads.  The
    comparison is BIT FOR BIT (``check_bits``).  ``sample`` of the plain, mix and reflect gathers stays the caller's duty (the
    header clamps it for the indexed gather only), so the tables keep it in range there.
  * Statistics, bounded leg: float64 NumPy over the windows as the gather forms them, with the bounds the project already
    states (``stats_bound``: two orderings of a float64 sum of S terms differ by at most S 2^-52 sum|x|); the float32 tables are
    the device's own float64 rounded once, bit for bit.  No other tolerance.
  * Statistics, exact leg: the series holds integers |x| <= 8, S and fold are powers of two, so every deviation, product, sum
    and quotient is exact in float64 whatever the order: ``mean`` and ``var`` equal the float64 reference bit for bit
    (``exact_in_fractions`` proves the reference exact with ``fractions.Fraction``).  fold = 3 divides by 3 in float32 and has
    no exact leg.
  * Both legs keep one vertex constant in time (where M > 1): its variance is exactly 0, its scale 1, its shift ``-mean``.
"""
import fractions
import os
import re
import types
import zlib

import numpy as np

from conftest import ROOT
from gcn_fmri_decoding_amd import series
from gcn_fmri_decoding_amd._lib import plane_stride

import guarded_buffers as gb

CSRC = os.path.join(ROOT, 'gcn_fmri_decoding_amd', 'csrc')
NAN = np.float32(np.nan)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

CONSTANT_FILES = {'GW_T': 'gather_piece.h', 'GW_U': 'gather_piece.h', 'GWM_MAX': 'series.hip', 'GWI_MAX': 'series.hip',
                  'WS_T': 'series.hip', 'WS_CG': 'series.hip', 'WS_ROWS': 'series.hip', 'WSI_CHUNKS': 'series.hip',
                  'WSI_MIN': 'series.hip', 'WD_T': 'augment.hip'}


def source_constant(file, name, csrc=CSRC):
    """``constexpr int NAME = value;`` of a source under csrc/ (entries without a geometry query)."""
    text = open(os.path.join(csrc, file)).read()
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % re.escape(name), text)
    assert m, '%s: no constexpr int %s' % (file, name)
    return int(m.group(1))


def constants(csrc=CSRC):
    """The kernels' constants as the sources under ``csrc`` state them."""
    return types.SimpleNamespace(**{name: source_constant(file, name, csrc) for name, file in CONSTANT_FILES.items()})


def source_bodies(csrc=CSRC):
    """``(the N of the mix kernel's bodies, the (fold, n) of the indexed kernel's)`` as series.hip instantiates them."""
    text = open(os.path.join(csrc, 'series.hip')).read()
    return (sorted(int(n) for n in re.findall(r'CG_MIX_CASE\((\d+)\)', text)),
            sorted((int(f), int(n)) for f, n in re.findall(r'CG_IDX_CASE\((\d+),\s*(\d+)\)', text)))


K = constants()

# ---------------------------------------------------------------------------------------------------------- dispatch arithmetic
# restated from series.hip / augment.hip / gather_piece.h; ``k``: a ``constants()`` namespace

SPECIALISED = tuple([(1, n) for n in range(1, 9)] + [(2, n) for n in range(1, 5)] + [(3, 1), (4, 1)])
GENERIC_NEIGHBOURS = ((1, 9), (2, 5), (3, 2), (4, 2), (5, 1), (16, 16), (16, 1), (1, 16))


def pieces(M, C):
    """16-byte pieces of one window."""
    return C * plane_stride(M) // 4


def gather_blocks(k, M, C):
    return -(-pieces(M, C) // (k.GW_T * k.GW_U))


def width(k, L):
    """Pieces per thread and pass of a body with L = N (mix) or fold * n (indexed) loads per piece."""
    return k.GW_U if L <= 4 else (k.GW_U // 2 if L <= 8 else k.GW_U // 4)


def passes(k, L):
    return k.GW_U // width(k, L)


def pass_fill(k, M, C, L):
    """[block][pass] -> how many of the pass's GW_T * U pieces lie inside the window."""
    per_pass, tile, n = k.GW_T * width(k, L), k.GW_T * k.GW_U, pieces(M, C)
    return [[max(0, min(per_pass, n - b * tile - p * per_pass)) for p in range(passes(k, L))] for b in range(gather_blocks(k, M, C))]


def channel_groups(k, C):
    return -(-C // k.WS_CG)


def row_chunks(k, Ttot):
    return -(-Ttot // k.WS_ROWS)


def wsi_chunk(k, S):
    return max(k.WSI_MIN, -(-S // k.WSI_CHUNKS))


def wsi_chunks(k, S):
    return -(-S // wsi_chunk(k, S))


STATS_SLABS = 4             # float64 [C][Mp] slabs of a chunk's partials: the heads of sum d and sum d^2, then their tails


def stats_count_bytes(k, Ttot, C):
    """The count table of window_stats: C - 1 + WS_CG zeros in front, Ttot counts, 4 behind, rounded up to 16 bytes."""
    return ((Ttot + C - 1 + k.WS_CG + 4) * 4 + 15) & ~15


def stats_workspace(k, Ttot, M, C):
    return stats_count_bytes(k, Ttot, C) + row_chunks(k, Ttot) * STATS_SLABS * C * plane_stride(M) * 8


def stats_indexed_workspace(k, S, M, C):
    return wsi_chunks(k, S) * STATS_SLABS * C * plane_stride(M) * 8


def drop_blocks(k, B, D):
    return -(-(B * D) // k.WD_T)


# --------------------------------------------------------------------------------------------------------------------- inputs

def rng(case_id):
    return np.random.RandomState(zlib.crc32(case_id.encode()) & 0x7FFFFFFF)


def series_planes(rs, Ttot, M, integers=False, const_vertex=None):
    """A staged series [Ttot, Mp] whose pad lanes hold NaN; ``integers``: values in [-8, 8]; ``const_vertex``: constant in time."""
    planes = np.full((Ttot, plane_stride(M)), NAN, np.float32)
    if integers:
        planes[:, :M] = rs.randint(-8, 9, size=(Ttot, M)).astype(np.float32)
    else:
        planes[:, :M] = (rs.randn(Ttot, M) * (1 + rs.rand(M)) + rs.randn(M)).astype(np.float32)
    if const_vertex is not None:
        planes[:, const_vertex] = planes[0, const_vertex]
    return planes


def tables(rs, C, M):
    Mp = plane_stride(M)
    scale, shift = np.full((C, Mp), NAN, np.float32), np.full((C, Mp), NAN, np.float32)
    scale[:, :M], shift[:, :M] = rs.rand(C, M) + 0.5, rs.randn(C, M)
    return scale, shift


def edge_rows(rs, n, last):
    """n window starts: 0, the last valid row, values outside [0, last] on both sides, the rest drawn from [0, last]."""
    rows = rs.randint(0, last + 1, size=n).astype(np.int64)
    for i, v in enumerate((last, 0, -1, last + 1, -2 ** 40, 2 ** 62, last, last)[:n]):
        rows[i] = v
    return rows


def sample_with_repeats(rs, S, B):
    """B indices into [0, S): a permutation with repeats that names the first and the last window."""
    pick = rs.randint(0, S, size=B).astype(np.int32)
    pick[0], pick[-1] = S - 1, 0
    if B > 2:
        pick[1] = pick[0]
    return pick


def clamp(v, lo, hi):
    return np.minimum(np.maximum(np.asarray(v, np.int64), lo), hi)


# ------------------------------------------------------------------------------------------------------------------ references

def apply_tables(x, scale, shift, M):
    """A rounded product, then a rounded sum (float32 NumPy), and the zero pad."""
    if scale is not None:
        x = ((x * scale[None]).astype(np.float32) + shift[None]).astype(np.float32)
    x = np.array(x, np.float32)
    x[..., M:] = 0
    return x


def mean32(terms):
    """float32 adds in ascending order, then ONE rounded division -- and only where there is more than one term."""
    acc = terms[0].astype(np.float32)
    for t in terms[1:]:
        acc = (acc + t).astype(np.float32)
    return (acc / np.float32(len(terms))).astype(np.float32) if len(terms) > 1 else acc


def folded_pieces(planes, idx, C, fold):
    """piece(s)[c][m] of every window of ``idx`` [S, C * fold], rows clamped into the series: [S, C, Mp] float32."""
    idx = clamp(idx, 0, planes.shape[0] - 1)
    return mean32([planes[idx[:, f * C:(f + 1) * C]] for f in range(fold)])


def gather_ref(s, inp):
    """The output [B, C, Mp] of the gather case of shape ``s`` on the inputs ``inp``."""
    planes, C, Ttot = inp['planes'], s.C, s.Ttot
    who = np.arange(s.B) if inp.get('sample') is None else inp['sample'].astype(np.int64)
    ch = np.arange(C)
    if s.kind == 'plain':
        x = planes[clamp(inp['rows'][who], 0, Ttot - C)[:, None] + ch[None, :]]
    elif s.kind == 'reflect':
        r = np.zeros(len(who), np.int64) if inp.get('tshift') is None else clamp(inp['tshift'][who], 0, C - 1)
        x = planes[clamp(inp['rows'][who], 0, Ttot - C)[:, None] + series.reflect_channels(C, r)]
    elif s.kind == 'mix':
        x = np.empty((s.B, C, planes.shape[1]), np.float32)
        for b, w in enumerate(who):
            n = int(clamp(inp['cnt'][w], 1, s.smax))
            x[b] = mean32([planes[int(clamp(inp['rows'][w, j], 0, Ttot - C)) + ch] for j in range(n)])
    else:
        piece = folded_pieces(planes, inp['idx'], C, s.fold)
        S = piece.shape[0]
        x = np.empty((s.B, C, planes.shape[1]), np.float32)
        for b, w in enumerate(who):
            if inp.get('src') is None:
                x[b] = piece[int(clamp(w, 0, S - 1))]
            else:
                w = int(clamp(w, 0, inp['src'].shape[0] - 1))
                n = int(clamp(inp['cnt'][w], 1, s.smax))
                x[b] = mean32([piece[int(clamp(inp['src'][w, j], 0, S - 1))] for j in range(n)])
    assert x.dtype == np.float32
    return apply_tables(x, inp.get('scale'), inp.get('shift'), s.M)


def gather_mean64(s, inp):
    """What ``gather_ref`` approximates, in float64, before the tables: (mean [B, C, M], max|source| [B, C, M], terms per mean)."""
    assert s.kind in ('mix', 'indexed') and inp.get('sample') is None
    planes, C, Ttot, ch = inp['planes'][:, :s.M].astype(np.float64), s.C, s.Ttot, np.arange(s.C)
    means, tops, terms = [], [], 1
    for w in range(s.B):
        if s.kind == 'mix':
            n = int(clamp(inp['cnt'][w], 1, s.smax))
            src = np.stack([planes[int(clamp(inp['rows'][w, j], 0, Ttot - C)) + ch] for j in range(n)])
        else:
            idx = clamp(inp['idx'], 0, Ttot - 1)
            if inp.get('src') is None:
                wins = [w]
            else:
                wins = [int(clamp(inp['src'][w, j], 0, idx.shape[0] - 1)) for j in range(int(clamp(inp['cnt'][w], 1, s.smax)))]
            src = np.stack([planes[idx[v, f * C:(f + 1) * C]] for v in wins for f in range(s.fold)])
        means.append(src.mean(axis=0))
        tops.append(np.abs(src).max(axis=0))
        terms = max(terms, src.shape[0])
    return np.stack(means), np.stack(tops), terms


def drop_ref(s, inp):
    """x after the drop and the mask of the elements it writes ([B, C, Mp] each)."""
    want, written = inp['x0'].copy(), np.zeros(inp['x0'].shape, bool)
    if s.B == 0 or s.D == 0:
        return want, written
    v = series.drop_vertices(s.seed, s.refill, inp['win'].astype(np.int64), s.D, s.M)                 # [B, D]
    p = v if inp.get('pos') is None else clamp(inp['pos'][v], 0, s.M - 1)
    for b in range(s.B):
        if inp.get('scale') is None:
            want[b][:, p[b]] = np.float32(s.drop_value)
        else:
            want[b][:, p[b]] = ((np.float32(s.drop_value) * inp['scale'][:, p[b]]).astype(np.float32) + inp['shift'][:, p[b]]).astype(np.float32)
        written[b][:, p[b]] = True
    return want, written


def stats_bound(x):
    """The bounds of test_window_stats_against_float64_and_sklearn (tests/test_gpu_fit_series.py), for windows x [S, C, M]
    float64: two orderings of a float64 sum of S terms differ by at most S 2^-52 sum|x|."""
    u = 2.0 ** -52
    sum_abs, sum_sq = np.abs(x).sum(axis=0), (x * x).sum(axis=0)
    ref_mean, ref_m2 = x.mean(axis=0), (x * x).mean(axis=0)
    b_mean = u * sum_abs
    b_var = u * sum_sq + 2 * np.abs(ref_mean) * b_mean + 4 * (u / 2) * (ref_m2 + ref_mean ** 2)
    return ref_mean, x.var(axis=0), b_mean, b_var


def stats_windows(s, inp):
    """The windows the statistics run over, as the gather forms them: [S, C, M] float64."""
    if s.kind == 'stats':
        x = inp['planes'][clamp(inp['rows'], 0, s.Ttot - s.C)[:, None] + np.arange(s.C)[None, :]]
    else:
        x = folded_pieces(inp['planes'], inp['idx'], s.C, s.fold)
    assert x.dtype == np.float32
    return x[..., :s.M].astype(np.float64)


def stats_ref(s, inp):
    return dict(zip(('mean', 'var', 'b_mean', 'b_var'), stats_bound(stats_windows(s, inp))))


def exact_in_fractions(x, ref):
    """True where the float64 ``ref`` mean and variance of the windows ``x`` [S, C, M] (multiples of 1/16) are the exact rationals."""
    xi = np.round(x * 16).astype(np.int64)
    assert np.array_equal(xi / 16.0, x)
    S = x.shape[0]
    s1, s2 = xi.sum(axis=0), (xi * xi).sum(axis=0)
    for i in np.ndindex(*s1.shape):
        a, q = int(s1[i]), int(s2[i])
        if fractions.Fraction(float(ref['mean'][i])) != fractions.Fraction(a, 16 * S):
            return False
        if fractions.Fraction(float(ref['var'][i])) != fractions.Fraction(S * q - a * a, 256 * S * S):
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------ comparisons

def check_bits(what, got, ref):
    """Bit for bit (a NaN equals the same NaN)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, got.dtype, ref.shape, ref.dtype)
    bad = gb.bits(got) != gb.bits(ref)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements differ from the reference, the first at %s: got %r, reference %r' % (
            what, int(bad.sum()), bad.size, list(at), got[at], ref[at]))


def check_stats(what, s, got, ref):
    """The comparison of both statistics entries: ``got`` {mean, var, scale, shift} [C, Mp] against ``ref`` (``stats_ref``).
    Returns the worst ``err / bound`` of (mean, var)."""
    M = s.M
    for k in ('mean', 'var', 'scale', 'shift'):
        assert not gb.bits(got[k][:, M:]).any(), '%s: the pad of %s is not zero' % (what, k)
    mean, var = got['mean'][:, :M], got['var'][:, :M]
    ratios = []
    for name, g in (('mean', mean), ('var', var)):
        err, bound = np.abs(g - ref[name]), ref['b_' + name]
        assert (err <= bound).all(), '%s: %s beyond the bound of test_gpu_fit_series at %d of %d entries' % (
            what, name, int((~(err <= bound)).sum()), err.size)
        ratios.append(float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0))))
    if s.leg == 'exact':
        check_bits(what + ' mean (exact leg)', mean, ref['mean'])
        check_bits(what + ' var (exact leg)', var, ref['var'])
    # the float32 tables are the float64 results rounded once (include/chebgcn.h): exactly, from the device's own float64
    zero = var == 0
    sd = np.sqrt(np.where(zero, 1.0, var))
    check_bits(what + ' scale', got['scale'][:, :M], np.where(zero, 1.0, 1.0 / sd).astype(np.float32))
    check_bits(what + ' shift', got['shift'][:, :M], np.where(zero, -mean, -mean / sd).astype(np.float32))
    if s.const_vertex is not None:
        v = s.const_vertex
        assert not gb.bits(var[:, v]).any(), '%s: the variance of the constant vertex is not exactly 0' % what
        check_bits(what + ' scale of the constant vertex', got['scale'][:, v], np.ones(s.C, np.float32))
        check_bits(what + ' shift of the constant vertex', got['shift'][:, v], (-mean[:, v]).astype(np.float32))
    return tuple(ratios)


# ----------------------------------------------------------------------------------------------------------------------- cases

class Case:
    """``id``; ``entry``: the chebgcn_* symbol; ``shape``: its integer arguments and the case's kind by name; ``built()`` -> a
    namespace, made once on the host and left unchanged: ``inp`` {name: host array or None} and ``ref``."""

    def __init__(self, id, entry, make, **shape):
        self.id, self.entry, self._make, self._built = id, 'chebgcn_' + entry, make, None
        self.shape = types.SimpleNamespace(**shape)

    def built(self):
        if self._built is None:
            self._built = self._make(self)
        return self._built

    def __repr__(self):
        return self.id


M_SWEEP, C_AT_M = (1, 5, 30, 31, 33, 64), 3
C_SWEEP, M_AT_C = (1, 127, 128, 129, 257), 30           # Mp = 32: 8, 1016, 1024, 1032 and 2056 pieces
WINDOWS = 9
MIX_PASS_C = (161, 225)                                  # a full block, then a block that ends inside pass 1 / inside the last pass
MIX_BOUNDARY_C, MIX_BOUNDARY_N = (32, 64, 96), (4, 8, 16)   # 256, 512, 768 pieces: windows that end on a pass boundary
SWEEP_SMAX, SWEEP_COUNTS = 3, (3, 1, 2, 0, -3, 8, INT32_MAX, INT32_MIN, 2)
REFLECT_C = (1, 2, 15)
INDEXED_C = {True: 225, False: 129}                      # specialised bodies: every pass live; the generic loop: two blocks


def _make_gather(c):
    s, rs = c.shape, rng(c.id)
    C, M, Ttot, S = s.C, s.M, s.Ttot, s.S
    inp = {'planes': series_planes(rs, Ttot, M), 'scale': None, 'shift': None, 'sample': None}
    if s.tables:
        inp['scale'], inp['shift'] = tables(rs, C, M)
    nwin = S
    if s.kind in ('plain', 'reflect'):
        inp['rows'] = edge_rows(rs, S, Ttot - C)
        if s.kind == 'reflect':
            shifts = rs.randint(0, C, size=S).astype(np.int64)
            for i, v in enumerate((0, 1, C - 1, -1, C, INT32_MAX, INT32_MIN)[:S]):
                shifts[i] = v
            inp['tshift'] = None if s.tshift_null else shifts.astype(np.int32)
    elif s.kind == 'mix':
        rows = np.stack([rs.permutation(Ttot - C + 1)[:s.smax] for _ in range(S)]).astype(np.int64)     # distinct rows per window
        rows.reshape(-1)[:8] = edge_rows(rs, 8, Ttot - C)[:min(8, rows.size)]
        inp['rows'], inp['cnt'] = rows, np.asarray(s.counts, np.int32)
        assert inp['cnt'].shape == (S,)
    else:
        idx = rs.randint(0, Ttot, size=(S, C * s.fold)).astype(np.int64)
        idx[0] = idx[0, 0]                                                              # rows that repeat
        if S > 1:
            idx[1] = (Ttot - 1 - np.arange(C * s.fold)) % Ttot                          # ... decrease
        if S > 2:
            idx[2, ::2], idx[2, 1::2] = 0, Ttot - 1                                     # ... and jump
            idx[2].reshape(-1)[:4] = (-1, Ttot, -2 ** 40, 2 ** 62)[:min(4, C * s.fold)]
        inp['idx'] = idx
        if s.src:
            nwin = s.W
            src = rs.randint(0, S, size=(nwin, s.smax)).astype(np.int64)
            src[-1].reshape(-1)[:3] = (-1, S, 2 ** 33)[:min(3, s.smax)]
            inp['src'], inp['cnt'] = src, np.asarray(s.counts, np.int32)
            assert inp['cnt'].shape == (nwin,)
    if s.sample:
        inp['sample'] = sample_with_repeats(rs, nwin, s.B)
        if s.kind == 'indexed' and s.B > 4:                                             # the one gather whose header clamps it
            inp['sample'][2:5] = (-1, nwin, INT32_MAX)
    else:
        assert s.B == nwin, 'the identity sample gathers every window'
    return types.SimpleNamespace(inp=inp, ref=gather_ref(s, inp))


def _gather(id, kind, M, C, tables, sample, S=WINDOWS, B=None, **kw):
    entry = {'plain': 'gather_windows', 'mix': 'gather_windows_mix', 'indexed': 'gather_windows_indexed',
             'reflect': 'gather_windows_reflect'}[kind]
    nwin = kw.get('W', S) if kw.get('src') else S
    return Case('%s-%s' % (id, 'tables' if tables else 'plain'), entry, _make_gather, kind=kind, M=M, C=C, Ttot=C + (40 if kind == 'mix' else 7), S=S,
                B=(WINDOWS if sample else nwin) if B is None else B, tables=tables, sample=sample, **kw)


def _gather_cases():
    cases = []
    for t in (False, True):
        for kind, kw in (('plain', {}), ('reflect', dict(tshift_null=False)), ('mix', dict(smax=SWEEP_SMAX, counts=SWEEP_COUNTS)),
                         ('indexed', dict(fold=1, n=1, src=False, smax=1))):
            for M in M_SWEEP:
                cases.append(_gather('%s-M%d-C%d' % (kind, M, C_AT_M), kind, M, C_AT_M, t, True, **kw))
            for C in C_SWEEP:
                cases.append(_gather('%s-M%d-C%d' % (kind, M_AT_C, C), kind, M_AT_C, C, t, False, **kw))
        # reflect: shifts 0, 1, C - 1 and clamped ones at C = 1, 2 and 15; no shift table at all
        for C in REFLECT_C:
            cases.append(_gather('reflect-shifts-C%d' % C, 'reflect', 33, C, t, False, S=7, tshift_null=False))
        cases.append(_gather('reflect-null-shifts', 'reflect', 33, 15, t, True, tshift_null=True))
        # mix: every N, every pass of every width live and a partial last pass; windows that end on a pass boundary
        for N in range(1, K.GWM_MAX + 1):
            for C in MIX_PASS_C:
                cases.append(_gather('mix-N%d-C%d' % (N, C), 'mix', M_AT_C, C, t, False, S=2, smax=K.GWM_MAX, counts=(N, N)))
        for N in MIX_BOUNDARY_N:
            for C in MIX_BOUNDARY_C:
                cases.append(_gather('mix-N%d-C%d' % (N, C), 'mix', M_AT_C, C, t, False, S=2, smax=K.GWM_MAX, counts=(N, N)))
        # indexed: every specialised body and the generic loop next to each; n = 1 with sources and without
        for fold, n in SPECIALISED + GENERIC_NEIGHBOURS:
            C = INDEXED_C[(fold, n) in SPECIALISED]
            cases.append(_gather('indexed-fold%d-n%d-src' % (fold, n), 'indexed', M_AT_C, C, t, True, S=5, B=5, W=3, fold=fold, n=n,
                                 src=True, smax=n, counts=(n, n, n + 9)))
            if n == 1:
                cases.append(_gather('indexed-fold%d-n1-nosrc' % fold, 'indexed', M_AT_C, C, t, False, S=3, fold=fold, n=1, src=False,
                                     smax=1))
    return cases


GATHERS = _gather_cases()

DROP_BD = ((1, 1), (5, 51), (8, 32), (1, 257))          # B * D = 1, 255, 256, 257
DROP_POS = ('null', 'perm', 'edge')


def _make_drop(c):
    s, rs = c.shape, rng(c.id)
    Mp = plane_stride(s.M)
    inp = {'x0': rs.randn(s.B, s.C, Mp).astype(np.float32),                              # the buffer holds data, pad included
           'win': np.concatenate([[0, INT32_MAX - 1, 77], rs.randint(0, 2 ** 20, size=s.B)])[:s.B].astype(np.int32),
           'pos': None, 'scale': None, 'shift': None}
    if s.pos != 'null':
        inp['pos'] = rs.permutation(s.M).astype(np.int32)
        if s.pos == 'edge':
            inp['pos'][::3] = np.resize(np.array([-1, s.M, INT32_MAX, INT32_MIN], np.int32), inp['pos'][::3].shape)
    if s.tables:
        inp['scale'], inp['shift'] = tables(rs, s.C, s.M)
    want, written = drop_ref(s, inp)
    return types.SimpleNamespace(inp=inp, ref=want, written=written)


def _drop_cases():
    cases = []
    for t in (False, True):
        for pos in DROP_POS:
            for B, D in DROP_BD:
                cases.append(Case('drop-B%d-D%d-%s-%s' % (B, D, pos, 'tables' if t else 'plain'), 'window_drop', _make_drop, kind='drop',
                                  B=B, D=D, M=33, C=2, pos=pos, tables=t, seed=0x9E3779B1, refill=4, drop_value=0.25))
            cases.append(Case('drop-M1-%s-%s' % (pos, 'tables' if t else 'plain'), 'window_drop', _make_drop, kind='drop', B=3, D=4,
                              M=1, C=3, pos=pos, tables=t, seed=12345, refill=0, drop_value=-1.5))
    return cases


DROPS = _drop_cases()

STATS_C = (1, 7, 8, 9, 16, 17)
STATS_T = ('C', 511, 512, 513, 514, 1024, 1025, 1027)
STATS_M = ((1, 9, 513), (512, 8, 514), (513, 17, 1027), (513, 1, 512))          # (M, C, Ttot): one vertex, one vertex tile, one past it
STATS_S = {'bounded': 37, 'exact': 32}
LEGS = ('bounded', 'exact')


def stats_rows(k, rs, Ttot, C, S, special=None):
    """S window starts: 0, the last one, one across and one on either side of every chunk boundary, repeated starts, starts outside
    [0, Ttot - C] on both sides; ``special``: 'equal' -- every window on one start."""
    last = Ttot - C
    if special == 'equal':
        return np.full(S, last // 2, np.int64)
    rows = rs.randint(0, last + 1, size=S).astype(np.int64)
    must = [0, last]
    for b in range(k.WS_ROWS, Ttot, k.WS_ROWS):
        must += [min(last, max(0, b - C // 2)), min(last, b - 1), min(last, b)]
    must += [must[-1], must[-1], -1, last + 1]
    if S >= len(must):
        rows[:len(must)] = must
    return rows


def _make_stats(c):
    s, rs = c.shape, rng(c.id)
    inp = {'planes': series_planes(rs, s.Ttot, s.M, integers=s.leg == 'exact', const_vertex=s.const_vertex)}
    if s.kind == 'stats':
        inp['rows'] = stats_rows(K, rs, s.Ttot, s.C, s.S, s.special)
    else:
        idx = rs.randint(0, s.Ttot, size=(s.S, s.C * s.fold)).astype(np.int64)
        idx[0, 0], idx[-1, -1] = 0, s.Ttot - 1
        if s.S > 2:
            idx[1].reshape(-1)[:2] = (-1, s.Ttot + 5)[:min(2, idx.shape[1])]
        inp['idx'] = idx
    return types.SimpleNamespace(inp=inp, ref=stats_ref(s, inp))


def _stats_case(leg, M, C, Ttot, S=None, special=None):
    T = C if Ttot == 'C' else Ttot
    S = (1 if T == C else STATS_S[leg]) if S is None else S
    id = 'stats-%s-M%d-C%d-T%s%s' % (leg, M, C, Ttot, '' if special is None else '-' + special)
    return Case(id, 'window_stats', _make_stats, kind='stats', leg=leg, M=M, C=C, Ttot=T, S=S, special=special,
                const_vertex=min(2, M - 1) if M > 1 else None)


STATS_INDEXED_S = (1, 15, 16, 17, 33, 512, 513, 545, 608)
STATS_INDEXED_FOLD = (1, 2, 3, 16)
STATS_INDEXED_C = (1, 3)
STATS_INDEXED_EXACT_S, STATS_INDEXED_EXACT_FOLD = (1, 16, 512), (1, 2, 16)


def _stats_cases():
    cases = []
    for leg in LEGS:
        for C in STATS_C:
            for T in STATS_T:
                cases.append(_stats_case(leg, 33, C, T))
        for M, C, T in STATS_M:
            cases.append(_stats_case(leg, M, C, T))
        cases.append(_stats_case(leg, 33, 9, 1027, S=16, special='equal'))
        cases.append(_stats_case(leg, 33, 9, 1027, S=1, special='one'))
        for S in STATS_INDEXED_S if leg == 'bounded' else STATS_INDEXED_EXACT_S:
            for fold in STATS_INDEXED_FOLD if leg == 'bounded' else STATS_INDEXED_EXACT_FOLD:
                for C in STATS_INDEXED_C:
                    cases.append(Case('stats_indexed-%s-S%d-fold%d-C%d' % (leg, S, fold, C), 'window_stats_indexed', _make_stats,
                                      kind='stats_indexed', leg=leg, M=33, C=C, Ttot=40, S=S, fold=fold, const_vertex=2))
    return cases


STATS = _stats_cases()
ALL = GATHERS + DROPS + STATS
ENTRIES = ('chebgcn_gather_windows', 'chebgcn_gather_windows_mix', 'chebgcn_gather_windows_indexed', 'chebgcn_gather_windows_reflect',
           'chebgcn_window_drop', 'chebgcn_window_stats', 'chebgcn_window_stats_indexed')


def of(entry, table=None):
    return [c for c in (ALL if table is None else table) if c.entry == 'chebgcn_' + entry]


def dispatch_name(c):
    """What chebgcn_last_dispatch() holds after the case's launch."""
    arm = '<tables>' if getattr(c.shape, 'tables', False) else '<plain>'
    return {'chebgcn_gather_windows': 'gather_windows_kernel' + arm, 'chebgcn_gather_windows_mix': 'gather_windows_mix_kernel' + arm,
            'chebgcn_gather_windows_indexed': 'gather_windows_indexed_kernel' + arm,
            'chebgcn_gather_windows_reflect': 'gather_windows_reflect_kernel' + arm, 'chebgcn_window_drop': 'window_drop_kernel' + arm,
            'chebgcn_window_stats': 'window_count_kernel + window_stats_partial_kernel + window_stats_finish_kernel',
            'chebgcn_window_stats_indexed': 'window_stats_indexed_partial_kernel + window_stats_finish_kernel'}[c.entry]
