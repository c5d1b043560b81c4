"""Buffer discipline of the analysis entry points of include/chebgcn.h, each called through ctypes with the argument list its
``ops`` wrapper uses, every output and every workspace a ``guarded_buffers.Guarded`` region at the weakest alignment the entry's
own argument check admits, the workspace EXACTLY the bytes its query promises (``searchlight_score``: the wrapper's formula,
restated here), never the cached one.  Per case:

  1. two runs into fresh regions, poison A (bytes 0xFF) then poison B (bytes 0x5A) in every output and workspace;
  2. after each run every guard band is intact and every input is byte-identical to its copy from before the call;
  3. the written part of every output is bit-identical between the runs and to what the public wrapper returns;
  4. the rest of every output holds what the header says, element by element: the fill it had ("untouched"), zero where the
     header promises zero, and nothing is asserted only where the header calls a region scratch; an output the call adds into
     starts from a non-zero base (7) and comes back as base + the wrapper's result on zeros;
  5. the wrapper's result against the family's host restatement, with that family's existing bound.

Inputs the header says are never read as data (the pad [M, Mp) of input planes, the pad columns of ``Xt``) are NaN.

The case table (``CASES``) is built on the host without a GPU: tests/test_analysis_buffer_refs.py checks its coverage of the
header, its arm claims, its workspace formulas and its references there.  Tile constants come from the libraries' geometry
queries, or -- where an entry has no query (series.hip) -- from the ``constexpr`` lines of its source.

Measured on an MI355X: the 54 cases take 5 s together, the slowest (cheb_filter-rolling-K4, which also creates its graph)
0.9 s.  Each of these changes to the library, built apart and never committed, fails cases here by name: the
chebgcn_window_stats_workspace query 16 bytes short ("guard changed", window_stats), the counts of window_stats not zeroed
("runs A/B differ"), finish_piece not zeroing the pad ("pad not zero", all 19 gather cases), sl_tally storing instead of adding
("base not kept", the LDA and SVM cases; "runs A/B differ", the naive-Bayes case).
"""
import ctypes
import types

import numpy as np
import pytest

from conftest import ROOT
from gcn_fmri_decoding_amd import _lib, series
from gcn_fmri_decoding_amd._lib import plane_stride

import guarded_buffers as gb
from window_kernel_cases import source_constant, stats_bound as _stats_bound        # (shared with tests/test_gpu_window_kernels.py)

pytestmark = pytest.mark.gpu

BASE = 7                                # what an added-into count holds before the call
WRITTEN, UNTOUCHED, ZERO, SCRATCH = 1, 0, 2, 3
NAN = np.float32(np.nan)


class Out:
    """One output pointer of a case: ``kind`` int8 array of ``shape`` (WRITTEN / UNTOUCHED / ZERO / SCRATCH per element, from the
    header); ``init``: host data the buffer holds before the call (in-place entries), ``base``: the scalar an accumulated-into
    buffer starts from, with ``accum`` 'add' or 'max'; ``wrap``: the key of the wrapper's result it is compared with."""

    def __init__(self, name, dtype, shape, align, kind=None, init=None, base=None, accum=None, wrap=None):
        self.name, self.dtype, self.shape, self.align = name, dtype, tuple(int(s) for s in shape), align
        self.kind = np.full(self.shape, WRITTEN, np.int8) if kind is None else np.broadcast_to(np.asarray(kind, np.int8), self.shape)
        self.init, self.base, self.accum, self.wrap = init, base, accum, name if wrap is None else wrap


def pad_kind(shape, M, pad):
    """WRITTEN on the vertices [0, M) of the last axis, ``pad`` on [M, Mp)."""
    k = np.full(shape, WRITTEN, np.int8)
    k[..., M:] = pad
    return k


class Case:
    """``id``; ``entries``: the chebgcn_* symbols it calls into guarded regions; ``make()`` -> a namespace, built once on the
    host:  inp {name: host array or None};  outs [Out];  ws {name: exact bytes (0: a NULL workspace)};  ws_formula {name: the
    header's formula restated, or None where the header gives none};  arms [(claim, reached)];  call(lib, d, o, w, stream) with
    d / o / w the device inputs, the output regions and the workspace regions by name (it raises on a refused call);
    wrapper(d) -> {name: device tensor};  reference(inp) -> {name: host float64 / exact reference on the defined region};
    compare(got, ref) asserts the family's bound."""

    def __init__(self, id, entries, make):
        self.id, self.entries, self._make, self._built = id, tuple(entries), make, None

    def built(self):
        if self._built is None:
            self._built = self._make()
        return self._built


CASES = []


def case(id, *entries):
    def deco(make):
        CASES.append(Case(id, entries, make))
        return make
    return deco


def P(r):
    """The ctypes pointer of a tensor, a Guarded region or None."""
    if r is None:
        return None
    return r.ptr if isinstance(r, gb.Guarded) else ctypes.c_void_p(r.data_ptr())


def ok(rc, what):
    _lib.check(rc, what)


def lib():
    return _lib.lib()


# ===================================================================================================== series.hip, augment.hip

def _series_planes(rs, Ttot, M):
    """A staged series whose pad lanes hold NaN (never read as data)."""
    Mp = plane_stride(M)
    planes = np.full((Ttot, Mp), NAN, np.float32)
    planes[:, :M] = (rs.randn(Ttot, M) * (1 + rs.rand(M)) + rs.randn(M)).astype(np.float32)
    return planes


def _tables(rs, C, M):
    Mp = plane_stride(M)
    scale, shift = np.full((C, Mp), NAN, np.float32), np.full((C, Mp), NAN, np.float32)
    scale[:, :M], shift[:, :M] = rs.rand(C, M) + 0.5, rs.randn(C, M)
    return scale, shift


def _apply_tables(x, scale, shift):
    """A rounded product, then a rounded sum (float32 NumPy), and the zero pad the header promises."""
    if scale is not None:
        x = (x * scale[None]).astype(np.float32) + shift[None]
    return x.astype(np.float32)


def _exact(got, ref, what):
    """Bit for bit on the entries the reference defines (a NaN in a float reference: not defined there)."""
    for name, r in ref.items():
        g = np.asarray(got[name])
        live = ~np.isnan(r) if r.dtype.kind == 'f' else np.ones(r.shape, bool)
        bad = live & (gb.bits(g) != gb.bits(r.astype(g.dtype)))
        assert not bad.any(), '%s: %s differs from the host restatement in %d of %d entries, first at %s' % (
            what, name, bad.sum(), live.sum(), tuple(np.argwhere(bad)[0]))


def _gather_case(id, entry, M, C, B, Ttot, tables, sample=True, mix=None, indexed=None, reflect=False):
    """One gather: ``mix`` the source count of every window (gather_windows_mix), ``indexed`` (fold, n) (gather_windows_indexed,
    n > 1: with sources), ``reflect``: time shifts."""
    @case(id, entry)
    def make():
        rs = np.random.RandomState(sum(map(ord, id)))
        Mp = plane_stride(M)
        S = 9
        planes = _series_planes(rs, Ttot, M)
        scale, shift = _tables(rs, C, M) if tables else (None, None)
        pick = rs.randint(0, S, size=B).astype(np.int32) if sample else None
        if pick is not None:
            pick[0], pick[-1] = S - 1, 0
        nwin = S
        inp = dict(planes=planes, scale=scale, shift=shift, sample=pick)
        rows = rs.randint(0, Ttot - C + 1, size=S).astype(np.int64)
        rows[0], rows[1] = Ttot - C, 0
        if mix is not None:
            smax = mix
            inp['rows'] = rs.randint(0, Ttot - C + 1, size=(S, smax)).astype(np.int64)
            inp['cnt'] = np.full(S, mix, np.int32)
            inp['cnt'][1] = 1
        elif indexed is not None:
            fold, n = indexed
            inp['idx'] = rs.randint(0, Ttot, size=(S, C * fold)).astype(np.int64)
            inp['idx'][0] = Ttot - 1
            inp['idx'][1] = 0
            if n > 1:
                nwin = S + 3
                inp['src'] = rs.randint(0, S, size=(nwin, n)).astype(np.int64)
                inp['cnt'] = np.full(nwin, n, np.int32)
                inp['cnt'][2] = 1
                if pick is not None:
                    pick[1] = nwin - 1
        else:
            inp['rows'] = rows
            if reflect:
                inp['tshift'] = rs.randint(0, C, size=S).astype(np.int32)
                inp['tshift'][0], inp['tshift'][1] = C - 1, 0
        Bn = B if sample else nwin
        assert Bn == B, 'the identity sample gathers every window: B must be their number'
        outs = [Out('out', 'float32', (B, C, Mp), 16, pad_kind((B, C, Mp), M, ZERO))]     # "the pad of every output plane is written as 0"

        def call(L, d, o, w, stream):
            g = d.get
            if mix is not None:
                ok(L.chebgcn_gather_windows_mix(P(g('planes')), Ttot, P(g('rows')), P(g('cnt')), smax, P(g('sample')), P(g('scale')),
                                                P(g('shift')), P(o['out']), B, M, C, stream), entry)
            elif indexed is not None:
                src = g('src')
                ok(L.chebgcn_gather_windows_indexed(P(g('planes')), Ttot, P(g('idx')), S, C * fold, fold, P(src), P(g('cnt')) if src is not None
                                                    else None, nwin, n if src is not None else 1, P(g('sample')), P(g('scale')),
                                                    P(g('shift')), P(o['out']), B, M, C, stream), entry)
            elif reflect:
                ok(L.chebgcn_gather_windows_reflect(P(g('planes')), Ttot, P(g('rows')), P(g('tshift')), P(g('sample')), P(g('scale')),
                                                    P(g('shift')), P(o['out']), B, M, C, stream), entry)
            else:
                ok(L.chebgcn_gather_windows(P(g('planes')), Ttot, P(g('rows')), P(g('sample')), P(g('scale')), P(g('shift')),
                                            P(o['out']), B, M, C, stream), entry)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            g = d.get
            if mix is not None:
                out = ops.gather_windows_mix(g('planes'), g('rows'), g('cnt'), M, C, g('sample'), g('scale'), g('shift'))
            elif indexed is not None:
                out = ops.gather_windows_indexed(g('planes'), g('idx'), M, C, fold, g('src'), g('cnt') if g('src') is not None else None,
                                                 g('sample'), g('scale'), g('shift'))
            elif reflect:
                out = ops.gather_windows_reflect(g('planes'), g('rows'), g('tshift'), M, C, g('sample'), g('scale'), g('shift'))
            else:
                out = ops.gather_windows(g('planes'), g('rows'), M, C, g('sample'), g('scale'), g('shift'))
            return {'out': out}

        def reference(inp):
            """The header's definition in float32 NumPy: adds in ascending order, one rounded division per level, the tables
            as two roundings (the restatements of test_gpu_fit_series / test_gpu_balance / test_gpu_events / test_gpu_augment)."""
            who = np.arange(nwin) if pick is None else pick
            win = lambda r: planes[np.asarray(r)[:, None] + np.arange(C)[None, :]]          # [n, C, Mp]
            if mix is not None:
                x = np.empty((B, C, Mp), np.float32)
                for b, wi in enumerate(who):
                    acc = win(inp['rows'][wi, :1])[0]
                    for j in range(1, inp['cnt'][wi]):
                        acc = acc + win(inp['rows'][wi, j:j + 1])[0]
                    x[b] = acc / np.float32(inp['cnt'][wi])
            elif indexed is not None:
                idx = inp['idx']
                piece = planes[idx[:, :C]]
                for f in range(1, fold):
                    piece = piece + planes[idx[:, f * C:(f + 1) * C]]
                if fold > 1:
                    piece = piece / np.float32(fold)
                x = np.empty((B, C, Mp), np.float32)
                for b, wi in enumerate(who):
                    if inp.get('src') is None:
                        x[b] = piece[wi]
                    else:
                        acc = piece[inp['src'][wi, 0]]
                        for j in range(1, inp['cnt'][wi]):
                            acc = acc + piece[inp['src'][wi, j]]
                        x[b] = acc / np.float32(inp['cnt'][wi]) if inp['cnt'][wi] > 1 else acc
            elif reflect:
                x = planes[rows[who][:, None] + series.reflect_channels(C, inp['tshift'][who])]
            else:
                x = win(rows[who])
            assert x.dtype == np.float32
            x = _apply_tables(x, scale, shift)
            x[..., M:] = 0
            return {'out': x}

        CMq = C * Mp // 4
        tile = source_constant('gather_piece.h', 'GW_T') * source_constant('gather_piece.h', 'GW_U')
        arms = [('%s_kernel<%s>' % (entry[len('chebgcn_'):], 'tables' if tables else 'plain'), True)]
        if 'two_blocks' in id:
            arms.append(('a second block along x with a ragged tail', tile < CMq < 2 * tile and CMq % tile != 0))
        else:
            arms.append(('one block along x', CMq <= tile))
            arms.append(('the pad begins inside a 16-byte piece', M % 4 != 0 and Mp > M))
        return types.SimpleNamespace(inp=inp, outs=outs, ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper,
                                     reference=reference, compare=lambda got, ref: _exact(got, ref, id))
    return make


for _t in (False, True):
    _s = '-tables' if _t else '-plain'
    _gather_case('gather_windows' + _s, 'chebgcn_gather_windows', 33, 3, 5, 20, _t)
    _gather_case('gather_windows_reflect' + _s, 'chebgcn_gather_windows_reflect', 33, 3, 5, 20, _t, reflect=True)
    for _n in (1, 3, 9):                                                                  # the three unroll widths
        _gather_case('gather_windows_mix-n%d%s' % (_n, _s), 'chebgcn_gather_windows_mix', 33, 3, 5, 20, _t, mix=_n)
    for _f, _n in ((1, 1), (2, 4), (3, 1), (5, 3)):                                       # (5, 3): the generic loop
        _gather_case('gather_windows_indexed-fold%d-n%d%s' % (_f, _n, _s), 'chebgcn_gather_windows_indexed', 33, 3, 5, 20, _t,
                     indexed=(_f, _n))
_gather_case('gather_windows-two_blocks', 'chebgcn_gather_windows', 360, 11, 2, 20, False)


def _stats_compare(id, M):
    def compare(got, ref):
        mean, var = got['mean'][:, :M], got['var'][:, :M]
        e_mean, e_var = np.abs(mean - ref['mean']), np.abs(var - ref['var'])
        print('%s: mean err / bound %.3g, var err / bound %.3g' % (id, (e_mean / ref['b_mean']).max(), (e_var / ref['b_var']).max()))
        assert (e_mean <= ref['b_mean']).all(), '%s: mean beyond the bound of test_gpu_fit_series' % id
        assert (e_var <= ref['b_var']).all(), '%s: var beyond the bound of test_gpu_fit_series' % id
        # the float32 tables are the float64 results rounded once (include/chebgcn.h): exactly, from the device's own float64
        sd = np.sqrt(var)
        assert (var > 0).all()
        _exact({'scale': got['scale'][:, :M], 'shift': got['shift'][:, :M]},
               {'scale': (1.0 / sd).astype(np.float32), 'shift': (-mean / sd).astype(np.float32)}, id)
    return compare


def _stats_outs(C, M):
    Mp = plane_stride(M)
    k = pad_kind((C, Mp), M, ZERO)                                                          # "the pad of all four is 0"
    return [Out('mean', 'float64', (C, Mp), 8, k), Out('var', 'float64', (C, Mp), 8, k), Out('scale', 'float32', (C, Mp), 4, k),
            Out('shift', 'float32', (C, Mp), 4, k)]


@case('window_stats', 'chebgcn_window_stats')
def _window_stats():
    M, C, S = 33, 9, 200
    rows_chunk, cg = source_constant('series.hip', 'WS_ROWS'), source_constant('series.hip', 'WS_CG')
    Ttot = rows_chunk + 3
    Mp = plane_stride(M)
    rs = np.random.RandomState(41)
    planes = _series_planes(rs, Ttot, M)
    rows = rs.randint(0, Ttot - C + 1, size=S).astype(np.int64)
    rows[:4] = (0, Ttot - C, Ttot - C, 0)
    rows[100:140] = rows[20]                                                                # repeated starts
    nws = int(lib().chebgcn_window_stats_workspace(Ttot, M, C))
    chunks = -(-Ttot // rows_chunk)
    formula = None            # the header gives no formula for this query (its count table has an undocumented lead)

    def call(L, d, o, w, stream):
        ok(L.chebgcn_window_stats(P(d['planes']), Ttot, P(d['rows']), S, P(o['mean']), P(o['var']), P(o['scale']), P(o['shift']), M, C,
                                  P(w['workspace']), nws, stream), 'chebgcn_window_stats')

    def wrapper(d):
        from gcn_fmri_decoding_amd import ops
        return dict(zip(('mean', 'var', 'scale', 'shift'), ops.window_stats(d['planes'], d['rows'], M, C)))

    def reference(inp):
        x = planes[rows[:, None] + np.arange(C)[None, :]][..., :M].astype(np.float64)       # [S, C, M]
        return dict(zip(('mean', 'var', 'b_mean', 'b_var'), _stats_bound(x)))

    arms = [('two channel groups, one channel in the last', -(-C // cg) == 2 and C % cg == 1),
            ('two chunks with a 3-row tail', chunks == 2 and Ttot % rows_chunk == 3)]
    return types.SimpleNamespace(inp=dict(planes=planes, rows=rows), outs=_stats_outs(C, M), ws={'workspace': nws},
                                 ws_formula={'workspace': formula}, arms=arms, call=call, wrapper=wrapper, reference=reference,
                                 compare=_stats_compare('window_stats', M), ws_align={'workspace': 16})


def _stats_indexed_case(fold):
    id = 'window_stats_indexed-fold%d' % fold

    @case(id, 'chebgcn_window_stats_indexed')
    def make():
        M, C, S, Ttot = 33, 3, 35, 40
        Mp = plane_stride(M)
        rs = np.random.RandomState(50 + fold)
        planes = _series_planes(rs, Ttot, M)
        idx = rs.randint(0, Ttot, size=(S, C * fold)).astype(np.int64)
        idx[0], idx[1] = Ttot - 1, 0
        nws = int(lib().chebgcn_window_stats_indexed_workspace(S, M, C))
        chunk = max(16, -(-S // 32))                                                        # "chunks of max(16, ceil(S / 32)) windows"
        chunks = -(-S // chunk)
        formula = chunks * 4 * C * Mp * 8                                                   # a partial per chunk: 4 [C][Mp] doubles

        def call(L, d, o, w, stream):
            ok(L.chebgcn_window_stats_indexed(P(d['planes']), Ttot, P(d['idx']), S, C * fold, fold, P(o['mean']), P(o['var']),
                                              P(o['scale']), P(o['shift']), M, C, P(w['workspace']), nws, stream), id)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            return dict(zip(('mean', 'var', 'scale', 'shift'), ops.window_stats_indexed(d['planes'], d['idx'], M, C, fold)))

        def reference(inp):
            piece = planes[idx[:, :C]]                                                      # as the gather forms them, in float32
            for f in range(1, fold):
                piece = piece + planes[idx[:, f * C:(f + 1) * C]]
            if fold > 1:
                piece = piece / np.float32(fold)
            assert piece.dtype == np.float32
            return dict(zip(('mean', 'var', 'b_mean', 'b_var'), _stats_bound(piece[..., :M].astype(np.float64))))

        arms = [('three chunks with a 3-window tail', chunks == 3 and S - 2 * chunk == 3),
                ('window_stats_indexed_partial_kernel<%d>' % (fold if fold <= 2 else 0), True)]
        return types.SimpleNamespace(inp=dict(planes=planes, idx=idx), outs=_stats_outs(C, M), ws={'workspace': nws},
                                     ws_formula={'workspace': formula}, arms=arms, call=call, wrapper=wrapper, reference=reference,
                                     compare=_stats_compare(id, M), ws_align={'workspace': 16})
    return make


for _f in (1, 2, 3):
    _stats_indexed_case(_f)


def _drop_case(with_pos, tables):
    id = 'window_drop-%s-%s' % ('pos' if with_pos else 'identity', 'tables' if tables else 'plain')

    @case(id, 'chebgcn_window_drop')
    def make():
        B, C, M, D, seed, refill, dv = 3, 2, 33, 5, 0x9E3779B1, 4, 0.25
        Mp = plane_stride(M)
        rs = np.random.RandomState(60 + 2 * with_pos + tables)
        x0 = rs.randn(B, C, Mp).astype(np.float32)                                          # the buffer holds data, pad included
        win = np.array([0, 2 ** 31 - 2, 77], np.int32)
        pos = rs.permutation(M).astype(np.int32) if with_pos else None
        scale, shift = _tables(rs, C, M) if tables else (None, None)
        v = series.drop_vertices(seed, refill, win.astype(np.int64), D, M)                  # [B, D]
        p = pos[v] if with_pos else v
        kind = np.full((B, C, Mp), UNTOUCHED, np.int8)                                      # "Nothing else is written ... the pad included"
        want = x0.copy()
        for b in range(B):
            kind[b][:, p[b]] = WRITTEN
            want[b][:, p[b]] = (np.float32(dv) * scale[:, p[b]]).astype(np.float32) + shift[:, p[b]] if tables else np.float32(dv)
        assert not kind[..., M:].any() and kind.sum() <= B * D * C

        def call(L, d, o, w, stream):
            ok(L.chebgcn_window_drop(P(o['x']), P(d['win']), B, M, C, D, seed, refill, P(d.get('pos')), P(d.get('scale')), P(d.get('shift')),
                                     dv, stream), id)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            import torch
            x = torch.as_tensor(x0).to(d['win'].device)
            return {'x': ops.window_drop(x, d['win'], M, D, seed, refill, d.get('pos'), d.get('scale'), d.get('shift'), dv)}

        arms = [('window_drop_kernel<%s>' % ('tables' if tables else 'plain'), True)]
        return types.SimpleNamespace(inp=dict(win=win, pos=pos, scale=scale, shift=shift), outs=[Out('x', 'float32', (B, C, Mp), 4, kind, init=x0)],
                                     ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper, reference=lambda inp: {'x': want},
                                     compare=lambda got, ref: _exact(got, ref, id))
    return make


for _pos in (False, True):
    for _t in (False, True):
        _drop_case(_pos, _t)


# ===================================================================================================== knn.hip

def _knn_case(N, D, k, metric, arm):
    id = 'knn-%s-%s' % (arm, metric)

    @case(id, 'chebgcn_knn')
    def make():
        import test_gpu_knn as K
        Np = plane_stride(N)
        z = K.features(N, D, seed=N * 7 + D, metric=metric, k=k)
        feat = np.zeros((D, Np), np.float32)                                                # "zero in the pad": the header's contract
        feat[:, :N] = z.T
        nws = int(lib().chebgcn_knn_workspace(N, D, k))
        code = {'euclidean': _lib.KNN_EUCLIDEAN, 'correlation': _lib.KNN_CORRELATION}[metric]

        def call(L, d, o, w, stream):
            ok(L.chebgcn_knn(P(d['feat']), N, D, k, code, P(o['dist']), P(o['idx']), P(w['workspace']), nws, stream), id)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            dist, idx = ops.knn(d['feat'], N, k, code)
            return {'dist': dist, 'idx': idx}

        def reference(inp):
            d64, i64 = K.knn64(z, k, metric)
            return {'d64': d64, 'i64': i64.astype(np.float64)}

        def compare(got, ref):
            """Check 1 and Check 2 of tests/test_gpu_knn.py with their bounds."""
            K.check1(z, metric, k, got['dist'], got['idx'].astype(np.int64), ref['d64'])
            assert K.check2(k, got['idx'].astype(np.int64), ref['d64'], ref['i64'].astype(np.int64)) <= K.CAP

        small, cb = source_constant('knn.hip', 'KNN_DSMALL'), source_constant('knn.hip', 'KNN_CB')
        arms = [('knn_%s_kernel' % arm, (D <= small) == (arm == 'direct'))]
        if arm == 'gram':
            arms.append(('several candidate blocks', N > 2 * cb))
        return types.SimpleNamespace(inp=dict(feat=feat), outs=[Out('dist', 'float32', (N, k), 4), Out('idx', 'int32', (N, k), 4)],
                                     ws={'workspace': nws}, ws_formula={'workspace': None}, arms=arms, call=call, wrapper=wrapper,
                                     reference=reference, compare=compare)
    return make


for _m in ('euclidean', 'correlation'):
    _knn_case(33, 3, 5, _m, 'direct')
    _knn_case(300, 9, 32, _m, 'gram')


@case('series_normalise', 'chebgcn_series_normalise')
def _series_normalise():
    import test_gpu_knn as K
    M, lengths = 33, (1, 5, 9)
    Mp, Ttot, R = plane_stride(M), sum(lengths), len(lengths)
    rs = np.random.RandomState(70)
    planes = _series_planes(rs, Ttot, M)
    planes[1:6, 4] = 1.25                                                                   # constant in the second run: zero there
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)

    def call(L, d, o, w, stream):
        ok(L.chebgcn_series_normalise(P(d['planes']), Ttot, P(d['offs']), R, M, 1.0, P(o['out']), stream), 'series_normalise')

    def wrapper(d):
        from gcn_fmri_decoding_amd import ops
        return {'out': ops.series_normalise(d['planes'], d['offs'], M)}

    def reference(inp):
        with np.errstate(all='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                return {'corr': K._mean_corr64([planes[a:b, :M] for a, b in zip(offs[:-1], offs[1:])])}

    def compare(got, ref):
        """The Gram matrix over t, divided by R, is the mean over runs of the per-run correlation: test_gpu_knn.py's BOUND."""
        zn = got['out'].astype(np.float64)
        assert (zn[0] == 0).all() and (zn[1:6, 4] == 0).all()
        assert np.abs(zn[:, :M].T @ zn[:, :M] / R - ref['corr']).max() <= K.BOUND

    return types.SimpleNamespace(inp=dict(planes=planes, offs=offs), outs=[Out('out', 'float32', (Ttot, Mp), 4, pad_kind((Ttot, Mp), M, ZERO))],
                                 ws={}, ws_formula={}, arms=[('runs of 1, 5 and 9 rows', True)], call=call, wrapper=wrapper,
                                 reference=reference, compare=compare)


# ===================================================================================================== parcellate.hip

def _parcellate_case(weighted):
    id = 'parcellate-%s' % ('weighted' if weighted else 'plain')

    @case(id, 'chebgcn_parcellate')
    def make():
        import test_parcellation_host as H
        from gcn_fmri_decoding_amd import Parcellation
        V, R, T = 63, 5, 3
        geo = lib().chebgcn_parcellate_query
        lab = H.make_labels(V, R, chunk=geo(0))
        wts = H.make_weights(lab) if weighted else None
        Pc = Parcellation(lab, weights=wts)
        x = H.make_series(T, V)
        ldx, ldo = V + 3, Pc.R + 5
        xbig = np.full((T, ldx), NAN, np.float32)                                           # ldx > V: columns of a wider tensor
        xbig[:, 1:V + 1] = x
        kind = np.full((T, ldo), UNTOUCHED, np.int8)                                        # ldo > R: the other columns are not out's
        kind[:, :Pc.R] = WRITTEN
        kind = kind.reshape(-1)[:(T - 1) * ldo + Pc.R]
        n_out = kind.size
        inp = dict(x=xbig, ptr=Pc.ptr, idx=Pc.idx, w=Pc.weights if weighted else None)

        def call(L, d, o, w, stream):
            xd = ctypes.c_void_p(d['x'].data_ptr() + 4)
            ok(L.chebgcn_parcellate(xd, ldx, P(d['ptr']), P(d['idx']), int(Pc.idx.size), P(d.get('w')), P(o['out']), ldo, T, V, Pc.R,
                                    _lib.PARCEL_MEAN, stream), id)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            import torch
            obig = torch.zeros((T, ldo), device=d['x'].device)
            ops.parcellate(d['x'][:, 1:V + 1], d['ptr'], d['idx'], Pc.R, w=d.get('w'), out=obig[:, :Pc.R])
            return {'out': obig.reshape(-1)[:n_out]}

        def reference(inp):
            return {'twin': Pc.reduce_host(x), 'ref64': H.ref64(lab, x, wts), 'bound': H.bound(lab, x, wts)}

        def compare(got, ref):
            a = np.concatenate([got['out'], np.zeros(T * ldo - n_out, np.float32)]).reshape(T, ldo)[:, :Pc.R]
            assert np.array_equal(gb.bits(a), gb.bits(ref['twin'])), '%s: differs from Parcellation.reduce_host' % id
            assert (np.abs(a.astype(np.float64) - ref['ref64']) <= ref['bound']).all(), '%s: beyond test_parcellation_host.bound' % id

        arms = [('parcellate_kernel<rows1, %s>' % ('weighted' if weighted else 'plain'), T < geo(2)), ('ldx > V and ldo > R', True)]
        return types.SimpleNamespace(inp=inp, outs=[Out('out', 'float32', (n_out,), 4, kind)], ws={}, ws_formula={}, arms=arms, call=call,
                                     wrapper=wrapper, reference=reference, compare=compare)
    return make


_parcellate_case(False)
_parcellate_case(True)


@case('parcel_expand', 'chebgcn_parcel_expand')
def _parcel_expand():
    import test_parcellation_host as H
    from gcn_fmri_decoding_amd import Parcellation
    geo = lib().chebgcn_parcellate_query
    per_block = geo(6) * source_constant('parcellate.hip', 'PE_T')                          # vertices of one expand workgroup
    V, B, fill = per_block + 2, 3, -2.5
    Pc = Parcellation(H.make_labels(V, 40, chunk=512))
    maps = np.random.RandomState(V + B).randn(B, Pc.R).astype(np.float32)

    def call(L, d, o, w, stream):
        ok(L.chebgcn_parcel_expand(P(d['maps']), P(d['region_of']), P(o['out']), B, Pc.R, V, fill, stream), 'parcel_expand')

    def wrapper(d):
        from gcn_fmri_decoding_amd import ops
        return {'out': ops.parcel_expand(d['maps'], d['region_of'], fill)}

    def reference(inp):
        return {'out': np.where(Pc.region_of[None, :] >= 0, maps[:, np.maximum(Pc.region_of, 0)], np.float32(fill)).astype(np.float32)}

    arms = [('a second block with a ragged 2-vertex tail', per_block < V < 2 * per_block and V % geo(6) == 2)]
    return types.SimpleNamespace(inp=dict(maps=maps, region_of=Pc.region_of), outs=[Out('out', 'float32', (B, V), 4)], ws={}, ws_formula={},
                                 arms=arms, call=call, wrapper=wrapper, reference=reference,
                                 compare=lambda got, ref: _exact(got, ref, 'parcel_expand'))


# ===================================================================================================== searchlight*.hip

def _sl_problem(seed=5):
    """The shared searchlight shape: S = 24 samples of M = 40 vertices, C = 3 classes, two test folds of 11 samples and two
    samples that train but are in no test fold of the launch (their rows of ``scores`` / ``predictions`` must stay untouched),
    rows of 1, 17 and 40 vertices (U = 3), a launch over the centres [1, 3) only."""
    import scipy.sparse as sp
    from gcn_fmri_decoding_amd import searchlight as sl
    S, M, C = 24, 40, 3
    rs = np.random.RandomState(seed)
    y = np.arange(S) % C
    fold = np.array([0] * 11 + [1] * 11 + [2] * 2)
    X = (100.0 + rs.randn(S, M) + 0.5 * rs.randn(C, M)[y]).astype(np.float32)
    rows = np.zeros((3, M))
    rows[0, 7] = 1
    rows[1, rs.permutation(M)[:17]] = 1
    rows[2, :] = 1
    balls = sp.csr_matrix(rows)
    assert np.diff(balls.indptr).tolist() == [1, 17, 40]
    return types.SimpleNamespace(S=S, M=M, C=C, U=3, u0=1, Ub=2, NMcall=2, scored=22, X=X, y=y, fold=fold, balls=balls, sl=sl)


def _sl_kinds(q, order):
    """WRITTEN / UNTOUCHED of scores [S, C, U], predictions [S, U] and correct [G, C, U] for a launch over the centres
    [u0, u0 + Ub) that scores the first ``scored`` samples of the plan's order (``sorig`` = order)."""
    sc = np.full((q.S, q.C, q.U), UNTOUCHED, np.int8)
    sc[np.ix_(order[:q.scored], np.arange(q.C), np.arange(q.u0, q.u0 + q.Ub))] = WRITTEN
    co = np.full((1, q.C, q.U), UNTOUCHED, np.int8)
    co[:, :, q.u0:q.u0 + q.Ub] = WRITTEN
    return sc, sc[:, 0, :].copy(), co


@case('searchlight_nb', 'chebgcn_searchlight_spread', 'chebgcn_searchlight_fit', 'chebgcn_searchlight_score')
def _searchlight_nb():
    q = _sl_problem()
    sl, S, M, C, U, u0, Ub, NM = q.sl, q.S, q.M, q.C, q.U, q.u0, q.Ub, q.NMcall
    NC = int(lib().chebgcn_searchlight_query(100 + C))
    a = sl._check(q.X, q.y, q.balls, q.fold, None, True, None, True, True, None, 'searchlight_nb')
    plan = sl._device_plan(a, NC)
    assert plan.NM == 3 and plan.test_ptr.tolist() == [0, 11, 22, 24] and np.array_equal(plan.order, np.arange(S))
    Sp = plane_stride(S)
    Xt = np.full((M, Sp), NAN, np.float32)                                                  # the pad columns [S, Sp) never reach a result
    Xt[:, :S] = q.X[plan.order].T
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    inp = dict(Xt=Xt, list_ptr=plan.list_ptr[:NM + 1], list_idx=plan.list_idx, class_ptr=plan.class_ptr[:NM * C + 1],
               class_idx=plan.class_idx, test_ptr=plan.test_ptr[:NM + 1], logprior=plan.logprior[:NM], sgroup=plan.sgroup,
               slabel=plan.slabel, sorig=i32(plan.order), rowptr=i32(a.indptr), colidx=i32(a.indices))
    nlist, nclass, nnz = int(plan.list_ptr[NM]), int(plan.class_ptr[NM * C]), int(a.indices.size)
    base_bytes = 8 * NM * Ub * NC                                                           # the formula of ops.searchlight_score
    k_sc, k_pr, k_co = _sl_kinds(q, plan.order)
    k_par = np.full((NM, M, NC, 2), WRITTEN, np.int8)
    k_par[:, :, C:, :] = ZERO                                                               # "mu = h = lg = 0 ... for the classes [C, NC)"
    outs = [Out('spread', 'float64', (NM, M), 8), Out('par', 'float64', (NM, M, NC, 2), 8, k_par),
            Out('lg', 'float64', (NM, M, NC), 8, k_par[..., 0]), Out('correct', 'int32', (1, C, U), 4, k_co, base=BASE, accum='add'),
            Out('scores', 'float64', (S, C, U), 8, k_sc), Out('predictions', 'uint8', (S, U), 1, k_pr)]

    def call(L, d, o, w, stream):
        ok(L.chebgcn_searchlight_spread(P(d['Xt']), S, M, P(d['list_ptr']), P(d['list_idx']), nlist, NM, P(o['spread']), stream), 'spread')
        eps = a.vs * o['spread'].t.max(dim=1).values                                        # (the caller's reduction: torch plumbing)
        ok(L.chebgcn_searchlight_fit(P(d['Xt']), S, M, P(d['class_ptr']), P(d['class_idx']), nclass, NM, C, 0, P(eps), P(o['par']),
                                     P(o['lg']), stream), 'fit')
        ok(L.chebgcn_searchlight_score(P(d['Xt']), S, M, P(d['rowptr']), P(d['colidx']), nnz, U, u0, Ub, P(d['test_ptr']), 11, NM, C,
                                       P(o['par']), P(o['lg']), P(d['logprior']), P(d['sgroup']), P(d['slabel']), P(d['sorig']), 1,
                                       P(w['base']), P(o['correct']), P(o['scores']), P(o['predictions']), stream), 'score')

    def wrapper(d):
        import torch
        from gcn_fmri_decoding_amd import ops
        dev = d['Xt'].device
        spread = ops.searchlight_spread(d['Xt'], S, d['list_ptr'], d['list_idx'])
        par, lg = ops.searchlight_fit(d['Xt'], S, d['class_ptr'], d['class_idx'], C, a.vs * spread.max(dim=1).values)
        correct = torch.zeros((1, C, U), dtype=torch.int32, device=dev)
        scores = torch.zeros((S, C, U), dtype=torch.float64, device=dev)
        pred = torch.zeros((S, U), dtype=torch.uint8, device=dev)
        ops.searchlight_score(d['Xt'], S, d['rowptr'], d['colidx'], u0, Ub, d['test_ptr'], 11, C, par, lg, d['logprior'], d['sgroup'],
                              d['slabel'], d['sorig'], correct, scores=scores, predictions=pred)
        return dict(spread=spread, par=par, lg=lg, correct=correct, scores=scores, predictions=pred)

    def reference(inp):
        ref, scale = sl.searchlight_host(q.X, q.y, q.balls, q.fold, scores=True, predictions=True, return_scale=True)
        return {'scores': ref.scores, 'scale': scale, 'predictions': ref.predictions.astype(np.float64)}

    def compare(got, ref):
        """The bound of tests/test_gpu_searchlight.py on every score the launch wrote."""
        import test_gpu_searchlight as G
        wr = k_sc == WRITTEN
        bound = G.BOUND * ref['scale']
        assert (np.abs(got['scores'] - ref['scores'])[wr] <= bound[wr]).all(), 'searchlight_nb: a score beyond BOUND * scale'
        top = np.sort(ref['scores'], axis=1)
        decided = (top[:, -1, :] - top[:, -2, :] > 2.0 * bound.max(axis=1)) & (k_pr == WRITTEN)
        assert np.array_equal(got['predictions'][decided], ref['predictions'].astype(np.uint8)[decided])
        hits = np.zeros((1, C, U), np.int32)
        np.add.at(hits, (0, q.y[:, None], np.arange(U)[None, :]), ((got['predictions'] == q.y[:, None]) & (k_pr == WRITTEN)).astype(np.int32))
        assert np.array_equal(got['correct'], hits), 'searchlight_nb: the counts are not what the predictions say'

    arms = [('searchlight_score_kernel<%d>' % NC, NC >= C), ('padding classes [C, NC)', NC > C),
            ('a batch of centres inside the rows', 0 < u0 and u0 + Ub <= U)]
    return types.SimpleNamespace(inp=inp, outs=outs, ws={'base': base_bytes}, ws_formula={'base': 8 * NM * Ub * NC}, arms=arms, call=call,
                                 wrapper=wrapper, reference=reference, compare=compare, ws_align={'base': 8})


def _sl_tables_of(q, classifier, **kw):
    """``(a, plan, inp)``: the checked arguments, the device plan and the host tables of the shared problem (the first two models)."""
    sl, S, M, C, NM = q.sl, q.S, q.M, q.C, q.NMcall
    NC = int(lib().chebgcn_searchlight_query(100 + C))
    a = sl._check(q.X, q.y, q.balls, q.fold, None, True, None, True, True, None, 'searchlight_' + classifier, classifier=classifier, **kw)
    plan = sl._device_plan(a, NC)
    assert plan.test_ptr.tolist() == [0, 11, 22, 24] and np.array_equal(plan.order, np.arange(S))
    Xt = np.full((M, plane_stride(S)), NAN, np.float32)
    Xt[:, :S] = q.X[plan.order].T
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    inp = dict(Xt=Xt, list_ptr=plan.list_ptr[:NM + 1], list_idx=plan.list_idx, class_ptr=plan.class_ptr[:NM * C + 1],
               class_idx=plan.class_idx, test_ptr=plan.test_ptr[:NM + 1], logprior=plan.logprior[:NM], sgroup=plan.sgroup,
               slabel=plan.slabel, sorig=i32(plan.order), rowptr=i32(a.indptr), colidx=i32(a.indices),
               centres=np.arange(q.u0, q.u0 + q.Ub, dtype=np.int32))
    return a, plan, inp, NC


def _fit_means(d, S, C, NM):
    """``par`` of chebgcn_searchlight_fit with eps = 0 (an input of the LDA and RDM entries), through the wrapper."""
    import torch
    from gcn_fmri_decoding_amd import ops
    d['par'] = ops.searchlight_fit(d['Xt'], S, d['class_ptr'], d['class_idx'], C, torch.zeros(NM, dtype=torch.float64, device=d['Xt'].device))[0]


@case('searchlight_lda-bucket32', 'chebgcn_searchlight_lda')
def _searchlight_lda():
    q = _sl_problem()
    S, M, C, U, Ub, NM = q.S, q.M, q.C, q.U, q.Ub, q.NMcall
    a, plan, inp, NC = _sl_tables_of(q, 'lda', shrinkage=0.1)
    bucket, geo = 32, lib().chebgcn_searchlight_lda_query
    nclass, nnz = int(plan.class_ptr[NM * C]), int(a.indices.size)
    live = np.array([False, True, False])           # centre 0 is not in the launch; centre 2 (40 vertices) is longer than the bucket:
    k_sc, k_pr, k_co = _sl_kinds(q, plan.order)     # "a row longer than the bucket (or empty) is skipped and nothing of it is written"
    for k in (k_sc, k_pr, k_co):
        k[..., ~live] = UNTOUCHED
    k_g = np.full((NM, U), UNTOUCHED, np.int8)
    k_g[:, live] = WRITTEN
    outs = [Out('correct', 'int32', (1, C, U), 4, k_co, base=BASE, accum='add'), Out('scores', 'float64', (S, C, U), 8, k_sc),
            Out('predictions', 'uint8', (S, U), 1, k_pr), Out('gamma', 'float64', (NM, U), 8, k_g)]

    def call(L, d, o, w, stream):
        ok(L.chebgcn_searchlight_lda(P(d['Xt']), S, M, P(d['rowptr']), P(d['colidx']), nnz, U, P(d['centres']), Ub, bucket, P(d['class_ptr']),
                                     P(d['class_idx']), nclass, P(d['test_ptr']), 11, NM, C, P(d['par']), P(d['logprior']), 0.1,
                                     P(d['sgroup']), P(d['slabel']), P(d['sorig']), 1, P(o['correct']), P(o['scores']), P(o['predictions']),
                                     P(o['gamma']), stream), 'searchlight_lda')

    def wrapper(d):
        import torch
        from gcn_fmri_decoding_amd import ops
        dev = d['Xt'].device
        res = dict(correct=torch.zeros((1, C, U), dtype=torch.int32, device=dev), scores=torch.zeros((S, C, U), dtype=torch.float64, device=dev),
                   predictions=torch.zeros((S, U), dtype=torch.uint8, device=dev), gamma=torch.zeros((NM, U), dtype=torch.float64, device=dev))
        ops.searchlight_lda(d['Xt'], S, d['rowptr'], d['colidx'], d['centres'], bucket, d['class_ptr'], d['class_idx'], d['test_ptr'], 11, C,
                            d['par'], d['logprior'], 0.1, d['sgroup'], d['slabel'], d['sorig'], res['correct'], scores=res['scores'],
                            predictions=res['predictions'], gamma_out=res['gamma'])
        return res

    def reference(inp):
        ref, scale = q.sl.searchlight_host(q.X, q.y, q.balls, q.fold, scores=True, predictions=True, return_scale=True, classifier='lda',
                                           shrinkage=0.1)
        return {'scores': ref.scores, 'scale': scale}

    def compare(got, ref):
        import test_gpu_searchlight_lda as G
        wr = k_sc == WRITTEN
        assert (np.abs(got['scores'] - ref['scores'])[wr] <= (G.BOUND * ref['scale'])[wr]).all(), 'searchlight_lda: beyond BOUND * scale'
        assert (got['gamma'][k_g == WRITTEN] == 0.1).all()

    lengths = np.diff(a.indptr)
    arms = [('searchlight_lda_kernel<32>', geo(100 + int(lengths[1])) == bucket), ('a row longer than the bucket', lengths[2] > bucket)]
    return types.SimpleNamespace(inp=inp, outs=outs, ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper, reference=reference,
                                 compare=compare, prepare=lambda d: _fit_means(d, S, C, NM))


@case('searchlight_svm-bucket32', 'chebgcn_searchlight_svm')
def _searchlight_svm():
    q = _sl_problem()
    S, M, C, U, Ub, NM = q.S, q.M, q.C, q.U, q.Ub, q.NMcall
    kw = dict(C=1.0, loss='squared_hinge', tol=1e-3, max_iter=1000)
    a, plan, inp, NC = _sl_tables_of(q, 'svc')
    inp['models'] = np.arange(NM, dtype=np.int32)
    bucket, geo = 32, lib().chebgcn_searchlight_svm_query
    nlist, nnz = int(plan.list_ptr[NM]), int(a.indices.size)
    k_sc, k_pr, k_co = _sl_kinds(q, plan.order)
    k_mu = np.full((NM, U), UNTOUCHED, np.int8)
    k_mu[:, q.u0:q.u0 + Ub] = WRITTEN
    outs = [Out('correct', 'int32', (1, C, U), 4, k_co, base=BASE, accum='add'), Out('scores', 'float64', (S, C, U), 8, k_sc),
            Out('predictions', 'uint8', (S, U), 1, k_pr), Out('sweeps', 'int32', (NM, U), 4, k_mu), Out('residual', 'float64', (NM, U), 8, k_mu)]

    def call(L, d, o, w, stream):
        ok(L.chebgcn_searchlight_svm(P(d['Xt']), S, M, P(d['rowptr']), P(d['colidx']), nnz, U, P(d['centres']), Ub, P(d['models']), NM, bucket,
                                     P(d['list_ptr']), P(d['list_idx']), nlist, P(d['test_ptr']), 11, NM, C, kw['C'], 0, kw['tol'],
                                     kw['max_iter'], P(d['sgroup']), P(d['slabel']), P(d['sorig']), 1, P(o['correct']), P(o['scores']),
                                     P(o['predictions']), P(o['sweeps']), P(o['residual']), stream), 'searchlight_svm')

    def wrapper(d):
        import torch
        from gcn_fmri_decoding_amd import ops
        dev = d['Xt'].device
        res = dict(correct=torch.zeros((1, C, U), dtype=torch.int32, device=dev), scores=torch.zeros((S, C, U), dtype=torch.float64, device=dev),
                   predictions=torch.zeros((S, U), dtype=torch.uint8, device=dev), sweeps=torch.zeros((NM, U), dtype=torch.int32, device=dev),
                   residual=torch.zeros((NM, U), dtype=torch.float64, device=dev))
        ops.searchlight_svm(d['Xt'], S, d['rowptr'], d['colidx'], d['centres'], d['models'], bucket, d['list_ptr'], d['list_idx'],
                            d['test_ptr'], 11, C, kw['C'], kw['loss'], kw['tol'], kw['max_iter'], d['sgroup'], d['slabel'], d['sorig'],
                            res['correct'], scores=res['scores'], predictions=res['predictions'], sweeps=res['sweeps'],
                            residual=res['residual'])
        return res

    def reference(inp):
        """``searchlight_host(classifier='svc')``: every operation separately rounded, so the device agrees bit for bit."""
        ref, info = q.sl.searchlight_host(q.X, q.y, q.balls, q.fold, scores=True, predictions=True, classifier='svc', return_solver=True, **kw)
        sc = np.where(k_sc == WRITTEN, ref.scores, np.nan)
        res = np.where(k_mu == WRITTEN, info.residual[:NM], np.nan)
        return {'scores': sc, 'residual': res, 'sweeps_f': np.where(k_mu == WRITTEN, info.sweeps[:NM], np.nan).astype(np.float64)}

    def compare(got, ref):
        _exact(got, {'scores': ref['scores'], 'residual': ref['residual']}, 'searchlight_svm')
        wr = k_mu == WRITTEN
        assert np.array_equal(got['sweeps'][wr], ref['sweeps_f'][wr].astype(np.int32)), 'searchlight_svm: sweeps differ from the host'

    n_train = int(np.diff(plan.list_ptr)[:NM].max())
    arms = [('searchlight_svm_kernel<32>', geo(100 + n_train) == bucket), ('rows of 17 and 40 vertices, any length served', True)]
    return types.SimpleNamespace(inp=inp, outs=outs, ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper, reference=reference,
                                 compare=compare)


@case('searchlight_rdm-bucket32', 'chebgcn_searchlight_rdm')
def _searchlight_rdm():
    q = _sl_problem()
    sl, S, M, C, U, Ub = q.sl, q.S, q.M, q.C, q.U, q.Ub
    part = np.arange(S) // 12                                                               # two cells that hold every class
    a = sl._check_rdm(q.X, q.y, q.balls, part, None, None, 0.1, None, 'searchlight_rdm')
    plan = sl._rdm_plan(a)
    NM, G, npairs, bucket = plan.NM, 1, C * (C - 1) // 2, 32
    assert NM == 2
    Xt = np.full((M, plane_stride(S)), NAN, np.float32)
    Xt[:, :S] = q.X[plan.order].T
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    inp = dict(Xt=Xt, cell_ptr=plan.cell_ptr, class_ptr=plan.class_ptr, class_idx=plan.class_idx, rowptr=i32(a.indptr), colidx=i32(a.indices),
               centres=np.arange(q.u0, q.u0 + Ub, dtype=np.int32))
    nnz = int(a.indices.size)
    live = np.array([False, True, False])           # centre 0: not in the launch; centre 2: longer than the bucket, "outputs untouched"
    k_r = np.full((G, npairs, U), UNTOUCHED, np.int8)
    k_r[..., live] = WRITTEN
    outs = [Out('rdm', 'float64', (G, npairs, U), 8, k_r), Out('gamma', 'float64', (G, U), 8, k_r[:, 0, :])]

    def call(L, d, o, w, stream):
        ok(L.chebgcn_searchlight_rdm(P(d['Xt']), S, M, P(d['rowptr']), P(d['colidx']), nnz, U, P(d['centres']), Ub, bucket, P(d['cell_ptr']),
                                     P(d['class_ptr']), P(d['class_idx']), S, NM, C, P(d['par']), 0.1, G, P(o['rdm']), P(o['gamma']), stream),
           'searchlight_rdm')

    def wrapper(d):
        import torch
        from gcn_fmri_decoding_amd import ops
        dev = d['Xt'].device
        res = dict(rdm=torch.zeros((G, npairs, U), dtype=torch.float64, device=dev), gamma=torch.zeros((G, U), dtype=torch.float64, device=dev))
        ops.searchlight_rdm(d['Xt'], S, d['rowptr'], d['colidx'], d['centres'], bucket, d['cell_ptr'], d['class_ptr'], d['class_idx'], C,
                            d['par'], 0.1, res['rdm'], gamma_out=res['gamma'])
        return res

    def reference(inp):
        ref, scale = sl.crossnobis_host(q.X, q.y, q.balls, part, shrinkage=0.1, return_scale=True)
        return {'rdm': ref.rdm, 'scale': scale}

    def compare(got, ref):
        import test_gpu_rsa as G_
        wr = k_r == WRITTEN
        assert (np.abs(got['rdm'] - ref['rdm'])[wr] <= (G_.BOUND * ref['scale'])[wr]).all(), 'searchlight_rdm: beyond BOUND * scale'
        assert (got['gamma'][0, live] == 0.1).all()

    geo = lib().chebgcn_searchlight_rdm_query
    lengths = np.diff(a.indptr)
    arms = [('searchlight_rdm_kernel<32>', geo(100 + int(lengths[1])) == bucket), ('a row longer than the bucket', lengths[2] > bucket)]
    return types.SimpleNamespace(inp=inp, outs=outs, ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper, reference=reference,
                                 compare=compare, prepare=lambda d: _fit_means(d, S, C, NM))


# ===================================================================================================== glm.hip, glm_trials.hip

def _glm_problem(k, seed):
    """Two runs of T = 7 and T = split + 1 rows, M = the vertices of a project workgroup + 1, designs of 17 columns (the
    coefficient rows) of rank 3 and ``k``, 5 contrasts per run inside the row space of its design, one group of both runs."""
    from gcn_fmri_decoding_amd import glm
    q = lib().chebgcn_glm_query
    M, P, C = q(0) + 1, 17, 5
    rng = np.random.RandomState(seed)
    runs, designs, contrasts = [], [], []
    for T, r in ((7, 3), (q(4) + 1, k)):
        Z = rng.randn(T, r)
        Z[:, -1] = 1.0
        A = rng.randn(r, P) if r < P else np.eye(P)
        X = Z @ A
        designs.append(glm.Design(X, ['x%d' % i for i in range(P)], ['x0']))
        contrasts.append(rng.randn(C, r) @ A)
        runs.append((100.0 + 2.0 * (Z[:, :-1] @ rng.randn(r - 1, M)) + rng.randn(T, M)).astype(np.float32))
    pl = glm._plan(runs, designs, contrasts, None, 'glm_problem')
    assert [tb.rank for tb in pl.tables] == [3, k] and pl.C == C
    offs = np.concatenate([[0], np.cumsum([tb.T for tb in pl.tables])]).astype(np.int64)
    Mp = plane_stride(M)
    planes = np.full((int(offs[-1]), Mp), NAN, np.float32)                                  # the pad of series never reaches a result
    planes[:, :M] = np.concatenate(runs)
    Q, U, un2, B, rank = glm._batch_tables(pl.tables, C)
    inp = dict(planes=planes, offs=offs, Q=Q, U=U, un2=un2, B=B, rank=rank, gptr=np.array([0, 2], np.int32), gruns=np.array([0, 1], np.int32))
    return types.SimpleNamespace(glm=glm, M=M, Mp=Mp, P=P, C=C, k=int(Q.shape[1]), R=2, Ttot=int(offs[-1]), runs=runs, designs=designs,
                                 contrasts=contrasts, pl=pl, inp=inp, split=q(4), panel=q(1))


def _glm_finish_outs(g, extra=()):
    """The outputs of a finish and of glm_combine.  The pad [M, Mp) of the finish outputs is scratch (include/chebgcn.h: it is
    written from the zero pads of the sums and never read); glm_combine's outputs have no pad."""
    R, C, P, M, Mp = g.R, g.C, g.P, g.M, g.Mp
    k64, k32, kb = pad_kind((R, C, Mp), M, SCRATCH), pad_kind((R, C, Mp), M, SCRATCH), pad_kind((R, P, Mp), M, SCRATCH)
    return [Out('eff64', 'float64', (R, C, Mp), 8, k64), Out('var64', 'float64', (R, C, Mp), 8, k64), Out('effect', 'float32', (R, C, Mp), 4, k32),
            Out('variance', 'float32', (R, C, Mp), 4, k32), Out('t', 'float32', (R, C, Mp), 4, k32), Out('beta', 'float32', (R, P, Mp), 4, kb),
            *extra, Out('g_effect', 'float32', (1, C, M), 4), Out('g_variance', 'float32', (1, C, M), 4), Out('g_t', 'float32', (1, C, M), 4)]


def _glm_result(g, got, ar1):
    """The kernels' outputs as ``first_level`` returns them."""
    betas = [got['beta'][i, :tb.X.shape[1], :g.M] for i, tb in enumerate(g.pl.tables)]
    dof = np.array([sum(tb.T - tb.rank for tb in g.pl.tables)], np.int64)
    res = g.glm.GLMResult(got['g_effect'], got['g_variance'], got['g_t'], dof, list(g.pl.keys), betas)
    return g.glm.GLMResultAR1(*res, [got['rho'][i, :g.M] for i in range(g.R)]) if ar1 else res


@case('glm_ols', 'chebgcn_glm_project', 'chebgcn_glm_finish', 'chebgcn_glm_combine')
def _glm_ols():
    g = _glm_problem(lib().chebgcn_glm_query(1) + 1, 81)
    R, C, P, M, Mp, k, Ttot = g.R, g.C, g.P, g.M, g.Mp, g.k, g.Ttot
    nws = int(lib().chebgcn_glm_workspace(R, M, k))
    assert nws == 8 * R * (k + 1) * Mp
    # a [R][k][Mp] and yy [R][Mp] in exactly glm_workspace bytes, yy behind a: "the pad of a and yy is written as zero"
    outs = [Out('ayy', 'float64', (R * (k + 1), Mp), 8, pad_kind((R * (k + 1), Mp), M, ZERO))] + _glm_finish_outs(g)

    def call(L, d, o, w, stream):
        a, yy = o['ayy'].ptr, ctypes.c_void_p(o['ayy'].address + 8 * R * k * Mp)
        ok(L.chebgcn_glm_project(P_(d['planes']), Ttot, P_(d['offs']), R, M, P_(d['Q']), k, a, yy, stream), 'glm_project')
        ok(L.chebgcn_glm_finish(a, yy, P_(d['offs']), Ttot, P_(d['rank']), P_(d['U']), P_(d['un2']), P_(d['B']), R, M, k, C, P, P_(o['eff64']),
                                P_(o['var64']), P_(o['effect']), P_(o['variance']), P_(o['t']), P_(o['beta']), stream), 'glm_finish')
        ok(L.chebgcn_glm_combine(P_(o['eff64']), P_(o['var64']), P_(d['gptr']), P_(d['gruns']), 2, R, 1, C, M, P_(o['g_effect']),
                                 P_(o['g_variance']), P_(o['g_t']), stream), 'glm_combine')

    def wrapper(d):
        import torch
        from gcn_fmri_decoding_amd import ops
        a, yy = ops.glm_project(d['planes'], d['offs'], M, d['Q'])
        ayy = torch.cat([a.reshape(R * k, Mp), yy]).clone()
        e64, v64 = (torch.zeros((R, C, Mp), dtype=torch.float64, device=a.device) for _ in range(2))
        e32, v32, t32, beta = ops.glm_finish(a, yy, d['offs'], Ttot, d['rank'], d['U'], d['un2'], M, B=d['B'], out64=(e64, v64), want32=True)
        ge, gv, gt = ops.glm_combine(e64, v64, d['gptr'], d['gruns'], M)
        return dict(ayy=ayy, eff64=e64, var64=v64, effect=e32, variance=v32, t=t32, beta=beta, g_effect=ge, g_variance=gv, g_t=gt)

    def reference(inp):
        ref = g.glm.first_level_host(g.runs, g.designs, g.contrasts, None, betas=True)
        return {'effect': ref.effect, 'variance': ref.variance, 't': ref.t}

    def compare(got, ref):
        """``against_host`` of tests/test_gpu_glm.py: its ``worst`` over its ``scales``."""
        import test_gpu_glm as G
        G.against_host('buffers_glm_ols', _glm_result(g, got, False), g.runs, g.designs, g.contrasts, None)

    arms = [('two panels of Q, the last of one column', g.panel < k <= 2 * g.panel and k % g.panel == 1),
            ('a run below the split and one above it', 7 < g.split < g.pl.tables[1].T),
            ('a second project workgroup of one vertex', M % lib().chebgcn_glm_query(0) == 1)]
    return types.SimpleNamespace(inp=g.inp, outs=outs, ws={}, ws_formula={}, ws_checked={'glm_workspace': (nws, 8 * R * (k + 1) * Mp)},
                                 arms=arms, call=call, wrapper=wrapper, reference=reference, compare=compare)


def _glm_ar1_case(rho):
    id = 'glm_ar1-%s' % ('estimated' if rho is None else 'given')

    @case(id, 'chebgcn_glm_project_ar1', 'chebgcn_glm_finish_ar1')
    def make():
        g = _glm_problem(9, 82)
        R, C, P, M, Mp, k, Ttot = g.R, g.C, g.P, g.M, g.Mp, g.k, g.Ttot
        W, D, E = g.glm._ar1_tables(g.pl.tables, k)
        inp = dict(g.inp, W=W, D=D, E=E)
        q = lib().chebgcn_glm_ar1_query
        nws = int(lib().chebgcn_glm_ar1_workspace(R, M, k))
        assert nws == 8 * R * (2 * k + 2) * Mp
        rows = R * (2 * k + 2)                          # ah [R][2k][Mp], then s0 [R][Mp], then s1 [R][Mp]: "Pad columns as for glm_project"
        outs = [Out('sums', 'float64', (rows, Mp), 8, pad_kind((rows, Mp), M, ZERO))] + _glm_finish_outs(
            g, extra=[Out('rho', 'float32', (R, Mp), 4, pad_kind((R, Mp), M, SCRATCH))])

        def call(L, d, o, w, stream):
            ah = o['sums'].ptr
            s0 = ctypes.c_void_p(o['sums'].address + 8 * R * 2 * k * Mp)
            s1 = ctypes.c_void_p(o['sums'].address + 8 * R * (2 * k + 1) * Mp)
            ok(L.chebgcn_glm_project_ar1(P_(d['planes']), Ttot, P_(d['offs']), R, M, P_(d['W']), k, ah, s0, s1, stream), 'glm_project_ar1')
            ok(L.chebgcn_glm_finish_ar1(ah, s0, s1, P_(d['planes']), P_(d['W']), P_(d['offs']), Ttot, P_(d['rank']), P_(d['D']), P_(d['E']),
                                        P_(d['U']), P_(d['B']), R, M, k, C, P, int(rho is not None), 0.0 if rho is None else rho,
                                        P_(o['eff64']), P_(o['var64']), P_(o['effect']), P_(o['variance']), P_(o['t']), P_(o['beta']),
                                        P_(o['rho']), stream), 'glm_finish_ar1')
            ok(L.chebgcn_glm_combine(P_(o['eff64']), P_(o['var64']), P_(d['gptr']), P_(d['gruns']), 2, R, 1, C, M, P_(o['g_effect']),
                                     P_(o['g_variance']), P_(o['g_t']), stream), 'glm_combine')

        def wrapper(d):
            import torch
            from gcn_fmri_decoding_amd import ops
            ah, s0, s1 = ops.glm_project_ar1(d['planes'], d['offs'], M, d['W'])
            sums = torch.cat([ah.reshape(R * 2 * k, Mp), s0, s1]).clone()
            e64, v64 = (torch.zeros((R, C, Mp), dtype=torch.float64, device=ah.device) for _ in range(2))
            e32, v32, t32, beta, rmap = ops.glm_finish_ar1(ah, s0, s1, d['planes'], d['W'], d['offs'], d['rank'], d['D'], d['E'], d['U'], M,
                                                           rho=rho, B=d['B'], out64=(e64, v64), want32=True)
            ge, gv, gt = ops.glm_combine(e64, v64, d['gptr'], d['gruns'], M)
            return dict(sums=sums, eff64=e64, var64=v64, effect=e32, variance=v32, t=t32, beta=beta, rho=rmap, g_effect=ge, g_variance=gv,
                        g_t=gt)

        def reference(inp):
            ref = g.glm.first_level_host(g.runs, g.designs, g.contrasts, None, betas=True, noise='ar1', rho=rho)
            return {'effect': ref.effect, 'variance': ref.variance, 't': ref.t, 'rho0': ref.rho[0], 'rho1': ref.rho[1]}

        def compare(got, ref):
            """``against_host`` of tests/test_gpu_glm_ar1.py: ``glm_ar1_common.distances`` at ``glm_ar1_common.EPS``; the vertices
            whose HOST rho sits at the clamp are named to it, as that test does for its sinusoid."""
            import glm_ar1_common as A
            import test_gpu_glm_ar1 as G
            clamped = sorted(set(np.flatnonzero(np.abs(ref['rho0']) >= A.RHO_FREE)) | set(np.flatnonzero(np.abs(ref['rho1']) >= A.RHO_FREE)))
            G.against_host('buffers_' + id, _glm_result(g, got, True), g.runs, g.designs, g.contrasts, None, rho=rho, clamped=clamped)

        arms = [('two panels of [Q | Qs]', g.panel < 2 * k <= 2 * g.panel), ('glm_finish_ar1_kernel<16>', q(100 + k) == 16),
                ('two solve groups of contrasts', q(1) < C <= 2 * q(1)), ('more coefficient rows than the bucket', P > q(100 + k))]
        return types.SimpleNamespace(inp=inp, outs=outs, ws={}, ws_formula={}, ws_checked={'glm_ar1_workspace': (nws, 8 * R * (2 * k + 2) * Mp)},
                                     arms=arms, call=call, wrapper=wrapper, reference=reference, compare=compare)
    return make


_glm_ar1_case(None)
_glm_ar1_case(0.3)


@case('glm_trials', 'chebgcn_glm_trials')
def _glm_trials():
    import test_gpu_single_trial as S
    from gcn_fmri_decoding_amd import glm
    q = lib().chebgcn_glm_trials_query
    n = q(1) + 1                                                                            # the smallest two-panel case of that file
    y, td = S.make_run(np.random.RandomState(100 + n), n=n)
    pl = glm._trial_plan(y, td, 'condition', ('beta', 't'), None, 'glm_trials')
    M, G, Mp = pl.M, pl.G, plane_stride(pl.M)
    Q, Z, toffs, qrank, own, rank, w, F = glm._trial_tables(pl.tables, G)
    Ttot, k, N, G1 = int(Q.shape[0]), int(Q.shape[1]), int(w.shape[0]), int(w.shape[1])
    planes = np.full((Ttot, Mp), NAN, np.float32)
    planes[:, :M] = y
    offs = np.array([0, Ttot], np.int64)
    inp = dict(planes=planes, offs=offs, Q=Q, Z=Z, toffs=toffs, qrank=qrank, own=own, rank=rank, w=w, F=F)
    kind = pad_kind((N, Mp), M, ZERO)                                                       # "pad columns are written as zero"
    outs = [Out('beta', 'float32', (N, Mp), 8, kind), Out('t', 'float32', (N, Mp), 8, kind)]  # (pointers aligned to 8 bytes)

    def prepare(d):
        from gcn_fmri_decoding_amd import ops
        a, yy = ops.glm_project(d['planes'], d['offs'], M, d['Q'])
        d['a'], d['yy'] = a.clone(), yy.clone()

    def call(L, d, o, w_, stream):
        ok(L.chebgcn_glm_trials(P_(d['planes']), Ttot, P_(d['offs']), 1, M, P_(d['Z']), n, P_(d['toffs']), P_(d['a']), P_(d['yy']), k,
                                P_(d['qrank']), P_(d['own']), P_(d['rank']), P_(d['w']), P_(d['F']), G1, N, P_(o['beta']), None, P_(o['t']),
                                stream), 'glm_trials')

    def wrapper(d):
        from gcn_fmri_decoding_amd import ops
        beta, _, t = ops.glm_trials(d['planes'], d['offs'], M, d['Z'], d['toffs'], d['a'], d['yy'], d['qrank'], d['own'], d['rank'], d['w'],
                                    d['F'], outputs=('beta', 't'))
        return {'beta': beta, 't': t}

    def reference(inp):
        ref = glm.single_trial_host(y, td, outputs=S.ALL)
        return {'beta': ref.beta, 'variance': ref.variance, 't': ref.t}

    def compare(got, ref):
        """``worst`` over ``scales`` of tests/test_gpu_single_trial.py, for the two maps the call forms."""
        s_b, s_v = S.scales(y, td, 'condition')
        pos = ref['variance'] > 0
        v = np.where(pos, ref['variance'], 1.0)
        s_t = np.where(pos, s_b / np.sqrt(v) + np.abs(ref['t']) * s_v / (2.0 * v), 0.0)
        assert S.worst(got['beta'][:, :M], ref['beta'], s_b) <= 1.0, 'glm_trials: beta beyond the bound of test_gpu_single_trial'
        assert S.worst(np.where(pos, got['t'][:, :M], 0.0), np.where(pos, ref['t'], 0.0), s_t) <= 1.0, 'glm_trials: t beyond the bound'

    arms = [('two panels of trial columns, the last of one', q(1) < n <= 2 * q(1) and n % q(1) == 1 and N == n)]
    return types.SimpleNamespace(inp=inp, outs=outs, ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper, reference=reference,
                                 compare=compare, prepare=prepare)


# ===================================================================================================== filter.hip

def _filter_case(arm_name, K):
    id = 'cheb_filter-%s-K%d' % (arm_name, K)
    arm = {'rolling': _lib.FILTER_ROLLING, 'stack': _lib.FILTER_STACK}[arm_name]

    @case(id, 'chebgcn_cheb_filter')
    def make():
        import test_gpu_filters as F
        from gcn_fmri_decoding_amd import GraphFilter
        M, n, J = 257, 5, 3
        Mp = plane_stride(M)
        L = F._lap(M)
        x = np.random.default_rng(K).standard_normal((n, M)).astype(np.float32)
        xp = np.full((n, Mp), NAN, np.float32)
        xp[:, :M] = x
        c = F._table(J, K).astype(np.float32)
        slabs = 0 if K == 1 else (2 if arm_name == 'rolling' else K)                       # "TWO slabs" rolling, "K slabs" stack
        formula = slabs * n * Mp * 4
        state = {}

        def prepare(d):
            from gcn_fmri_decoding_amd import ops
            g = state['g'] = ops.Graph(L, d['x'].device)
            assert g.Mp == Mp and (arm_name != 'stack' or g.on_chip), 'the stack case needs a graph with an on-chip image'
            nws = ops.cheb_filter_workspace(g, n, K, J, arm)
            assert K == 1 or nws == formula, '%s: chebgcn_cheb_filter_workspace says %d bytes, the header %d' % (id, nws, formula)

        def call(L_, d, o, w, stream):
            ok(L_.chebgcn_cheb_filter(state['g'].handle, P_(d['x']), P_(d['coeff']), P_(o['y']), P_(w['workspace']), n, K, J, arm, stream), id)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            return {'y': ops.cheb_filter(state['g'], d['x'], d['coeff'], arm=arm)}

        def reference(inp):
            return {'y': GraphFilter(L, coeffs=c.astype(np.float64), relabel=None).apply_host(x)}

        def compare(got, ref):
            """The standing bound of tests/test_gpu_filters.py: max|device - host| <= REL max|host| per filter."""
            y = got['y'][:, :, :M].astype(np.float64)
            for j in range(J):
                assert np.abs(y[j] - ref['y'][j]).max() <= F.REL * np.abs(ref['y'][j]).max(), '%s: filter %d beyond REL' % (id, j)

        # "the pad [M, Mp) of every plane of y and of the workspace is scratch"
        outs = [Out('y', 'float32', (J, n, Mp), 16, pad_kind((J, n, Mp), M, SCRATCH))]
        arms = [('a NULL workspace at K = 1' if K == 1 else 'exactly %d slabs of workspace' % slabs, (formula == 0) == (K == 1)),
                ('a second workgroup of one vertex; plane groups of 4 and 1', M == 257 and n == 5)]
        return types.SimpleNamespace(inp=dict(x=xp, coeff=c), outs=outs, ws={'workspace': formula}, ws_formula={'workspace': formula},
                                     arms=arms, call=call, wrapper=wrapper, reference=reference, compare=compare, prepare=prepare)
    return make


_filter_case('rolling', 4)
_filter_case('stack', 4)
_filter_case('rolling', 1)


# ===================================================================================================== cluster.hip

def _signflip_case(packed):
    id = 'signflip_t-%s' % ('packed' if packed else 'drawn')

    @case(id, 'chebgcn_signflip_t')
    def make():
        from gcn_fmri_decoding_amd import stats
        S, M, Pb, p0, seed = 33, 257, 3, 2, 11
        rs = np.random.RandomState(90 + packed)
        x = (rs.randn(S, M) + 0.3).astype(np.float32)
        x[:, 5] = 0.5                                                                       # a constant vertex: t = 0
        xd = x.astype(np.float64)
        qv = np.zeros(M)
        for j in range(S):
            qv = qv + xd[j] * xd[j]
        if packed:
            neg = rs.randint(0, 2, size=(Pb, S)).astype(np.int64)
            words = np.zeros((Pb, (S + 31) // 32), np.uint32)
            for j in range(S):
                words[:, j >> 5] |= (neg[:, j] << (j & 31)).astype(np.uint32)
            signs = (1 - 2 * neg).astype(np.int8)
        else:
            words = None
            signs = stats.sign_flips(S, p0 + Pb, seed)[0][p0:p0 + Pb]
        inp = dict(x=x, q=qv, bits=None if words is None else words.view(np.int32))

        def call(L, d, o, w, stream):
            ok(L.chebgcn_signflip_t(P_(d['x']), P_(d['q']), P_(d.get('bits')), P_(o['t']), S, M, p0, Pb, seed, stream), id)

        def wrapper(d):
            from gcn_fmri_decoding_amd import ops
            return {'t': ops.signflip_t(d['x'], d['q'], p0, Pb, seed, bits=d.get('bits'))}

        arms = [('two words of packed signs' if packed else 'drawn signs from a later permutation', (S + 31) // 32 == 2 and p0 > 0)]
        return types.SimpleNamespace(inp=inp, outs=[Out('t', 'float32', (Pb, M), 4)], ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper,
                                     reference=lambda inp: {'t': stats.t_host(x, signs)}, compare=lambda got, ref: _exact(got, ref, id))
    return make


_signflip_case(False)
_signflip_case(True)


@case('perm_glm_t', 'chebgcn_perm_glm_t')
def _perm_glm_t():
    import test_gpu_design_test as D
    from gcn_fmri_decoding_amd import stats
    q = lib().chebgcn_perm_glm_query
    r, S = 17, 19
    M, Pb = q(0) + 1, q(100 + r) + 1
    e, qv, Uf, u, unorm2, dof, rows = D.kernel_case(S, r, M, Pb, True, seed=S + M)
    inp = dict(e=e, q=qv, Uf=Uf, u=u, rows=np.ascontiguousarray(rows).view(np.int32))

    def call(L, d, o, w, stream):
        ok(L.chebgcn_perm_glm_t(P_(d['e']), P_(d['q']), P_(d['Uf']), P_(d['u']), unorm2, dof, P_(d['rows']), P_(o['t']), S, M, r, Pb, stream),
           'perm_glm_t')

    def wrapper(d):
        from gcn_fmri_decoding_amd import ops
        return {'t': ops.perm_glm_t(d['e'], d['q'], d['Uf'], d['u'], unorm2, dof, d['rows'])}

    arms = [('two column panels, the last of one column', q(2) < r <= 2 * q(2) and r % q(2) == 1),
            ('a second workgroup of one vertex and of one permutation', M % q(0) == 1 and Pb % q(100 + r) == 1)]
    return types.SimpleNamespace(inp=inp, outs=[Out('t', 'float32', (Pb, M), 4)], ws={}, ws_formula={}, arms=arms, call=call, wrapper=wrapper,
                                 reference=lambda inp: {'t': stats.perm_t_host(e, qv, Uf, u, unorm2, dof, rows)},
                                 compare=lambda got, ref: _exact(got, ref, 'perm_glm_t'))


def _cluster_case(mode_name, arm_name, wants):
    id = 'cluster_enhance-%s-%s-%s' % (mode_name, arm_name, '+'.join(wants))
    mode = {'max': _lib.CLUSTER_MAX, 'extent': _lib.CLUSTER_EXTENT, 'tfce': _lib.CLUSTER_TFCE}[mode_name]
    arm = {'onchip': _lib.CLUSTER_ONCHIP, 'streamed': _lib.CLUSTER_STREAMED, 'plain': _lib.CLUSTER_AUTO}[arm_name]

    @case(id, 'chebgcn_cluster_enhance')
    def make():
        import map_test_cases as MC
        from gcn_fmri_decoding_amd import stats
        M, Pb, NH = 300, 3, 6
        q = lib().chebgcn_cluster_query
        A = MC.random_graph(M, 4, 3)
        ptr, idx = stats.edges(A, M)
        rs = np.random.RandomState(95)
        z = rs.randn(Pb, M)
        t = (z + 0.5 * (A @ z.T).T).astype(np.float32)                                      # smooth along the edges: clusters of several vertices
        top = float(t.max())
        step = top / (NH + 0.5)                                                             # the highest map has exactly NH heights
        thr = 0.8
        pl = types.SimpleNamespace(M=M, stat=mode_name, H=2.0, E=0.5, threshold=thr)
        hf, hw, ep = (None, None, None) if mode_name == 'max' else stats._tables(pl, step, NH)
        nh = 1 if mode_name == 'extent' else NH
        nws = int(lib().chebgcn_cluster_enhance_workspace(Pb, M, mode, arm))
        formula = q(5) * Pb * M if arm_name == 'streamed' else 0                            # state_bytes * Pb * M, streamed arm only
        inp = dict(t=t, ptr=ptr, idx=idx, hf=hf, hw=hw, ep=ep)
        outs = [o for o in (Out('out', 'float64', (Pb, M), 8), Out('labels', 'int32', (Pb, M), 4), Out('pmax', 'float64', (Pb,), 8))
                if o.name in wants]
        if mode_name != 'max':
            outs.append(Out('status', 'int32', (1,), 4, base=BASE, accum='max'))             # atomicMax only: the larger of the two stays

        def call(L, d, o, w, stream):
            ok(L.chebgcn_cluster_enhance(P_(d.get('ptr')) if mode_name != 'max' else None, P_(d.get('idx')) if mode_name != 'max' else None,
                                         int(idx.size) if mode_name != 'max' else 0, P_(d['t']), 0, P_(d.get('hf')), P_(d.get('hw')), nh,
                                         P_(d.get('ep')), step, P_(o.get('out')), P_(o.get('labels')), P_(o.get('pmax')), P_(o.get('status')),
                                         P_(w.get('workspace')), nws, Pb, M, mode, arm, stream), id)

        def wrapper(d):
            import torch
            from gcn_fmri_decoding_amd import ops
            status = torch.zeros(1, dtype=torch.int32, device=d['t'].device)
            out, labels, pmax = ops.cluster_enhance(d['t'], mode, d.get('ptr'), d.get('idx'), d.get('hf'), d.get('hw'), d.get('ep'), step=step,
                                                    NH=nh, want_out='out' in wants, want_labels='labels' in wants, want_max='pmax' in wants,
                                                    arm=arm, status=status)
            res = {k: v for k, v in (('out', out), ('labels', labels), ('pmax', pmax)) if v is not None}
            if mode_name != 'max':
                res['status'] = status
            return res

        def reference(inp):
            both = [stats.enhance_host(t[p], ptr, idx, mode_name, hf, hw, ep, step) for p in range(Pb)]
            out = np.stack([b[0] for b in both])
            return {'out': out, 'labels_f': np.stack([b[1] for b in both]).astype(np.float64), 'pmax': out.max(axis=1)}

        def compare(got, ref):
            """Bit for bit equal to ``stats.enhance_host`` (the header: "equal to the host restatement")."""
            want = {'out': ref['out'], 'pmax': ref['pmax']}
            _exact({k: got[k] for k in want if k in got}, {k: v for k, v in want.items() if k in got}, id)
            if 'labels' in got:
                assert np.array_equal(got['labels'], ref['labels_f'].astype(np.int32)), id + ': labels differ from the host'
            assert 'status' not in got or int(got['status'][0]) == 0

        arms = [('on chip: no workspace' if arm_name != 'streamed' else 'streamed: exactly state_bytes * Pb * M bytes',
                 (nws > 0) == (arm_name == 'streamed') and M <= q(0)),
                ('%d heights' % nh, mode_name == 'max' or int(np.floor(np.float64(top) / np.float64(step))) == NH)]
        return types.SimpleNamespace(inp=inp, outs=outs, ws={'workspace': nws} if arm_name == 'streamed' else {},
                                     ws_formula={'workspace': formula} if arm_name == 'streamed' else {}, arms=arms, call=call, wrapper=wrapper,
                                     reference=reference, compare=compare)
    return make


_cluster_case('tfce', 'onchip', ('out', 'labels', 'pmax'))
_cluster_case('extent', 'onchip', ('pmax',))
_cluster_case('tfce', 'streamed', ('out',))
_cluster_case('extent', 'streamed', ('out', 'labels', 'pmax'))
_cluster_case('max', 'plain', ('out', 'pmax'))


# ===================================================================================================== the protocol

P_ = P

def _run(c, b, tag, fill, dev):
    """One run of case ``c`` into fresh regions pre-filled with ``fill``: the regions after the call, guards and inputs checked."""
    import torch
    d = {k: torch.as_tensor(v).to(dev) for k, v in b.inp.items() if v is not None}
    if hasattr(b, 'prepare'):
        b.prepare(d)                                                                        # inputs another entry's wrapper makes
    before = {k: t.clone() for k, t in d.items()}
    o = {s.name: gb.Guarded(s.shape, s.dtype, fill, dev, s.align, init=s.init, base=s.base) for s in b.outs}
    w = {k: (gb.Guarded((n,), 'uint8', fill, dev, getattr(b, 'ws_align', {}).get(k, 16)) if n else None) for k, n in b.ws.items()}
    b.call(lib(), d, o, w, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, r in list(o.items()) + [(k, r) for k, r in w.items() if r is not None]:
        r.check('%s (%s), run %s, %s' % (c.id, ', '.join(c.entries), tag, k))
    for k, t in d.items():
        same = torch.equal(t.view(torch.uint8) if t.dtype != torch.uint8 else t, before[k].view(torch.uint8) if t.dtype != torch.uint8 else before[k])
        assert same, '%s (%s), run %s: input changed -- %s is not byte-identical to its copy from before the call' % (
            c.id, ', '.join(c.entries), tag, k)
    return {k: r.host() for k, r in o.items()}, d


def _initial(s, fill):
    """What output ``s`` held before the call."""
    if s.init is not None:
        return np.ascontiguousarray(s.init, gb._NP[s.dtype]).reshape(s.shape)
    if s.base is not None:
        return np.full(s.shape, s.base, gb._NP[s.dtype])
    return gb.filled(fill, s.dtype, s.shape)


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_entry_on_guarded_poisoned_buffers(c):
    import torch
    dev = torch.device('cuda', 0)
    b = c.built()
    who = '%s (%s)' % (c.id, ', '.join(c.entries))
    runs = {}
    for tag, fill in gb.FILLS:
        runs[tag], d = _run(c, b, tag, fill, dev)
    wrap = {k: t.cpu().numpy() for k, t in b.wrapper(d).items()} if b.wrapper is not None else None
    for s in b.outs:
        a, z = runs['A'][s.name], runs['B'][s.name]
        wr = s.kind == WRITTEN
        differ = wr & (gb.bits(a) != gb.bits(z))
        assert not differ.any(), '%s: runs A/B differ -- %d written entries of %s depend on what the buffers held, first at %s' % (
            who, differ.sum(), s.name, tuple(np.argwhere(differ)[0]))
        for tag, fill in gb.FILLS:
            got = runs[tag][s.name]
            init = _initial(s, fill)
            keep = (s.kind == UNTOUCHED) & (gb.bits(got) != gb.bits(init))
            rule = 'base not kept' if s.base is not None else 'untouched part written'
            assert not keep.any(), '%s, run %s: %s -- %d entries of %s the header leaves untouched changed, first at %s' % (
                who, tag, rule, keep.sum(), s.name, tuple(np.argwhere(keep)[0]))
            zero = (s.kind == ZERO) & (gb.bits(got) != 0)
            assert not zero.any(), '%s, run %s: pad not zero -- %d entries of %s the header promises as 0 are not, first at %s' % (
                who, tag, zero.sum(), s.name, tuple(np.argwhere(zero)[0]))
        if wrap is not None and s.wrap in wrap:
            ref = wrap[s.wrap].reshape(s.shape)
            if s.accum == 'add':
                ref = (ref + s.base).astype(ref.dtype)
            elif s.accum == 'max':
                ref = np.maximum(ref, s.base).astype(ref.dtype)
            # the written part and the promised zeros; an in-place buffer (init) as a whole: the wrapper started from the same data
            live = wr if s.accum else ((s.kind != SCRATCH) if s.init is not None else (wr | (s.kind == ZERO)))
            bad = live & (gb.bits(a) != gb.bits(ref.astype(a.dtype)))
            rule = 'base not kept' if s.accum else 'differs from the wrapper'
            assert not bad.any(), '%s: %s -- %d entries of %s are not %s, first at %s: %r against %r' % (
                who, rule, bad.sum(), s.name, 'base + the wrapper\'s count' if s.accum else 'what the public wrapper returns',
                tuple(np.argwhere(bad)[0]), a[bad][0], ref[bad][0])
    if wrap is not None:
        b.compare(wrap, b.reference(b.inp))
