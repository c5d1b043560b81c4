"""Host companion of tests/test_gpu_window_kernels.py: the case tables of tests/window_kernel_cases.py reach every body and
boundary of the window gathers and window statistics they name (asserted from the shapes and the restated dispatch arithmetic
alone, so a changed constant fails here instead of silently losing an edge), the references are what they claim to be, and a
NumPy stand-in of each kernel's index arithmetic -- block, pass, unroll, clamp, chunk -- equals the reference on every case
while each planted fault fails the comparison the device module uses on at least one case.  No GPU."""
import os
import re
import shutil

import numpy as np
import pytest

from gcn_fmri_decoding_amd import _lib, series
from gcn_fmri_decoding_amd._lib import plane_stride

import guarded_buffers as gb
import window_kernel_cases as K

TABLES = (False, True)


def shapes(entry, **where):
    return [c.shape for c in K.of(entry) if all(getattr(c.shape, a, None) == v for a, v in where.items())]


# ------------------------------------------------------------------------------------------------------------------------ reach

def reach(k):
    """{claim: holds} for the case tables under the constants ``k``: every edge the tables exist for, from shapes alone."""
    r = {}
    tile = k.GW_T * k.GW_U
    mix_n, idx_bodies = K.source_bodies()
    r['the mix kernel has one body per N = 1 .. GWM_MAX'] = mix_n == list(range(1, k.GWM_MAX + 1))
    r['the specialised (fold, n) bodies are the restated ones'] = idx_bodies == sorted(K.SPECIALISED)
    for entry, kind in (('gather_windows', 'plain'), ('gather_windows_mix', 'mix'), ('gather_windows_indexed', 'indexed'),
                        ('gather_windows_reflect', 'reflect')):
        for t in TABLES:
            ss, tag = shapes(entry, tables=t), '%s<%s>: ' % (kind, 'tables' if t else 'plain')
            Mq = plane_stride(K.M_AT_C) // 4
            n = {K.pieces(s.M, s.C) for s in ss if s.M == K.M_AT_C}
            r[tag + 'one plane, a tile less a plane, a tile, a tile and a plane, two tiles and a plane'] = \
                {Mq, tile - Mq, tile, tile + Mq, 2 * tile + Mq} <= n
            r[tag + 'one block, two and three'] = {1, 2, 3} <= {K.gather_blocks(k, s.M, s.C) for s in ss}
            Ms = {s.M for s in ss}
            r[tag + 'the pad begins inside a piece at M % 4 = 1, 2, 3'] = {1, 2, 3} <= {M % 4 for M in Ms if M > 4}
            r[tag + 'whole pieces of pad, no pad, one vertex'] = any(plane_stride(M) - M >= 8 for M in Ms) and \
                any(plane_stride(M) == M for M in Ms) and 1 in Ms
            r[tag + 'sample absent and with repeats'] = {True, False} <= {s.sample for s in ss}
            r[tag + 'at most 9 windows a launch'] = all(s.B <= 9 for s in ss)
    for t in TABLES:
        ss, tag = shapes('gather_windows_mix', tables=t), 'mix<%s>: ' % ('tables' if t else 'plain')
        full = [s for s in ss if s.smax == k.GWM_MAX]
        r[tag + 'no count above GWM_MAX'] = all(s.smax <= k.GWM_MAX for s in ss)
        for N in range(1, k.GWM_MAX + 1):
            fills = [K.pass_fill(k, s.M, s.C, N) for s in full if set(s.counts) == {N}]
            per_pass = k.GW_T * K.width(k, N)
            r[tag + 'N = %d: a block with every pass full' % N] = any(all(f == per_pass for f in b) for fill in fills for b in fill)
            r[tag + 'N = %d: a block whose LAST pass is partial' % N] = any(0 < b[-1] < per_pass and all(f == per_pass for f in b[:-1])
                                                                        for fill in fills for b in fill)
            r[tag + 'N = %d: a block that ends inside pass %d' % (N, min(1, K.passes(k, N) - 1))] = any(
                0 < b[min(1, len(b) - 1)] < per_pass and not any(b[2:]) for fill in fills for b in fill)
        for N in K.MIX_BOUNDARY_N:
            ends = {K.pieces(s.M, s.C) for s in full if set(s.counts) == {N}}
            r[tag + 'N = %d: windows of 1, 2 and 3 quarter tiles' % N] = {tile // 4, tile // 2, 3 * tile // 4} <= ends
        r[tag + 'one N of each width at the pass boundaries'] = {K.width(k, N) for N in K.MIX_BOUNDARY_N} == \
            {k.GW_U, k.GW_U // 2, k.GW_U // 4} and len({k.GW_U, k.GW_U // 2, k.GW_U // 4}) == 3
        sweep = [s for s in ss if s.smax < k.GWM_MAX]
        r[tag + 'counts below 1 and above smax'] = any(min(s.counts) < 1 and max(s.counts) > s.smax for s in sweep)
        ss, tag = shapes('gather_windows_indexed', tables=t), 'indexed<%s>: ' % ('tables' if t else 'plain')
        r[tag + 'fold and n up to GWI_MAX'] = max(s.fold for s in ss) == k.GWI_MAX == max(s.n for s in ss) and \
            {(k.GWI_MAX, k.GWI_MAX), (k.GWI_MAX, 1), (1, k.GWI_MAX)} <= {(s.fold, s.n) for s in ss}
        for body in K.SPECIALISED:
            mine = [s for s in ss if (s.fold, s.n) == body and s.src]
            L = body[0] * body[1]
            per_pass = k.GW_T * K.width(k, L)
            r[tag + 'body %s with sources, every pass full and a partial last pass' % (body,)] = any(
                any(all(f == per_pass for f in b) for b in fill) and any(0 < b[-1] < per_pass and all(f == per_pass for f in b[:-1]) for b in fill)
                for fill in (K.pass_fill(k, s.M, s.C, L) for s in mine))
            if body[1] == 1:
                r[tag + 'body %s without sources' % (body,)] = any((s.fold, s.n) == body and not s.src for s in ss)
        have = {(s.fold, s.n) for s in ss}
        r[tag + 'the generic loop on both sides of the bodies'] = set(K.GENERIC_NEIGHBOURS) <= have and \
            not set(K.GENERIC_NEIGHBOURS) & set(K.SPECIALISED) and \
            all(any((f + df, n + dn) in K.GENERIC_NEIGHBOURS for df, dn in ((0, 1), (1, 0))) for f, n in ((1, 8), (2, 4), (3, 1), (4, 1)))
        r[tag + 'the generic loop over two blocks with a tail'] = all(
            K.gather_blocks(k, s.M, s.C) == 2 and K.pieces(s.M, s.C) % tile for s in ss if (s.fold, s.n) in K.GENERIC_NEIGHBOURS)
        ss = shapes('gather_windows_reflect', tables=t)
        r['reflect<%d>: shifts 0, 1, C - 1 and clamped ones at C = 1, 2 and 15' % t] = {1, 2, 15} <= {s.C for s in ss if s.S == 7} and \
            any(s.tshift_null for s in ss)
        ss = shapes('window_drop', tables=t)
        r['drop<%d>: B * D = 1, WD_T - 1, WD_T, WD_T + 1' % t] = all({1, k.WD_T - 1, k.WD_T, k.WD_T + 1} <= {s.B * s.D for s in ss if s.pos == pos}
                                                                   for pos in K.DROP_POS)
        r['drop<%d>: one block and two' % t] = {1, 2} <= {K.drop_blocks(k, s.B, s.D) for s in ss}
        r['drop<%d>: M = 1 with every kind of pos' % t] = {s.pos for s in ss if s.M == 1} == set(K.DROP_POS)
        r['drop<%d>: more draws than vertices' % t] = any(s.D > s.M for s in ss)
    for leg in K.LEGS:
        ss, tag = shapes('window_stats', leg=leg), 'stats %s: ' % leg
        G, R = k.WS_CG, k.WS_ROWS
        at33 = {(s.C, s.Ttot) for s in ss if s.M == 33 and s.special is None}
        Cs = (1, G - 1, G, G + 1, 2 * G, 2 * G + 1)
        r[tag + 'C around one and two channel groups, each at every Ttot edge'] = \
            {(C, T) for C in Cs for T in (R - 1, R, R + 1, R + 2, 2 * R, 2 * R + 1, 2 * R + 3)} | {(C, C) for C in Cs} <= at33
        r[tag + 'a third group of one channel'] = any(K.channel_groups(k, s.C) == 3 and s.C % G == 1 for s in ss)
        r[tag + 'chunk tails of 1, 2 and 3 rows, a full last chunk'] = {0, 1, 2, 3} <= {s.Ttot % R for s in ss if s.Ttot > R}
        r[tag + 'a last turn of 1, 2 and 3 rows'] = {1, 2, 3} <= {(s.Ttot % R) % 4 for s in ss}
        r[tag + 'Ttot = C with one window'] = all(any(s.Ttot == s.C == C and s.S == 1 for s in ss) for C in Cs)
        Mps = {plane_stride(s.M) for s in ss}
        r[tag + 'one vertex, one vertex tile, one past it'] = 1 in {s.M for s in ss} and 2 * k.WS_T in Mps and \
            any(2 * k.WS_T < Mp <= 2 * k.WS_T + 32 for Mp in Mps)
        r[tag + 'every window on one start, and one window'] = any(s.special == 'equal' for s in ss) and \
            any(s.special == 'one' and s.S == 1 and s.Ttot > s.C for s in ss)
        r[tag + 'a constant vertex wherever M > 1'] = all((s.const_vertex is not None) == (s.M > 1) for s in ss)
        if leg == 'exact':
            r[tag + 'S a power of two'] = all(s.S & (s.S - 1) == 0 for s in ss)
        ss, tag = shapes('window_stats_indexed', leg=leg), 'stats_indexed %s: ' % leg
        Ss, mn, ch = {s.S for s in ss}, k.WSI_MIN, k.WSI_CHUNKS
        if leg == 'bounded':
            r[tag + 'one chunk to two: S = 1, MIN - 1, MIN, MIN + 1, 2 MIN + 1'] = {1, mn - 1, mn, mn + 1, 2 * mn + 1} <= Ss
            r[tag + 'the chunk grows and the count falls: S = MIN CHUNKS, + 1'] = {mn * ch, mn * ch + 1} <= Ss and \
                K.wsi_chunks(k, mn * ch) == ch and K.wsi_chunk(k, mn * ch + 1) == mn + 1 and K.wsi_chunks(k, mn * ch + 1) == ch - 1
            r[tag + 'chunks of MIN .. MIN + 3 windows: unroll tails 0, 1, 2, 3'] = \
                {mn, mn + 1, mn + 2, mn + 3} <= {K.wsi_chunk(k, S) for S in Ss} and mn % 4 == 0
            r[tag + 'a last turn of 1, 2, 3 and 4 windows, in a full chunk or in the last'] = {0, 1, 2, 3} <= \
                {n % 4 for S in Ss for n in (K.wsi_chunk(k, S) if S > K.wsi_chunk(k, S) else S, S - (K.wsi_chunks(k, S) - 1) * K.wsi_chunk(k, S))}
            r[tag + 'every S at fold 1, 2, 3, GWI_MAX and C = 1, 3'] = \
                {(s.S, s.fold, s.C) for s in ss} == {(S, f, C) for S in Ss for f in (1, 2, 3, k.GWI_MAX) for C in (1, 3)}
        else:
            r[tag + 'S and fold powers of two, one chunk and CHUNKS of them'] = \
                all(s.S & (s.S - 1) == 0 and s.fold & (s.fold - 1) == 0 for s in ss) and {1, mn, mn * ch} <= Ss and \
                {1, 2, k.GWI_MAX} <= {s.fold for s in ss}
    return r


def test_case_ids_are_unique_and_every_entry_occurs():
    ids = [c.id for c in K.ALL]
    assert len(ids) == len(set(ids))
    assert {c.entry for c in K.ALL} == set(K.ENTRIES)
    for e in K.ENTRIES + ('chebgcn_window_stats_workspace', 'chebgcn_window_stats_indexed_workspace'):
        assert e in _lib.SIGNATURES, e


def test_the_tables_reach_every_body_and_boundary():
    missed = [claim for claim, holds in reach(K.K).items() if not holds]
    assert not missed, missed


CHANGED = {'GW_T': 128, 'GW_U': 8, 'GWM_MAX': 8, 'GWI_MAX': 8, 'WS_T': 128, 'WS_CG': 4, 'WS_ROWS': 256, 'WSI_CHUNKS': 16, 'WSI_MIN': 8,
           'WD_T': 128}


@pytest.mark.parametrize('name', sorted(K.CONSTANT_FILES))
def test_a_changed_constant_fails_the_reach_test(name, tmp_path):
    """A copy of the sources with one constant changed: the tables no longer reach what they claim, and ``reach`` says so."""
    for f in set(K.CONSTANT_FILES.values()):
        shutil.copy(os.path.join(K.CSRC, f), str(tmp_path))
    path = os.path.join(str(tmp_path), K.CONSTANT_FILES[name])
    text, n = re.subn(r'(constexpr\s+int\s+%s\s*=\s*)\d+' % name, r'\g<1>%d' % CHANGED[name], open(path).read())
    assert n == 1
    open(path, 'w').write(text)
    k = K.constants(str(tmp_path))
    assert getattr(k, name) == CHANGED[name] != getattr(K.K, name)
    missed = [claim for claim, holds in reach(k).items() if not holds]
    print('%s = %d: %d claims no longer hold, e.g. %s' % (name, CHANGED[name], len(missed), missed[:2]))
    assert missed


def test_the_inputs_hold_the_edges_the_tables_claim():
    """Rows at 0 and at the last valid row, rows / counts / shifts / sources / indices (and the indexed gather's samples) outside
    their range on both sides, samples with repeats in range elsewhere, NaN in every pad, table entries past cnt valid."""
    for c in K.GATHERS:
        s, inp = c.shape, c.built().inp
        assert np.isnan(inp['planes'][:, s.M:]).all() and not np.isnan(inp['planes'][:, :s.M]).any()
        if s.tables:
            assert np.isnan(inp['scale'][:, s.M:]).all() and np.isnan(inp['shift'][:, s.M:]).all()
        last = s.Ttot - s.C
        if s.kind in ('plain', 'reflect', 'mix'):
            rows = inp['rows'].reshape(-1)
            assert {0, last} <= set(rows.tolist()) and rows.min() < 0 and rows.max() > last
            if inp['sample'] is not None:
                assert inp['sample'].min() == 0 and inp['sample'].max() == s.S - 1 and len(set(inp['sample'].tolist())) < s.B
        if s.kind == 'reflect' and not s.tshift_null:
            assert {0, min(1, s.C - 1), s.C - 1} <= set(inp['tshift'].tolist()) and inp['tshift'].min() < 0 and inp['tshift'].max() >= s.C
        if s.kind == 'mix':
            assert inp['rows'].shape == (s.S, s.smax)
            for w, n in enumerate(K.clamp(inp['cnt'], 1, s.smax) if s.smax == K.K.GWM_MAX else ()):
                beyond = K.clamp(inp['rows'][w, n:], 0, last)
                assert n == s.smax or (len(set(beyond.tolist()) - set(K.clamp(inp['rows'][w, :n], 0, last).tolist())) > 0)
        if s.kind == 'indexed':
            idx = inp['idx']
            assert idx.shape == (s.S, s.C * s.fold) and len(set(idx[0].tolist())) == 1
            if idx.shape[1] > 1:
                assert (np.diff(idx[1]) < 0).sum() >= idx.shape[1] - 1 - idx.shape[1] // s.Ttot          # it wraps at row 0
            if s.S > 2:
                assert idx[2].min() < 0 and (idx[2].max() >= s.Ttot or idx.shape[1] == 1)
            if s.src:
                assert inp['src'].min() < 0 and (inp['src'].max() >= s.S or s.smax == 1) and inp['cnt'].max() > s.smax
                assert (K.clamp(inp['cnt'], 1, s.smax) == s.n).all()
            if inp['sample'] is not None:
                nwin = s.W if s.src else s.S
                assert inp['sample'].min() < 0 and inp['sample'].max() >= nwin
    for c in K.DROPS:
        s, inp = c.shape, c.built().inp
        assert (inp['pos'] is None) == (s.pos == 'null')
        if s.pos == 'perm':
            assert sorted(inp['pos'].tolist()) == list(range(s.M))
        if s.pos == 'edge':
            assert inp['pos'].min() < 0 or inp['pos'].max() >= s.M
        assert c.built().written.any() and not c.built().written[..., s.M:].any()
        if s.D > 1:
            v = series.drop_vertices(s.seed, s.refill, inp['win'].astype(np.int64), s.D, s.M)
            assert s.M > 1 or (v == 0).all()
    for c in K.of('window_stats'):
        s, rows = c.shape, c.built().inp['rows']
        last = s.Ttot - s.C
        assert rows.shape == (s.S,)
        if s.special is None and s.S > 1:
            got = set(rows.tolist())
            assert {0, last} <= got and rows.min() < 0 and rows.max() > last and len(got) < s.S
            for b in range(K.K.WS_ROWS, s.Ttot, K.K.WS_ROWS):
                assert any(r < b <= r + s.C - 1 for r in rows) or s.C == 1 or b > last + s.C - 1, (c.id, b)
                assert (min(last, b - 1) in got) and (min(last, b) in got)
        if s.special == 'equal':
            assert len(set(rows.tolist())) == 1 and s.S > 1
    for c in K.of('window_stats_indexed'):
        s, idx = c.shape, c.built().inp['idx']
        assert idx.shape == (s.S, s.C * s.fold)
        if s.S > 2:
            assert idx.min() < 0 and (idx.max() >= s.Ttot or idx.shape[1] == 1)


# ------------------------------------------------------------------------------------------------------------------ references

def test_the_float32_restatements_lie_within_the_projects_bound_of_the_float64_mean():
    """|restatement - float64 mean| <= n 2^-23 max|x| over the n terms of a mean (tests/test_gpu_balance.py), before the tables."""
    checked = 0
    for c in K.GATHERS:
        s = c.shape
        if s.kind not in ('mix', 'indexed') or s.tables or s.sample:
            continue
        b = c.built()
        mean, top, terms = K.gather_mean64(s, b.inp)
        err = np.abs(b.ref[:, :, :s.M] - mean)
        assert (err <= terms * 2.0 ** -23 * top).all(), c.id
        assert not gb.bits(b.ref[:, :, s.M:]).any()
        checked += 1
    assert checked >= 2 * K.K.GWM_MAX + len(K.SPECIALISED)


def test_the_plain_restatement_is_a_copy_of_the_series():
    for c in K.of('gather_windows'):
        s, b = c.shape, c.built()
        if s.tables:
            continue
        who = np.arange(s.B) if b.inp['sample'] is None else b.inp['sample']
        for i, w in enumerate(who):
            r = int(min(max(b.inp['rows'][w], 0), s.Ttot - s.C))
            assert np.array_equal(gb.bits(b.ref[i, :, :s.M]), gb.bits(b.inp['planes'][r:r + s.C, :s.M]))


def test_the_reflect_restatement_is_numpys_symmetric_pad():
    for c in K.of('gather_windows_reflect'):
        s, b = c.shape, c.built()
        if s.tables or s.tshift_null:
            continue
        who = np.arange(s.B) if b.inp['sample'] is None else b.inp['sample']
        for i, w in enumerate(who):
            r0 = int(min(max(b.inp['rows'][w], 0), s.Ttot - s.C))
            sh = int(min(max(b.inp['tshift'][w], 0), s.C - 1))
            x = b.inp['planes'][r0:r0 + s.C, :s.M]
            assert np.array_equal(gb.bits(b.ref[i, :, :s.M]), gb.bits(np.pad(x, ((s.C, s.C), (0, 0)), 'symmetric')[sh + s.C:sh + 2 * s.C]))


def test_the_exact_cases_are_exact():
    n = 0
    for c in K.STATS:
        s, b = c.shape, c.built()
        x = K.stats_windows(s, b.inp)
        assert x.shape == (s.S, s.C, s.M)
        if s.leg == 'exact':
            assert np.abs(x).max() <= 8
            assert K.exact_in_fractions(x, b.ref), c.id
            n += 1
        if s.const_vertex is not None:
            assert not b.ref['var'][:, s.const_vertex].any()
    assert n == len([c for c in K.STATS if c.shape.leg == 'exact']) > 50


def test_the_workspace_formulas_are_the_sources():
    """The restated byte counts (the library's own queries are compared with them on the device)."""
    k = K.K
    assert K.stats_count_bytes(k, 515, 9) == ((515 + 9 - 1 + 8 + 4) * 4 + 15) // 16 * 16
    assert K.stats_workspace(k, 515, 33, 9) == K.stats_count_bytes(k, 515, 9) + 2 * 4 * 9 * 64 * 8
    assert K.stats_indexed_workspace(k, 35, 33, 3) == 3 * 4 * 3 * 64 * 8


# ------------------------------------------------------------------------------------------------------------------- stand-ins
# The kernels' index arithmetic in NumPy.  ``fault``: None, or the one planted fault.

def _zero_pad(r, e, Mq, M, fault):
    m = 4 * (e % Mq)
    outer = (m + 3 > M) if fault == 'pad rule m + 3 > M' else (m + 3 >= M)
    lanes = m[:, None] + np.arange(4)[None, :]
    r[outer[:, None] & ((lanes >= M) | (np.arange(4)[None, :] == 3))] = 0
    return r


def sim_gather(k, c, fault=None):
    """gather_windows_kernel, _mix_, _indexed_ and _reflect_kernel: workgroup (block of GW_T * GW_U pieces, window b), passes of
    GW_T * U pieces, U pieces per thread."""
    s, inp = c.shape, c.built().inp
    planes, C, M, Ttot = inp['planes'], s.C, s.M, s.Ttot
    Mq = planes.shape[1] // 4
    CMq, tile = C * Mq, k.GW_T * k.GW_U
    series4 = planes.reshape(-1, 4)
    scale4 = None if inp['scale'] is None else inp['scale'].reshape(-1, 4)
    shift4 = None if inp['shift'] is None else inp['shift'].reshape(-1, 4)
    out = gb.filled(gb.FILL_B, np.float32, (s.B, CMq, 4))
    blocks = CMq // tile if fault == 'the tail block not launched' else -(-CMq // tile)
    f32 = np.float32
    for b in range(s.B):
        w = b if inp['sample'] is None else int(inp['sample'][b])
        if s.kind in ('plain', 'reflect'):
            L, row = 1, int(K.clamp(inp['rows'][w], 0, Ttot - C))
            r_ = 0 if s.kind == 'plain' or inp['tshift'] is None else int(K.clamp(inp['tshift'][w], 0, C - 1))

            def value(e):
                ch, q = e // Mq, e % Mq
                j = ch + r_
                j = np.where(j < C, j, 2 * C - (2 if fault == 'the reflection off by one at j = C' else 1) - j)
                return series4[(row + j) * Mq + q]
        elif s.kind == 'mix':
            n = L = int(K.clamp(inp['cnt'][w], 1, s.smax))
            src = [int(K.clamp(inp['rows'][w, j], 0, Ttot - C)) for j in range(n)]

            def value(e):
                r = series4[src[0] * Mq + e]
                for j in range(1, n - 1 if fault == 'the last source dropped' else n):
                    r = (r + series4[src[j] * Mq + e]).astype(f32)
                if n > 1:
                    r = (r / f32(s.smax if fault == 'division by smax' else n)).astype(f32)
                return r
        else:
            S, fold = inp['idx'].shape[0], s.fold
            n = 1
            if s.src:
                w = int(K.clamp(w, 0, inp['src'].shape[0] - 1))
                n = int(K.clamp(inp['cnt'][w], 1, s.smax))
                sw = [int(K.clamp(inp['src'][w, j], 0, S - 1)) for j in range(n)]
            else:
                sw = [int(K.clamp(w, 0, S - 1))]
            L = fold * n if (fold, n) in K.SPECIALISED else 0           # 0: the generic loop, one piece at a time
            idx = inp['idx']

            def value(e):
                ch, q = e // Mq, e % Mq
                r = None
                for j in range(n):
                    x = series4[K.clamp(idx[sw[j], ch], 0, Ttot - 1) * Mq + q]
                    for f in range(1, fold):
                        x = (x + series4[K.clamp(idx[sw[j], f * C + ch], 0, Ttot - 1) * Mq + q]).astype(f32)
                    if fold > 1 and fault != 'the fold division omitted':
                        x = (x / f32(fold)).astype(f32)
                    r = x if j == 0 else (r + x).astype(f32)
                return (r / f32(n)).astype(f32) if n > 1 else r
        U = K.width(k, L) if L else 1
        P = k.GW_U // U
        lanes = (np.arange(U)[:, None] * k.GW_T + np.arange(k.GW_T)[None, :]).reshape(-1)
        for bx in range(blocks):
            for p in range(P - 1 if fault == 'the last pass skipped' and P > 1 else P):
                e = bx * tile + p * k.GW_T * U + lanes
                e = e[e < CMq]
                if not e.size:
                    continue
                r = np.array(value(e), f32)
                if scale4 is not None:
                    r = ((r * scale4[e]).astype(f32) + shift4[e]).astype(f32)
                out[b, e] = _zero_pad(r, e, Mq, M, fault)
    return out.reshape(s.B, C, 4 * Mq)


def sim_drop(k, c, fault=None):
    """window_drop_kernel: one thread per draw, WD_T a workgroup."""
    s, inp = c.shape, c.built().inp
    x = inp['x0'].copy()
    total = s.B * s.D
    blocks = total // k.WD_T if fault == 'the tail block not launched' else -(-total // k.WD_T)
    t = np.arange(blocks * k.WD_T)
    t = t[t < total]
    b, d = t // s.D, t % s.D
    u = series.aug_draw(s.seed, s.refill, inp['win'].astype(np.int64)[b], d.astype(np.uint64))
    p = ((u * np.uint64(s.M)) >> np.uint64(32)).astype(np.int64)
    if inp['pos'] is not None:
        p = K.clamp(inp['pos'][p], 0, s.M - 1)
    for ch in range(s.C):
        v = np.full(len(t), np.float32(s.drop_value), np.float32)
        if inp['scale'] is not None:
            v = ((v * inp['scale'][ch, p]).astype(np.float32) + inp['shift'][ch, p]).astype(np.float32)
        x[b, ch, p] = v
    return x


def _finish(planes, part, S, M, delta):
    """window_stats_finish_kernel: the chunks' partials in index order, then the tables; the pad of all four zero.  The kernels
    carry every sum as a pair of doubles; the stand-in, whose subject is the index arithmetic, reaches the same accuracy in
    plain float64 by summing the deviations from the FIRST window (``delta`` [C, Mp]: first window - series[0]), which is the
    same mean and variance in exact arithmetic and exact on the exact leg."""
    a, q = np.zeros(part.shape[2:]), np.zeros(part.shape[2:])
    for g in range(part.shape[0]):
        a, q = a + part[g, 0], q + part[g, 1]
    da = a / float(S)
    mu = (planes[0].astype(np.float64)[None, :] + delta) + da
    va = q / float(S) - da * da
    with np.errstate(invalid='ignore'):
        va = np.where(va > 0, va, np.where(np.isnan(va), va, 0.0))
        zero = va == 0
        sd = np.sqrt(np.where(zero, 1.0, va))
        got = {'mean': mu, 'var': va, 'scale': np.where(zero, 1.0, 1.0 / sd).astype(np.float32),
               'shift': np.where(zero, -mu, -mu / sd).astype(np.float32)}
    for v in got.values():
        v[:, M:] = 0
    return got


def sim_stats(k, c, fault=None):
    """window_count_kernel + window_stats_partial_kernel (tile of vertices x group of WS_CG channels, chunk of WS_ROWS rows, four
    rows a turn) + finish.  Float64 sums in NumPy's order: exact on the exact leg, inside the bound on the other."""
    s, inp = c.shape, c.built().inp
    planes, C, Ttot, R = inp['planes'], s.C, s.Ttot, k.WS_ROWS
    lead = C - 1 + k.WS_CG
    cnt = np.zeros(lead + Ttot + 4, np.int64)
    np.add.at(cnt, lead + K.clamp(inp['rows'], 0, Ttot - C), 1)
    G = Ttot // R if fault == 'the chunk count floored' else -(-Ttot // R)
    part = np.full((G, 2, C, planes.shape[1]), np.nan)
    base = planes[0].astype(np.float64)
    delta = planes[int(K.clamp(inp['rows'][0], 0, Ttot - C)) + np.arange(C)].astype(np.float64) - base
    for g in range(G):
        u0, u1 = g * R, min(g * R + R, Ttot)
        if fault == 'the rows of a chunk tail dropped':
            u1 = u0 + (u1 - u0) // 4 * 4
        rows = np.arange(u0, u1)
        d = planes[rows].astype(np.float64) - base
        for c0 in range(0, C, k.WS_CG):
            nc = min(k.WS_CG, C - c0) - (1 if fault == 'a channel group ends one channel early' else 0)
            for ch in range(c0, c0 + nc):
                wgt = cnt[lead + rows - ch + (1 if fault == 'the count table read one row off' else 0)].astype(np.float64)
                live = wgt != 0
                dc = d[live] - delta[ch]
                part[g, 0, ch] = (wgt[live, None] * dc).sum(axis=0)
                part[g, 1, ch] = (wgt[live, None] * dc * dc).sum(axis=0)
    return _finish(planes, part, s.S, s.M, delta)


def sim_stats_indexed(k, c, fault=None):
    """window_stats_indexed_partial_kernel (channel c, chunk of wsi_chunk(S) windows, four windows a turn behind a clamped
    window index) + finish."""
    s, inp = c.shape, c.built().inp
    planes, C, S = inp['planes'], s.C, s.S
    idx = K.clamp(inp['idx'], 0, s.Ttot - 1)
    terms = [planes[idx[:, f * C:(f + 1) * C]] for f in range(s.fold)]
    piece = terms[0]
    for t in terms[1:]:
        piece = (piece + t).astype(np.float32)
    if s.fold > 1 and fault != 'the fold division omitted':
        piece = (piece / np.float32(s.fold)).astype(np.float32)
    chunk = K.wsi_chunk(k, S)
    G = S // chunk if fault == 'the chunk count floored' else -(-S // chunk)
    part = np.full((G, 2, C, planes.shape[1]), np.nan)
    base = planes[0].astype(np.float64)
    delta = piece[0].astype(np.float64) - base
    for g in range(G):
        w0, w1 = g * chunk, min(g * chunk + chunk, S)
        wins = [min(wb + i, w1 - 1) for wb in range(w0, w1, 4) for i in range(4)
                if (wb + i <= w1 if fault == 'the last window of a chunk counted twice' else wb + i < w1)]
        d = (piece[wins].astype(np.float64) - base) - delta
        part[g, 0], part[g, 1] = d.sum(axis=0), (d * d).sum(axis=0)
    return _finish(planes, part, S, s.M, delta)


def compare(k, c, fault=None):
    """The stand-in of the case's kernel against the case's reference, with the comparison the device module uses."""
    b, kind = c.built(), c.shape.kind
    if kind == 'drop':
        K.check_bits(c.id, sim_drop(k, c, fault), b.ref)
    elif kind == 'stats':
        K.check_stats(c.id, c.shape, sim_stats(k, c, fault), b.ref)
    elif kind == 'stats_indexed':
        K.check_stats(c.id, c.shape, sim_stats_indexed(k, c, fault), b.ref)
    else:
        K.check_bits(c.id, sim_gather(k, c, fault), b.ref)


def test_the_unfaulted_stand_ins_equal_the_reference_on_every_case():
    for c in K.ALL:
        compare(K.K, c)


GATHER_KINDS, STATS_KINDS = ('plain', 'mix', 'indexed', 'reflect'), ('stats', 'stats_indexed')
FAULTS = [('the last pass skipped', ('mix',)), ('the last pass skipped', ('indexed',)), ('the last source dropped', ('mix',)),
          ('division by smax', ('mix',)), ('the fold division omitted', ('indexed',)), ('the fold division omitted', ('stats_indexed',)),
          ('the reflection off by one at j = C', ('reflect',)), ('pad rule m + 3 > M', GATHER_KINDS),
          ('a channel group ends one channel early', ('stats',)), ('the rows of a chunk tail dropped', ('stats',)),
          ('the count table read one row off', ('stats',)), ('the chunk count floored', ('stats',)),
          ('the chunk count floored', ('stats_indexed',)), ('the last window of a chunk counted twice', ('stats_indexed',)),
          ('the tail block not launched', ('plain',)), ('the tail block not launched', ('drop',))]


@pytest.mark.parametrize('fault,kinds', FAULTS, ids=['%s (%s)' % (f, '/'.join(ks)) for f, ks in FAULTS])
def test_a_planted_fault_is_caught(fault, kinds):
    """One fault in the stand-in of the kernels of ``kinds``: the device module's comparison fails on at least one case, in both
    tables arms of the gathers."""
    # (the exact leg of the indexed statistics has chunks of 1 and 16 windows only -- S must be a power of two -- so it cannot
    # see a fault in the unroll tail: the statistics' faults must be caught in the table as a whole)
    groups = [dict()] if kinds[0] in STATS_KINDS else [dict(tables=t) for t in TABLES]
    for where in groups:
        caught = []
        for c in K.ALL:
            if c.shape.kind in kinds and all(getattr(c.shape, a) == v for a, v in where.items()):
                try:
                    compare(K.K, c, fault)
                except AssertionError:
                    caught.append(c.id)
        print('%s, %s: caught by %d cases, e.g. %s' % (fault, where, len(caught), caught[:3]))
        assert caught, (fault, where)
