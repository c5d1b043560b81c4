"""The float64 restatements tests/test_gpu_spectral_kernels.py uses as truth for the kernels of csrc/spectral.hip, on written-out
values and against an explicit loop over the reduction index, and the host-side figures that test relies on: the exactness
inequality of its exact leg, the launch geometry restated from the constants of spectral.hip, the case tables, the buffers
every launch is given, and that "bit-equal" discriminates -- the exact leg's inputs tell each restatement from its near misses
(a mask off by one, analysis for synthesis, W[m] transposed, a window dropped, a k dropped).  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gcn_fmri_decoding_amd._lib import SIGNATURES, plane_stride

import test_gpu_spectral_kernels as T

SOURCE = open(os.path.join(ROOT, 'gcn_fmri_decoding_amd', 'csrc', 'spectral.hip')).read()
BOTH = (False, True)


# ------------------------------------------------------------------------------------------------------------ restatements

def test_restatements_on_written_out_values():
    x, U = [[1, 2], [3, 4]], [[1, 2], [3, 4]]
    assert T.transform_ref(x, U, False).tolist() == [[7, 10], [15, 22]]                 # x U
    assert T.transform_ref(x, U, True).tolist() == [[5, 11], [11, 25]]                  # x U^T
    W = [[[1, 2], [3, 4]], [[5, 6], [7, 8]]]                                            # W[m][o][f], M = 2
    p = [[[1, 2], [3, 4]]]                                                              # planes [b][f or o][m], B = 1
    assert T.mix_fwd_ref(W, p).tolist() == [[[7, 34], [15, 46]]]                        # m = 0: W[0] (1, 3); m = 1: W[1] (2, 4)
    assert T.mix_bwd_x_ref(W, p).tolist() == [[[10, 38], [14, 44]]]                     # W[m]^T on the same columns
    dyh = [[[1, 2]], [[3, 4]]]                                                          # B = 2, Fout = 1
    xh = [[[1, 2], [3, 4]], [[5, 6], [7, 8]]]                                           # Fin = 2
    assert T.mix_bwd_w_ref(dyh, xh).tolist() == [[[16, 24]], [[28, 40]]]
    Bs = [[1, 2], [3, 4], [5, 6]]                                                       # M = 3, K = 2
    assert T.spline_ref(Bs, [[1, 0, -1], [2, 1, 0]]).tolist() == [[5, 2, -1], [11, 4, -3], [17, 6, -5]]
    assert T.spline_bwd_ref(Bs, [[1, 2], [3, 4], [5, 6]]).tolist() == [[35, 44], [44, 56]]
    # a frequency mixes only its own column, a window only its own planes
    one = np.zeros((2, 2, 3))
    one[1, 0, 2] = 1
    Wr = np.arange(1, 13).reshape(3, 2, 2)
    y = T.mix_fwd_ref(Wr, one)
    assert np.count_nonzero(y) == 2 and y[1, :, 2].tolist() == [Wr[2, 0, 0], Wr[2, 1, 0]]


def _loops(job_or_name, a, b, transpose=False):
    """The six operations as explicit loops over the reduction index, in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if job_or_name == 'transform':
        x, U = a, b
        out = np.zeros((x.shape[0], U.shape[0]))
        for m in range(U.shape[0]):
            out += x[:, m:m + 1] * (U[:, m] if transpose else U[m, :])[None, :]
        return out
    if job_or_name == 'mix':
        W, p = a, b
        M, Fout, Fin = W.shape
        out = np.zeros((p.shape[0], Fin if transpose else Fout, M))
        for i in range(Fout if transpose else Fin):
            Wi = W[:, i, :] if transpose else W[:, :, i]                               # [M, No]
            out += Wi.T[None, :, :] * p[:, i:i + 1, :]
        return out
    if job_or_name == 'bwd_w':
        dyh, xh = a, b
        out = np.zeros((dyh.shape[2], dyh.shape[1], xh.shape[1]))
        for w in range(dyh.shape[0]):
            out += dyh[w].T[:, :, None] * xh[w].T[:, None, :]
        return out
    Bs, V = a, b
    if transpose:                                                                      # expand_bwd: over m
        out = np.zeros((Bs.shape[1], V.shape[1]))
        for m in range(Bs.shape[0]):
            out += Bs[m][:, None] * V[m][None, :]
        return out
    out = np.zeros((Bs.shape[0], V.shape[1]))
    for k in range(Bs.shape[1]):
        out += Bs[:, k:k + 1] * V[k][None, :]
    return out


def test_restatements_equal_a_loop_over_the_reduction_index():
    """On the exact leg's integers the two formulations agree exactly; on the round-off leg's within float64 round-off."""
    eps = np.finfo(np.float64).eps
    for exact in BOTH:
        def same(got, ref, n):
            assert got.shape == ref.shape
            assert np.array_equal(got, ref) if exact else np.abs(got - ref).max() <= 4 * n * eps * max(np.abs(ref).max(), 1.0)
        for c in (T.Tr(5, 3), T.Tr(33, 65)):
            x, U = T.transform_data(c, exact)
            for tr in BOTH:
                same(T.transform_ref(x, U, tr), _loops('transform', x, U, tr), c.M)
        for c in (T.Mix(3, 2, 5, 7), T.Mix(5, 9, 8, 65)):
            for tr in BOTH:
                W, p = T.mix_data(c, exact, tr)
                same((T.mix_bwd_x_ref if tr else T.mix_fwd_ref)(W, p), _loops('mix', W, p, tr), max(c.Fin, c.Fout))
        for c in (T.Bww(3, 2, 5, 7), T.Bww(9, 5, 7, 130)):
            dyh, xh = T.bwd_w_data(c, exact)
            same(T.mix_bwd_w_ref(dyh, xh), _loops('bwd_w', dyh, xh), c.B)
        for c in (T.Spl(3, 2, 5), T.Spl(100, 7, 257)):
            for bwd in BOTH:
                Bs, V = T.spline_data(c, exact, bwd)
                same((T.spline_bwd_ref if bwd else T.spline_ref)(Bs, V), _loops('spline', Bs, V, bwd), max(c.M, c.K))


# ------------------------------------------------------------------------------------------------------------ jobs and buffers

def _jobs(c, exact):
    """name -> Job of every launch the GPU file makes for case ``c``."""
    if isinstance(c, T.Tr):
        return {'transform<%d>' % tr: T.transform_job(c, exact, tr) for tr in BOTH}
    if isinstance(c, T.Mix):
        return {'mix<%d>' % tr: T.mix_job(c, exact, tr) for tr in BOTH}
    if isinstance(c, T.Bww):
        return {'bwd_w': T.bwd_w_job(c, exact)}
    return {'spline<%d>' % bwd: T.spline_job(c, exact, bwd) for bwd in BOTH}


def _ids(c):
    return type(c).__name__ + '-' + T.case_id(c)


def _buffer_shapes(job):
    """(shapes of the two inputs, shape of the output) that the entry point's header comment gives for ``job.args``."""
    a = job.args
    if job.entry == 'chebgcn_spectral_transform':
        Mp = plane_stride(a[1])
        return [(a[0], Mp), (Mp, Mp)], (a[0], Mp)
    if job.entry.startswith('chebgcn_spectral_mix'):
        B, M, Fin, Fout = a
        Mp = plane_stride(M)
        return {'chebgcn_spectral_mix_fwd': ([(B, Fin, Mp), (M, Fout, Fin)], (B * Fout, Mp)),
                'chebgcn_spectral_mix_bwd_x': ([(B, Fout, Mp), (M, Fout, Fin)], (B * Fin, Mp)),
                'chebgcn_spectral_mix_bwd_w': ([(B, Fout, Mp), (B, Fin, Mp)], (M, Fout * Fin))}[job.entry]
    M, K, C = a
    if job.entry == 'chebgcn_spectral_spline_expand':
        return [(M, K), (K, C)], (M, C)
    return [(M, K), (M, C)], (K, C)


@pytest.mark.parametrize('c', T.ALL_CASES, ids=_ids)
def test_every_launch_is_given_the_buffers_its_arguments_describe(c):
    """Shapes and types of the inputs and of the output of every job against the entry point's own layout; NaN over every input
    plane's pad with +Inf in one plane; a zero pad in the basis; no denormal and, in the exact leg, no zero operand; the
    exactness inequality; a reference that is an fp32 number; a positive round-off bound wherever the reference is not 0."""
    for exact in BOTH:
        for name, job in _jobs(c, exact).items():
            ins, out = _buffer_shapes(job)
            assert job.entry in SIGNATURES and len(SIGNATURES[job.entry][1]) == 3 + len(job.args) + 1
            assert [i.shape for i in job.ins] == ins and all(i.dtype == np.float32 for i in job.ins), (name, ins)
            assert (job.rows, job.cols) == out and job.ref.shape == job.absdot.shape == (job.rows, job.data)
            assert job.expect in T.ARMS and job.expect.split('<')[0] in SOURCE
            assert T.exact_leg_is_exact(job.n) and job.n >= 1
            planes = {'chebgcn_spectral_transform': [0], 'chebgcn_spectral_mix_fwd': [0], 'chebgcn_spectral_mix_bwd_x': [0],
                      'chebgcn_spectral_mix_bwd_w': [0, 1]}.get(job.entry, [])
            for k, a in enumerate(job.ins):
                if k in planes:
                    M = job.args[1]
                    flat = a.reshape(-1, a.shape[-1])
                    assert np.isfinite(flat[:, :M]).all() and not np.isfinite(flat[:, M:]).any()
                    assert job.data == M or job.entry == 'chebgcn_spectral_mix_bwd_w'
                    if a.shape[-1] > M:
                        assert np.isinf(flat[flat.shape[0] // 2, M:]).all()
                        assert np.isnan(flat[:, M:]).sum() == (flat.shape[0] - 1) * (a.shape[-1] - M)
                    a = flat[:, :M]
                elif job.entry == 'chebgcn_spectral_transform':
                    M = job.args[1]
                    assert not a[M:].any() and not a[:, M:].any()
                    a = a[:M, :M]
                assert np.isfinite(a).all() and not ((a != 0) & (np.abs(a) < T.TINY)).any()
                if exact:
                    assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 4 and np.abs(a).min() >= 1
            if exact:
                assert np.array_equal(job.ref.astype(np.float32).astype(np.float64), job.ref) and np.abs(job.ref).max() <= 16 * job.n
                assert np.array_equal(job.ref, np.round(job.ref))
            else:
                assert (job.absdot >= np.abs(job.ref) * (1 - 1e-12)).all()


def test_exact_leg_is_exact_at_its_limit():
    """16 n + 1 < 2^24: the sums of n products of magnitude <= 16 and one more unit stay below 2^24, where fp32 holds every
    integer."""
    assert T.exact_leg_is_exact(2 ** 20 - 1) and not T.exact_leg_is_exact(2 ** 20)
    assert np.float32(16 * (2 ** 20 - 1)) + np.float32(1) == 16 * (2 ** 20 - 1) + 1
    assert np.float32(2 ** 24) + np.float32(1) == 2 ** 24                                # ... and past it they do not
    assert max(max(j.n for j in _jobs(c, True).values()) for c in T.ALL_CASES) == 130


# ------------------------------------------------------------------------------------------------------------ discrimination

def _differs(what, ref, mutant):
    assert ref.shape == mutant.shape, what
    assert (ref != mutant).any(), what + ': the exact leg cannot see this mutant'
    return (ref != mutant).mean()


@pytest.mark.parametrize('c', T.ALL_CASES, ids=_ids)
def test_exact_leg_tells_the_restatement_from_its_near_misses(c):
    """For every case the exact leg's reference differs from: the reduction without its last term (a mask off by one) and, no
    operand being 0, in EVERY element; analysis for synthesis (M > 1); W[m] read as [Fin][Fout] (Fin * Fout > 1); bwd_w without
    its first, its last, or any one wave's first window; the spline sums without one k (one m for the gradient)."""
    if isinstance(c, T.Tr):
        x, U = T.transform_data(c, True)
        for tr in BOTH:
            ref = T.transform_ref(x, U, tr)
            less = T.transform_ref(x[:, :-1], U[:, :-1] if tr else U[:-1], tr)
            assert _differs('mask', ref, less) == 1.0
            if c.M > 1:                                        # a 1 x 1 basis is its own transpose: the same function
                assert not np.array_equal(U, U.T)
                _differs('analysis for synthesis', ref, T.transform_ref(x, U, not tr))
    elif isinstance(c, T.Mix):
        for tr in BOTH:
            W, p = T.mix_data(c, True, tr)
            ref_fn = T.mix_bwd_x_ref if tr else T.mix_fwd_ref
            ref = ref_fn(W, p)
            less = ref_fn(W[:, :-1] if tr else W[:, :, :-1], p[:, :-1])
            assert _differs('mask', ref, less) == 1.0
            if c.Fin * c.Fout > 1:                             # a 1 x 1 W[m] is its own transpose: the same function
                Wt = W.reshape(c.M, c.Fin, c.Fout).transpose(0, 2, 1)                    # o * Fin + i read as i * Fout + o
                assert not np.array_equal(W, Wt)
                if c.Fin == c.Fout:
                    assert all(not np.array_equal(Wm, Wm.T) for Wm in W)
                _differs('W[m] transposed', ref, ref_fn(Wt, p))
    elif isinstance(c, T.Bww):
        dyh, xh = T.bwd_w_data(c, True)
        ref = T.mix_bwd_w_ref(dyh, xh)
        starts = {b for b, e in T.bwd_w_geometry(c.B, c.M, c.Fin, c.Fout)['ranges'] if e > b} | {0, c.B - 1}
        for w in sorted(starts):
            keep = [b for b in range(c.B) if b != w]
            assert _differs('window %d dropped' % w, ref, T.mix_bwd_w_ref(dyh[keep], xh[keep])) == 1.0
        if c.Fin * c.Fout > 1:
            _differs('dW[m] transposed', ref.reshape(c.M, -1), ref.transpose(0, 2, 1).reshape(c.M, -1))
    else:
        for bwd in BOTH:
            Bs, V = T.spline_data(c, True, bwd)
            ref = (T.spline_bwd_ref if bwd else T.spline_ref)(Bs, V)
            for drop in sorted({0, (c.M if bwd else c.K) - 1}):
                if bwd:
                    keep = [m for m in range(c.M) if m != drop]
                    less = T.spline_bwd_ref(Bs[keep], V[keep])
                else:
                    keep = [k for k in range(c.K) if k != drop]
                    less = T.spline_ref(Bs[:, keep], V[keep])
                assert _differs('term %d dropped' % drop, ref, less) == 1.0


def test_round_off_leg_draws_its_spline_basis_from_bspline_basis():
    """Every row of the round-off leg's Bs is a partition of unity with at most degree + 1 non-zero entries."""
    for c in T.SPL_CASES:
        Bs, _ = T.spline_data(c, False, False)
        assert Bs.shape == (c.M, c.K) and Bs.dtype == np.float32 and (Bs >= 0).all()
        assert np.abs(Bs.sum(axis=1) - 1).max() <= 1e-6 and (np.count_nonzero(Bs, axis=1) <= min(4, c.K)).all()
    assert any((np.count_nonzero(T.spline_data(c, False, False)[0], axis=1) == 4).any() for c in T.SPL_CASES)


# ------------------------------------------------------------------------------------------------------------ geometry

def _constants():
    found = {}
    for line in re.findall(r'^constexpr int ([^;]+);', SOURCE, re.M):
        for name, value in re.findall(r'(\w+)\s*=\s*(\d+)', line):
            found[name] = int(value)
    return found


def test_geometry_is_restated_from_the_kernels_constants():
    k = _constants()
    assert (k['TR_ROWS'], k['TR_COLS']) == (T.TR_ROWS, T.TR_COLS) and (k['MIX_NB'], k['MIX_OT']) == (T.MIX_NB, T.MIX_OT)
    assert (k['WG_OT'], k['WG_IT']) == (T.WG_OT, T.WG_IT)
    # four tiles, four window groups, four partial sums per workgroup; the grids as the entry points compute them
    for text in ('const int tile = blockIdx.x * 4 + wave;', 'dim3 grid((unsigned)((tiles + 3) / 4));',
                 'const int ntc = (Mp + TR_COLS - 1) / TR_COLS;', 'const bool two = j0 + 32 < Mp;',
                 'const int b0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * MIX_NB;',
                 'dim3 grid((Mp + 63) / 64, (B + 4 * MIX_NB - 1) / (4 * MIX_NB), (No + MIX_OT - 1) / MIX_OT);',
                 'const int nb = (B + 3) / 4;', 'const int bb = min(wave * nb, B), be = min(bb + nb, B);',
                 'dim3 grid((M + 63) / 64, (Fout + WG_OT - 1) / WG_OT, (Fin + WG_IT - 1) / WG_IT);',
                 'dim3((C + 255) / 256, M)', 'dim3((C + 255) / 256, K)'):
        assert text in SOURCE, text
    assert T.TR_WAVES == T.MIX_WAVES == T.WG_WAVES == 4
    g = T.transform_geometry(33, 65)
    assert g == dict(Mp=96, ntc=2, tiles=4, groups=1, idle=0, two_last=False, clamped=31, turns=3)
    assert T.transform_geometry(1, 1) == dict(Mp=32, ntc=1, tiles=1, groups=1, idle=3, two_last=False, clamped=31, turns=1)
    assert T.transform_geometry(129, 130)['tiles'] == 15 and T.transform_geometry(129, 32)['tiles'] == 5
    assert T.transform_geometry(64, 64)['two_last'] and T.transform_geometry(64, 128)['two_last']
    assert T.mix_geometry(17, 100, 33) == (2, 2, 5) and T.mix_geometry(16, 64, 8) == (1, 1, 1) and T.mix_geometry(5, 65, 32) == (2, 1, 4)
    assert T.bwd_w_geometry(5, 130, 9, 17) == dict(grid=(3, 3, 3), nb=2, ranges=[(0, 2), (2, 4), (4, 5), (5, 5)])
    assert T.bwd_w_geometry(1, 1, 1, 1)['ranges'] == [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert T.bwd_w_geometry(33, 63, 9, 8)['ranges'] == [(0, 9), (9, 18), (18, 27), (27, 33)]
    for arm in T.ARMS:
        assert 'note_dispatch("%s")' % arm in SOURCE, arm


def test_case_tables():
    reach = T.table_reach()
    assert set(reach) == set(T.ARMS) and all(reach[a] for a in T.ARMS)
    assert [len(reach[a]) for a in T.ARMS] == [13, 13, 8, 8, 8, 8, 8]
    # a table that misses an arm is told so
    saved = T.TR_CASES[:]
    try:
        T.TR_CASES[:] = [c for c in saved if c.M % 8 != 6]
        with pytest.raises(AssertionError, match='every M % 8'):
            T.table_reach()
    finally:
        T.TR_CASES[:] = saved
    saved = T.BWW_CASES[:]
    try:
        T.BWW_CASES[:] = [c for c in saved if c.Fin <= T.WG_IT] + [T.Bww(5, 4, 17, 130), T.Bww(9, 3, 7, 130)]
        with pytest.raises(AssertionError):
            T.table_reach()
    finally:
        T.BWW_CASES[:] = saved


def test_refusals_cover_every_entry_point():
    """The refused calls: every pointer of every entry point NULL in turn, in == out where the kernel reads what it writes, the
    shapes past each launch limit; the expected status is the one CG_REQUIRE returns."""
    name, value = T.require_status()
    header = open(os.path.join(ROOT, 'include', 'chebgcn.h')).read()
    assert name == 'CHEBGCN_EINVAL' and value < 0 and re.search(r'CHEBGCN_OK\s*=\s*0\b', header)
    calls = T.refused_calls()
    entries = [n for n in SIGNATURES if n.startswith('chebgcn_spectral_')]
    assert sorted(entries) == sorted(T.REFUSED_SHAPES) and len(entries) == 6
    for e in entries:
        mine = [c for c in calls if c[0] == e]
        assert sorted(c[2] for c in mine if c[2] is not None) == [0, 1, 2]
        assert any(c[3] for c in mine) == (e in T.IN_PLACE_REFUSED)
        assert all(len(c[4]) == len(SIGNATURES[e][1]) - 4 for c in mine)
    said = {(c[0].replace('chebgcn_spectral_', ''), c[1]) for c in calls}
    assert said >= {('transform', 'R = 0'), ('transform', 'R < 0'), ('transform', 'M > 32768'), ('mix_fwd', 'M > 32768'),
                    ('mix_bwd_x', 'M > 32768'), ('mix_bwd_w', 'M > 32768'), ('spline_expand', 'M > 65535'),
                    ('spline_expand_bwd', 'K > 65535')}
    # each limit as the source states it
    for text in ('R > 0 && M > 0 && M <= 32768', 'in != out', 'xh != yh', 'dyh != dxh', 'M > 0 && M <= 65535 && K > 0 && C > 0',
                 'M > 0 && K > 0 && K <= 65535 && C > 0'):
        assert text in SOURCE, text
    assert SOURCE.count('M <= 32768') == 4
