"""The window gathers and window statistics of csrc/series.hip and csrc/augment.hip at their edges: ``chebgcn_gather_windows``,
``_mix``, ``_indexed``, ``_reflect``, ``chebgcn_window_drop``, ``chebgcn_window_stats`` and ``chebgcn_window_stats_indexed``, each
called through ctypes with the argument list its ``ops`` wrapper uses, and through the wrapper.  Cases, references and
comparisons: tests/window_kernel_cases.py, checked on the host by tests/test_window_kernel_refs.py.  Per case:

  1. two runs into fresh ``guarded_buffers.Guarded`` regions, poison A (bytes 0xFF) then poison B (bytes 0x5A) in every output
     and workspace; series, tables and outputs of the gathers at 16-byte alignment and no more, int64 tables at 8, int32 at 4;
     a workspace is EXACTLY the ``*_workspace()`` byte count, which equals the restated formula;
  2. ``chebgcn_last_dispatch()`` after every call: ``<plain>`` / ``<tables>`` of every gather and drop launch, the count, partial
     and finish kernels of both statistics entries;
  3. after each run every guard band is intact and every input is byte-identical to its host copy;
  4. the two runs agree bit for bit on all of every output;
  5. gathers and drop: bit for bit the float32 restatement of include/chebgcn.h (pad zero; for the drop, every element the
     draws do not name keeps what it held).  The pad [M, Mp) of the series and of the tables holds NaN;
  6. statistics: ``window_kernel_cases.check_stats`` -- the bounds of tests/test_gpu_fit_series.py against float64 on both legs,
     mean and var bit for bit on the exact leg, the float32 tables bit for bit the device's own float64 rounded once, the
     constant vertex at variance 0, scale 1, shift -mean; ``window_stats`` gives the same bits under a permutation of rows;
  7. bit for bit what the ``ops`` wrapper returns on ordinary tensors.

Cross identities (all exact): mix at n = 1 is the plain gather; the indexed gather on contiguous indices is the plain gather
and, with sources, the mix gather at every N; reflect at shift 0 and without shifts is the plain gather; ``window_stats_indexed``
at fold 1 on contiguous indices lies within the same bound of ``window_stats`` and gives identical tables where the float64
results agree.

Measured on an MI355X: the module's 477 tests take 4.5 s together (the 462 guarded cases 1.2 s of it; the slowest is the first
launch of the process, plain-M1-C3-plain, 0.37 s; every other case 0.01 s or less).  Every bit-for-bit leg holds: all 234 gather
cases and 30 drop cases equal the float32 restatement, all cross identities hold, and mean and var of the 72 exact statistics
cases equal the float64 reference.  Worst ``err / bound`` of the bounded leg: ``window_stats`` mean 0 (every mean is the
reference's, bit for bit), var 0.089 (stats-bounded-M512-C8-T514); ``window_stats_indexed`` mean 0, var 0.115
(stats_indexed-bounded-S17-fold16-C1).  On contiguous indices the two statistics entries agree bit for bit in all four tables.

The bug this module found and the library fixed: with plain float64 sums of the deviations and of
their squares, 11 bounded cases missed the var bound -- every case of ONE window (stats-bounded-M33-C8-TC, -C9-TC, -C16-TC,
-C17-TC, -C9-T1027-one, stats_indexed-bounded-S1-fold1-C3, -S1-fold3-C1, -S1-fold16-C3: a variance of 1e-17 and so a scale of
1e8 where 0 and 1 are due) and few windows folded 16 times (stats_indexed-bounded-S15-fold16-C3, -S33-fold16-C3), whose spread
is small beside their distance from series[0].  The sums are pairs of doubles since; the same cases pass at the ratios above.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, ops
from gcn_fmri_decoding_amd._lib import plane_stride

import guarded_buffers as gb
import window_kernel_cases as K

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DTYPES = {np.dtype(np.float32): 'float32', np.dtype(np.float64): 'float64', np.dtype(np.int32): 'int32', np.dtype(np.int64): 'int64'}
F32, F64 = 'float32', 'float64'
TIMES = {}                      # case id -> seconds
RATIOS = {}                     # statistics case id -> (mean err / bound, var err / bound)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(r):
    return None if r is None else r.ptr


def dev(host):
    return None if host is None else torch.as_tensor(np.array(host)).to(DEV)


def region(host, fill, float_align):
    """A guarded input region that holds ``host`` (None: a NULL pointer)."""
    if host is None:
        return None
    host = np.ascontiguousarray(host)
    align = float_align if host.dtype == np.float32 else host.dtype.itemsize
    return gb.Guarded(host.shape, DTYPES[host.dtype], fill, DEV, align=align, init=host)


def two_fills(what, dispatch, inputs, outputs, ws_bytes, call, float_align=16):
    """Rules 1 - 4.  ``inputs`` {name: host array or None}; ``outputs`` {name: (shape, dtype name, align, init or None)};
    ``call(d, o, w)`` -> the entry's return code, with d / o the regions by name and w the workspace region (None without).
    Returns the outputs of run A as host arrays."""
    t0 = time.perf_counter()
    runs = {}
    for tag, fill in gb.FILLS:
        d = {k: region(v, fill, float_align) for k, v in inputs.items()}
        o = {k: gb.Guarded(shape, dtype, fill, DEV, align=align, init=init) for k, (shape, dtype, align, init) in outputs.items()}
        w = gb.Guarded((ws_bytes,), 'uint8', fill, DEV, align=16) if ws_bytes else None
        _lib.check(call(d, o, w), what)
        assert _lib.last_dispatch() == dispatch, (what, _lib.last_dispatch())
        torch.cuda.synchronize()
        for k, r in list(d.items()) + list(o.items()) + [('workspace', w)]:
            if r is not None:
                r.check('%s, fill %s, %s' % (what, tag, k))
        for k, r in d.items():
            if r is not None:
                assert np.array_equal(gb.bits(r.host().reshape(-1)), gb.bits(np.ascontiguousarray(inputs[k]).reshape(-1))), \
                    '%s, fill %s: input %s changed' % (what, tag, k)
        runs[tag] = {k: r.host() for k, r in o.items()}
    for k in outputs:
        a, b = gb.bits(runs['A'][k]), gb.bits(runs['B'][k])
        assert np.array_equal(a, b), '%s: runs A/B differ on %s at %d of %d elements, the first at %s' % (
            what, k, int((a != b).sum()), a.size, np.argwhere(a != b)[0].tolist())
    TIMES[what] = TIMES.get(what, 0.0) + time.perf_counter() - t0
    return runs['A']


# ====================================================================================================================== gathers

def gather_call(s, L):
    """``call(d, o, w)`` of a gather case of shape ``s``."""
    tail = lambda d, o: (P(d['sample']), P(d['scale']), P(d['shift']), P(o['out']), s.B, s.M, s.C, stream())
    if s.kind == 'plain':
        return lambda d, o, w: L.chebgcn_gather_windows(P(d['planes']), s.Ttot, P(d['rows']), *tail(d, o))
    if s.kind == 'reflect':
        return lambda d, o, w: L.chebgcn_gather_windows_reflect(P(d['planes']), s.Ttot, P(d['rows']), P(d['tshift']), *tail(d, o))
    if s.kind == 'mix':
        return lambda d, o, w: L.chebgcn_gather_windows_mix(P(d['planes']), s.Ttot, P(d['rows']), P(d['cnt']), s.smax, *tail(d, o))
    return lambda d, o, w: L.chebgcn_gather_windows_indexed(P(d['planes']), s.Ttot, P(d['idx']), s.S, s.C * s.fold, s.fold, P(d.get('src')),
                                                            P(d.get('cnt')), s.W if s.src else s.S, s.smax, *tail(d, o))


def gather_wrapper(s, inp):
    t = {k: dev(v) for k, v in inp.items()}
    rest = (t['sample'], t['scale'], t['shift'])
    if s.kind == 'plain':
        return ops.gather_windows(t['planes'], t['rows'], s.M, s.C, *rest)
    if s.kind == 'reflect':
        return ops.gather_windows_reflect(t['planes'], t['rows'], t['tshift'], s.M, s.C, *rest)
    if s.kind == 'mix':
        return ops.gather_windows_mix(t['planes'], t['rows'], t['cnt'], s.M, s.C, *rest)
    return ops.gather_windows_indexed(t['planes'], t['idx'], s.M, s.C, s.fold, t.get('src'), t.get('cnt'), *rest)


@pytest.mark.parametrize('c', K.GATHERS, ids=repr)
def test_gather(c):
    b, s = c.built(), c.shape
    shape = (s.B, s.C, plane_stride(s.M))
    got = two_fills(c.id, K.dispatch_name(c), b.inp, {'out': (shape, F32, 16, None)}, 0, gather_call(s, _lib.lib()))['out']
    K.check_bits(c.id, got, b.ref)
    assert not gb.bits(got[..., s.M:]).any(), '%s: pad not zero' % c.id
    K.check_bits(c.id + ' (wrapper)', gather_wrapper(s, b.inp).cpu().numpy(), got)
    assert _lib.last_dispatch() == K.dispatch_name(c)


def _contiguous(rows, C):
    return (rows.reshape(-1, 1) + np.arange(C)[None, :]).astype(np.int64)


@pytest.mark.parametrize('tables', [False, True], ids=['plain', 'tables'])
def test_cross_identities_of_the_gathers(tables):
    """Mix at n = 1, reflect at shift 0 and without shifts, indexed on contiguous indices: the plain gather; indexed with sources
    on contiguous indices: the mix gather at every N.  Bit for bit, over two blocks with a partial last pass."""
    M, C, S = K.M_AT_C, K.MIX_PASS_C[0], 6
    rs = K.rng('cross-%d' % tables)
    Ttot = C + 40
    planes = dev(K.series_planes(rs, Ttot, M))
    scale, shift = (dev(t) for t in K.tables(rs, C, M)) if tables else (None, None)
    rows = rs.randint(0, Ttot - C + 1, size=S).astype(np.int64)
    rows[:2] = (0, Ttot - C)
    sample = dev(K.sample_with_repeats(rs, S, 5))
    plain = ops.gather_windows(planes, dev(rows), M, C, sample, scale, shift).cpu().numpy()
    assert np.isfinite(plain).all() and not gb.bits(plain[..., M:]).any()
    smax = K.K.GWM_MAX
    table = rs.randint(0, Ttot - C + 1, size=(S, smax)).astype(np.int64)
    table[:, 0] = rows
    one = ops.gather_windows_mix(planes, dev(table), dev(np.ones(S, np.int32)), M, C, sample, scale, shift).cpu().numpy()
    K.check_bits('mix at n = 1 against the plain gather', one, plain)
    for name, tshift in (('zero shifts', dev(np.zeros(S, np.int32))), ('no shifts', None)):
        K.check_bits('reflect with %s against the plain gather' % name,
                     ops.gather_windows_reflect(planes, dev(rows), tshift, M, C, sample, scale, shift).cpu().numpy(), plain)
    K.check_bits('indexed on contiguous indices against the plain gather',
                 ops.gather_windows_indexed(planes, dev(_contiguous(rows, C)), M, C, 1, None, None, sample, scale, shift).cpu().numpy(), plain)
    # every window of the mix table as a window of idx; src names them
    idx, src = dev(_contiguous(table.reshape(-1), C)), dev(np.arange(S * smax, dtype=np.int64).reshape(S, smax))
    for N in range(1, smax + 1):
        cnt = dev(np.full(S, N, np.int32))
        mix = ops.gather_windows_mix(planes, dev(table), cnt, M, C, sample, scale, shift).cpu().numpy()
        assert _lib.last_dispatch() == 'gather_windows_mix_kernel<%s>' % ('tables' if tables else 'plain')
        ind = ops.gather_windows_indexed(planes, idx, M, C, 1, src, cnt, sample, scale, shift).cpu().numpy()
        assert _lib.last_dispatch() == 'gather_windows_indexed_kernel<%s>' % ('tables' if tables else 'plain')
        K.check_bits('indexed with sources against mix at N = %d' % N, ind, mix)


# ========================================================================================================================= drop

@pytest.mark.parametrize('c', K.DROPS, ids=repr)
def test_window_drop(c):
    b, s = c.built(), c.shape
    L = _lib.lib()
    inp = {k: v for k, v in b.inp.items() if k != 'x0'}
    got = two_fills(c.id, K.dispatch_name(c), inp, {'x': (b.inp['x0'].shape, F32, 4, b.inp['x0'])}, 0,
                    lambda d, o, w: L.chebgcn_window_drop(P(o['x']), P(d['win']), s.B, s.M, s.C, s.D, s.seed, s.refill, P(d['pos']),
                                                          P(d['scale']), P(d['shift']), s.drop_value, stream()), float_align=4)['x']
    K.check_bits(c.id, got, b.ref)                  # what the draws name is written, everything else -- the pad too -- kept
    assert (gb.bits(got) != gb.bits(b.inp['x0']))[b.written].all() and not (gb.bits(got) != gb.bits(b.inp['x0']))[~b.written].any()
    t = {k: dev(v) for k, v in b.inp.items()}
    wrap = ops.window_drop(t['x0'], t['win'], s.M, s.D, s.seed, s.refill, t['pos'], t['scale'], t['shift'], s.drop_value)
    K.check_bits(c.id + ' (wrapper)', wrap.cpu().numpy(), got)


@pytest.mark.parametrize('B,D', [(3, 0), (0, 5)])
def test_window_drop_without_draws_enqueues_nothing(B, D):
    M, C = 33, 2
    x0 = K.rng('drop-nothing').randn(max(B, 1), C, plane_stride(M)).astype(np.float32)
    for tag, fill in gb.FILLS:
        x = gb.Guarded(x0.shape, F32, fill, DEV, align=4, init=x0)
        win = region(np.arange(max(B, 1), dtype=np.int32), fill, 4)
        _lib.check(_lib.lib().chebgcn_window_drop(P(x), P(win), B, M, C, D, 7, 0, None, None, None, 0.5, stream()), 'window_drop')
        assert _lib.last_dispatch() == ''
        torch.cuda.synchronize()
        x.check('window_drop B = %d, D = %d' % (B, D))
        K.check_bits('window_drop B = %d, D = %d' % (B, D), x.host(), x0)


# =================================================================================================================== statistics

def stats_outputs(s):
    shape = (s.C, plane_stride(s.M))
    return {'mean': (shape, F64, 8, None), 'var': (shape, F64, 8, None), 'scale': (shape, F32, 4, None), 'shift': (shape, F32, 4, None)}


@pytest.mark.parametrize('c', K.of('window_stats'), ids=repr)
def test_window_stats(c):
    b, s = c.built(), c.shape
    L = _lib.lib()
    nws = int(L.chebgcn_window_stats_workspace(s.Ttot, s.M, s.C))
    assert nws == K.stats_workspace(K.K, s.Ttot, s.M, s.C)
    got = two_fills(c.id, K.dispatch_name(c), b.inp, stats_outputs(s), nws, lambda d, o, w: L.chebgcn_window_stats(
        P(d['planes']), s.Ttot, P(d['rows']), s.S, P(o['mean']), P(o['var']), P(o['scale']), P(o['shift']), s.M, s.C, P(w), nws, stream()))
    RATIOS[c.id] = K.check_stats(c.id, s, got, b.ref)
    print('%s: mean err / bound %.3g, var err / bound %.3g' % ((c.id,) + RATIOS[c.id]))
    planes = dev(b.inp['planes'])
    for name, rows in (('wrapper', b.inp['rows']), ('rows permuted', K.rng(c.id + '-perm').permutation(b.inp['rows']))):
        again = ops.window_stats(planes, dev(rows), s.M, s.C)
        assert _lib.last_dispatch() == K.dispatch_name(c)
        for k, t in zip(('mean', 'var', 'scale', 'shift'), again):
            K.check_bits('%s (%s) %s' % (c.id, name, k), t.cpu().numpy(), got[k])


@pytest.mark.parametrize('c', K.of('window_stats_indexed'), ids=repr)
def test_window_stats_indexed(c):
    b, s = c.built(), c.shape
    L = _lib.lib()
    nws = int(L.chebgcn_window_stats_indexed_workspace(s.S, s.M, s.C))
    assert nws == K.stats_indexed_workspace(K.K, s.S, s.M, s.C)
    got = two_fills(c.id, K.dispatch_name(c), b.inp, stats_outputs(s), nws, lambda d, o, w: L.chebgcn_window_stats_indexed(
        P(d['planes']), s.Ttot, P(d['idx']), s.S, s.C * s.fold, s.fold, P(o['mean']), P(o['var']), P(o['scale']), P(o['shift']), s.M, s.C,
        P(w), nws, stream()))
    RATIOS[c.id] = K.check_stats(c.id, s, got, b.ref)
    print('%s: mean err / bound %.3g, var err / bound %.3g' % ((c.id,) + RATIOS[c.id]))
    again = ops.window_stats_indexed(dev(b.inp['planes']), dev(b.inp['idx']), s.M, s.C, s.fold)
    assert _lib.last_dispatch() == K.dispatch_name(c)
    for k, t in zip(('mean', 'var', 'scale', 'shift'), again):
        K.check_bits('%s (wrapper) %s' % (c.id, k), t.cpu().numpy(), got[k])


@pytest.mark.parametrize('c', [c for c in K.of('window_stats') if c.shape.M == 33 and c.shape.C in (1, 9) and c.shape.Ttot in (9, 513, 1027)
                               and c.shape.special is None], ids=repr)
def test_window_stats_indexed_on_contiguous_indices_agrees_with_window_stats(c):
    """fold 1, idx[s] = the rows of window s: float64 results within the same bound of the float64 reference and of
    window_stats' own, and identical tables wherever the float64 results agree; on the exact leg everything agrees bit for bit."""
    b, s = c.built(), c.shape
    planes = dev(b.inp['planes'])
    a = [t.cpu().numpy() for t in ops.window_stats(planes, dev(b.inp['rows']), s.M, s.C)]
    idx = _contiguous(K.clamp(b.inp['rows'], 0, s.Ttot - s.C), s.C)
    i = [t.cpu().numpy() for t in ops.window_stats_indexed(planes, dev(idx), s.M, s.C, 1)]
    shape = types_of(s, kind='stats_indexed', fold=1)
    K.check_stats(c.id + ' (indexed)', shape, dict(zip(('mean', 'var', 'scale', 'shift'), i)), b.ref)
    d_mean, d_var = np.abs(a[0][:, :s.M] - i[0][:, :s.M]), np.abs(a[1][:, :s.M] - i[1][:, :s.M])
    print('%s: |window_stats - indexed| / bound: mean %.3g, var %.3g' % (
        c.id, np.max(d_mean / np.maximum(b.ref['b_mean'], 1e-300)), np.max(d_var / np.maximum(b.ref['b_var'], 1e-300))))
    assert (d_mean <= b.ref['b_mean']).all() and (d_var <= b.ref['b_var']).all()
    same = (gb.bits(a[0]) == gb.bits(i[0])) & (gb.bits(a[1]) == gb.bits(i[1]))
    assert same[:, s.M:].all() and (s.leg != 'exact' or same.all())
    assert (gb.bits(a[2]) == gb.bits(i[2]))[same].all() and (gb.bits(a[3]) == gb.bits(i[3]))[same].all()


def types_of(s, **changes):
    import types
    return types.SimpleNamespace(**dict(vars(s), **changes))


def test_zz_record_the_measured_figures():
    """Last in the module: the total, the slowest case and the worst fractions of the statistics bounds go to the record."""
    if not TIMES or not RATIOS:
        return                                          # the cases above did not run in this process
    slowest = max(TIMES, key=TIMES.get)
    worst = {}
    for entry in ('stats-', 'stats_indexed-'):
        mine = {k: v for k, v in RATIOS.items() if k.startswith(entry)}
        if mine:
            km, kv = max(mine, key=lambda k: mine[k][0]), max(mine, key=lambda k: mine[k][1])
            worst.update({entry + 'mean': mine[km][0], entry + 'mean_case': km, entry + 'var': mine[kv][1], entry + 'var_case': kv})
    record_measured('window_kernels', cases=len(TIMES), total_seconds=sum(TIMES.values()), slowest=slowest,
                    slowest_seconds=TIMES[slowest], **worst)
