"""The staging and feature-mean kernels of csrc/pointwise.hip at their edges, and the buffer discipline of the optimizer, loss and
scalar entries of the training step.  Every entry is called through ctypes with the argument list its ``ops`` wrapper uses;
every pointer -- inputs too -- is a ``guarded_buffers.Guarded`` region at 4-byte alignment (these entries check no alignment:
4 is the weakest they admit; int64 labels at 8).  Cases and references: tests/staging_kernel_cases.py, checked on the host by
tests/test_staging_kernel_refs.py.  Per case:

  1. two runs into fresh regions, poison A (bytes 0xFF) then poison B (bytes 0x5A) in every output;
  2. after each run every guard band is intact and every input is byte-identical to its host copy from before the call;
  3. the two runs agree bit for bit on all of the output ("runs A/B differ" otherwise): nothing unwritten, nothing read that
     nobody wrote;
  4. ``perm_data``, ``to_plane``, ``from_plane``, ``feature_mean_bwd``: bit for bit the NumPy reference, the pad [M, Mp) of plane
     outputs zero; ``feature_mean_fwd``: within (F + 1) 2^-24 mean_f|x| of the float64 mean AND bit for bit the float32
     restatement (ascending f, one division);
  5. bit for bit what the public wrapper returns on ordinary tensors (``ops.perm_data``, ``ops.from_plane``, ``ops.plane_storage``
     on a non-view tensor, ``ops.FeatureMean``; the ``ops`` optimizer, loss and softmax wrappers).

The optimizer, loss and scalar entries get 1 - 3 and 5 only: their values are the job of tests/test_gpu_dispatch.py.
``sq_partials`` is a region of EXACTLY chebgcn_adam_partials(n) floats.

Measured on an MI355X: the module's 186 tests take 4.0 s together (the 164 guarded cases 0.6 to 1.0 s of it); the slowest are
the first call of each kind in the process (0.84 s for the first autograd backward, 0.35 s for the first launch,
perm_data-F1), then the n = 4096 * 256 + 1 optimizer cases at 0.01 to 0.08 s.  ``feature_mean_fwd`` matches the float32
restatement bit for bit in all 11 cases, quotient included; its worst distance from the float64 mean is 0.296 of the bound
(mean_fwd-M33-F7; 0.286 at M = 257, F = 9; 0.077 at F = 65).

Each of these changes to the library, built apart and never committed, fails cases here by name:
  (a) feature_mean_fwd_kernel adds the clamped duplicate plane (no ``if (f0 + u < F)``): the 9 mean_fwd cases with F % 8 != 0
      (F = 9 at the four M of its sweep; F = 1, 7, 9, 17, 65 at M = 33) fail the bound; F = 8 and 16 pass.
  (b) perm_data_kernel keeps ``t`` for a column without a source vertex: 48 tests -- perm_data-fakes, -edge, the test of the
      outside entries, the M sweep's fake vertices, and through "pad not zero" / the reference every perm_data and to_plane
      case with M < Mp (the pad columns take the same path); only to_plane-M64-F1 and -F17 (no pad, no fake vertex) pass.
  (c) perm_data_kernel's gather loop ends after one turn: the 16 perm_data and to_plane cases with F >= 17 and a stored column
      beyond the first turn (F = 17, 33, 252 of the F sweep; M = 33 ... 129 at F = 17) fail; M = 1 at F = 17 passes, rightly --
      the second turn of 64 elements holds columns 60 ... 63, which are not below Mp = 32.
  (d) the optimizer kernels launched with at most 4095 workgroups: the 7 cases of n = 4096 * 256 + 1 that have sq_partials
      fail with "runs A/B differ on sq at 1 of 4096 elements, the first at [4095]".
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
import staging_kernel_cases as K

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DTYPES = {np.dtype(np.float32): 'float32', np.dtype(np.int32): 'int32', np.dtype(np.int64): 'int64'}
TIMES = {}                      # case id -> seconds, for the closing record
MEAN_FRACTIONS = {}             # feature_mean_fwd case id -> worst |got - float64 mean| / bound


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(gb.bits(a), gb.bits(b))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def region(host, fill, align=None):
    """A guarded input region that holds ``host`` (None: a NULL pointer)."""
    if host is None:
        return None
    host = np.ascontiguousarray(host)
    name = DTYPES[host.dtype]
    return gb.Guarded(host.shape or (1,), name, fill, DEV, align=align or host.dtype.itemsize, init=host.reshape(host.shape or (1,)))


def P(r):
    return None if r is None else r.ptr


def dev(host):
    return None if host is None else torch.as_tensor(np.array(host)).to(DEV)


def two_fills(what, inputs, outputs, call):
    """Rules 1 - 3.  ``inputs`` {name: host array or None}; ``outputs`` {name: (shape, dtype name, align, init or None)} -- an
    output with ``init`` is updated in place; ``call(d, o)`` -> the entry's return code, with d / o the regions by name.  Returns
    the outputs of run A as host arrays."""
    t0 = time.perf_counter()
    runs = {}
    for tag, fill in gb.FILLS:
        d = {k: region(v, fill) for k, v in inputs.items()}
        o = {k: gb.Guarded(shape, dtype, fill, DEV, align=align, init=init) for k, (shape, dtype, align, init) in outputs.items()}
        _lib.check(call(d, o), what)
        torch.cuda.synchronize()
        for k, r in list(d.items()) + list(o.items()):
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
    # wholly written: an element no run wrote holds the bytes of fill A after run A and those of fill B after run B, so it is
    # among the differences above (an element may hold the bytes of ONE fill in both runs: a NaN the header promises)
    TIMES[what] = TIMES.get(what, 0.0) + time.perf_counter() - t0
    return runs['A']


def exact(what, got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    bad = gb.bits(got) != gb.bits(ref)
    assert not bad.any(), '%s: %d of %d elements differ from the reference, the first at %s: got %r, reference %r' % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


def pad_zero(what, planes, M):
    assert not gb.bits(planes[..., M:]).any(), '%s: pad not zero' % what


F32 = 'float32'


# ============================================================================================================= staging kernels

@pytest.mark.parametrize('c', K.staging('perm_data'), ids=repr)
def test_perm_data(c):
    b, s = c.built(), c.shape
    Mp = plane_stride(s.M)
    L = _lib.lib()
    got = two_fills(c.id, b.inp, {'out': ((s.S, s.F, Mp), F32, 4, None)},
                    lambda d, o: L.chebgcn_perm_data(P(d['x']), P(d['perm']), P(d['sample']), P(o['out']), s.S, s.N, s.M, s.F, stream()))['out']
    exact(c.id, got, b.ref)
    pad_zero(c.id, got, s.M)
    if s.kind == 'identity':
        assert s.sample is None
        wrap = ops.plane_storage(dev(b.inp['x']))
    else:
        wrap = ops.perm_data(dev(b.inp['x']), dev(b.inp['perm']), dev(b.inp['sample']))
    exact(c.id + ' (wrapper)', wrap.cpu().numpy(), got)
    if K.oracle_defined(b.inp['perm'], s.N):
        from oracle import coarsening_ref
        xs = b.inp['x'] if b.inp['sample'] is None else b.inp['x'][b.inp['sample']]
        exact(c.id + ' (oracle)', K.from_plane_ref(got, s.M), coarsening_ref.perm_data_3d(xs, b.inp['perm']).astype(np.float32))


def test_perm_data_entries_outside_the_vertex_range_give_zero():
    """The ``edge`` permutation: every output column whose entry is outside [0, N) -- N, N + 1, 2^31 - 1, -1, -2^31 -- is exactly
    0; the neighbouring columns are exact copies."""
    c = next(c for c in K.staging('perm_data') if c.shape.kind == 'edge')
    b, s = c.built(), c.shape
    x, perm = b.inp['x'], b.inp['perm'].astype(np.int64)
    out = ops.perm_data(dev(x), dev(b.inp['perm'])).cpu().numpy()
    outside = (perm < 0) | (perm >= s.N)
    assert {int(v) for v in perm[outside]} == {s.N, s.N + 1, K.INT32_MAX, -1, K.INT32_MIN}
    for i in range(s.M):
        if outside[i]:
            assert not gb.bits(out[:, :, i]).any(), 'column %d (perm %d) is not zero' % (i, perm[i])
        else:
            assert same(out[:, :, i], x[:, perm[i], :]), 'column %d (perm %d) is no copy' % (i, perm[i])
    assert any(outside[i] and not outside[i - 1] and not outside[i + 1] for i in range(1, s.M - 1))


@pytest.mark.parametrize('c', K.staging('to_plane'), ids=repr)
def test_to_plane(c):
    b, s = c.built(), c.shape
    L = _lib.lib()
    got = two_fills(c.id, b.inp, {'out': ((s.B, s.F, plane_stride(s.M)), F32, 4, None)},
                    lambda d, o: L.chebgcn_to_plane(P(d['x']), P(o['out']), s.B, s.M, s.F, stream()))['out']
    exact(c.id, got, b.ref)
    pad_zero(c.id, got, s.M)
    x = dev(b.inp['x'])
    assert not ops._is_plane_view(x)
    storage = ops.plane_storage(x)
    exact(c.id + ' (wrapper)', storage.cpu().numpy(), got)
    # the round trip, bit for bit
    exact(c.id + ' (round trip)', ops.from_plane(storage, s.M).cpu().numpy(), b.inp['x'])


@pytest.mark.parametrize('c', K.staging('from_plane'), ids=repr)
def test_from_plane(c):
    b, s = c.built(), c.shape
    L = _lib.lib()
    got = two_fills(c.id, b.inp, {'out': ((s.B, s.M, s.F), F32, 4, None)},
                    lambda d, o: L.chebgcn_from_plane(P(d['xp']), P(o['out']), s.B, s.M, s.F, stream()))['out']
    exact(c.id, got, b.ref)                 # the NaN of the input's pad lanes reaches nothing
    exact(c.id + ' (wrapper)', ops.from_plane(dev(b.inp['xp']), s.M).cpu().numpy(), got)


@pytest.mark.parametrize('c', K.staging('feature_mean_fwd'), ids=repr)
def test_feature_mean_fwd(c):
    """Bit for bit the float32 restatement (no fast-math in the build; hipcc rounds float32 division correctly by default), and
    within the stated bound of the float64 mean."""
    b, s = c.built(), c.shape
    L = _lib.lib()
    got = two_fills(c.id, b.inp, {'y': ((s.B, s.M), F32, 4, None)},
                    lambda d, o: L.chebgcn_feature_mean_fwd(P(d['x']), P(o['y']), s.B, s.M, s.F, stream()))['y']
    err = np.abs(got.astype(np.float64) - b.ref64)
    frac = float((err / b.bound).max())
    MEAN_FRACTIONS[c.id] = frac
    print('%s: worst |got - float64 mean| / bound = %.4f; %d of %d elements off the float32 restatement' % (
        c.id, frac, int((gb.bits(got) != gb.bits(b.ref)).sum()), got.size))
    assert (err <= b.bound).all(), '%s: %.3f of the bound' % (c.id, frac)
    exact(c.id, got, b.ref)
    exact(c.id + ' (wrapper)', ops.FeatureMean.apply(dev(b.inp['x']), s.M).cpu().numpy(), got)


@pytest.mark.parametrize('c', K.staging('feature_mean_bwd'), ids=repr)
def test_feature_mean_bwd(c):
    b, s = c.built(), c.shape
    L = _lib.lib()
    got = two_fills(c.id, b.inp, {'dx': ((s.B, s.F, plane_stride(s.M)), F32, 4, None)},
                    lambda d, o: L.chebgcn_feature_mean_bwd(P(d['dy']), P(o['dx']), s.B, s.M, s.F, stream()))['dx']
    exact(c.id, got, b.ref)
    pad_zero(c.id, got, s.M)
    # the wrapper: FeatureMean's backward (x itself plays no part in it)
    x = torch.zeros((s.B, s.F, plane_stride(s.M)), device=DEV, requires_grad=True)
    ops.FeatureMean.apply(x, s.M).backward(dev(b.inp['dy']))
    exact(c.id + ' (wrapper)', x.grad.cpu().numpy(), got)


@pytest.mark.parametrize('M,F', [(65, 17), (97, 5)])
def test_autograd_of_the_layout_change_and_the_feature_mean(M, F):
    """``ToPlane.apply(x).backward(g)`` gives exactly ``from_plane(g)``; ``FeatureMean`` backward exactly the reference."""
    rs = K.rng('autograd-%d-%d' % (M, F))
    B, Mp = 2, plane_stride(M)
    x = dev(K.data(rs, B, M, F)).requires_grad_(True)
    g = K.planes_of(K.data(rs, B, M, F), K.NAN)
    ops.ToPlane.apply(x).backward(dev(g))
    exact('ToPlane backward', x.grad.cpu().numpy(), K.from_plane_ref(g, M))
    exact('ToPlane backward (wrapper)', x.grad.cpu().numpy(), ops.from_plane(dev(g), M).cpu().numpy())
    xs = dev(K.planes_of(K.data(rs, B, M, F), K.NAN)).requires_grad_(True)
    gy = K.data(rs, B, M)
    y = ops.FeatureMean.apply(xs, M)
    y.backward(dev(gy))
    exact('FeatureMean backward', xs.grad.cpu().numpy(), K.feature_mean_bwd_ref(gy, F))
    assert xs.grad.shape == (B, F, Mp)


def refusals():
    """(id, entry, arguments by position with 'OUT' for the poisoned output and 'IN' for a valid input): refused by argument
    only -- S, B, M, N, F as small as the refused argument lets them be."""
    big = 65536
    return [
        ('perm_data-F253', 'chebgcn_perm_data', ('IN', 'PERM', None, 'OUT', 1, 1, 1, K.F_MAX + 1)),
        ('perm_data-S65536', 'chebgcn_perm_data', ('IN', 'PERM', None, 'OUT', big, 1, 1, 1)),
        ('perm_data-identity-M-not-N', 'chebgcn_perm_data', ('IN', None, None, 'OUT', 1, 2, 1, 1)),
        ('perm_data-null-x', 'chebgcn_perm_data', (None, 'PERM', None, 'OUT', 1, 1, 1, 1)),
        ('perm_data-null-out', 'chebgcn_perm_data', ('IN', 'PERM', None, None, 1, 1, 1, 1)),
        ('to_plane-null-x', 'chebgcn_to_plane', (None, 'OUT', 1, 1, 1)),
        ('to_plane-null-out', 'chebgcn_to_plane', ('IN', None, 1, 1, 1)),
        ('to_plane-F253', 'chebgcn_to_plane', ('IN', 'OUT', 1, 1, K.F_MAX + 1)),
        ('from_plane-F253', 'chebgcn_from_plane', ('IN', 'OUT', 1, 1, K.F_MAX + 1)),
        ('from_plane-B65536', 'chebgcn_from_plane', ('IN', 'OUT', big, 1, 1)),
        ('from_plane-null-x', 'chebgcn_from_plane', (None, 'OUT', 1, 1, 1)),
        ('from_plane-null-out', 'chebgcn_from_plane', ('IN', None, 1, 1, 1)),
        ('feature_mean_fwd-B65536', 'chebgcn_feature_mean_fwd', ('IN', 'OUT', big, 1, 1)),
        ('feature_mean_fwd-null-x', 'chebgcn_feature_mean_fwd', (None, 'OUT', 1, 1, 1)),
        ('feature_mean_fwd-null-y', 'chebgcn_feature_mean_fwd', ('IN', None, 1, 1, 1)),
        ('feature_mean_bwd-B65536', 'chebgcn_feature_mean_bwd', ('IN', 'OUT', big, 1, 1)),
        ('feature_mean_bwd-null-dy', 'chebgcn_feature_mean_bwd', (None, 'OUT', 1, 1, 1)),
        ('feature_mean_bwd-null-dx', 'chebgcn_feature_mean_bwd', ('IN', None, 1, 1, 1)),
    ]


@pytest.mark.parametrize('id,entry,args', refusals(), ids=[r[0] for r in refusals()])
def test_refusals_enqueue_nothing(id, entry, args):
    """Each returns non-zero and leaves a poisoned output byte-identical (it holds what a one-sample call of the refused width
    would write, so a launch that went ahead would show)."""
    n = 32 * (K.F_MAX + 1)
    inp = region(np.full(n, 3.0, np.float32), gb.FILL_B)
    perm = region(np.zeros(1, np.int32), gb.FILL_B)
    out = gb.Guarded((n,), F32, gb.FILL_A, DEV, align=4)
    real = {'IN': inp.ptr, 'OUT': out.ptr, 'PERM': perm.ptr}
    rc = getattr(_lib.lib(), entry)(*[real.get(a, a) if isinstance(a, str) else a for a in args], stream())
    torch.cuda.synchronize()
    assert rc != 0, '%s: accepted' % id
    assert _lib.lib().chebgcn_last_error()
    out.check(id)
    assert same(out.host(), gb.filled(gb.FILL_A, np.float32, (n,))), '%s: the output changed' % id
    assert same(inp.host(), np.full(n, 3.0, np.float32))


# ========================================================================================= optimizer, loss and scalar entries

H = K.ADAM_HYPER
HYPER = (H['beta1'], H['beta2'], H['eps'], H['grad_scale'], H['l2'])


@pytest.mark.parametrize('c', K.OPTIMIZER, ids=repr)
def test_optimizer_buffers(c):
    """p, m, v are regions of exactly n floats updated in place, g and the device step size inputs, sq_partials a region of
    exactly chebgcn_adam_partials(n) floats, wholly written."""
    L = _lib.lib()
    host = K.adam_inputs(c.n)
    nparts = L.chebgcn_adam_partials(c.n)
    assert nparts == K.adam_partials(c.n)
    inputs = {'g': host['g'], 'lr': np.float32([H['lr_t']]) if c.lr_dev else None}
    outputs = {k: ((c.n,), F32, 4, host[k]) for k in 'pmv'}
    if c.sq:
        outputs['sq'] = ((nparts,), F32, 4, None)
    fn = getattr(L, c.entry)

    def call(d, o):
        head = (P(o['p']), P(d['g']), P(o['m']), P(o['v']), c.n)
        if c.entry == 'chebgcn_adam_step':
            return fn(*head, H['lr_t'], *HYPER, stream())
        if c.entry == 'chebgcn_adam_step_dev':
            return fn(*head, P(d['lr']), *HYPER, stream())
        reg = () if c.n_reg is None else (c.n_reg,)
        return fn(*head, *reg, 0.0 if c.lr_dev else H['lr_t'], P(d['lr']), *HYPER, P(o['sq']), stream())

    got = two_fills(c.id, inputs, outputs, call)
    # the wrapper on ordinary tensors
    t = {k: dev(host[k]) for k in 'pgmv'}
    lr = dev(np.float32([H['lr_t']])) if c.lr_dev else H['lr_t']
    kw = dict(beta1=H['beta1'], beta2=H['beta2'], eps=H['eps'], grad_scale=H['grad_scale'], l2=H['l2'])
    sq = torch.full((nparts,), float('nan'), device=DEV) if c.sq else None
    if not c.sq:
        ops.adam_step(t['p'], t['g'], t['m'], t['v'], lr, **kw)
    elif c.n_reg is None:
        assert ops.adam_step_sq(t['p'], t['g'], t['m'], t['v'], lr, sq, **kw) == nparts
    else:
        wrapper = ops.adam_step_sq_all if c.entry == 'chebgcn_adam_step_sq_all' else ops.nadam_step_sq_all
        assert wrapper(t['p'], t['g'], t['m'], t['v'], c.n_reg, lr, sq, **kw) == nparts
    for k in 'pmv':
        exact('%s (wrapper) %s' % (c.id, k), t[k].cpu().numpy(), got[k])
    assert same(t['g'].cpu().numpy(), host['g'])
    assert not same(got['p'], host['p']) and not same(got['m'], host['m']) and not same(got['v'], host['v'])
    if c.sq:
        exact('%s (wrapper) sq_partials' % c.id, sq.cpu().numpy(), got['sq'])
        assert np.isfinite(got['sq']).all()
        if c.n_reg == 0:
            assert not got['sq'].any()


@pytest.mark.parametrize('c', K.LOSS, ids=lambda c: c.id)
def test_loss_bookkeeping_buffers(c):
    L = _lib.lib()
    h = K.LOSS_HYPER
    parts = K.loss_partials(c.nparts) if c.nparts else None
    inputs = {'ce': np.float32([h['ce']]), 'parts': parts, 'corr': np.float32([h['corr']]) if c.corr_dev else None}
    outputs = {'ema': ((1,), F32, 4, np.float32([h['ema']])), 'avg': ((1,), F32, 4, None)}
    if c.loss_out:
        outputs['loss'] = ((1,), F32, 4, None)
    got = two_fills(c.id, inputs, outputs, lambda d, o: L.chebgcn_loss_bookkeeping(
        P(d['ce']), P(d['parts']), c.nparts, h['half_reg'], P(o['ema']), h['decay'], 0.0 if c.corr_dev else h['corr'], P(d['corr']),
        P(o.get('loss')), P(o['avg']), stream()))
    ema = dev(np.float32([h['ema']]))
    avg = ops.loss_bookkeeping(dev(np.float32(h['ce'])), dev(parts), c.nparts, h['half_reg'], ema,
                               dev(np.float32([h['corr']])) if c.corr_dev else h['corr'], decay=h['decay'])
    exact(c.id + ' (wrapper) ema', ema.cpu().numpy(), got['ema'])
    exact(c.id + ' (wrapper) loss_average', avg.cpu().numpy().reshape(1), got['avg'])
    assert got['ema'][0] != np.float32(h['ema'])
    if c.loss_out and c.nparts == 0:
        exact(c.id + ' loss', got['loss'], np.float32([h['ce']]))          # ce + half_reg * 0


@pytest.mark.parametrize('c', K.SCALARS, ids=lambda c: c.id)
def test_set_scalars_buffers(c):
    L = _lib.lib()
    got = two_fills(c.id, {}, {'dst': ((2,), F32, 4, None)}, lambda d, o: L.chebgcn_set_scalars(P(o['dst']), c.v0, c.v1, stream()))
    exact(c.id, got['dst'], np.float32([c.v0, c.v1]))


@pytest.mark.parametrize('c', K.XENT, ids=lambda c: c.id)
def test_softmax_xent_buffers(c):
    """dlogits is wholly written and the bytes behind it stay; a label outside [0, C) makes its row of dlogits and the loss
    NaN, as the header says, and no other row."""
    L = _lib.lib()
    logits, labels = K.xent_inputs(c)
    got = two_fills(c.id, {'logits': logits, 'labels': labels}, {'loss': ((1,), F32, 4, None), 'dlogits': ((c.B, c.C), F32, 4, None)},
                    lambda d, o: L.chebgcn_softmax_xent(P(d['logits']), P(d['labels']), int(c.int64), P(o['loss']), P(o['dlogits']),
                                                        c.B, c.C, stream()))
    nan_rows = np.isnan(got['dlogits']).all(axis=1)
    assert np.array_equal(nan_rows, np.isnan(got['dlogits']).any(axis=1))
    want = np.zeros(c.B, bool)
    if c.bad:
        want[c.B // 2] = True
    assert np.array_equal(nan_rows, want), (np.flatnonzero(nan_rows), np.flatnonzero(want))
    assert bool(np.isnan(got['loss'][0])) == c.bad
    loss, dz = ops.softmax_xent(dev(logits), dev(labels))
    exact(c.id + ' (wrapper) loss', loss.cpu().numpy().reshape(1), got['loss'])
    exact(c.id + ' (wrapper) dlogits', dz.cpu().numpy(), got['dlogits'])


def test_zz_record_the_measured_figures():
    """Last in the module: the total, the slowest case and the worst fraction of the feature-mean bound go to the record."""
    if not TIMES or not MEAN_FRACTIONS:
        return                                          # the cases above did not run in this process
    slowest = max(TIMES, key=TIMES.get)
    worst = max(MEAN_FRACTIONS, key=MEAN_FRACTIONS.get)
    record_measured('staging_kernels', cases=len(TIMES), total_seconds=sum(TIMES.values()), slowest=slowest,
                    slowest_seconds=TIMES[slowest], worst_mean_bound_fraction=MEAN_FRACTIONS[worst], worst_mean_case=worst)
