"""What tests/test_gpu_staging_kernels.py (on the device) and tests/test_staging_kernel_refs.py (on the host) share: the case
tables of the staging and feature-mean kernels of csrc/pointwise.hip -- ``perm_data_kernel``, ``from_plane_kernel``,
``feature_mean_fwd_kernel``, ``feature_mean_bwd_kernel`` -- with their references, and the tables of the optimizer, loss and
scalar entries whose buffer discipline the device module pins.  Plain helpers, built on the host without a GPU.

Inputs are ``randn + 100`` cast to float32, so that float32 sums round visibly; the seed is fixed per case (crc32 of its id);
``B`` or ``S`` is at most 3.  Lanes the header says are never read as data (the pad [M, Mp) of input planes) hold NaN.

References
  * ``perm_data``, ``to_plane``, ``from_plane``: NumPy fancy indexing.  They are copies: the comparison is BIT FOR BIT.  An entry
    of ``perm`` outside [0, N) gives 0 (include/chebgcn.h), the pad [M, Mp) of the planes is 0.  Where ``perm`` has at least N
    entries, none of them negative, the same comes out of ``oracle.coarsening_ref.perm_data_3d``.
  * ``feature_mean_fwd``, two references.  (1) The float64 mean, with the bound, per element,
        |got - ref| <= (F + 1) 2^-24 mean_f|x|:
    the F - 1 sequential float32 additions leave the sum s within gamma_{F-1} sum_f|x_f| <= (F - 1) u (1 + F u) F mean_f|x| of
    the true one, i.e. the quotient within (F - 1) u (1 + F u) mean_f|x|; the one rounded division adds u |s| / F <=
    u (1 + gamma_{F-1}) mean_f|x|; together at most (F u + F^2 u^2) mean_f|x|, and F^2 u^2 <= u for F <= 4096 = 2^12
    (u = 2^-24), far beyond the 252 planes the staging kernels admit.  (2) A float32 restatement of the kernel's
    own order: ``np.float32`` additions in ascending f from the first plane, then one division by float32(F).  The build passes
    no fast-math and hipcc rounds float32 division correctly by default, so the kernel must match it BIT FOR BIT.
  * ``feature_mean_bwd``: ``float32(dy) / float32(F)`` broadcast over f, bit for bit; the pad [M, Mp) of dx is 0.

Cases: the smallest shapes that reach each edge of the kernels.  ``perm_data_kernel`` gathers 64 F elements in turns of 4 x 256
with a clamped tail, transposes through a [F][65] LDS tile and stores under ``i < Mp``: F = 1 leaves three quarters of the
workgroup on the clamp, F = 16 is exactly one turn, F = 17 starts a second turn of 64 elements, F = 252 is the last width the
64 KB LDS check admits; M = 1 and M = 65 put columns of the last block beyond Mp, M = 97 a block across [M, Mp).
``from_plane_kernel`` has the same tile with the two index forms swapped.  ``feature_mean_fwd_kernel`` adds eight planes per
turn behind a clamped plane index, so F % 8 != 0 away from F = 7 is where a duplicated or dropped plane shows.
"""
import types
import zlib

import numpy as np

from gcn_fmri_decoding_amd._lib import plane_stride

U = 2.0 ** -24                          # unit round-off of float32
NAN = np.float32(np.nan)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

ENTRIES = ('chebgcn_perm_data', 'chebgcn_to_plane', 'chebgcn_from_plane', 'chebgcn_feature_mean_fwd', 'chebgcn_feature_mean_bwd',
           'chebgcn_adam_step', 'chebgcn_adam_step_dev', 'chebgcn_adam_step_sq', 'chebgcn_adam_step_sq_all',
           'chebgcn_nadam_step_sq_all', 'chebgcn_loss_bookkeeping', 'chebgcn_set_scalars', 'chebgcn_softmax_xent')

F_SWEEP = (1, 3, 4, 5, 16, 17, 33, 252)
M_SWEEP = (1, 33, 64, 65, 97, 129)
F_OF_M_SWEEP = (1, 17)
F_MAX = 252                             # 65 F floats of LDS <= 64 KB
MEAN_M_SWEEP, MEAN_F_AT_M = (1, 255, 256, 257), 9
MEAN_F_SWEEP, MEAN_M_AT_F = (1, 7, 8, 9, 16, 17, 65), 33


def rng(case_id):
    return np.random.RandomState(zlib.crc32(case_id.encode()) & 0x7FFFFFFF)


def data(rs, *shape):
    """``randn + 100`` as float32."""
    return (rs.randn(*shape) + 100.0).astype(np.float32)


def planes_of(rows, pad):
    """[B, M, F] rows -> [B, F, Mp] planes, ``pad`` in the lanes [M, Mp)."""
    B, M, F = rows.shape
    out = np.full((B, F, plane_stride(M)), pad, np.float32)
    out[:, :, :M] = rows.transpose(0, 2, 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ references

def perm_data_ref(x, perm, sample, M):
    """out[s][f][i] = x[sample[s]][perm[i]][f] where 0 <= perm[i] < N, else 0 (i < M); 0 in the pad.  [S, F, Mp] float32."""
    N = x.shape[1]
    idx = np.arange(M, dtype=np.int64) if perm is None else np.asarray(perm, np.int64)
    assert idx.shape == (M,)
    xs = x if sample is None else x[np.asarray(sample, np.int64)]
    real = (idx >= 0) & (idx < N)
    rows = np.zeros((xs.shape[0], M, x.shape[2]), np.float32)
    rows[:, real, :] = xs[:, idx[real], :]
    return planes_of(rows, 0.0)


def oracle_defined(perm, N):
    """``oracle.coarsening_ref.perm_data_3d`` is defined for a ``perm`` of at least N entries, and gives what the header says
    where none of them is negative (NumPy would count a negative entry from the end)."""
    return perm is not None and len(perm) >= N and int(np.min(perm)) >= 0


def from_plane_ref(xp, M):
    """[B, F, Mp] planes -> [B, M, F] rows."""
    return np.ascontiguousarray(xp[:, :, :M].transpose(0, 2, 1))


def feature_mean_ref64(x, M):
    return x[:, :, :M].astype(np.float64).mean(axis=1)


def feature_mean_bound(x, M):
    F = x.shape[1]
    return (F + 1) * U * np.abs(x[:, :, :M].astype(np.float64)).mean(axis=1)


def feature_mean_ref32(x, M):
    """The kernel's own order in float32: planes added in ascending f onto the first, one division."""
    F = x.shape[1]
    s = x[:, 0, :M].astype(np.float32)
    for f in range(1, F):
        s = (s + x[:, f, :M]).astype(np.float32)
    return (s / np.float32(F)).astype(np.float32)


def feature_mean_bwd_ref(dy, F):
    B, M = dy.shape
    dx = np.zeros((B, F, plane_stride(M)), np.float32)
    dx[:, :, :M] = (dy.astype(np.float32) / np.float32(F)).astype(np.float32)[:, None, :]
    return dx


# --------------------------------------------------------------------------------------------------------------- staging cases

class Case:
    """``id``; ``entry``: the chebgcn_* symbol; ``shape``: its integer arguments by name; ``built()`` -> a namespace, made once on
    the host and left unchanged: ``inp`` {name: host array or None}, ``ref`` (the exact reference of the output), and for
    feature_mean_fwd ``ref64`` and ``bound`` too."""

    def __init__(self, id, entry, make, **shape):
        self.id, self.entry, self._make, self._built = id, entry, make, None
        self.shape = types.SimpleNamespace(**shape)

    def built(self):
        if self._built is None:
            self._built = self._make(self)
        return self._built

    def __repr__(self):
        return self.id


def edge_perm(rs, N, M):
    """Valid entries with N, N + 1, 2^31 - 1, -1 and -2^31 scattered among them: in the first and the last column, on both
    sides of the boundary of the 64-column blocks, and in the middle."""
    perm = rs.randint(0, N, M).astype(np.int64)
    special = {0: -1, 13: N, 40: INT32_MIN, 63: INT32_MAX, 64: INT32_MIN, 70: N + 1, 81: INT32_MAX, M - 1: -1}
    for i, v in special.items():
        perm[i] = v
    return perm.astype(np.int32)


def make_perm(kind, rs, N, M):
    if kind == 'identity':
        assert M == N
        return None
    if kind == 'fakes':
        assert M > N
        return rs.permutation(M).astype(np.int32)
    if kind == 'subset':
        assert M <= N
        return rs.permutation(N)[:M].astype(np.int32)
    if kind == 'repeats':
        return rs.randint(0, N, M).astype(np.int32)
    if kind == 'edge':
        return edge_perm(rs, N, M)
    raise ValueError(kind)


def _make_perm_data(c):
    s, rs = c.shape, rng(c.id)
    x = data(rs, s.S_total, s.N, s.F)
    perm = make_perm(s.kind, rs, s.N, s.M)
    sample = None if s.sample is None else np.asarray(s.sample, np.int32)
    return types.SimpleNamespace(inp={'x': x, 'perm': perm, 'sample': sample}, ref=perm_data_ref(x, perm, sample, s.M))


def _make_to_plane(c):
    s, rs = c.shape, rng(c.id)
    x = data(rs, s.B, s.M, s.F)
    return types.SimpleNamespace(inp={'x': x}, ref=planes_of(x, 0.0))


def _make_from_plane(c):
    s, rs = c.shape, rng(c.id)
    rows = data(rs, s.B, s.M, s.F)
    return types.SimpleNamespace(inp={'xp': planes_of(rows, NAN)}, ref=rows)


def _make_mean_fwd(c):
    s, rs = c.shape, rng(c.id)
    x = planes_of(data(rs, s.B, s.M, s.F), NAN)
    return types.SimpleNamespace(inp={'x': x}, ref=feature_mean_ref32(x, s.M), ref64=feature_mean_ref64(x, s.M),
                                 bound=feature_mean_bound(x, s.M))


def _make_mean_bwd(c):
    s, rs = c.shape, rng(c.id)
    dy = data(rs, s.B, s.M)
    return types.SimpleNamespace(inp={'dy': dy}, ref=feature_mean_bwd_ref(dy, s.F))


def _perm_case(id, N, M, F, kind, S_total=2, sample=None):
    S = S_total if sample is None else len(sample)
    return Case(id, 'chebgcn_perm_data', _make_perm_data, S=S, S_total=S_total, N=N, M=M, F=F, kind=kind, sample=sample)


def _staging_cases():
    cases = []
    for F in F_SWEEP:
        cases.append(_perm_case('perm_data-F%d' % F, 70, 65, F, 'subset'))
    for F in F_OF_M_SWEEP:
        for M in M_SWEEP:
            N = max(1, M - 9)
            cases.append(_perm_case('perm_data-M%d-F%d' % (M, F), N, M, F, 'fakes' if M > N else 'subset'))
    for kind, N in (('fakes', 88), ('subset', 120), ('repeats', 40), ('edge', 88), ('identity', 97)):
        cases.append(_perm_case('perm_data-%s' % kind, N, 97, 5, kind))
    for name, sample in (('null', None), ('reversed', [2, 1, 0]), ('repeated', [2, 0, 2]), ('one', [1])):
        cases.append(_perm_case('perm_data-sample-%s' % name, 88, 97, 5, 'fakes', S_total=3, sample=sample))
    for entry, short, make in (('chebgcn_to_plane', 'to_plane', _make_to_plane), ('chebgcn_from_plane', 'from_plane', _make_from_plane)):
        for F in F_SWEEP:
            cases.append(Case('%s-F%d' % (short, F), entry, make, B=2, M=65, F=F))
        for F in F_OF_M_SWEEP:
            for M in M_SWEEP:
                cases.append(Case('%s-M%d-F%d' % (short, M, F), entry, make, B=2, M=M, F=F))
    for entry, short, make in (('chebgcn_feature_mean_fwd', 'mean_fwd', _make_mean_fwd),
                               ('chebgcn_feature_mean_bwd', 'mean_bwd', _make_mean_bwd)):
        for M in MEAN_M_SWEEP:
            cases.append(Case('%s-M%d-F%d' % (short, M, MEAN_F_AT_M), entry, make, B=2, M=M, F=MEAN_F_AT_M))
        for F in MEAN_F_SWEEP:
            cases.append(Case('%s-M%d-F%d' % (short, MEAN_M_AT_F, F), entry, make, B=3, M=MEAN_M_AT_F, F=F))
    return cases


STAGING = _staging_cases()


def staging(entry):
    return [c for c in STAGING if c.entry == 'chebgcn_' + entry]


# ---------------------------------------------------------------------------------- optimizer, loss and scalar entries (buffers)
# No value references here: tests/test_gpu_dispatch.py keeps that job.  The device module compares with the ``ops`` wrappers.

ADAM_N = (1, 255, 256, 257, 4096 * 256 + 1)
ADAM_HYPER = dict(lr_t=1.25e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.5, l2=5e-4)


def adam_partials(n):
    """chebgcn_adam_partials restated: one partial per workgroup of 256, at most 4096 workgroups."""
    return min(4096, (n + 255) // 256)


class OptCase:
    """One optimizer call: ``entry`` over ``n`` variables, the first ``n_reg`` regularised (None: the entry takes no n_reg);
    ``lr_dev``: the step size is read from device memory (always for adam_step_dev, never for adam_step)."""

    def __init__(self, entry, n, n_reg, lr_dev):
        self.entry, self.n, self.n_reg, self.lr_dev = entry, n, n_reg, lr_dev
        self.sq = entry not in ('chebgcn_adam_step', 'chebgcn_adam_step_dev')
        self.id = '%s-n%d%s%s' % (entry[len('chebgcn_'):], n, '' if n_reg is None else '-reg%d' % n_reg,
                                  '-lrdev' if lr_dev and entry != 'chebgcn_adam_step_dev' else '')

    def __repr__(self):
        return self.id


_adam_inputs = {}


def adam_inputs(n):
    """p, g, m, v of ``n`` variables (shared by the cases of that size; nobody changes them)."""
    if n not in _adam_inputs:
        rs = rng('adam-%d' % n)
        _adam_inputs[n] = {'p': rs.randn(n).astype(np.float32), 'g': rs.randn(n).astype(np.float32),
                           'm': (0.1 * rs.randn(n)).astype(np.float32), 'v': (0.01 * rs.randn(n) ** 2).astype(np.float32)}
    return _adam_inputs[n]


def _opt_cases():
    cases = []
    for n in ADAM_N:
        cases.append(OptCase('chebgcn_adam_step', n, None, False))
        cases.append(OptCase('chebgcn_adam_step_dev', n, None, True))
        cases.append(OptCase('chebgcn_adam_step_sq', n, None, n == 256))
        for entry in ('chebgcn_adam_step_sq_all', 'chebgcn_nadam_step_sq_all'):
            for n_reg in sorted({0, n // 3, n}):
                cases.append(OptCase(entry, n, n_reg, n == 256))
    return cases


OPTIMIZER = _opt_cases()

LOSS_NPARTS = (0, 1, 1025, 4096)
LOSS = [types.SimpleNamespace(id='loss_bookkeeping-parts%d-%s-%s' % (nparts, 'lossout' if loss_out else 'nolossout',
                                                                    'corrdev' if corr_dev else 'corrval'),
                              entry='chebgcn_loss_bookkeeping', nparts=nparts, loss_out=loss_out, corr_dev=corr_dev)
        for nparts in LOSS_NPARTS for loss_out in (False, True) for corr_dev in (False, True)]
LOSS_HYPER = dict(half_reg=2.5e-4, decay=0.9, corr=1.0 / (1.0 - 0.9 ** 3), ce=1.7, ema=0.6)


def loss_partials(nparts):
    return np.abs(rng('loss-%d' % nparts).randn(nparts)).astype(np.float32) + np.float32(0.5)


SCALARS = [types.SimpleNamespace(id='set_scalars-%d' % i, entry='chebgcn_set_scalars', v0=v0, v1=v1)
           for i, (v0, v1) in enumerate(((1.25e-3, 3.69), (-0.0, 1e-30)))]

XENT_SHAPES = ((1, 2), (257, 22), (33, 45))


def xent_inputs(c):
    """Logits and labels of a softmax case; ``c.bad``: row B // 2 carries a label outside [0, C) -- C itself as int32, and as
    int64 a value whose low 32 bits are the valid label 1."""
    rs = rng(c.id)
    logits = (3.0 * rs.randn(c.B, c.C)).astype(np.float32)
    labels = rs.randint(0, c.C, c.B).astype(np.int64 if c.int64 else np.int32)
    if c.bad:
        labels[c.B // 2] = 2 ** 32 + 1 if c.int64 else c.C
    return logits, labels


XENT = [types.SimpleNamespace(id='softmax_xent-B%d-C%d-%s-%s' % (B, C, 'int64' if int64 else 'int32', 'bad' if bad else 'valid'),
                              entry='chebgcn_softmax_xent', B=B, C=C, int64=int64, bad=bad)
        for (B, C) in XENT_SHAPES for int64 in (False, True) for bad in (False, True)]


def entries_reached():
    return ({c.entry for c in STAGING} | {c.entry for c in OPTIMIZER} | {c.entry for c in LOSS} | {c.entry for c in SCALARS}
            | {c.entry for c in XENT})
