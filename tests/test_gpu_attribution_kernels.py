"""The ten attribution kernels (csrc/saliency.hip, csrc/occlusion.hip, csrc/gradcam.hip, csrc/saliency_tile.h) and the
gather they share with chebgcn_perm_data, BY NAME, against float64 at their tile and channel edges.  Needs an MI355X: ``-m gpu``.

No model, no graph, no checkpoint: plain tensors in, plain tensors out.  Every case

* names its kernel through ``chebgcn_last_dispatch()`` (perm_data notes none),
* compares EVERY element of every output with a NumPy float64 restatement of the header comments of the three .hip files
  (the ``ref_*`` functions below; tests/test_attribution_kernel_refs.py ties each of them to a literal nested-loop
  transcription on a machine without a GPU),
* poisons the pad [M, Mp) of every input plane with NaN, pre-fills every output with a sentinel and surrounds it with a
  sentinel margin of at least one row on both sides ("not written" and "written outside" are both visible),
* runs twice and asserts the two results bit-identical (where ops.py allocates the output itself, the second run is the
  ops wrapper, which thereby is held to the same values).

Bounds, with u = 2^-24 (nothing here is tuned to what the kernels return):

* selections and copies are bit-exact: occlusion_rows, saliency_reduce 'gradient' at steps = 1, the one-hot seed, cls_out,
  perm_data, the 'logit' drop (one fp32 subtraction);
* fp32 sums and products in a fixed order: |got - ref| <= n u sum|terms| per element, n = the roundings of that element.
  path: the coefficient a_j = (j + 1/2) / steps is formed in fp32 by the kernel ((float)j + 0.5f) * (1.f / steps); the
  reference takes that fp32 a_j (as gradcam_map's reference takes the fp32 alpha), which leaves the 3 roundings of
  b + a (x - b) over the terms |b| and |a (x - b)|.  reduce: steps - 1 additions, one product for 'grad_x_input', two for
  'integrated' (again with the fp32 1 / steps) and one more rounding for x - x0 where a baseline is given.  gradcam_map:
  F fused multiply-adds over |w_f a_f|.  The compiler may contract b + a * d into an fma; the bound covers both;
* gradcam_weights: float64 sums rounded once: one fp32 ulp of the reference, plus 2^-53 sum|g| for the float64 additions
  themselves (1e-9 of an ulp on random planes; the cancelling plane is built from multiples of 2^-10, whose float64 sums
  are exact in any order);
* float64 class sums: the reference adds the fp32 rows of a class in window order into one float64 and adds that to the
  previous accumulator, as the kernel does: bit-identical;
* expf / logf arithmetic: the bound test_softmax_xent_vs_float64 asserts for the same arithmetic: 2e-6 of the row's largest
  |dlogit| (seed), 2e-6 (max_k |z_k - max z| + log C + 1) per score and the sum of the two for a drop.

Measured on the MI355X: every launch at the channel limits succeeds (saliency_path at F = 126 with 65 520 bytes of dynamic
LDS beside its 256-byte static table, perm_data at F = 252, occlusion_rows at F = 125) and returns the right values.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_measured

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F64 = np.float64
ISENT = -0x5A5A5A5A5A5A5A5B        # sentinel of the int64 outputs


def plane_stride(M):
    return (int(M) + 31) & ~31


# ------------------------------------------------------------------------------------
# the references: NumPy on the host, float64 unless the operation is a pure selection (then the input's dtype, for bits)
# ------------------------------------------------------------------------------------

def ref_gather(x, perm, M):
    """x [..., N, F] rows -> planes [..., F, Mp]: position i holds vertex perm[i] (identity without a table), 0 where
    perm[i] is outside [0, N) and on the pad [M, Mp)."""
    x = np.asarray(x)
    N, F = x.shape[-2:]
    perm = np.arange(M) if perm is None else np.asarray(perm, np.int64)
    ok = (perm >= 0) & (perm < N)
    out = np.zeros(x.shape[:-2] + (F, plane_stride(M)), x.dtype)
    picked = np.where(ok[:, None], x[..., np.where(ok, perm, 0), :], x.dtype.type(0))
    out[..., :M] = np.swapaxes(picked, -1, -2)
    return out


def ref_perm_data(x, perm, sample, M):
    return ref_gather(np.asarray(x)[np.asarray(sample)] if sample is not None else x, perm, M)


def path_coefficients(steps):
    """a_j = (j + 1/2) / steps as the kernel forms it in fp32: ((float)j + 0.5f) * (1.f / (float)steps)."""
    inv = np.float32(1.0) / np.float32(steps)
    return (np.arange(steps, dtype=np.float32) + np.float32(0.5)) * inv


def ref_path(x, perm, sample, x0, steps, R, M):
    """Rows w*steps + j = x0 + a_j (x[sample[w]] - x0) as planes [R, F, Mp]; zero rows behind the windows; (ref, bound)."""
    X = ref_gather(np.asarray(x, F64)[np.asarray(sample)], perm, M)                     # [nw, F, Mp]
    B0 = ref_gather(np.asarray(x0, F64), perm, M) if x0 is not None else np.zeros(X.shape[1:])
    a = path_coefficients(steps).astype(F64)
    term = a[None, :, None, None] * (X[:, None] - B0[None, None])                       # [nw, steps, F, Mp]
    nw, F, Mp = X.shape
    ref, bound = np.zeros((R, F, Mp)), np.zeros((R, F, Mp))
    ref[:nw * steps] = (B0[None, None] + term).reshape(nw * steps, F, Mp)
    bound[:nw * steps] = (3 * U * (np.abs(B0)[None, None] + np.abs(term))).reshape(nw * steps, F, Mp)
    return ref, bound


def ref_reduce(dx, x, order, sample, x0, nw, steps, M, method, absolute):
    """Planes dx [>= nw*steps, F, Mp] (internal order) -> rows [nw, M, F] in the caller's order: the steps of a window summed,
    times 1, x or (x - x0) / steps, optionally |.|; (ref, bound)."""
    dx = np.asarray(dx)
    F = dx.shape[1]
    d = dx[:nw * steps, :, :M].astype(F64).reshape(nw, steps, F, M)
    order = np.arange(M) if order is None else np.asarray(order, np.int64)

    def rows(p):                                        # [nw, F, M] internal -> [nw, M, F] caller's
        r = np.empty((nw, M, F))
        r[:, order, :] = np.swapaxes(p, 1, 2)
        return r

    g, t = rows(d.sum(1)), rows(np.abs(d).sum(1))
    n = steps - 1
    if method != 'gradient':
        xs = np.asarray(x, F64)[np.asarray(sample)]
        if method == 'grad_x_input':
            g, t, n = xs * g, np.abs(xs) * t, n + 1
        else:
            inv = float(np.float32(1.0) / np.float32(steps))
            dd = xs - (np.asarray(x0, F64)[None] if x0 is not None else 0.0)
            g, t, n = dd * (g * inv), np.abs(dd) * (t * inv), n + 2 + (x0 is not None)
    return (np.abs(g) if absolute else g), n * U * t


def ref_class_sums(rows, cls, acc):
    """acc[k] + (the fp32 rows of class k added in window order into one float64); classes without a window untouched."""
    rows = np.asarray(rows, np.float32).reshape(len(cls), -1)
    acc = np.asarray(acc, F64)
    s = np.zeros(acc.shape, F64).reshape(acc.shape[0], -1)
    seen = np.zeros(acc.shape[0], bool)
    for w, k in enumerate(np.asarray(cls)):
        if 0 <= k < acc.shape[0]:
            s[k] += rows[w].astype(F64)
            seen[k] = True
    out = acc.copy()
    out[seen] = acc[seen] + s.reshape(acc.shape)[seen]
    return out


def ref_occlusion_rows(x, perm, gid, x0, r0, R, G, M):
    """Rows r0 .. r0 + R of an occlusion run as planes [R, F, Mp] in x's dtype: window r // (G + 1) with the positions of
    group r % (G + 1) - 1 (slot 0: none) set to the baseline (0 without one); 0 on the pad and past S (G + 1)."""
    x = np.asarray(x)
    S, N, F = x.shape
    Mp = plane_stride(M)
    r = r0 + np.arange(R, dtype=np.int64)
    w, j = r // (G + 1), r % (G + 1)
    g = np.where(j == 0, G, j - 1)
    P = ref_gather(np.concatenate([x, np.zeros((1, N, F), x.dtype)]), perm, M)         # window S: the zero rows
    B0 = ref_gather(np.asarray(x0, x.dtype), perm, M) if x0 is not None else np.zeros((F, Mp), x.dtype)
    gp = np.full(Mp, -1, np.int64)
    gp[:M] = np.asarray(gid)
    hit = (gp[None, :] == g[:, None]) & (w < S)[:, None]
    return np.where(hit[:, None, :], B0[None], P[np.minimum(w, S)])


def ref_class_score(z, c, score):
    """s = z_c or log softmax(z)_c of rows z [R, C] (float64) for classes c [R]; (s, the bound of one fp32 score)."""
    z = np.asarray(z, F64)
    R, C = z.shape
    zc = z[np.arange(R), c]
    if score == 'logit':
        return zc, np.zeros(R)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    return zc - lse, 2e-6 * (np.abs(z - m[:, None]).max(1) + np.log(C) + 1.0)


def ref_occlusion_drop(z, cls, S, G, score):
    """(ref [S], drop [S, G], bound of ref, bound of drop) from the logits [>= S (G + 1), C] of a whole run.  The bound of a
    drop is the sum of its two scores' bounds; under 'logit' the scores are exact and the one fp32 subtraction rounds once
    (the GPU test compares that one with the fp32 difference bit for bit as well)."""
    z = np.asarray(z, F64)[:S * (G + 1)]
    s, b = ref_class_score(z, np.repeat(np.asarray(cls, np.int64), G + 1), score)
    s, b = s.reshape(S, G + 1), b.reshape(S, G + 1)
    drop = s[:, :1] - s[:, 1:]
    return s[:, 0], drop, b[:, 0], (U * np.abs(drop) if score == 'logit' else b[:, :1] + b[:, 1:])


def ref_seed(z, t, score):
    """d score / d logits of rows z [B, C] for classes t [B]: e_t, or e_t - softmax(z) with 1 - p_t as the sum of the other
    classes' shares (the float64 difference would cancel on a confident row); (d, bound [B, 1])."""
    z = np.asarray(z, F64)
    B, C = z.shape
    ar = np.arange(B)
    if score == 'logit':
        d = np.zeros((B, C))
        d[ar, t] = 1.0
        return d, np.zeros((B, 1))
    e = np.exp(z - z.max(1, keepdims=True))
    d = -e / e.sum(1, keepdims=True)
    others = e.copy()
    others[ar, t] = 0.0
    d[ar, t] = others.sum(1) / e.sum(1)
    return d, 2e-6 * np.abs(d).max(1, keepdims=True)


def ref_gradcam_weights(G, N):
    """alpha [nw, F] = the mean over the N vertices of the planes G [nw, F, Mp]; (ref, bound = one fp32 ulp of ref + the
    float64 additions' own 2^-53 sum|g|)."""
    g = np.asarray(G)[:, :, :N].astype(F64)
    ref = g.sum(-1) / N
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(F64)
    return ref, ulp + 2.0 ** -53 * np.abs(g).sum(-1)


def ref_gradcam_map(A, W, N, P, relu, order, ldo):
    """Rows [nw, ldo]: level vertex i (reference vertex j = order[i]) writes sum_f w a, max(0, .) with relu, to the outputs
    [j P, (j + 1) P); W is alpha [nw, F] or the planes G [nw, F, Mp].  NaN = keeps the sentinel: the tail [N P, ldo) and the
    outputs of a table entry outside [0, N).  (ref, bound)."""
    a = np.asarray(A)[:, :, :N].astype(F64)
    W = np.asarray(W, F64)
    terms = (W[:, :, :N] if W.ndim == 3 else W[:, :, None]) * a
    F = a.shape[1]
    cam, cb = terms.sum(1), F * U * np.abs(terms).sum(1)
    if relu:
        cam = np.maximum(cam, 0.0)
    order = np.arange(N) if order is None else np.asarray(order, np.int64)
    ok = (order >= 0) & (order < N)
    idx = (order[ok][:, None] * P + np.arange(P)[None, :]).reshape(-1)
    nw = a.shape[0]
    ref, bound = np.full((nw, ldo), np.nan), np.zeros((nw, ldo))
    ref[:, idx] = np.repeat(cam[:, ok], P, axis=1)
    bound[:, idx] = np.repeat(cb[:, ok], P, axis=1)
    return ref, bound


# ------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def L():
    from gcn_fmri_decoding_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _ok(rc, what):
    from gcn_fmri_decoding_amd import _lib
    _lib.check(rc, what)


def _named(name):
    from gcn_fmri_decoding_amd import _lib
    assert _lib.last_dispatch() == name, (_lib.last_dispatch(), name)


def _refused(L, rc, word):
    """A CG_REQUIRE rejection: -1 before any launch, the reason in chebgcn_last_error()."""
    msg = L.chebgcn_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


class Guarded:
    """An output of ``shape`` filled with a sentinel, inside one allocation with a sentinel margin of at least one row (and a
    multiple of 32 elements, so that the output keeps the allocation's alignment) in front and behind."""

    def __init__(self, shape, dtype, dev, fill=None):
        self.fill = fill if fill is not None else (float('nan') if dtype.is_floating_point else ISENT)
        n = int(np.prod(shape))
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        self.m = max(32, (row + 31) // 32 * 32)
        self.full = torch.full((self.m + n + self.m,), self.fill, dtype=dtype, device=dev)
        self.t = self.full[self.m:self.m + n].view(shape)

    def refill(self):
        self.full.fill_(self.fill)

    def margins_intact(self):
        edge = torch.cat([self.full[:self.m], self.full[self.full.numel() - self.m:]])
        return bool(torch.isnan(edge).all()) if self.fill != self.fill else bool((edge == self.fill).all())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, ref):
    return np.array_equal(_bits(got), _bits(np.asarray(ref, got.dtype)))


def _within(got, ref, bound, what):
    """Every element: finite and |got - ref| <= bound (exactly equal where the bound is 0); a NaN in ``ref`` stands for
    "keeps the NaN sentinel".  Returns the worst ratio to the bound."""
    got = np.asarray(got, F64)
    keep = np.isnan(ref)
    assert np.array_equal(np.isnan(got), keep), '%s: %d elements not written / %d written that must keep the sentinel' % (
        what, int((np.isnan(got) & ~keep).sum()), int((~np.isnan(got) & keep).sum()))
    err = np.where(keep, 0.0, np.abs(got - np.where(keep, 0.0, ref)))
    bound = np.broadcast_to(bound, err.shape)
    bad = err > bound
    assert not bad.any(), '%s: %d of %d elements beyond the bound, worst |err| %.3e at bound %.3e' % (
        what, int(bad.sum()), err.size, err[bad].max(), bound[bad][np.argmax(err[bad])])
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _poison_planes(planes, M):
    planes = np.array(planes, np.float32)
    planes[..., M:] = np.nan
    return planes


def _fake_perm(rs, N, M):
    """A random injection of the N vertices into M positions; the M - N fake positions (entries >= N) scattered."""
    return rs.permutation(np.concatenate([np.arange(N), N + np.arange(M - N)])).astype(np.int32) if M != N else None


# ------------------------------------------------------------------------------------
# perm_data: the shared gather at its channel limit (F * 65 * 4 <= 64 KB)
# ------------------------------------------------------------------------------------

def test_perm_data_channel_limit(dev, L):
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(252)
    N, M, F, S = 90, 100, 252, 4
    x = rs.randn(S, N, F).astype(np.float32)
    perm = _fake_perm(rs, N, M)
    sample = np.array([3, 0, 3], np.int32)
    out = Guarded((3, F, plane_stride(M)), torch.float32, dev)
    xd, pd, sd = _to(x, dev), _to(perm, dev), _to(sample, dev)
    ops.perm_data(xd, pd, sd, out=out.t)
    got = out.t.cpu().numpy()
    assert _same_bits(got, ref_perm_data(x, perm, sample, M)) and out.margins_intact()
    out.refill()
    ops.perm_data(xd, pd, sd, out=out.t)
    assert _same_bits(out.t.cpu().numpy(), got)
    xb = torch.zeros((1, N, 253), device=dev)
    ob = Guarded((1, 253, plane_stride(M)), torch.float32, dev)
    _refused(L, L.chebgcn_perm_data(_p(xb), _p(pd), None, _p(ob.t), 1, N, M, 253, _s()), 'too large')
    assert bool(torch.isnan(ob.full).all())


# ------------------------------------------------------------------------------------
# saliency_path
# ------------------------------------------------------------------------------------

PATH_CASES = [(90, 100, 3, 3, 1, 4), (360, 360, 16, 2, 5, 13), (1100, 1200, 17, 3, 4, 12), (37, 37, 1, 1, 7, 7),
              (64, 64, 126, 2, 2, 5), (5000, 5040, 2, 2, 3, 8)]


@pytest.mark.parametrize('with_baseline', [False, True], ids=['zero', 'baseline'])
@pytest.mark.parametrize('N,M,F,nw,steps,R', PATH_CASES, ids=['N%d_M%d_F%d_nw%d_s%d_R%d' % c for c in PATH_CASES])
def test_saliency_path(dev, L, N, M, F, nw, steps, R, with_baseline):
    """Every row w*steps + j, the zero rows behind the windows (R not a multiple of steps: the ``r >= R`` break), zero pads,
    zero at fake positions; F = 17 (the gather's second turn), F = 126 (the limit of chebgcn_saliency_supported)."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(N + 7 * F + steps)
    S = nw + 2
    x = rs.randn(S, N, F).astype(np.float32)
    x0 = rs.randn(N, F).astype(np.float32) if with_baseline else None
    perm = _fake_perm(rs, N, M)
    sample = rs.randint(0, S, nw).astype(np.int32)
    if nw > 1:
        sample[-1] = sample[0]                          # a repeat
    Mp = plane_stride(M)
    out = Guarded((R, F, Mp), torch.float32, dev)
    xd, pd, sd, bd = _to(x, dev), _to(perm, dev), _to(sample, dev), _to(x0, dev)
    _ok(L.chebgcn_saliency_path(_p(xd), _p(pd), _p(sd), _p(bd), _p(out.t), nw, steps, R, N, M, F, _s()), 'saliency_path')
    _named('saliency_path_kernel')
    got = out.t.cpu().numpy()
    assert out.margins_intact()
    ref, bound = ref_path(x, perm, sample, x0, steps, R, M)
    ratio = _within(got, ref, bound, 'path')
    assert not got[nw * steps:].any() and not got[:, :, M:].any()
    if perm is not None:
        assert not got[:, :, :M][:, :, perm >= N].any()
    record_measured('attr_path[%d,%d,%d,%d,%d,%d,%s]' % (N, M, F, nw, steps, R, with_baseline), ratio_to_bound=ratio)
    again = ops.saliency_path(xd, pd, sd, bd, R, steps, M)
    _named('saliency_path_kernel')
    assert torch.equal(again, out.t)


def test_saliency_path_refusals(dev, L):
    x, s = torch.zeros((2, 64, 127), device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    out = Guarded((4, 127, 64), torch.float32, dev)
    assert L.chebgcn_saliency_supported(126) == 1 and L.chebgcn_saliency_supported(127) == 0
    _refused(L, L.chebgcn_saliency_path(_p(x), None, _p(s), None, _p(out.t), 2, 2, 4, 64, 64, 127, _s()), 'too large')
    _refused(L, L.chebgcn_saliency_path(_p(x), None, _p(s), None, _p(out.t), 2, 2, 3, 64, 64, 3, _s()), 'bad shape')   # nw steps > R
    assert bool(torch.isnan(out.full).all())


# ------------------------------------------------------------------------------------
# saliency_reduce: saliency_rows_kernel (+ saliency_class_sum_kernel)
# ------------------------------------------------------------------------------------

REDUCE_CASES = [(20000, 3, 9, 1), (360, 2, 200, 2), (100, 15, 4, 32), (1200, 126, 2, 3), (65, 1, 1, 1), (63, 7, 5, 4)]
# the case of each method that also forms the class sums (C = 4, one class absent, acc pre-filled)
REDUCE_SUMS = {'gradient': (360, 2, 200, 2), 'grad_x_input': (63, 7, 5, 4), 'integrated': (100, 15, 4, 32)}


@pytest.mark.parametrize('method', ['gradient', 'grad_x_input', 'integrated'])
@pytest.mark.parametrize('M,F,nw,steps', REDUCE_CASES, ids=['M%d_F%d_nw%d_s%d' % c for c in REDUCE_CASES])
def test_saliency_reduce(dev, L, M, F, nw, steps, method):
    """wy = max(1, min(nw, ceil(1024 / ceil(M / 64)))) blocks along the windows: (20000, ., 9) has wy = 4 (blocks walk two or
    three windows: the strided loop), (360, ., 200) wy = 171 (some blocks two windows, some one); M = 65, 63, 100, 1200 are no
    multiples of 64; F = 126 is the limit.  x absolute x baseline x order, every element."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(M + 13 * F + nw + steps)
    Mp = plane_stride(M)
    S = nw + 1
    dx = _poison_planes(rs.randn(nw * steps + 1, F, Mp), M)                # one plane row more than the windows use
    x = rs.randn(S, M, F).astype(np.float32)
    sample = rs.randint(0, S, nw).astype(np.int32)
    x0 = rs.randn(M, F).astype(np.float32)
    order = rs.permutation(M).astype(np.int32)
    dxd, xd, sd, bd, od = _to(dx, dev), _to(x, dev), _to(sample, dev), _to(x0, dev), _to(order, dev)
    out = Guarded((nw, M, F), torch.float32, dev)
    sums = REDUCE_SUMS[method] == (M, F, nw, steps)
    C = 4
    cls = rs.choice([0, 1, 3], nw).astype(np.int64)                         # class 2 has no window
    cd = _to(cls, dev)
    acc0 = rs.randn(C, M, F)
    worst = 0.0
    for absolute in (False, True):
        for base in ((None, x0) if method == 'integrated' else (None,)):
            for perm in (order, None):
                what = 'reduce[%s,abs=%s,base=%s,order=%s]' % (method, absolute, base is not None, perm is not None)
                args = (dxd, xd if method != 'gradient' else None, od if perm is not None else None,
                        sd if method != 'gradient' else None, bd if base is not None else None, steps, method, absolute)
                acc = Guarded((C, M, F), torch.float64, dev) if sums else None
                results = []
                for _ in range(2):
                    out.refill()
                    if sums:
                        acc.refill()
                        acc.t.copy_(torch.as_tensor(acc0))
                        ops.saliency_reduce(*args, out.t, cls=cd, acc=acc.t)
                        _named('saliency_rows_kernel + saliency_class_sum_kernel')
                        results.append((out.t.clone(), acc.t.clone()))
                        assert acc.margins_intact()
                    else:
                        ops.saliency_reduce(*args, out.t)
                        _named('saliency_rows_kernel')
                        results.append((out.t.clone(),))
                    assert out.margins_intact()
                assert all(torch.equal(a, b) for a, b in zip(*results)), what + ': two runs differ'
                got = results[0][0].cpu().numpy()
                ref, bound = ref_reduce(dx, x, perm, sample, base, nw, steps, M, method, absolute)
                worst = max(worst, _within(got, ref, bound, what))
                if method == 'gradient' and steps == 1:
                    assert _same_bits(got, ref), what + ': a copy must be bit-exact'
                if sums:
                    got_acc = results[0][1].cpu().numpy()
                    assert _same_bits(got_acc, ref_class_sums(got, cls, acc0)), what + ': class sums'
                    assert _same_bits(got_acc[2], acc0[2])
    record_measured('attr_reduce[%d,%d,%d,%d,%s]' % (M, F, nw, steps, method), ratio_to_bound=worst)


def test_saliency_reduce_refusals(dev, L):
    dx = torch.zeros((2, 127, 64), device=dev)
    out = Guarded((2, 64, 127), torch.float32, dev)
    _refused(L, L.chebgcn_saliency_reduce(_p(dx), None, None, None, None, 2, 1, 64, 127, 0, 0, _p(out.t), None, 0, None, _s()),
             'too large')
    assert bool(torch.isnan(out.full).all())


# ------------------------------------------------------------------------------------
# saliency_class_sum_kernel through chebgcn_occlusion_class_sums
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('S,G,C', [(2500, 300, 7), (1024, 256, 3), (1025, 1, 2), (10, 1000, 5)])
def test_class_sums(dev, S, G, C):
    """Chunks of 1024 windows (2500: three, 1024: exactly one, 1025: one and a single window), 256 elements per block (300 and
    1000 are no multiples, G = 1 a single element); one class absent; acc pre-filled; a second call accumulates on the first."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(S + G)
    drop = rs.randn(S, G).astype(np.float32)
    absent = C // 2
    cls = rs.choice([k for k in range(C) if k != absent], S).astype(np.int64)
    acc0 = rs.randn(C, G)
    dd, cd = _to(drop, dev), _to(cls, dev)
    ref1 = ref_class_sums(drop, cls, acc0)
    ref2 = ref_class_sums(drop, cls, ref1)
    acc = Guarded((C, G), torch.float64, dev)
    runs = []
    for _ in range(2):
        acc.refill()
        acc.t.copy_(torch.as_tensor(acc0))
        ops.occlusion_class_sums(dd, cd, acc.t)
        _named('saliency_class_sum_kernel')
        first = acc.t.cpu().numpy()
        ops.occlusion_class_sums(dd, cd, acc.t)
        runs.append((first, acc.t.cpu().numpy()))
        assert acc.margins_intact()
    assert _same_bits(runs[0][0], ref1) and _same_bits(runs[0][1], ref2)
    assert _same_bits(runs[0][0][absent], acc0[absent]) and _same_bits(runs[0][1][absent], acc0[absent])
    assert _same_bits(runs[1][0], runs[0][0]) and _same_bits(runs[1][1], runs[0][1])


# ------------------------------------------------------------------------------------
# saliency_seed
# ------------------------------------------------------------------------------------

def _seed_logits(rs, B, C):
    """8 * randn (as test_softmax_xent_vs_float64), with two rows built by hand: one class ahead of the rest by 30."""
    z = (rs.randn(B, C) * 8).astype(np.float32)
    lead = np.zeros(B, np.int64)
    if C > 1:
        for r in range(min(B, 2)):
            z[r] = rs.randn(C).astype(np.float32)
            lead[r] = (r + 1) % C
            z[r, lead[r]] = z[r].max() + np.float32(30.0)
    return z, lead


def _seed_run(L, z, targets, rep, nvalid, score, want_grad, dev):
    """One guarded launch: (dlogits or None, cls_out) as NumPy, margins checked."""
    B, C = z.shape
    nwin = (B + rep - 1) // rep
    dz = Guarded((B, C), torch.float32, dev) if want_grad else None
    cls = Guarded((nwin,), torch.int64, dev)
    _ok(L.chebgcn_saliency_seed(_p(z), _p(targets), rep, nvalid, {'logit': 0, 'logprob': 1}[score],
                                _p(dz.t) if want_grad else None, _p(cls.t), B, C, _s()), 'saliency_seed')
    _named('saliency_seed_kernel<%s>' % ('target' if targets is not None else 'argmax'))
    assert cls.margins_intact() and (dz is None or dz.margins_intact())
    return (dz.t.cpu().numpy() if want_grad else None), cls.t.cpu().numpy()


SEED_CASES = [(1, 1, 1, 1), (64, 5, 1, 64), (65, 22, 1, 60), (200, 7, 8, 187), (1000, 33, 32, 1000)]


@pytest.mark.parametrize('given', [True, False], ids=['target', 'argmax'])
@pytest.mark.parametrize('score', ['logit', 'logprob'])
@pytest.mark.parametrize('B,C,rep,nvalid', SEED_CASES, ids=['B%d_C%d_rep%d_nv%d' % c for c in SEED_CASES])
def test_saliency_seed(dev, L, B, C, rep, nvalid, score, given):
    """64 rows per block with rep > 1 and nvalid < B; C = 1; a confident row under 'logprob', right (the target leads by 30) and
    wrong (another class does); rows >= nvalid exactly 0 and their cls_out untouched; want_grad=False; a target of C and of -1."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(B + C + rep)
    z, lead = _seed_logits(rs, B, C)
    nwin, nlive = (B + rep - 1) // rep, (nvalid + rep - 1) // rep
    t = rs.randint(0, C, nwin).astype(np.int64)
    if given and C > 1:
        t[0] = lead[0]                                  # confident and right
        if rep == 1:
            t[1] = (lead[1] + 1) % C                    # confident and wrong
    zd = _to(z, dev)
    td = _to(t, dev) if given else None
    t_row = t[np.arange(B) // rep] if given else torch.argmax(torch.as_tensor(z), 1).numpy()
    got, cls = _seed_run(L, zd, td, rep, nvalid, score, True, dev)
    ref, bound = ref_seed(z[:nvalid], t_row[:nvalid], score)
    ratio = _within(got[:nvalid], ref, bound, 'seed')
    if score == 'logit':
        assert _same_bits(got[:nvalid], ref)
    assert _same_bits(got[nvalid:], np.zeros((B - nvalid, C)))
    assert np.array_equal(cls[:nlive], t_row[::rep][:nlive]) and (cls[nlive:] == ISENT).all()
    record_measured('attr_seed[%d,%d,%d,%d,%s,%s]' % (B, C, rep, nvalid, score, given), ratio_to_bound=ratio)
    # the ops wrapper is the second run; then without the gradient
    cls2 = Guarded((nwin,), torch.int64, dev)
    again = ops.saliency_seed(zd, td, rep, nvalid, score, cls_out=cls2.t)
    assert _same_bits(again.cpu().numpy(), got) and np.array_equal(cls2.t.cpu().numpy(), cls) and cls2.margins_intact()
    none, cls3 = _seed_run(L, zd, td, rep, nvalid, score, False, dev)
    assert none is None and np.array_equal(cls3, cls)
    assert ops.saliency_seed(zd, td, rep, nvalid, score, cls_out=cls2.t, want_grad=False) is None
    if given:
        for bad in (C, -1):
            tb = t.copy()
            wb = nlive // 2
            tb[wb] = bad
            gb, cb = _seed_run(L, zd, _to(tb, dev), rep, nvalid, score, True, dev)
            rows = (np.arange(B) // rep == wb) & (np.arange(B) < nvalid)
            assert rows.any() and np.isnan(gb[rows]).all() and _same_bits(gb[~rows], got[~rows])
            assert np.array_equal(cb[:nlive], tb[:nlive])


def test_saliency_seed_argmax_ties_and_nan(dev, L):
    """The argmax rule is torch.argmax's: the first maximum wins a tie, a NaN counts as the largest value (the first one)."""
    rs = np.random.RandomState(5)
    B, C = 130, 9
    z = rs.randint(-3, 4, (B, C)).astype(np.float32)    # small integers: exact ties in most rows
    z[3, 4] = np.nan
    z[4, [2, 6]] = np.nan
    z[5, 0] = np.nan
    z[6, C - 1] = np.nan
    z[7] = 2.0
    z[8, [1, 5]] = np.inf
    want = torch.argmax(torch.as_tensor(z), 1).numpy()
    assert want[3] == 4 and want[4] == 2 and want[5] == 0 and want[6] == C - 1 and want[7] == 0 and want[8] == 1
    got, cls = _seed_run(L, _to(z, dev), None, 1, B, 'logit', True, dev)
    assert np.array_equal(cls, want)
    assert _same_bits(got, ref_seed(np.zeros((B, C)), want, 'logit')[0])
    got2, cls2 = _seed_run(L, _to(z, dev), None, 1, B, 'logit', True, dev)
    assert _same_bits(got2, got) and np.array_equal(cls2, cls)


# ------------------------------------------------------------------------------------
# occlusion_rows
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,M,F', [(90, 100, 3), (1200, 1200, 2), (64, 64, 125)])
@pytest.mark.parametrize('G', [1, 7, 8, 100])
def test_occlusion_rows(dev, L, G, N, M, F):
    """G + 1 against the 8-row chunk of a workgroup: 2 (four windows per workgroup), 8, 9 (straddling), 101; passes that start
    on neither a window nor a chunk boundary, whose length is no multiple of 8, and that run 11 rows past S (G + 1); F = 125 is
    the limit of chebgcn_occlusion_supported.  Bit for bit, with and without a baseline."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(G + N + F)
    S, G1 = 5, G + 1
    x = rs.randn(S, N, F).astype(np.float32)
    x0 = rs.randn(N, F).astype(np.float32)
    perm = _fake_perm(rs, N, M)
    gid = rs.randint(-1, G, M).astype(np.int32)
    used = min(G, M)                                    # every id used (as far as there are positions: G = 100 at M = 64)
    gid[rs.permutation(M)[:used]] = np.arange(used)
    xd, bd, pd, gd = _to(x, dev), _to(x0, dev), _to(perm, dev), _to(gid, dev)
    r_last = (S - 1) * G1 + G1 // 2                     # inside the last window
    for r0, R in [(0, 8), (0, 37), (13, 24), (r_last, S * G1 - r_last + 11)]:
        out = Guarded((R, F, plane_stride(M)), torch.float32, dev)
        for base, based in ((None, None), (x0, bd)):
            out.refill()
            _ok(L.chebgcn_occlusion_rows(_p(xd), _p(pd), _p(gd), _p(based), _p(out.t), r0, R, S, G, N, M, F, _s()),
                'occlusion_rows')
            _named('occlusion_rows_kernel')
            got = out.t.cpu().numpy()
            assert out.margins_intact()
            ref = ref_occlusion_rows(x, perm, gid, base, r0, R, G, M)
            assert _same_bits(got, ref), 'rows r0=%d R=%d baseline=%s: %d elements differ' % (
                r0, R, base is not None, int((_bits(got) != _bits(ref)).sum()))
            assert not got[:, :, M:].any() and not got[max(0, S * G1 - r0):].any()
            again = ops.occlusion_rows(xd, pd, gd, based, r0, R, G, M)
            _named('occlusion_rows_kernel')
            assert torch.equal(again, out.t)


def test_occlusion_rows_refusals(dev, L):
    x, gid = torch.zeros((1, 64, 126), device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
    out = Guarded((8, 126, 64), torch.float32, dev)
    assert L.chebgcn_occlusion_supported(125) == 1 and L.chebgcn_occlusion_supported(126) == 0
    _refused(L, L.chebgcn_occlusion_rows(_p(x), None, _p(gid), None, _p(out.t), 0, 8, 1, 7, 64, 64, 126, _s()), 'too large')
    assert bool(torch.isnan(out.full).all())


# ------------------------------------------------------------------------------------
# occlusion_score
# ------------------------------------------------------------------------------------

def _score_run(ops, z, cls, S, G, score, cut, dev):
    """The run's rows cut into passes of ``cut`` rows (None: one pass), every pass a full ``cut`` rows (NaN logits behind the
    last row of the run), ref carried from pass to pass; (ref [S], drop [S, G]) as NumPy."""
    total, C = S * (G + 1), z.shape[1]
    cut = total if cut is None else cut
    npass = (total + cut - 1) // cut
    zp = np.full((npass * cut, C), np.nan, np.float32)
    zp[:total] = z
    zd, cd = _to(zp, dev), _to(cls, dev)
    ref, drop = Guarded((S,), torch.float32, dev), Guarded((S, G), torch.float32, dev)
    for k in range(npass):
        ops.occlusion_score(zd[k * cut:(k + 1) * cut], k * cut, G, cd, score, ref.t, drop.t)
        _named('occlusion_score_kernel<%s>' % score)
    assert ref.margins_intact() and drop.margins_intact()
    return ref.t.cpu().numpy(), drop.t.cpu().numpy()


@pytest.mark.parametrize('score', ['logit', 'logprob'])
@pytest.mark.parametrize('S,G,C', [(5, 7, 5), (3, 100, 22), (40, 8, 1)])
def test_occlusion_score(dev, S, G, C, score):
    """One pass, passes of 64 and of 13 rows (the reference row of a window in an earlier pass: ``ref[w]`` read; more than 64
    rows: several blocks): the three [S, G] tables bit-identical and within the bound; 'logit': one fp32 subtraction, bit for
    bit; a class of C for one window: its drops NaN, the others unchanged."""
    from gcn_fmri_decoding_amd import ops
    rs = np.random.RandomState(S + G + C)
    total = S * (G + 1)
    z = (rs.randn(total, C) * 8).astype(np.float32)
    cls = rs.randint(0, C, S).astype(np.int64)
    if C > 1:                                           # window 0: a confident reference row that is right, window 1: wrong;
        for w, lead in ((0, cls[0]), (1, (cls[1] + 1) % C)):      # and the opposite in their first occluded row
            for j, k in ((0, lead), (1, (lead + 1) % C)):
                row = rs.randn(C).astype(np.float32)
                row[k] = row.max() + np.float32(30.0)
                z[w * (G + 1) + j] = row
    sref, dref, bref, bdrop = ref_occlusion_drop(z, cls, S, G, score)
    runs = [_score_run(ops, z, cls, S, G, score, cut, dev) for cut in (None, 64, 13, None)]
    for ref_k, drop_k in runs[1:]:
        assert _same_bits(ref_k, runs[0][0]) and _same_bits(drop_k, runs[0][1])
    got_ref, got_drop = runs[0]
    r1, r2 = _within(got_ref, sref, bref, 'score ref'), _within(got_drop, dref, bdrop, 'score drop')
    if score == 'logit':
        z3 = z.reshape(S, G + 1, C)[np.arange(S), :, cls]                              # [S, G + 1] float32
        assert _same_bits(got_ref, z3[:, 0]) and _same_bits(got_drop, z3[:, :1] - z3[:, 1:])
    record_measured('attr_occlusion_score[%d,%d,%d,%s]' % (S, G, C, score), ref_ratio_to_bound=r1, drop_ratio_to_bound=r2)
    bad = cls.copy()
    bad[S // 2] = C
    for cut in (None, 13):
        ref_b, drop_b = _score_run(ops, z, bad, S, G, score, cut, dev)
        keep = np.arange(S) != S // 2
        assert np.isnan(drop_b[S // 2]).all() and np.isnan(ref_b[S // 2])
        assert _same_bits(drop_b[keep], got_drop[keep]) and _same_bits(ref_b[keep], got_ref[keep])


# ------------------------------------------------------------------------------------
# gradcam_weights
# ------------------------------------------------------------------------------------

def _cancelling_plane(rs, N):
    """Values of magnitude 512 .. 2048 whose sum is exactly 1: pairs +-k / 1024 and a single 1, shuffled.  Multiples of 2^-10
    below 2^11: every float64 partial sum is exact in any order; fp32 partial sums (up to ~1e5) are not."""
    k = rs.randint(1 << 19, 1 << 21, (N - 1) // 2).astype(F64) / 1024.0
    v = np.concatenate([k, -k, [1.0], np.zeros((N - 1) % 2)])
    return rs.permutation(v).astype(np.float32)


@pytest.mark.parametrize('N', [1, 2, 3, 5, 1023, 1024, 1025, 4095, 4097, 20476])
def test_gradcam_weights(dev, L, N):
    """Seven planes of N vertices (N = 1, 2, 3, N = 1, 2, 3 mod 4, around one and four turns of the 1024-vertex stride); one
    plane whose sum cancels to 1 from terms of ~1e3 (a float32 accumulator misses it by far more than an ulp); NaN pads."""
    rs = np.random.RandomState(N)
    F, Mp = 7, plane_stride(N)
    g = rs.randn(1, F, Mp).astype(np.float32)
    g[0, 1] *= 1e3
    if N >= 3:
        g[0, 3, :N] = _cancelling_plane(rs, N)
        assert float(g[0, 3, :N].astype(F64).sum()) == 1.0
    g = _poison_planes(g, N)
    gd = _to(g, dev)
    alpha = Guarded((1, F), torch.float32, dev)
    runs = []
    for _ in range(2):
        alpha.refill()
        _ok(L.chebgcn_gradcam_weights(_p(gd), 1, F, N, _p(alpha.t), _s()), 'gradcam_weights')
        _named('gradcam_weights_kernel')
        assert alpha.margins_intact()
        runs.append(alpha.t.cpu().numpy())
    assert _same_bits(runs[0], runs[1])
    ref, bound = ref_gradcam_weights(g, N)
    ratio = _within(runs[0], ref.astype(np.float32).astype(F64), bound, 'weights')
    if N >= 3:
        assert runs[0][0, 3] == np.float32(1.0 / N)
    record_measured('attr_gradcam_weights[%d]' % N, ratio_to_bound=ratio)


# ------------------------------------------------------------------------------------
# gradcam_map
# ------------------------------------------------------------------------------------

def _cam_inputs(rs, nw, F, N, dev):
    Mp = plane_stride(N)
    A = _poison_planes(rs.randn(nw, F, Mp), N)
    G = _poison_planes(rs.randn(nw, F, Mp), N)
    return A, G, _to(A, dev), _to(G, dev)


def _cam_alpha(L, Gd, nw, F, N, dev):
    alpha = torch.empty((nw, F), dtype=torch.float32, device=dev)
    _ok(L.chebgcn_gradcam_weights(_p(Gd), nw, F, N, _p(alpha), _s()), 'gradcam_weights')
    return alpha


def _cam_run(L, Ad, Gd, alpha, order_d, nw, F, N, P, relu, ldo, dev):
    out = Guarded((nw, ldo), torch.float32, dev)
    runs = []
    for _ in range(2):
        out.refill()
        _ok(L.chebgcn_gradcam_map(_p(Ad), _p(Gd) if alpha is None else None, _p(alpha), _p(order_d), nw, F, N, P, int(relu),
                                  _p(out.t), ldo, _s()), 'gradcam_map')
        _named('gradcam_map_kernel<%s>' % ('grad_x_activation' if alpha is None else 'gradcam'))
        assert out.margins_intact()
        runs.append(out.t.clone())
    assert torch.equal(runs[0], runs[1]) or _same_bits(runs[0].cpu().numpy(), runs[1].cpu().numpy())
    return runs[0].cpu().numpy()


CAM_CASES = [(1, 1, 1, 1), (360, 16, 1, 3), (1025, 5, 4, 2), (3000, 7, 64, 2), (20476, 3, 1, 2), (100, 33, 8, 4)]


@pytest.mark.parametrize('method', ['gradcam', 'grad_x_activation'])
@pytest.mark.parametrize('N,F,P,nw', CAM_CASES, ids=['N%d_F%d_P%d_nw%d' % c for c in CAM_CASES])
def test_gradcam_map(dev, L, N, F, P, nw, method):
    """N over several 1024-vertex tiles with P > 1 and an order table; F = 1, 3, 5, 7, 33 (no multiples of the unroll of 4);
    ldo = N P and N P + 12 (the tail keeps the sentinel); relu on and off.  'gradcam' takes the fp32 alpha the weights kernel
    returned (checked on its own in test_gradcam_weights) as the reference's weights."""
    rs = np.random.RandomState(N + F + P)
    A, G, Ad, Gd = _cam_inputs(rs, nw, F, N, dev)
    alpha = _cam_alpha(L, Gd, nw, F, N, dev) if method == 'gradcam' else None
    W = alpha.cpu().numpy() if alpha is not None else G
    order = rs.permutation(N).astype(np.int32)
    od = _to(order, dev)
    worst = 0.0
    for relu in (False, True):
        for perm, pd in ((None, None), (order, od)):
            for ldo in (N * P, N * P + 12):
                got = _cam_run(L, Ad, Gd, alpha, pd, nw, F, N, P, relu, ldo, dev)
                ref, bound = ref_gradcam_map(A, W, N, P, relu, perm, ldo)
                worst = max(worst, _within(got, ref, bound, 'map[relu=%s,order=%s,ldo=%d]' % (relu, perm is not None, ldo)))
                if relu:
                    assert (got[:, :N * P] >= 0).all()
    record_measured('attr_gradcam_map[%d,%d,%d,%d,%s]' % (N, F, P, nw, method), ratio_to_bound=worst)


@pytest.mark.parametrize('method', ['gradcam', 'grad_x_activation'])
def test_gradcam_map_malformed_order(dev, L, method):
    """Two entries of the order table outside [0, N) (-1 and N) write nothing: exactly the 2 P outputs of the two reference
    vertices nobody maps to keep the sentinel, everything else is right."""
    rs = np.random.RandomState(77)
    N, F, P, nw = 1500, 6, 4, 2
    A, G, Ad, Gd = _cam_inputs(rs, nw, F, N, dev)
    alpha = _cam_alpha(L, Gd, nw, F, N, dev) if method == 'gradcam' else None
    order = rs.permutation(N).astype(np.int32)
    order[5], order[1300] = -1, N
    got = _cam_run(L, Ad, Gd, alpha, _to(order, dev), nw, F, N, P, False, N * P, dev)
    ref, bound = ref_gradcam_map(A, alpha.cpu().numpy() if alpha is not None else G, N, P, False, order, N * P)
    assert int(np.isnan(ref[0]).sum()) == 2 * P
    _within(got, ref, bound, 'map with a malformed table')


def test_gradcam_refusals(dev, L):
    N, F, P = 64, 3, 2
    A = torch.zeros((1, F, 64 + 4), device=dev).view(-1)
    al = torch.zeros((1, F), device=dev)
    out = Guarded((1, N * P), torch.float32, dev)
    a, g = A[:F * 64], A[:F * 64]

    def call(a, g, al, P, ldo):
        return L.chebgcn_gradcam_map(_p(a), _p(g), _p(al), None, 1, F, N, P, 0, _p(out.t), ldo, _s())

    _refused(L, call(a, None, al, P, N * P - 1), 'hold fewer')
    _refused(L, call(a, None, al, 3, N * 3), 'bad shape')
    _refused(L, call(a, g, al, P, N * P), 'exactly one')
    _refused(L, call(a, None, None, P, N * P), 'exactly one')
    _refused(L, call(A[1:1 + F * 64], None, al, P, N * P), 'aligned')
    assert bool(torch.isnan(out.full).all())
    w = Guarded((1, F), torch.float32, dev)
    _refused(L, L.chebgcn_gradcam_weights(_p(A[1:1 + F * 64]), 1, F, N, _p(w.t), _s()), 'aligned')
    assert bool(torch.isnan(w.full).all())
