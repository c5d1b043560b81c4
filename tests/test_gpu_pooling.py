"""Every pooling kernel arm of csrc/pointwise.hip against a float64 NumPy restatement of b1relu / b2relu + mpool1 / apool1
(lib_new/models_gcn.py:619-648) and their gradients, at pool sizes 1 ... 128.  Needs an MI355X: ``-m gpu``.

The restatement behaves like ``_pool_ref`` of test_gpu_round6.py: the first maximum wins; where ``relu`` is set and the maximum
is not positive no gradient flows; an average member behind a ReLU takes its share only where it was positive.  The bias add is
one fp32 rounding (TF's fp32 add), everything after it is float64.  Pooled outputs and dy are selections of fp32 values times
1 or a power of two, so they are compared bit for bit; the fp32 average also against the float64 mean within p * 2^-24.

The shape tables follow the dispatch arithmetic of the entry points: ``_brelu_bwd_arm`` and ``_scatter_geometry`` restate it,
every call asserts that ``_lib.last_dispatch()`` names the arm the restatement predicts, and
``test_tables_reach_every_arm`` asserts that the tables reach every arm and every geometry of pool_scatter_bwd_kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, ops
from gcn_fmri_decoding_amd._lib import BIAS_FILTER, BIAS_NONE, BIAS_VERTEX, POOL_AVG, POOL_MAX, plane_stride

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BK = ['CHEBGCN_BIAS_NONE', 'CHEBGCN_BIAS_FILTER', 'CHEBGCN_BIAS_VERTEX']
LDS = 160 * 1024
MASK_REFUSED = 'average pooling keeps a ReLU mask only for pool <= 8'


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, n, fill=float('nan'), dtype=torch.float32):
    """host [..., k] -> device [..., n] with ``fill`` in the pad (poison: the pad is never read as data)."""
    t = torch.full(a.shape[:-1] + (n,), fill, dtype=dtype)
    t[..., :a.shape[-1]] = torch.as_tensor(a)
    return t.to(DEV)


def _twice(fn):
    """Run a launch twice into fresh poisoned buffers: (the dispatch it reached, the first run's outputs); the two runs bit-identical."""
    a = fn()
    name = _lib.last_dispatch()
    b = fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x is not None:
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), '%s: two runs differ' % name
    return name, [x.cpu().numpy() if x is not None else None for x in a]


# ------------------------------------------------------------------------------------------------------------ restatement

def _inputs(rs, B, F, M, p):
    """Pre-bias activations [B, F, M] fp32 and the two biases, with the edges pooling kernels get wrong: tied maxima (one of
    them on members past the eighth), a cluster entirely below zero and one entirely at zero (under ReLU: no gradient)."""
    x = rs.randn(B, F, M).astype(np.float32)
    bf = (0.1 * rs.randn(F)).astype(np.float32)
    bv = (0.1 * rs.randn(F, M)).astype(np.float32)
    if p > 1:
        c = x.reshape(B, F, M // p, p)
        Mo = M // p
        bf[:] = np.minimum(bf, 0.2)
        c[:, :, 0, -2:] = 7.5                                # tie of the last two members: member p - 2 wins
        if Mo > 1:
            c[:, :, 1, 0] = c[:, :, 1, -1] = 6.5             # tie of the first and the last member: member 0 wins
        if Mo > 2:
            c[:, :, 2, :] = -np.abs(c[:, :, 2, :]) - 0.5     # all negative (with either bias)
        if Mo > 3:
            c[:, :, 3, :] = -0.25                            # (stays <= 0 after either bias)
        if Mo > 4:
            c[:, :, 4, :] = 0.0                              # all exactly zero without a bias
        bv[:, :5 * p] = 0.0                                  # the ties and signs survive a per-vertex bias
    return x, bf, bv


def _ref(x, bias, bias_kind, p, kind, relu):
    """The restatement on [B, F, M]: dict(v = fp32 pre-ReLU activations, out = fp32 pooled [B, F, Mo] (in-order fp32 sum for the
    average), out64 (float64 mean), arg = the forward's byte (max: first winner; average: bit i = member i < 8 positive),
    sel = pool_gather's byte (max: 0xFF where relu and the maximum is not positive), g = d(out_j)/d(x_v) [B, F, M] float64)."""
    B, F, M = x.shape
    if bias_kind == BIAS_FILTER:
        v = (x + bias[None, :, None]).astype(np.float32)
    elif bias_kind == BIAS_VERTEX:
        v = (x + bias[None, :, :M]).astype(np.float32)
    else:
        v = x
    a = np.maximum(v, np.float32(0)) if relu else v
    r = {'v': v}
    if p == 1:
        r.update(out=a, out64=a.astype(np.float64), arg=None, sel=None,
                 g=(v > 0).astype(np.float64) if relu else np.ones(v.shape))
        return r
    c = a.reshape(B, F, M // p, p)
    if kind == POOL_MAX:
        out = c.max(axis=3)
        arg = c.argmax(axis=3)                               # first maximum
        g = np.zeros(c.shape)
        np.put_along_axis(g, arg[..., None], 1.0, axis=3)
        dead = (out <= 0) if relu else np.zeros(out.shape, bool)
        g *= ~dead[..., None]
        r.update(out=out, out64=out.astype(np.float64), arg=arg.astype(np.uint8),
                 sel=np.where(dead, 0xFF, arg).astype(np.uint8))
    else:
        s = c[..., 0].copy()
        for i in range(1, p):                                # members added in order, like the kernels
            s = s + c[..., i]
        pos = c > 0
        mask = np.zeros(s.shape, np.int64)
        for i in range(min(p, 8)):
            mask |= pos[..., i].astype(np.int64) << i
        g = np.full(c.shape, 1.0 / p) * (pos if relu else 1.0)
        r.update(out=s * np.float32(1.0 / p), out64=c.astype(np.float64).mean(axis=3), arg=mask.astype(np.uint8),
                 sel=mask.astype(np.uint8), abs64=np.abs(c.astype(np.float64)).mean(axis=3))
    r['g'] = g.reshape(B, F, M)
    return r


def _relu_mask(v, Mp):
    """The ReLU mask contract_fwd leaves at pool 1: [B][F][Mp/4] bytes, bit i of byte q = vertex 4q + i positive (pad: 0)."""
    B, F, M = v.shape
    bits = np.zeros((B, F, Mp), np.uint8)
    bits[:, :, :M] = v > 0
    q = bits.reshape(B, F, Mp // 4, 4)
    return (q[..., 0] | (q[..., 1] << 1) | (q[..., 2] << 2) | (q[..., 3] << 3)).astype(np.uint8)


def _dy_ref(dout, g, p):
    return (np.repeat(dout.astype(np.float64), p, axis=2) * g).astype(np.float32)


def _check_out(what, got, r, M, p):
    Mo = M // p
    assert np.array_equal(got[:, :, :Mo], r['out']), '%s: pooled output differs' % what
    assert np.all(got[:, :, Mo:] == 0), '%s: the pooled planes\' padding is not zeroed' % what
    if 'abs64' in r:
        err = np.abs(got[:, :, :Mo] - r['out64'])
        assert np.all(err <= p * 2.0 ** -24 * r['abs64']), '%s: average vs float64: %.3e' % (what, err.max())


def _check_dbias(what, db, dy_ref, bias_kind, M, pad_zero):
    B = dy_ref.shape[0]
    if bias_kind == BIAS_VERTEX:
        ref = dy_ref.astype(np.float64).sum(axis=0)
        err = np.abs(db[:, :M] - ref).max()
        assert err <= 1e-6 * max(np.abs(ref).max(), 1e-30) * np.sqrt(B), '%s: per-vertex bias gradient %.3e' % (what, err)
        if pad_zero:
            assert np.all(db[:, M:] == 0), '%s: bias gradient padding' % what
    elif bias_kind == BIAS_FILTER:
        ref = dy_ref.astype(np.float64).sum(axis=(0, 2))
        err = np.abs(db - ref).max()
        assert err <= 2e-6 * np.abs(dy_ref).astype(np.float64).sum(axis=(0, 2)).max(), '%s: per-filter bias gradient %.3e' % (what, err)


# ------------------------------------------------------------------------------------------------------------ dispatch restatement

def _scatter_fits(M, p):
    return 2 * plane_stride(M // p) * 8 <= LDS


def _pool_bwd_parts(B, F, bias_kind):
    n = (512 + F - 1) // F
    if bias_kind != BIAS_NONE:
        n = min(n, max(1, B // 8))
    return max(1, min(n, B))


def _scatter_geometry(M, p, B, F, bias_kind):
    """(EPT, NT, prefetched, passes) of pool_scatter_bwd_kernel (pool_scatter_launch)."""
    Mp, Mpo = plane_stride(M), plane_stride(M // p)
    big = Mp // 4 > 2048
    nt = 1024 if big else 512
    if big:
        vs = min(8, (Mp // 4 + 4 * nt - 1) // (4 * nt))
        ept = 4 if Mpo <= 4096 else 8
    else:
        npb = _pool_bwd_parts(B, F, bias_kind)
        vs = max(1, min(min(4, (512 + npb * F - 1) // (npb * F)), (Mp // 4 + 511) // 512))
        ept = 2 if Mpo <= 1024 else 8
    qpz = (Mp // 4 + vs - 1) // vs
    return ept, nt, Mpo <= ept * nt, (qpz + 4 * nt - 1) // (4 * nt)


def _scatter_name(bias_kind, mapped=False):
    name = 'pool_scatter_bwd_kernel<%s>%s' % (BK[bias_kind], '<map>' if mapped else '')
    return name + (' + pool_bias_reduce_kernel<%s>' % BK[bias_kind] if bias_kind else '')


def _brelu_bwd_arm(M, p, B, F, relu, bias_kind, ws, dy, mask):
    """The kernels chebgcn_brelu_pool_bwd enqueues, as chebgcn_last_dispatch() names them."""
    Mp = plane_stride(M)
    if p > 1 and dy and Mp >= 2048 and _scatter_fits(M, p) and (bias_kind == BIAS_NONE or ws):
        return _scatter_name(bias_kind)
    fine = ((Mp // 4 + 63) // 64) * F < 512                 # bias_grad_blocks
    if p == 1 and not relu and not dy:
        name = 'bias_grad_sum_kernel<%s,%d>' % (BK[bias_kind], 16 if fine else 4)
    elif p == 1 and relu and mask:
        name = 'bias_grad_relu_kernel<%s,%d>' % (BK[bias_kind], 16 if fine else 4)
    else:
        parts = 1 if ((M + 255) // 256) * F >= 1024 else 4 if ((M + 63) // 64) * F >= 1024 else 8
        name = 'brelu_pool_bwd_kernel<%s,%d>' % (BK[bias_kind], parts)
    return name + (' + bias_filter_reduce_kernel' if bias_kind == BIAS_FILTER else '')


def _bwd_combos(p):
    """(kind, relu, bias_kind, ws, dy, mask) calls of chebgcn_brelu_pool_bwd for a layer of pool p."""
    out = []
    for bias_kind in (BIAS_NONE, BIAS_FILTER, BIAS_VERTEX):
        for ws in (True, False):
            if p == 1:
                for relu, dy, mask in ((0, True, False), (0, False, False), (1, True, True), (1, False, True), (1, True, False)):
                    if dy or bias_kind != BIAS_NONE:
                        out.append((POOL_MAX, relu, bias_kind, ws, dy, mask))
                continue
            for kind in (POOL_MAX, POOL_AVG):
                for relu in (0, 1):
                    if kind == POOL_AVG and relu and p > 8:
                        continue                             # refused: test_backwards_refuse_an_avg_relu_mask_past_8
                    for dy in ((True, False) if bias_kind != BIAS_NONE else (True,)):
                        out.append((kind, relu, bias_kind, ws, dy, kind == POOL_MAX or bool(relu)))
    return out


# ------------------------------------------------------------------------------------------------------------ chebgcn_brelu_pool_fwd

# brelu_pool_fwd_kernel: a thread per pooled vertex, a serial loop over the members; no LDS and no size limit
FWD = [
    (40, 1, 3, 5),            # pool 1: b1relu / b2relu on their own
    (2048, 2, 3, 5),
    (2048, 4, 1, 33),
    (2048, 8, 17, 1),
    (2016, 16, 3, 5),         # the pool sizes the 8-bit mask does not reach: 16 ... 128
    (2080, 32, 3, 1),         # odd Mo = 65: a padded pooled plane
    (16384, 64, 1, 5),
    (128, 128, 17, 1),        # Mo = 1
    (8192, 128, 3, 5),
]


@pytest.mark.parametrize('M,p,B,F', FWD)
def test_brelu_pool_fwd(M, p, B, F):
    lib = _lib.lib()
    rs = np.random.RandomState(M + p + B + F)
    x, bf, bv = _inputs(rs, B, F, M, p)
    Mp, Mo, Mpo = plane_stride(M), M // p, plane_stride(M // p)
    xd = _dev(x, Mp)
    biases = {BIAS_NONE: None, BIAS_FILTER: torch.as_tensor(bf).to(DEV), BIAS_VERTEX: _dev(bv, Mp)}
    for kind in ((POOL_MAX,) if p == 1 else (POOL_MAX, POOL_AVG)):
        for relu in (0, 1):
            for bias_kind in (BIAS_NONE, BIAS_FILTER, BIAS_VERTEX):
                keep = p > 1 and not (kind == POOL_AVG and relu and p > 8)

                def run():
                    out = torch.full((B, F, Mpo), float('nan'), device=DEV)
                    arg = torch.full((B, F, Mpo), 0x5A, dtype=torch.uint8, device=DEV) if keep else None
                    _lib.check(lib.chebgcn_brelu_pool_fwd(_P(xd), _P(biases[bias_kind]), bias_kind, _P(out), _P(arg), B, M, F, p,
                                                          kind, relu, _stream()), 'brelu_pool_fwd')
                    return out, arg
                name, (out, arg) = _twice(run)
                assert name == 'brelu_pool_fwd_kernel', name
                r = _ref(x, bf if bias_kind == BIAS_FILTER else bv, bias_kind, p, kind, relu)
                what = 'brelu_pool_fwd M=%d p=%d kind=%d relu=%d bias=%d' % (M, p, kind, relu, bias_kind)
                _check_out(what, out, r, M, p)
                if keep:
                    assert np.array_equal(arg[:, :, :Mo], r['arg']), what + ': argmax / mask bytes differ'
    if p > 8:
        arg = torch.zeros((B, F, Mpo), dtype=torch.uint8, device=DEV)
        out = torch.empty((B, F, Mpo), device=DEV)
        with pytest.raises(_lib.ChebgcnError, match=MASK_REFUSED):
            _lib.check(lib.chebgcn_brelu_pool_fwd(_P(xd), None, BIAS_NONE, _P(out), _P(arg), B, M, F, p, POOL_AVG, 1, _stream()),
                       'brelu_pool_fwd')


# ------------------------------------------------------------------------------------------------------------ chebgcn_pool_gather_fwd

# pool_gather_fwd_kernel: the source plane in LDS (Mp * 4 bytes <= 160 KB), 256 threads, 512 from Mp = 8192 on; p = 4 with a
# 16-byte aligned map: one int4 record per pooled vertex ('aligned'); the identity, any other pool or a misaligned map: the
# generic loop
GATHER = [
    (2048, 2, 3, 5),
    (4096, 4, 3, 5),          # p = 4: the int4 path (mapped), the generic loop (identity, misaligned map)
    (1024, 8, 3, 5),
    (2016, 16, 17, 1),
    (2080, 32, 3, 1),         # odd Mo
    (12288, 64, 1, 3),        # 512 threads
    (8192, 128, 1, 5),
    (128, 128, 3, 5),         # Mo = 1
    (16384, 16, 1, 3),
    (20480, 2, 1, 2),
    (20544, 2, 1, 1),         # Mpo = 10272: gathers, the backward refuses (test_pool_scatter_bwd)
]


@pytest.mark.parametrize('M,p,B,F', GATHER)
def test_pool_gather_fwd(M, p, B, F):
    lib = _lib.lib()
    rs = np.random.RandomState(3 * M + p + B + F)
    x, _, _ = _inputs(rs, B, F, M, p)
    Mp, Mo, Mpo = plane_stride(M), M // p, plane_stride(M // p)
    src, dst = rs.permutation(M), rs.permutation(Mo)
    pmap, _ = ops.pool_maps(p, src, dst, M, DEV)
    shifted = torch.empty(M + 1, dtype=torch.int32, device=DEV)
    shifted[1:] = pmap
    maps = {'identity': None, 'mapped': pmap}
    if p == 4:
        maps['misaligned'] = shifted[1:]                     # 4 bytes past a 16-byte boundary: the generic loop
        assert maps['misaligned'].data_ptr() % 16 != 0
    for relu in (0, 1):
        y_ref = np.maximum(x, 0) if relu else x              # what contract_fwd(pool = 1, relu) leaves
        refs = {kind: _ref(y_ref, None, BIAS_NONE, p, kind, relu) for kind in (POOL_MAX, POOL_AVG)}
        for mname, pm in maps.items():
            yd = _dev(y_ref if pm is None else y_ref[:, :, src], Mp)
            for kind in (POOL_MAX, POOL_AVG):
                r = refs[kind]
                keep = not (kind == POOL_AVG and relu and p > 8)

                def run():
                    out = torch.full((B, F, Mpo), float('nan'), device=DEV)
                    sel = torch.full((B, F, Mpo), 0x5A, dtype=torch.uint8, device=DEV) if keep else None
                    _lib.check(lib.chebgcn_pool_gather_fwd(_P(yd), _P(pm), _P(out), _P(sel), B, M, F, p, kind, relu, _stream()),
                               'pool_gather_fwd')
                    return out, sel
                name, (out, sel) = _twice(run)
                assert name == ('pool_gather_fwd_kernel' if pm is None else 'pool_gather_fwd_kernel<map>'), name
                what = 'pool_gather_fwd M=%d p=%d %s kind=%d relu=%d' % (M, p, mname, kind, relu)
                perm = slice(None) if pm is None else dst
                o_int = dict(r, out=r['out'][:, :, perm], out64=r['out64'][:, :, perm])
                if 'abs64' in r:
                    o_int['abs64'] = r['abs64'][:, :, perm]
                _check_out(what, out, o_int, M, p)
                if keep:
                    assert np.array_equal(sel[:, :, :Mo], r['sel'][:, :, perm]), what + ': selection bytes differ'
    if p > 8:
        sel = torch.zeros((B, F, Mpo), dtype=torch.uint8, device=DEV)
        out = torch.empty((B, F, Mpo), device=DEV)
        with pytest.raises(_lib.ChebgcnError, match=MASK_REFUSED):
            _lib.check(lib.chebgcn_pool_gather_fwd(_P(yd), None, _P(out), _P(sel), B, M, F, p, POOL_AVG, 1, _stream()), 'pool_gather_fwd')


def test_pool_gather_fwd_refuses_a_plane_past_the_lds():
    lib = _lib.lib()
    M = 40992                                                # Mp * 4 = 163968 bytes > 160 KB
    y = torch.zeros((1, 1, plane_stride(M)), device=DEV)
    out = torch.empty((1, 1, plane_stride(M // 2)), device=DEV)
    with pytest.raises(_lib.ChebgcnError, match='does not fit the LDS'):
        _lib.check(lib.chebgcn_pool_gather_fwd(_P(y), None, _P(out), None, 1, M, 1, 2, POOL_MAX, 0, _stream()), 'pool_gather_fwd')
    M = 40960                                                # exactly 160 KB
    y = torch.zeros((1, 1, M), device=DEV)
    out = torch.empty((1, 1, M // 2), device=DEV)
    _lib.check(lib.chebgcn_pool_gather_fwd(_P(y), None, _P(out), None, 1, M, 1, 2, POOL_MAX, 0, _stream()), 'pool_gather_fwd')
    torch.cuda.synchronize()
    assert torch.all(out == 0)


# ------------------------------------------------------------------------------------------------------------ chebgcn_pool_scatter_bwd

# pool_scatter_bwd_kernel<BIAS, HAS_OUT, EPT, NT> (_scatter_geometry): Mp <= 8192 -> NT 512, EPT 2 (Mpo <= 1024) or 8; larger
# planes -> NT 1024, EPT 4 (Mpo <= 4096) or 8; entries prefetched a window ahead while Mpo <= EPT * NT; another pass over the
# windows for every 4 * NT source quads of a gridDim.z split beyond the first
SCATTER = [
    (2016, 16, 3, 5),         # (2, 512); Mp = 2016, below brelu_pool_bwd's threshold (this entry point takes any plane)
    (2048, 16, 17, 1),        # (2, 512), source quads split over gridDim.z; two batch parts with a bias
    (2080, 32, 3, 5),         # (2, 512), odd Mo
    (4096, 2, 3, 5),          # (8, 512)
    (8192, 128, 1, 33),       # (2, 512), Mo = 64
    (128, 128, 3, 5),         # (2, 512), Mo = 1
    (16384, 16, 3, 1),        # (4, 1024)
    (16384, 2, 1, 3),         # (8, 1024), prefetched
    (20480, 2, 1, 2),         # (8, 1024), Mpo = 10240: exactly 160 KB of LDS, the non-prefetch loop
    (262144, 32, 1, 1),       # (8, 1024), 2 passes
    (1048576, 128, 1, 1),     # (8, 1024), 8 passes
]


@pytest.mark.parametrize('M,p,B,F', SCATTER)
def test_pool_scatter_bwd(M, p, B, F):
    lib = _lib.lib()
    rs = np.random.RandomState(5 * M + p + B + F)
    x, _, _ = _inputs(rs, B, F, M, p)
    Mp, Mo, Mpo = plane_stride(M), M // p, plane_stride(M // p)
    do = rs.randn(B, F, Mo).astype(np.float32)
    src, dst = rs.permutation(M), rs.permutation(Mo)
    _, smap = ops.pool_maps(p, src, dst, M, DEV)
    for relu in (0, 1):
        y_ref = np.maximum(x, 0) if relu else x
        for kind in (POOL_MAX, POOL_AVG):
            if kind == POOL_AVG and relu and p > 8:
                continue                                     # refused: test_backwards_refuse_an_avg_relu_mask_past_8
            r = _ref(y_ref, None, BIAS_NONE, p, kind, relu)
            for mapped in (False, True):
                perm = dst if mapped else slice(None)
                dout = _dev(do[:, :, perm], Mpo)
                # the forward's selection bytes (pool_gather_fwd's, checked bit for bit in test_pool_gather_fwd); NULL for the
                # average without ReLU: every member takes its share
                sel = None if (kind == POOL_AVG and not relu) else _dev(r['sel'][:, :, perm], Mpo, 0x5A, torch.uint8)
                dy_ref = _dy_ref(do, r['g'], p)
                dy_int = dy_ref[:, :, src] if mapped else dy_ref
                for bias_kind in (BIAS_NONE, BIAS_FILTER, BIAS_VERTEX):
                    nws = lib.chebgcn_pool_scatter_bwd_workspace(B, M, F, p, bias_kind)
                    assert (nws > 0) == (bias_kind != BIAS_NONE)
                    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
                    sm = smap if mapped else None

                    def run():
                        dy = torch.full((B, F, Mp), float('nan'), device=DEV)
                        db = None if bias_kind == BIAS_NONE else torch.full((F,) if bias_kind == BIAS_FILTER else (F, Mp), float('nan'),
                                                                          device=DEV)
                        _lib.check(lib.chebgcn_pool_scatter_bwd(_P(dout), _P(sel), _P(sm), _P(dy), _P(db), bias_kind, B, M, F, p, kind,
                                                                relu, _P(ws), nws, _stream()), 'pool_scatter_bwd')
                        return dy, db
                    name, (dy, db) = _twice(run)
                    assert name == _scatter_name(bias_kind, mapped), name
                    what = 'pool_scatter_bwd M=%d p=%d geo=%s kind=%d relu=%d mapped=%d bias=%d' % (
                        M, p, _scatter_geometry(M, p, B, F, bias_kind), kind, relu, mapped, bias_kind)
                    assert np.array_equal(dy[:, :, :M], dy_int), what + ': dy differs'
                    assert np.all(dy[:, :, M:] == 0), what + ': dy padding'
                    _check_dbias(what, db, dy_int, bias_kind, M, True)
                    if bias_kind != BIAS_NONE and kind == POOL_MAX and relu == 0 and not mapped:
                        dyn = torch.empty((B, F, Mp), device=DEV)
                        dbn = torch.empty((F,) if bias_kind == BIAS_FILTER else (F, Mp), device=DEV)
                        with pytest.raises(_lib.ChebgcnError, match='needs a workspace'):
                            _lib.check(lib.chebgcn_pool_scatter_bwd(_P(dout), _P(sel), None, _P(dyn), _P(dbn), bias_kind, B, M, F, p,
                                                                    kind, relu, None, 0, _stream()), 'pool_scatter_bwd')


def test_pool_scatter_bwd_refuses_a_pooled_plane_past_the_lds():
    """Mpo = 10240 (160 KB of LDS) runs (test_pool_scatter_bwd); Mpo = 10272 does not fit and is refused."""
    lib = _lib.lib()
    M = 20544
    dout = torch.zeros((1, 1, plane_stride(M // 2)), device=DEV)
    sel = torch.zeros((1, 1, plane_stride(M // 2)), dtype=torch.uint8, device=DEV)
    dy = torch.empty((1, 1, plane_stride(M)), device=DEV)
    with pytest.raises(_lib.ChebgcnError, match='does not fit the LDS'):
        _lib.check(lib.chebgcn_pool_scatter_bwd(_P(dout), _P(sel), None, _P(dy), None, BIAS_NONE, 1, M, 1, 2, POOL_MAX, 0, None, 0,
                                                _stream()), 'pool_scatter_bwd')


# ------------------------------------------------------------------------------------------------------------ chebgcn_brelu_pool_bwd

BWD = [
    (40, 1, 3, 5),            # pool 1: bias_grad_sum / bias_grad_relu <., 16>, brelu_pool_bwd_kernel <., 8>
    (16384, 1, 3, 33),        # pool 1: bias_grad_sum / bias_grad_relu <., 4>, brelu_pool_bwd_kernel <., 1>
    (2016, 16, 1, 128),       # Mp = 2016 < 2048: brelu_pool_bwd_kernel <., 1>
    (2016, 16, 3, 33),        # brelu_pool_bwd_kernel <., 4>
    (2016, 16, 17, 5),        # brelu_pool_bwd_kernel <., 8>
    (128, 128, 3, 5),         # brelu_pool_bwd_kernel <., 8>, Mo = 1
    (2048, 16, 17, 5),        # pool_scatter_bwd_kernel (2, 512) with a workspace (or no bias), brelu_pool_bwd_kernel <., 8> without
    (2080, 32, 3, 1),         # pool_scatter_bwd_kernel (2, 512), odd Mo
    (4096, 2, 3, 5),          # pool_scatter_bwd_kernel (8, 512)
    (8192, 128, 3, 5),        # pool_scatter_bwd_kernel (2, 512); brelu_pool_bwd_kernel <., 4> without a workspace
    (16384, 16, 3, 1),        # pool_scatter_bwd_kernel (4, 1024)
    (16384, 2, 1, 3),         # pool_scatter_bwd_kernel (8, 1024)
    (20480, 2, 1, 2),         # pool_scatter_bwd_kernel (8, 1024), the non-prefetch loop
    (20544, 2, 1, 1),         # the pooled plane does not fit: brelu_pool_bwd_kernel <., 8> whatever the caller gives
    (262144, 32, 1, 1),       # pool_scatter_bwd_kernel (8, 1024), 2 passes
]


@pytest.mark.parametrize('M,p,B,F', BWD)
def test_brelu_pool_bwd(M, p, B, F):
    lib = _lib.lib()
    rs = np.random.RandomState(7 * M + p + B + F)
    x, bf, bv = _inputs(rs, B, F, M, p)
    Mp, Mo, Mpo = plane_stride(M), M // p, plane_stride(M // p)
    do = rs.randn(B, F, Mo).astype(np.float32)
    dout = _dev(do, Mpo)
    refs = {}
    for kind, relu, bias_kind, ws, has_dy, has_mask in _bwd_combos(p):
        # the forward these gradients belong to: its output and its byte (pool 1: the ReLU mask of contract_fwd)
        key = (kind, relu, bias_kind)
        if key not in refs:
            r = _ref(x, bf if bias_kind == BIAS_FILTER else bv, bias_kind, p, kind, relu)
            out = _dev(r['out'], Mpo)
            if p == 1:
                arg = torch.as_tensor(_relu_mask(r['v'], Mp)).to(DEV)
            else:
                arg = None if (kind == POOL_AVG and not relu) else _dev(r['arg'], Mpo, 0x5A, torch.uint8)
            refs[key] = (out, arg, _dy_ref(do, r['g'], p))
        out, arg, dy_ref = refs[key]
        mask = arg if has_mask else None
        n = lib.chebgcn_brelu_pool_bwd_workspace(B, M, F, p, bias_kind)
        wsd = torch.empty(max(n, 1), dtype=torch.uint8, device=DEV) if ws else None
        what = 'brelu_pool_bwd M=%d p=%d B=%d F=%d kind=%d relu=%d bias=%d ws=%d dy=%d mask=%d' % (
            M, p, B, F, kind, relu, bias_kind, ws, has_dy, has_mask)

        def run():
            dy = torch.full((B, F, Mp), float('nan'), device=DEV) if has_dy else None
            db = None if bias_kind == BIAS_NONE else torch.full((F,) if bias_kind == BIAS_FILTER else (F, Mp), float('nan'), device=DEV)
            _lib.check(lib.chebgcn_brelu_pool_bwd(_P(dout), _P(out), _P(mask), _P(dy), _P(db), bias_kind, B, M, F, p, kind, relu,
                                                  _P(wsd), n if ws else 0, _stream()), 'brelu_pool_bwd')
            return dy, db
        if bias_kind == BIAS_FILTER and not ws:
            with pytest.raises(_lib.ChebgcnError, match='needs a workspace'):
                run()
            continue
        name, (dy, db) = _twice(run)
        want = _brelu_bwd_arm(M, p, B, F, relu, bias_kind, ws, has_dy, has_mask)
        assert name == want, (what, name, want)
        scatter = name.startswith('pool_scatter_bwd_kernel')
        if has_dy:
            assert np.array_equal(dy[:, :, :M], dy_ref), what + ': dy differs'
            if scatter:
                assert np.all(dy[:, :, M:] == 0), what + ': dy padding'
        _check_dbias(what, db, dy_ref, bias_kind, M, scatter)


def test_backwards_refuse_an_avg_relu_mask_past_8():
    """The forwards keep an average pooling's ReLU mask for pool <= 8 only (8 bits): both backwards refuse such a mask too,
    instead of passing no gradient to the members past the eighth."""
    lib = _lib.lib()
    B, F, M = 2, 3, 4096
    for p in (16, 128):
        Mpo = plane_stride(M // p)
        dout = torch.zeros((B, F, Mpo), device=DEV)
        out = torch.ones((B, F, Mpo), device=DEV)
        sel = torch.full((B, F, Mpo), 0xFF, dtype=torch.uint8, device=DEV)
        dy = torch.empty((B, F, M), device=DEV)
        with pytest.raises(_lib.ChebgcnError, match=MASK_REFUSED):
            _lib.check(lib.chebgcn_pool_scatter_bwd(_P(dout), _P(sel), None, _P(dy), None, BIAS_NONE, B, M, F, p, POOL_AVG, 1, None, 0,
                                                    _stream()), 'pool_scatter_bwd')
        for Mx in (M, 1024):                                 # the 16-byte-store kernel's planes and the scalar kernel's
            dy = torch.empty((B, F, plane_stride(Mx)), device=DEV)
            with pytest.raises(_lib.ChebgcnError, match=MASK_REFUSED):
                _lib.check(lib.chebgcn_brelu_pool_bwd(_P(dout), _P(out), _P(sel), _P(dy), None, BIAS_NONE, B, Mx, F, p, POOL_AVG, 1,
                                                      None, 0, _stream()), 'brelu_pool_bwd')


def test_tables_reach_every_arm():
    """The shape tables above reach every kernel arm the issue of this file lists (by the dispatch restatement, which every
    call checks against chebgcn_last_dispatch())."""
    arms = set()
    for M, p, B, F in BWD:
        for kind, relu, bias_kind, ws, dy, mask in _bwd_combos(p):
            if not (bias_kind == BIAS_FILTER and not ws):
                arms.update(_brelu_bwd_arm(M, p, B, F, relu, bias_kind, ws, dy, mask).split(' + '))
    names = {a.split('<')[0] + ('<%s>' % a.split(',')[1].rstrip('>') if ',' in a else '') for a in arms}
    for want in ('bias_grad_sum_kernel<4>', 'bias_grad_sum_kernel<16>', 'bias_grad_relu_kernel<4>', 'bias_grad_relu_kernel<16>',
                 'brelu_pool_bwd_kernel<1>', 'brelu_pool_bwd_kernel<4>', 'brelu_pool_bwd_kernel<8>', 'pool_scatter_bwd_kernel',
                 'bias_filter_reduce_kernel', 'pool_bias_reduce_kernel'):
        assert want in names, (want, sorted(names))
    for bias_kind in (BIAS_FILTER, BIAS_VERTEX):
        assert 'pool_bias_reduce_kernel<%s>' % BK[bias_kind] in arms
    geos = [_scatter_geometry(M, p, B, F, BIAS_NONE) for M, p, B, F in SCATTER if _scatter_fits(M, p)]
    assert {g[:2] for g in geos} == {(2, 512), (8, 512), (4, 1024), (8, 1024)}
    assert any(not g[2] for g in geos), 'no shape takes the non-prefetch loop'
    assert any(g[3] > 1 for g in geos), 'no shape takes a second pass'
    assert {p for _, p, _, _ in FWD} == {1, 2, 4, 8, 16, 32, 64, 128}
    assert {p for _, p, _, _ in GATHER} == {2, 4, 8, 16, 32, 64, 128}
    record_measured('pooling_tables', arms=sorted(arms), geometries=sorted(set(geos)))


# ------------------------------------------------------------------------------------------------------------ ops.BiasReluPool

@pytest.mark.parametrize('p', [16, 64])
@pytest.mark.parametrize('kind', [POOL_MAX, POOL_AVG])
def test_bias_relu_pool_autograd_without_relu(kind, p):
    """mpool1 / apool1 as cgcnn calls them (ops.BiasReluPool, relu=False, no bias): forward and autograd backward at pools the
    8-bit mask does not reach, on a plane that takes the 16-byte-store gradient kernel."""
    M, B, F = 4096, 3, 5
    rs = np.random.RandomState(p + kind)
    x, _, _ = _inputs(rs, B, F, M, p)
    Mo = M // p
    xd = _dev(x, plane_stride(M)).requires_grad_(True)
    w = rs.randn(B, F, Mo).astype(np.float32)
    log = _lib.dispatch_log
    _lib.dispatch_log = []
    try:
        y = ops.BiasReluPool.apply(xd, None, M, p, kind, False, BIAS_NONE)
        (y[:, :, :Mo] * torch.as_tensor(w).to(DEV)).sum().backward()
        torch.cuda.synchronize()
        names = [n for _, n in _lib.dispatch_log]
    finally:
        _lib.dispatch_log = log
    assert names == ['brelu_pool_fwd_kernel', 'pool_scatter_bwd_kernel<CHEBGCN_BIAS_NONE>'], names
    r = _ref(x, None, BIAS_NONE, p, kind, 0)
    _check_out('BiasReluPool p=%d kind=%d' % (p, kind), y.detach().cpu().numpy(), r, M, p)
    g = xd.grad.cpu().numpy()
    assert np.array_equal(g[:, :, :M], _dy_ref(w, r['g'], p)), 'BiasReluPool p=%d kind=%d: gradient differs' % (p, kind)
