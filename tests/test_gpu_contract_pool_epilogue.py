"""The pooling epilogue the contraction kernels share (fwd_epilogue_row, csrc/contract_common.h: bias, ReLU, pooling over p
consecutive vertices, the side byte) on every forward kernel that compiles it in, at pool 2 ... 128, against a float64 NumPy
restatement of b1relu / b2relu + mpool1 / apool1 (lib_new/models_gcn.py:619-648).  Needs an MI355X: ``-m gpu``.

The entries are called directly (chebgcn_contract_fwd, chebgcn_contract_fwd_bf16).  ``fwd_arm`` / ``bf16_arm`` restate the
dispatch arithmetic, every call asserts that ``_lib.last_dispatch()`` names the kernel the restatement predicts, and
``test_tables_reach_every_arm`` asserts that the case table reaches the seven kernels with pooling:

    contract_fwd_kernel<1>, contract_fwd_kernel<2>, contract_fwd_ring_kernel<pool>, contract_fwd_splitk_kernel,
    contract_fwd_bf16_kernel<P,4>, <P,4,tiles2>, <P,4,tiles4>

Every case runs two legs.

Exact leg: stack values are integers in [-4, 4], weights and biases multiples of 1/8 in [-1, 1], Fin*K <= 368.  Every product
and every partial sum is then a multiple of 1/8 of magnitude <= 1472 + 1 (14 bits): exact in fp32 in any summation order, and
exact with bf16 operands (the low parts of the three-pass split are zero).  The average is an exact sum (<= 2^24 / 8 at
p = 128) divided by a power of two.  So the pooled output over [0, M/p) and the side byte equal the restatement bit for bit --
no tolerance.  Integer data ties constantly; ``edge_census`` asserts on the host, before a case is trusted, that its reference
holds a window whose first maximum is tied with a later member and does not sit at index 0 (p = 2: a tie of its two members),
for p >= 8 one whose tied members lie in different lanes (four vertices per lane), and with ReLU a window with no positive
member (output 0.0, index 0).  ``_plant`` puts one of each into every case, the draw adds thousands.  Each launch runs twice
into freshly poisoned buffers; the two runs are bit-identical.

Round-off leg: standard-normal stack, weights and bias scaled as in test_contraction_arm_vs_float64; the pooled output
against the float64 pooling of float64 sums, relative to max |pre-activation| (maximum and mean over a window do not expand a
max-norm error): 1e-5 for the fp32 kernels and for bf16 in three passes, 1e-2 for bf16 in one pass -- the bounds
test_gpu_dispatch.py holds these kernels to.  The byte is not compared there (picks may flip under rounding).

The side byte: max pooling -- the index inside the window of the first maximum (after bias and ReLU); average pooling at
pool 2 ... 8 -- bit i set where member i is > 0 (after bias and ReLU); average pooling beyond 8 -- unspecified (the entries
refuse it together with ReLU, test_avg_relu_mask_past_8_is_refused), never asserted here.

Pad contract.  include/chebgcn.h: "the pad [M, Mp) of every plane is scratch: kernels may write it and never read it as
data".  For the contraction that means (read off the kernels):
  * the pads of its inputs (stack planes, per-vertex bias rows) may hold anything: the lanes of [M, Mp) do read them, but M is
    a multiple of p, so a pooling window never mixes pad and data and those lanes' results go to the pad of the output only.
    Here every input pad is NaN; the exact leg could not pass if a pad value reached a window of [0, M/p).
  * the pad [M/p, Mpo) of an output row and of a byte row is scratch as well: the kernels store whatever the lanes of
    [M, p * Mpo) hold (the pooled input pad -- NaN here --, zeros, or an aliased vertex 0), only inside that row's pad, or leave
    it untouched.  Nothing is promised about it and nothing is asserted about its VALUES.  What is asserted: no store leaves the
    [B][Fout][Mpo] block (sentinel rows in front of and behind both buffers stay intact; a store into a neighbouring row's data
    would break the bit-for-bit comparison), and the consumers do not read it as data: the round trip hands the buffers, pads as
    the contraction left them, to chebgcn_brelu_pool_bwd and requires the exact gradient.  The next layer's recurrence takes its
    operands by column index < M and ops.plane_empty hands out uninitialised pads all along (its tests poison the pad of x).
"""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import BIAS_FILTER, BIAS_NONE, BIAS_VERTEX, POOL_AVG, POOL_MAX, plane_stride

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
REL = 1e-5                # fp32 kernels, and bf16 in three passes (test_gpu_dispatch.py REL)
BF16_REL = 1e-2           # bf16 in one pass (test_gpu_dispatch.py BF16_REL)
MASK_REFUSED = 'average pooling keeps a ReLU mask only for pool <= 8'
POOLS = (2, 4, 8, 16, 32, 64, 128)
N, F, V = BIAS_NONE, BIAS_FILTER, BIAS_VERTEX
MAX, AVG = POOL_MAX, POOL_AVG


# ------------------------------------------------------------------------------------------------------------ restatement

def epilogue_ref(y, bias_kind, bias, relu, pool, pool_kind):
    """fwd_epilogue_row in float64.  y [B, F, M]: the sums before the bias; bias: [F] (BIAS_FILTER), [F, M] (BIAS_VERTEX) or
    None.  Returns dict(v = pre-activations (after the bias), a = activations after ReLU [B, F, M], out = pooled [B, F, M/p],
    byte = uint8 [B, F, M/p]:
    max pooling -- index of the first maximum; average, p <= 8 -- bit i = member i > 0; average beyond 8 and p = 1 -- None)."""
    y = np.asarray(y, np.float64)
    B, Fo, M = y.shape
    if bias_kind == BIAS_FILTER:
        v = y + np.asarray(bias, np.float64)[None, :, None]
    elif bias_kind == BIAS_VERTEX:
        v = y + np.asarray(bias, np.float64)[None, :, :M]
    else:
        v = y
    a = np.maximum(v, 0.0) if relu else v
    if pool == 1:
        return dict(v=v, a=a, out=a, byte=None)
    assert M % pool == 0
    c = a.reshape(B, Fo, M // pool, pool)
    if pool_kind == POOL_MAX:
        return dict(v=v, a=a, out=c.max(axis=3), byte=c.argmax(axis=3).astype(np.uint8))       # argmax: the first maximum
    byte = None
    if pool <= 8:
        byte = np.zeros(c.shape[:3], np.uint8)
        for i in range(pool):
            byte |= (c[..., i] > 0).astype(np.uint8) << i
    return dict(v=v, a=a, out=c.sum(axis=3) / pool, byte=byte)


def epilogue_grad_ref(dout, r, relu, pool, pool_kind):
    """d(loss)/d(y) [B, F, M] float64 of ``r = epilogue_ref(y, ...)`` for d(loss)/d(out) = dout [B, F, M/p]: the maximum's
    gradient goes to the member the byte names, the average's in equal shares to all, then the ReluGrad on the activations."""
    dout = np.asarray(dout, np.float64)
    B, Fo, Mo = dout.shape
    if pool == 1:
        g = dout.copy()
    elif pool_kind == POOL_MAX:
        g = np.zeros((B, Fo, Mo, pool))
        np.put_along_axis(g, r['byte'].astype(np.int64)[..., None], dout[..., None], axis=3)
    else:
        g = np.repeat(dout[..., None] / pool, pool, axis=3)
    g = g.reshape(B, Fo, Mo * pool)
    return g * (r['a'] > 0) if relu else g


def edge_census(r, relu, pool, pool_kind):
    """Counts of the windows of a reference that carry the edges a wrong epilogue gets wrong: ``tie`` -- the first maximum is
    tied with a later member and is not member 0 (p = 2: members 0 and 1 tie); ``straddle`` -- such a tie whose last tied member
    sits in another lane (four members per lane) than the first; ``dead`` -- no positive member."""
    B, Fo, M = r['a'].shape
    c = r['a'].reshape(B, Fo, M // pool, pool)
    mx = c.max(axis=3)
    first = c.argmax(axis=3)
    tied = c == mx[..., None]
    last = pool - 1 - tied[..., ::-1].argmax(axis=3)
    tie = (last > first) & ((first != 0) | (pool == 2))
    return dict(tie=int(tie.sum()), straddle=int((tie & (last // 4 != first // 4)).sum()), dead=int((mx <= 0).sum()))


def assert_edges(what, r, relu, pool, pool_kind):
    n = edge_census(r, relu, pool, pool_kind)
    if pool_kind == POOL_MAX:
        assert n['tie'] > 0, '%s: the reference holds no tied first maximum away from index 0' % what
        if pool >= 8:
            assert n['straddle'] > 0, '%s: the reference holds no tie across a lane boundary' % what
    if relu:
        assert n['dead'] > 0, '%s: the reference holds no window without a positive member' % what
    return n


# ------------------------------------------------------------------------------------------------------------ dispatch restatement

def ring_rows(FinK):
    return (FinK + 15) // 16 * 16


def small_launch(B, M):
    return (M + 511) // 512 * B < 512                        # two workgroups per CU of 256


def fwd_arm(B, M, FinK, Fout, pool, bias_kind):
    """The kernel chebgcn_contract_fwd launches (pool > 1)."""
    if Fout > 32:
        return 'contract_fwd_kernel<2>'
    if small_launch(B, M):
        return 'contract_fwd_splitk_kernel'
    if ring_rows(FinK) * 136 <= 48 * 1024 and (bias_kind != BIAS_FILTER or Fout >= 4):
        return 'contract_fwd_ring_kernel<pool>' if pool > 1 else 'contract_fwd_ring_kernel'
    return 'contract_fwd_kernel<1>'


def bf16_arm(Fout, passes):
    """The kernel chebgcn_contract_fwd_bf16 launches: fwd_bf16_tiles(Fout) vertex tiles per work item."""
    tiles = 4 if Fout <= 64 else 2 if Fout <= 128 else 1
    return 'contract_fwd_bf16_kernel<%d,4%s>' % (passes, {4: ',tiles4', 2: ',tiles2', 1: ''}[tiles])


Case = collections.namedtuple('Case', 'entry B M Fin K Fout pool kind relu bias byte')


def case_arm(c):
    if c.entry == 'f32':
        return fwd_arm(c.B, c.M, c.Fin * c.K, c.Fout, c.pool, c.bias)
    return bf16_arm(c.Fout, 3 if c.entry == 'bf16x3' else 1)


def case_id(c):
    return '%s-B%d-M%d-%dx%d-F%d-p%d-%s%s-%s%s' % (c.entry, c.B, c.M, c.Fin, c.K, c.Fout, c.pool, 'avg' if c.kind else 'max',
                                                  '-relu' if c.relu else '', 'nfv'[c.bias], '' if c.byte else '-nobyte')


# Planes: M = p * odd wherever p <= 32 (below 32 that makes Mp > M); a last 128-vertex wave tile that is only partly inside
# the plane (130, 396, 168, 48, 160, 400, 1088 = 1056 + 32, 1056); later waves of a workgroup that leave at m0 >= M (384: three
# of four, 640: the second workgroup keeps one; 130 ... 168: one or two); planes of exactly 128 and 512 vertices; p = 64 on
# M = 128 k + 64 (448, 1088).  A big launch needs B >= 512 / ceil(M / 512): 512, 256 (M = 640), 171 (M = 1056, 1088).
CASES = [Case(*t) for t in [
    # contract_fwd_splitk_kernel: small launches, Fout <= 32
    ('f32', 3, 130, 2, 2, 5, 2, MAX, 1, F, 1),
    ('f32', 2, 396, 3, 1, 3, 4, MAX, 0, V, 1),               # an odd number of reduction rows
    ('f32', 3, 168, 7, 5, 24, 8, MAX, 1, N, 1),              # 35 rows: a second ring round for wave 0
    ('f32', 3, 48, 2, 2, 5, 16, MAX, 1, V, 1),
    ('f32', 2, 160, 2, 2, 24, 32, MAX, 1, F, 1),
    ('f32', 3, 448, 3, 2, 32, 64, MAX, 0, N, 1),
    ('f32', 2, 640, 2, 2, 5, 128, MAX, 1, V, 1),
    ('f32', 2, 128, 2, 2, 3, 128, MAX, 1, N, 1),             # one pooled vertex
    ('f32', 2, 1088, 2, 2, 32, 32, MAX, 1, V, 1),
    ('f32', 3, 130, 2, 2, 5, 2, AVG, 1, V, 1),
    ('f32', 2, 396, 2, 2, 24, 4, AVG, 1, N, 1),
    ('f32', 2, 160, 1, 3, 32, 8, AVG, 1, F, 1),
    ('f32', 2, 400, 2, 2, 5, 16, AVG, 1, F, 0),              # the average beyond 8 with ReLU: no byte
    ('f32', 2, 448, 2, 2, 5, 64, AVG, 0, V, 1),              # ... without ReLU: a byte buffer is taken, its content unspecified
    # contract_fwd_ring_kernel<pool>: big launches, Fout <= 32, Fin*K <= 352
    ('f32', 512, 130, 2, 2, 5, 2, MAX, 1, F, 1),
    ('f32', 512, 396, 3, 1, 3, 4, MAX, 0, V, 1),             # three filters: the ring kernel unless the bias is per filter
    ('f32', 512, 168, 2, 2, 24, 8, MAX, 1, N, 1),
    ('f32', 512, 160, 2, 2, 3, 8, MAX, 1, N, 1),
    ('f32', 512, 48, 2, 2, 5, 16, MAX, 1, V, 1),
    ('f32', 512, 160, 2, 2, 32, 32, MAX, 1, F, 1),
    ('f32', 171, 1088, 7, 5, 32, 32, MAX, 1, V, 1),          # 35 rows: three ring rounds
    ('f32', 171, 1088, 2, 2, 5, 64, MAX, 1, V, 1),
    ('f32', 512, 512, 2, 2, 5, 64, MAX, 1, N, 1),
    ('f32', 256, 640, 2, 2, 5, 128, MAX, 1, F, 1),
    ('f32', 512, 384, 2, 2, 24, 128, MAX, 0, N, 1),
    ('f32', 512, 128, 2, 2, 5, 128, MAX, 1, V, 1),
    ('f32', 512, 130, 2, 2, 5, 2, AVG, 1, N, 1),
    ('f32', 512, 396, 2, 2, 5, 4, AVG, 1, F, 1),
    ('f32', 512, 168, 2, 2, 5, 8, AVG, 1, V, 1),
    ('f32', 512, 160, 2, 2, 5, 32, AVG, 1, F, 0),
    ('f32', 512, 384, 2, 2, 5, 128, AVG, 0, V, 1),
    # contract_fwd_kernel<1>: big launches of three filters with a per-filter bias, and of more than 352 reduction rows
    ('f32', 512, 130, 2, 2, 3, 2, MAX, 1, F, 1),
    ('f32', 512, 396, 2, 2, 3, 4, MAX, 1, F, 1),
    ('f32', 512, 168, 2, 2, 3, 8, MAX, 0, F, 1),
    ('f32', 512, 48, 2, 2, 3, 16, MAX, 1, F, 1),
    ('f32', 512, 160, 3, 3, 3, 32, MAX, 1, F, 1),
    ('f32', 171, 1088, 2, 2, 3, 64, MAX, 1, F, 1),
    ('f32', 256, 640, 2, 2, 3, 128, MAX, 1, F, 1),
    ('f32', 171, 1056, 16, 23, 5, 32, MAX, 1, V, 1),         # 368 rows, a stack of 266 MB
    ('f32', 512, 396, 2, 2, 3, 4, AVG, 1, F, 1),
    ('f32', 512, 168, 2, 2, 3, 8, AVG, 1, F, 1),
    ('f32', 512, 384, 2, 2, 3, 16, AVG, 0, F, 1),
    # contract_fwd_kernel<2>: more than 32 filters, launches of either size
    ('f32', 3, 130, 2, 2, 40, 2, MAX, 1, F, 1),
    ('f32', 2, 396, 2, 2, 64, 4, MAX, 0, V, 1),
    ('f32', 3, 168, 2, 2, 70, 8, MAX, 1, N, 1),
    ('f32', 512, 160, 2, 2, 40, 8, MAX, 1, F, 1),
    ('f32', 2, 48, 2, 2, 128, 16, MAX, 1, V, 1),
    ('f32', 2, 160, 3, 3, 256, 32, MAX, 1, F, 1),
    ('f32', 2, 1088, 2, 2, 40, 64, MAX, 1, V, 1),
    ('f32', 2, 640, 2, 2, 70, 128, MAX, 1, F, 1),
    ('f32', 3, 384, 2, 2, 40, 128, MAX, 1, N, 1),
    ('f32', 2, 130, 2, 2, 70, 2, AVG, 1, V, 1),
    ('f32', 2, 396, 2, 2, 40, 4, AVG, 1, N, 1),
    ('f32', 2, 168, 2, 2, 64, 8, AVG, 1, F, 1),
    ('f32', 2, 400, 2, 2, 40, 16, AVG, 1, V, 0),
    ('f32', 2, 448, 2, 2, 70, 64, AVG, 0, N, 1),
    # contract_fwd_bf16_kernel<P,4,tiles4>: at most 64 filters, four vertex tiles per work item
    ('bf16x3', 3, 130, 2, 2, 5, 2, MAX, 1, F, 1),
    ('bf16x1', 2, 168, 2, 2, 24, 8, MAX, 1, V, 1),
    ('bf16x3', 2, 48, 3, 3, 3, 16, MAX, 1, V, 1),
    ('bf16x3', 2, 160, 2, 2, 40, 32, MAX, 0, N, 1),
    ('bf16x3', 100, 1088, 2, 2, 32, 64, MAX, 1, V, 1),       # 300 work items on 256 workgroups: some take a second one
    ('bf16x1', 2, 640, 2, 2, 64, 128, MAX, 1, F, 1),
    ('bf16x3', 3, 130, 2, 2, 64, 2, AVG, 1, V, 1),
    ('bf16x1', 2, 396, 2, 2, 5, 4, AVG, 1, N, 1),
    ('bf16x3', 2, 168, 2, 2, 32, 8, AVG, 1, F, 1),
    ('bf16x1', 2, 384, 2, 2, 40, 128, AVG, 0, V, 1),
    # contract_fwd_bf16_kernel<P,4,tiles2>: 65 ... 128 filters
    ('bf16x3', 2, 130, 2, 2, 70, 2, MAX, 1, V, 1),
    ('bf16x1', 3, 168, 2, 2, 128, 8, MAX, 1, F, 1),
    ('bf16x3', 2, 160, 2, 2, 70, 32, MAX, 1, N, 1),
    ('bf16x3', 2, 448, 2, 2, 70, 64, MAX, 1, F, 1),
    ('bf16x1', 2, 640, 2, 2, 128, 128, MAX, 0, V, 1),
    ('bf16x1', 2, 168, 2, 2, 70, 8, AVG, 1, V, 1),
    ('bf16x3', 2, 400, 2, 2, 128, 16, AVG, 1, F, 0),
    # contract_fwd_bf16_kernel<P,4>: more than 128 filters (136: beyond the issue's list, so that a filter tile is cut here too)
    ('bf16x3', 2, 130, 2, 2, 256, 2, MAX, 1, F, 1),
    ('bf16x1', 2, 168, 2, 2, 256, 8, MAX, 1, V, 1),
    ('bf16x3', 2, 160, 2, 2, 136, 32, MAX, 1, V, 1),
    ('bf16x3', 8, 1088, 2, 2, 256, 64, MAX, 1, V, 1),        # 72 workgroups, nine vertex tiles: the XCD-aware tile order
    ('bf16x1', 2, 640, 2, 2, 256, 128, MAX, 1, N, 1),
    ('bf16x1', 3, 384, 3, 3, 256, 128, MAX, 0, F, 1),
    ('bf16x3', 2, 396, 2, 2, 256, 4, AVG, 1, V, 1),
]]


# ------------------------------------------------------------------------------------------------------------ launching

@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, 'the dispatch arms asserted here assume 256 CUs'
    return _lib.lib()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


F_SENTINEL, B_SENTINEL, B_POISON = -12345.0, 0xA5, 0x5A


def _guarded(rows, Mpo, dtype):
    """A [rows, Mpo] buffer (NaN / 0x5A poison) inside a larger one with sentinel rows on both sides: (whole, inside, guard rows)."""
    g = 256 // Mpo + 2                                       # at least two 128-vertex tiles' worth on either side
    if dtype == torch.float32:
        whole = torch.full((rows + 2 * g, Mpo), float('nan'), device=DEV)
        sent = F_SENTINEL
    else:
        whole = torch.full((rows + 2 * g, Mpo), B_POISON, dtype=torch.uint8, device=DEV)
        sent = B_SENTINEL
    whole[:g] = sent
    whole[g + rows:] = sent
    return whole, whole[g:g + rows], g, sent


def _launch(lib, c, stack, W, bias):
    """One launch of case ``c`` into fresh guarded buffers: (out [B, Fout, Mpo], byte or None), sentinels checked."""
    Mpo = plane_stride(c.M // c.pool)
    rows = c.B * c.Fout
    o_whole, out, g, o_sent = _guarded(rows, Mpo, torch.float32)
    b_whole, byte, _, b_sent = _guarded(rows, Mpo, torch.uint8) if c.byte else (None, None, g, None)
    if c.entry == 'f32':
        rc = lib.chebgcn_contract_fwd(_P(stack), _P(W), _P(bias), c.bias, _P(out), _P(byte), c.B, c.M, c.Fin, c.K, c.Fout,
                                      c.pool, c.kind, c.relu, _stream())
        want = case_arm(c)
    else:
        nws = lib.chebgcn_contract_fwd_bf16_workspace(c.Fin, c.K, c.Fout)
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        rc = lib.chebgcn_contract_fwd_bf16(_P(stack), _P(W), _P(bias), c.bias, _P(out), _P(byte), c.B, c.M, c.Fin, c.K, c.Fout,
                                           c.pool, c.kind, c.relu, 3 if c.entry == 'bf16x3' else 1, _P(ws), nws, _stream())
        want = 'pack_w_bf16_kernel + ' + case_arm(c)
    _lib.check(rc, 'contract_fwd')
    assert _lib.last_dispatch() == want, (case_id(c), _lib.last_dispatch(), want)
    torch.cuda.synchronize()
    for whole, sent in ((o_whole, o_sent), (b_whole, b_sent)):
        if whole is not None:
            assert bool((whole[:g] == sent).all()) and bool((whole[g + rows:] == sent).all()), \
                '%s: a store left the buffer (sentinel rows changed)' % case_id(c)
    shape = (c.B, c.Fout, Mpo)
    return out.view(shape), byte.view(shape) if byte is not None else None


def _twice(lib, c, stack, W, bias):
    a = _launch(lib, c, stack, W, bias)
    b = _launch(lib, c, stack, W, bias)
    for x, y in zip(a, b):
        if x is not None:
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), '%s: two runs differ' % case_id(c)
    return a


def _seed(c):
    return zlib.crc32(case_id(c).encode()) % (2 ** 31)


def _plant(c, stack, W, bias):
    """One tie and one dead window for filter 0 (exact leg).  Tie: the LAST window of window-batch 0 (it lies in the plane's last,
    possibly partial, wave tile) is all zero but for members 1 and p - 1 (p = 2: 0 and 1), which hold 4 in reduction row 0;
    W[0][0] = 1, so filter 0 sees 4 + bias at those two and the bias elsewhere.  Dead: the first window of the last
    window-batch is all zero, and filter 0's bias is -1/2 per filter, 0 per vertex in both windows."""
    p, M = c.pool, c.M
    t0 = M - p
    stack[:, 0, :, t0:M] = 0
    stack[0, 0, 0, [t0 + (1 if p > 2 else 0), t0 + p - 1]] = 4
    stack[:, c.B - 1, :, 0:p] = 0
    W[0, 0] = 1.0
    if c.bias == BIAS_FILTER:
        bias[0] = -0.5
    elif c.bias == BIAS_VERTEX:
        bias[0, t0:M] = 0
        bias[0, 0:p] = 0


def _inputs(c, exact):
    """(stack [K, B, Fin, Mp], W [Fin*K, Fout], bias) on the device, every pad NaN."""
    Mp = plane_stride(c.M)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(_seed(c) + (0 if exact else 1))
    FinK = c.Fin * c.K
    bshape = {BIAS_NONE: None, BIAS_FILTER: (c.Fout,), BIAS_VERTEX: (c.Fout, Mp)}[c.bias]
    if exact:
        stack = torch.randint(-4, 5, (c.K, c.B, c.Fin, Mp), generator=gen, device=DEV, dtype=torch.int32).float()
        W = torch.randint(-8, 9, (FinK, c.Fout), generator=gen, device=DEV, dtype=torch.int32).float() / 8
        bias = torch.randint(-8, 9, bshape, generator=gen, device=DEV, dtype=torch.int32).float() / 8 if bshape else None
        _plant(c, stack, W, bias)
    else:
        stack = torch.randn((c.K, c.B, c.Fin, Mp), generator=gen, device=DEV)
        W = torch.randn((FinK, c.Fout), generator=gen, device=DEV) * (0.5 / np.sqrt(FinK))
        bias = torch.randn(bshape, generator=gen, device=DEV) * 0.3 if bshape else None
    stack[..., c.M:] = float('nan')
    if c.bias == BIAS_VERTEX:
        bias[:, c.M:] = float('nan')
    return stack, W, bias


def _sums64(c, stack, W):
    """The sums before the bias in float64, [B, Fout, M] on the host (rows fin*K + k, models_gcn.py:611-617)."""
    S = stack[..., :c.M].permute(2, 0, 1, 3).reshape(c.Fin * c.K, c.B, c.M).double()
    return torch.einsum('rbm,ro->bom', S, W.double()).cpu().numpy()


def _host_bias(c, bias):
    if bias is None:
        return None
    b = bias.double().cpu().numpy()
    return b[:, :c.M] if c.bias == BIAS_VERTEX else b


def _byte_is_specified(c):
    return bool(c.byte) and (c.kind == POOL_MAX or c.pool <= 8)


def _exact_leg(lib, c):
    """Returns (stack, W, bias, reference, out, byte): the device buffers as the launch left them."""
    what = case_id(c)
    stack, W, bias = _inputs(c, True)
    r = epilogue_ref(_sums64(c, stack, W), c.bias, _host_bias(c, bias), c.relu, c.pool, c.kind)
    census = assert_edges(what, r, c.relu, c.pool, c.kind)
    ref32 = r['out'].astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), r['out']), what + ': the exact leg\'s reference is not exact in fp32'
    out, byte = _twice(lib, c, stack, W, bias)
    Mo = c.M // c.pool
    got = out[:, :, :Mo].cpu().numpy()
    bad = got.view(np.uint32) != (ref32 + np.float32(0)).view(np.uint32)          # (+ 0: the reference's zeros are +0)
    assert not bad.any(), '%s: %d of %d pooled values differ from the restatement, first at %s: %r against %r' % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref32[bad][0])
    if _byte_is_specified(c):
        gb = byte[:, :, :Mo].cpu().numpy()
        bad = gb != r['byte']
        assert not bad.any(), '%s: %d of %d side bytes differ from the restatement, first at %s: %d against %d' % (
            what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), gb[bad][0], r['byte'][bad][0])
    return stack, W, bias, r, out, byte, census


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_pool_epilogue_vs_float64(lib, c):
    """Exact leg: bit for bit, twice.  Round-off leg: the project's bounds.

    The three-pass cases here sum four or nine products per output.  There the split-bf16 arithmetic without its lo*lo term
    is 1.08e-05 of max |pre-activation| off on bf16x3-B100-M1088-2x2-F32-p64-max-relu-v (hi*hi + hi*lo + lo*hi of the same
    operands in float64, no kernel involved; the kernel measured 1.07e-05), above the 1e-5 held here; reductions of at most two
    k-steps therefore keep the lo*lo term (csrc/contract_bf16.hip, CG_BF16_LOLO_KSTEPS): 0.70e-05 on that case."""
    what = case_id(c)
    census = _exact_leg(lib, c)[-1]
    stack, W, bias = _inputs(c, False)
    r = epilogue_ref(_sums64(c, stack, W), c.bias, _host_bias(c, bias), c.relu, c.pool, c.kind)
    scale = np.abs(r['v']).max()                             # max |pre-activation|
    out, _ = _launch(lib, c, stack, W, bias)
    got = out[:, :, :c.M // c.pool].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - r['out']).max() / scale)
    bound = BF16_REL if c.entry == 'bf16x1' else REL
    print('%s: round-off %.3e of max |pre| (bound %.0e), edges %r' % (what, err, bound, census))
    record_measured('pool_epilogue_vs_float64[%s]' % what, arm=case_arm(c), roundoff=err, bound=bound, **census)
    assert err <= bound, '%s (%s): %.3e of max |pre-activation|' % (what, case_arm(c), err)


# ------------------------------------------------------------------------------------------------------------ further checks

@pytest.mark.parametrize('entry', ['f32', 'bf16x3'])
def test_avg_relu_mask_past_8_is_refused(lib, entry):
    """Average pooling with ReLU and a byte buffer at pool 16: an error that names the rule, and nothing is launched."""
    c = Case(entry, 2, 160, 2, 2, 5, 16, AVG, 1, N, 1)
    stack, W, _ = _inputs(c, True)
    Mpo = plane_stride(c.M // c.pool)
    out = torch.full((c.B, c.Fout, Mpo), F_SENTINEL, device=DEV)
    byte = torch.full((c.B, c.Fout, Mpo), B_SENTINEL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = _lib.last_dispatch()
    if entry == 'f32':
        rc = lib.chebgcn_contract_fwd(_P(stack), _P(W), None, N, _P(out), _P(byte), c.B, c.M, c.Fin, c.K, c.Fout, c.pool, AVG, 1,
                                      _stream())
    else:
        nws = lib.chebgcn_contract_fwd_bf16_workspace(c.Fin, c.K, c.Fout)
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        rc = lib.chebgcn_contract_fwd_bf16(_P(stack), _P(W), None, N, _P(out), _P(byte), c.B, c.M, c.Fin, c.K, c.Fout, c.pool, AVG,
                                           1, 3, _P(ws), nws, _stream())
    assert rc != 0
    assert MASK_REFUSED in lib.chebgcn_last_error().decode()
    with pytest.raises(_lib.ChebgcnError, match=MASK_REFUSED):
        _lib.check(rc, 'contract_fwd')
    assert _lib.last_dispatch() == before, 'a refused call enqueued %s' % _lib.last_dispatch()
    torch.cuda.synchronize()
    assert bool((out == F_SENTINEL).all()) and bool((byte == B_SENTINEL).all()), 'a refused call wrote its outputs'


# One round trip per pool size on the fp32 path: (case, the average with ReLU as well).  2064 = 16 * 129 takes the gradient's
# 16-byte-store kernel (Mp >= 2048), the others its scalar kernel.
ROUND_TRIPS = [Case(*t) for t in [
    ('f32', 3, 130, 2, 2, 5, 2, MAX, 1, F, 1),
    ('f32', 3, 396, 2, 2, 5, 4, MAX, 1, V, 1),
    ('f32', 512, 168, 2, 2, 5, 8, MAX, 1, F, 1),
    ('f32', 3, 2064, 2, 2, 5, 16, MAX, 1, F, 1),
    ('f32', 3, 160, 2, 2, 40, 32, MAX, 1, V, 1),
    ('f32', 3, 448, 2, 2, 5, 64, MAX, 0, N, 1),
    ('f32', 256, 640, 2, 2, 3, 128, MAX, 1, F, 1),
]]


@pytest.mark.parametrize('c0', ROUND_TRIPS, ids=case_id)
def test_round_trip_through_brelu_pool_bwd(lib, c0):
    """The out and byte buffers exactly as the contraction left them (pads included) and a random dout with a NaN pad go to
    chebgcn_brelu_pool_bwd: dy and the bias gradient equal the restated gradient under test_gpu_pooling.py's rules (dy bit for
    bit: a selection of fp32 values times 1 or a power of two)."""
    from test_gpu_pooling import _brelu_bwd_arm, _check_dbias
    kinds = (MAX, AVG) if (c0.pool <= 8 and c0.relu) else (MAX,)
    for kind in kinds:
        c = c0._replace(kind=kind)
        what = 'round trip ' + case_id(c)
        stack, W, bias, r, out, byte, _ = _exact_leg(lib, c)
        B, Fo, M, p = c.B, c.Fout, c.M, c.pool
        Mp, Mo, Mpo = plane_stride(M), M // p, plane_stride(M // p)
        rs = np.random.RandomState(_seed(c) % 1000)
        do = rs.randn(B, Fo, Mo).astype(np.float32)
        dout = torch.full((B, Fo, Mpo), float('nan'))
        dout[:, :, :Mo] = torch.as_tensor(do)
        dout = dout.to(DEV)
        dy_ref = epilogue_grad_ref(do, r, c.relu, p, kind).astype(np.float32)
        nws = lib.chebgcn_brelu_pool_bwd_workspace(B, M, Fo, p, c.bias)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
        dy = torch.full((B, Fo, Mp), float('nan'), device=DEV)
        db = None if c.bias == BIAS_NONE else torch.full((Fo,) if c.bias == BIAS_FILTER else (Fo, Mp), float('nan'), device=DEV)
        _lib.check(lib.chebgcn_brelu_pool_bwd(_P(dout), _P(out.contiguous()), _P(byte.contiguous()), _P(dy), _P(db), c.bias, B, M,
                                              Fo, p, kind, c.relu, _P(ws), nws, _stream()), 'brelu_pool_bwd')
        name = _lib.last_dispatch()
        assert name == _brelu_bwd_arm(M, p, B, Fo, c.relu, c.bias, True, True, True), (what, name)
        torch.cuda.synchronize()
        dy = dy.cpu().numpy()
        assert np.array_equal(dy[:, :, :M], dy_ref), what + ': dy differs'
        scatter = name.startswith('pool_scatter_bwd_kernel')
        if scatter:
            assert np.all(dy[:, :, M:] == 0), what + ': dy padding'
        _check_dbias(what, None if db is None else db.cpu().numpy(), dy_ref, c.bias, M, scatter)


FP32_ARMS = ('contract_fwd_kernel<1>', 'contract_fwd_kernel<2>', 'contract_fwd_ring_kernel<pool>', 'contract_fwd_splitk_kernel')
BF16_ARMS = ('contract_fwd_bf16_kernel<%d,4>', 'contract_fwd_bf16_kernel<%d,4,tiles2>', 'contract_fwd_bf16_kernel<%d,4,tiles4>')


def table_reach():
    """kernel -> its cases, after asserting that the case table reaches the seven forward kernels that compile fwd_epilogue_row
    in, with pooling: every pool size 2 ... 128 on each fp32 kernel, at least 2, 8, 32, 128 on each bf16 kernel; both pooling
    kinds, the bias kinds, ReLU on and off on each fp32 kernel.  Host arithmetic only."""
    assert 60 <= len(CASES) <= 90 and len(set(CASES)) == len(CASES)
    reach = collections.defaultdict(list)
    for c in CASES:
        assert c.pool in POOLS and c.M % c.pool == 0 and c.B >= 2 and c.Fin * c.K <= 368, c
        assert not (c.kind == AVG and c.relu and c.byte and c.pool > 8), c          # refused by the entries
        reach[case_arm(c)].append(c)
    for arm in FP32_ARMS:
        cs = reach[arm]
        assert {c.pool for c in cs} == set(POOLS), (arm, sorted({c.pool for c in cs}))
        assert {c.pool for c in cs if c.kind == MAX and c.byte} == set(POOLS), arm
        assert {c.pool for c in cs if c.kind == AVG and c.relu and c.byte} >= {4, 8}, arm
        assert any(c.kind == AVG and c.pool > 8 for c in cs), arm
        assert {c.relu for c in cs} == {0, 1}, arm
        # (contract_fwd_kernel<1> is reached by a per-filter bias on three filters, or by more than 352 reduction rows)
        assert {c.bias for c in cs} >= ({F, V} if arm == 'contract_fwd_kernel<1>' else {N, F, V}), arm
    for stem in BF16_ARMS:
        cs = reach[stem % 1] + reach[stem % 3]
        assert reach[stem % 1] and reach[stem % 3], stem
        assert {c.pool for c in cs} >= {2, 8, 32, 128}, (stem, sorted({c.pool for c in cs}))
        assert {c.kind for c in cs} == {MAX, AVG} and {c.bias for c in cs} == {N, F, V}, stem
    assert set(reach) == set(FP32_ARMS) | {s % n for s in BF16_ARMS for n in (1, 3)}, sorted(reach)
    # both ways into contract_fwd_kernel<1>, a big launch of contract_fwd_kernel<2>, both kinds of the average beyond 8
    one = reach['contract_fwd_kernel<1>']
    assert any(c.Fout == 3 and c.bias == F for c in one) and any(c.Fin * c.K > 352 for c in one)
    assert any(not small_launch(c.B, c.M) for c in reach['contract_fwd_kernel<2>'])
    assert {c.pool for c in CASES if c.kind == AVG and c.relu and c.byte} == {2, 4, 8}
    assert any(c.kind == AVG and c.pool > 8 and c.relu and not c.byte for c in CASES)
    assert any(c.kind == AVG and c.pool > 8 and not c.relu for c in CASES)
    assert {c.Fout for c in CASES} >= {3, 5, 24, 32, 40, 64, 70, 128, 256}
    assert {c.pool for c in ROUND_TRIPS} == set(POOLS) and all(c.entry == 'f32' for c in ROUND_TRIPS)
    return reach


def test_tables_reach_every_arm():
    """The case table reaches every kernel with pooling (``table_reach``, by the dispatch restatement, which every launch checks
    against chebgcn_last_dispatch())."""
    reach = table_reach()
    record_measured('contract_pool_epilogue_tables', arms={a: sorted({c.pool for c in cs}) for a, cs in sorted(reach.items())},
                    cases=len(CASES))
