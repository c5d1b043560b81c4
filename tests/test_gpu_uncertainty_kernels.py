"""The Monte-Carlo dropout kernels called directly on plain tensors -- chebgcn_fc_fwd_dropout (csrc/head.hip) and
chebgcn_mc_reduce (csrc/uncertainty.hip) -- against float64 NumPy at the edges of their tiles, chunks and waves, in the style
of tests/test_gpu_head_kernels.py (whose device plumbing this file uses).  Needs an MI355X: ``-m gpu``.

chebgcn_fc_fwd_dropout.  The masks come from ``uncertainty.dropout_keep`` (checked against the header's formula on the host,
tests/test_uncertainty_host.py).  Every case runs two legs, each with (bias, ReLU) and (no bias, no ReLU):

Exact leg: x integers in [-4, 4], W and the bias multiples of 1/8 in [-1, 1], keep = 0.5, so a kept value is 2 x exactly.
Every partial sum is a multiple of 1/8 of magnitude <= 8 n + 1, exact in fp32 in any order while 64 n + 8 < 2^24: the result
equals the float64 restatement with NO tolerance, so one wrong mask bit, window number, sample number or feature index shows.
Two runs of every leg into freshly poisoned outputs are bit-identical (on the round-off leg, where the order of a sum shows
in its last bits, that is the check of the wave-order and split reductions).

Round-off leg: standard-normal x, W / sqrt(I), keep = 0.8; with x~ = mask * x * float32(1 / keep) in float64,
    |got - ref| <= (n + 3) 2^-24 (|x~| @ |W| + |b|) + 2^-24 |ref|
-- the any-order bound of test_gpu_head_kernels.py plus the one rounding of the kept value.

Poison: the columns [I, ldx) of every x row are NaN (+Inf in one row); y and the workspace lie between guard rows of a sentinel
that must be intact; ``win`` holds scattered window numbers on both sides of 2^31; ``last_dispatch()`` names the predicted arm.

chebgcn_mc_reduce.  Logits are multiples of 1/8 (votes and ties exact), with planted exact ties, rows saturated at +-80 and
one NaN row; ``votes``, ``agreement`` and ``label`` are compared exactly (the inputs are adjusted on the host until the top-2
gap of the float64 mean probabilities is either exactly 0 by symmetry -- two identical columns -- or above 1e-3), the mean
probabilities within 1e-5 and the three entropies within 1e-5 max(1, log C) of float64."""
import collections
import zlib

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib, ops, uncertainty
from test_gpu_head_kernels import (DEV, SENTINEL, U, Guarded, _dev, _P, _stream, assert_exact, assert_same_bits, fwd_dispatch,
                                   roundoff_ratio)
from test_gpu_head_kernels import _fc_fwd as _fc_plain

pytestmark = pytest.mark.gpu
SEED = 0x5EED


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ fc_fwd_dropout

Case = collections.namedtuple('Case', 'S B I O ldx shared s0 gap layer')


def _c(S, B, I, O, ldx=None, shared=True, s0=0, gap=0, layer=0):
    return Case(S, B, I, O, ldx or (I + 3) & ~3, shared, s0, gap, layer)


FC_CASES = [
    _c(1, 1, 1, 1),
    _c(2, 31, 31, 32, s0=1),
    _c(3, 32, 32, 33, shared=False, s0=5, layer=1),
    _c(2, 33, 33, 1, 36, s0=2),                                   # NaN row tails
    _c(1, 33, 31, 33, 64, shared=False, gap=8, layer=2),          # a whole NaN half-chunk is loaded; samples 8 floats apart
    _c(3, 1, 33, 33, 48, shared=False, s0=1000, layer=15),
    _c(3, 32, 1, 32, shared=False, gap=4, layer=1),
    _c(2, 31, 512, 1),                                            # 16 chunks: two trips of the wave loop, no split
    _c(3, 33, 512, 32, shared=False, s0=7, layer=3),
    _c(1, 1, 513, 1, s0=3),                                       # the smallest split: 2 x 1 x 1 workgroups
    _c(2, 32, 513, 33, 520, shared=False, s0=1, layer=1),         # split, per-sample, NaN tails
    _c(3, 33, 513, 33, s0=31),                                    # split, shared, every tile edge
]
KEEP = {True: 0.5, False: 0.8}


def fc_id(c):
    return 'S%d-%dx%dx%d-ldx%d-%s-s0_%d-site%d%s' % (c.S, c.B, c.I, c.O, c.ldx, 'shared' if c.shared else 'per_sample', c.s0, c.layer,
                                                      '-gap%d' % c.gap if c.gap else '')


def fc_splits(c):
    tiles = c.S * ((c.O + 31) // 32) * ((c.B + 31) // 32)
    return max(1, min(512 // tiles, (c.I + 511) // 512))


def fc_dispatch(c):
    kind = 'shared' if c.shared else 'per_sample'
    if fc_splits(c) > 1:
        return 'fc_fwd_dropout_kernel<%s, split> + fc_fwd_reduce_kernel' % kind
    return 'fc_fwd_dropout_kernel<%s>' % kind


def test_case_table_reaches_every_value_and_arm():
    """The table holds every size the kernel can go wrong at, and every arm (host arithmetic only)."""
    assert {c.B for c in FC_CASES} == {1, 31, 32, 33} and {c.O for c in FC_CASES} == {1, 32, 33}
    assert {c.I for c in FC_CASES} == {1, 31, 32, 33, 512, 513} and {c.S for c in FC_CASES} == {1, 2, 3}
    arms = {fc_dispatch(c) for c in FC_CASES}
    assert arms == {'fc_fwd_dropout_kernel<shared>', 'fc_fwd_dropout_kernel<per_sample>',
                    'fc_fwd_dropout_kernel<shared, split> + fc_fwd_reduce_kernel',
                    'fc_fwd_dropout_kernel<per_sample, split> + fc_fwd_reduce_kernel'}
    split = [c for c in FC_CASES if fc_splits(c) > 1]
    assert any(c.B == 1 and c.O == 1 and c.I == 513 for c in split) and not any(c.I <= 512 for c in split)
    assert any(c.s0 > 0 for c in FC_CASES) and any(c.ldx > c.I for c in FC_CASES) and any(c.ldx >= c.I + 16 for c in FC_CASES)
    assert any(c.gap for c in FC_CASES) and any(c.layer == 15 for c in FC_CASES)
    assert all(64 * c.I + 8 < 2 ** 24 and c.ldx % 4 == 0 and c.ldx >= c.I for c in FC_CASES)
    assert len({fc_id(c) for c in FC_CASES}) == len(FC_CASES)
    record_measured('uncertainty_kernel_tables', arms=sorted(arms))


def fc_windows(c):
    """Scattered window numbers on both sides of 2^31 (uint32 values; the kernel takes them as int32 bit patterns)."""
    w = (np.arange(c.B, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(2 ** 31 - 3 + c.B)) % np.uint64(2 ** 32)
    w[::3] = np.arange(c.B, dtype=np.uint64)[::3] * np.uint64(5) + np.uint64(1)            # small ones too
    return w.astype(np.int64)


def fc_inputs(c, exact):
    """(x [S' = 1 or S, B, ldx] with NaN tails, W [I, O], b [O]) in fp32 on the host."""
    rs = np.random.RandomState((zlib.crc32(fc_id(c).encode()) + (0 if exact else 1)) % (2 ** 31))
    ns = 1 if c.shared else c.S
    x = np.full((ns, c.B, c.ldx), np.nan, np.float32)
    x[:, :, :c.I] = rs.randint(-4, 5, (ns, c.B, c.I)) if exact else rs.randn(ns, c.B, c.I)
    if c.ldx > c.I:
        x[:, c.B // 2, c.I:] = np.inf
    if exact:
        W, b = (rs.randint(-8, 9, (c.I, c.O)) / 8.0).astype(np.float32), (rs.randint(-8, 9, c.O) / 8.0).astype(np.float32)
    else:
        W, b = (rs.randn(c.I, c.O) / np.sqrt(c.I)).astype(np.float32), (0.1 * rs.randn(c.O)).astype(np.float32)
    return x, W, b


def fc_masked(c, x, keep):
    """x~ [S, B, I] in float64: mask * x * float32(1 / keep), by the NumPy masks."""
    inv = np.float64(uncertainty.dropout_threshold(keep)[1])
    win = fc_windows(c)
    out = np.empty((c.S, c.B, c.I))
    for s in range(c.S):
        m = uncertainty.dropout_keep(SEED, c.s0 + s, c.layer, win, c.I, keep)
        out[s] = np.where(m, x[0 if c.shared else s, :, :c.I].astype(np.float64) * inv, 0.0)
    return out


def _x_device(c, x):
    """x on the device: [B, ldx], or S matrices c.B * c.ldx + c.gap floats apart (the gaps hold NaN)."""
    if c.shared:
        return _dev(x[0]), 0
    sx = c.B * c.ldx + c.gap
    flat = np.full((c.S, sx), np.nan, np.float32)
    flat[:, :c.B * c.ldx] = x.reshape(c.S, -1)
    return _dev(flat), sx


def _fc_dropout(lib, c, xd, sx, Wd, bd, wind, relu, keep, what, seed=SEED):
    y = Guarded(c.S * c.B, c.O)
    ns = fc_splits(c)
    nws = lib.chebgcn_fc_fwd_dropout_workspace(c.S, c.B, c.I, c.O)
    assert nws == (ns * c.S * c.B * c.O * 4 if ns > 1 else 0), (what, nws, ns)
    ws = Guarded(1, nws // 4) if nws else None
    T, inv = uncertainty.dropout_threshold(keep)
    _lib.check(lib.chebgcn_fc_fwd_dropout(_P(xd), c.ldx, sx, _P(Wd), _P(bd), _P(y.t), _P(ws.t) if ws else None, nws, _P(wind), c.S, c.B,
                                          c.I, c.O, relu, seed, c.s0, c.layer, T, float(inv), _stream()), 'fc_fwd_dropout')
    assert _lib.last_dispatch() == fc_dispatch(c), (what, _lib.last_dispatch())
    torch.cuda.synchronize()
    y.check(what + ' y')
    if ws:
        ws.check(what + ' workspace')
    return y.t.view(c.S, c.B, c.O)


@pytest.mark.parametrize('c', FC_CASES, ids=fc_id)
def test_fc_forward_dropout_vs_float64(lib, c):
    assert lib.chebgcn_fc_fwd_dropout_supported(c.S, c.B, c.I, c.O) == 1
    wind = torch.as_tensor(fc_windows(c).astype(np.uint32).view(np.int32)).to(DEV)
    ratios = {}
    for exact in (True, False):
        keep = KEEP[exact]
        x, W, b = fc_inputs(c, exact)
        xt = fc_masked(c, x, keep)
        assert 0 < (xt != 0).sum() or c.I * c.B * c.S < 8
        pre = xt @ W.astype(np.float64)                                                   # [S, B, O]
        bound = None if exact else (c.I + 3) * U * (np.abs(xt) @ np.abs(W.astype(np.float64)))
        (xd, sx), Wd, bd = _x_device(c, x), _dev(W), _dev(b)
        for bias, relu in ((1, 1), (0, 0)):
            what = 'fc_fwd_dropout %s %s%s%s' % (fc_id(c), 'exact' if exact else 'round-off', ' bias' if bias else '', ' relu' if relu else '')
            ref = pre + b.astype(np.float64) if bias else pre
            ref = np.maximum(ref, 0.0) if relu else ref
            got = _fc_dropout(lib, c, xd, sx, Wd, bd if bias else None, wind, relu, keep, what)
            if exact:
                assert_exact(what, got, ref)
                assert_same_bits(what, got, _fc_dropout(lib, c, xd, sx, Wd, bd if bias else None, wind, relu, keep, what))
            else:
                full = bound + (c.I + 3) * U * np.abs(b.astype(np.float64)) if bias else bound
                ratios['bias%d_relu%d' % (bias, relu)] = roundoff_ratio(what, got, ref, full)
                assert_same_bits(what, got, _fc_dropout(lib, c, xd, sx, Wd, bd if bias else None, wind, relu, keep, what))
    record_measured('fc_forward_dropout_vs_float64[%s]' % fc_id(c), arm=fc_dispatch(c), splits=fc_splits(c), **ratios)


@pytest.mark.parametrize('B,I,O,ldx', [(5, 37, 6, 40),             # no split, ragged tile, NaN row tails
                                       (8, 1100, 12, 1100),        # three splits, through fc_fwd_reduce_kernel
                                       (33, 64, 33, 64)])          # two tiles each way
def test_fc_forward_dropout_that_keeps_everything_is_fc_forward(lib, B, I, O, ldx):
    """One sample of a shared input with keep = 1 (inv_keep = 1, every draw below 2^32 - 1 kept) is chebgcn_fc_fwd bit for bit:
    the two kernels are one tile body, the same loads, guards, wave order and split reduction.  Round-off inputs, so the order
    of every sum shows in the last bits."""
    c = _c(1, B, I, O, ldx)
    win = fc_windows(c)
    T, inv = uncertainty.dropout_threshold(1.0)
    assert T == 2 ** 32 - 1 and inv == 1.0
    # a draw of exactly 2^32 - 1 would be dropped: a seed under which this case has none
    seed = next(s for s in range(SEED, SEED + 64) if uncertainty.dropout_keep(s, c.s0, c.layer, win, I, 1.0).all())
    x, W, b = fc_inputs(c, False)
    xd, Wd, bd = _dev(x[0]), _dev(W), _dev(b)
    wind = torch.as_tensor(win.astype(np.uint32).view(np.int32)).to(DEV)
    split = fc_splits(c) > 1
    assert fwd_dispatch(B, I, O) == ('fc_fwd_kernel<split> + fc_fwd_reduce_kernel' if split else 'fc_fwd_kernel')
    assert fc_dispatch(c) == ('fc_fwd_dropout_kernel<shared, split> + fc_fwd_reduce_kernel' if split else 'fc_fwd_dropout_kernel<shared>')
    for relu in (1, 0):
        what = 'fc_fwd_dropout keep 1 %s%s' % (fc_id(c), ' relu' if relu else '')
        plain = _fc_plain(lib, c, xd, Wd, bd, relu, what + ' (plain)')                      # (both assert their dispatch strings)
        drop = _fc_dropout(lib, c, xd, 0, Wd, bd, wind, relu, 1.0, what, seed=seed)
        assert bool(torch.isfinite(plain).all()) and bool((plain != 0).any())
        assert torch.equal(drop[0], plain), what + ': the dropout kernel with nothing dropped is not the plain kernel'


def test_fc_forward_dropout_refuses_unaligned_rows(lib):
    """A row stride that is no multiple of 4 floats, an x one float past a 16-byte boundary: CHEBGCN_EUNSUPPORTED, y untouched."""
    for ldx, offset in ((38, 0), (40, 1)):
        c = _c(2, 4, 37, 5, ldx)
        x, W, b = fc_inputs(c._replace(ldx=40), True)
        xd = _dev(x[0, :, :ldx], offset)
        wind = torch.zeros(c.B, dtype=torch.int32, device=DEV)
        y = Guarded(c.S * c.B, c.O, poison=SENTINEL)
        torch.cuda.synchronize()
        before = _lib.last_dispatch()
        rc = lib.chebgcn_fc_fwd_dropout(_P(xd), ldx, 0, _P(_dev(W)), _P(_dev(b)), _P(y.t), None, 0, _P(wind), c.S, c.B, c.I, c.O, 1, SEED,
                                        0, 0, 1 << 31, 2.0, _stream())
        assert rc == -4, (ldx, offset, rc)
        assert _lib.last_dispatch() == before
        torch.cuda.synchronize()
        assert y.untouched()


def test_ops_wrapper_pads_odd_rows_and_chains_sites(lib):
    """ops.fc_forward_dropout on a dense [B, 9] input (row stride 9: copied to rows of 12) and on its own [S, B, 6] output
    (row stride 6: copied), exact against the restatement; a wrong ``win`` is refused."""
    B, S, s0, keep = 5, 3, 2, 0.5
    rs = np.random.RandomState(3)
    x = rs.randint(-4, 5, (B, 9)).astype(np.float32)
    W1, b1 = (rs.randint(-8, 9, (9, 6)) / 8.0).astype(np.float32), (rs.randint(-8, 9, 6) / 8.0).astype(np.float32)
    W2, b2 = (rs.randint(-2, 3, (6, 4))).astype(np.float32), (rs.randint(-8, 9, 4) / 8.0).astype(np.float32)
    win = np.array([7, 0, 2 ** 31 + 1, 3, 2 ** 32 - 1], np.int64)
    wind = torch.as_tensor(win.astype(np.uint32).view(np.int32)).to(DEV)
    T, inv = uncertainty.dropout_threshold(keep)
    xd = torch.as_tensor(x).to(DEV)
    h = ops.fc_forward_dropout(xd, _dev(W1), _dev(b1), True, wind, S, s0, 0, SEED, T, inv)
    assert _lib.last_dispatch() == 'fc_fwd_dropout_kernel<shared>' and h.shape == (S, B, 6)
    z = ops.fc_forward_dropout(h, _dev(W2), _dev(b2), False, wind, S, s0, 1, SEED, T, inv)
    assert _lib.last_dispatch() == 'fc_fwd_dropout_kernel<per_sample>' and z.shape == (S, B, 4)
    href, zref = np.empty((S, B, 6)), np.empty((S, B, 4))
    for s in range(S):
        m0 = uncertainty.dropout_keep(SEED, s0 + s, 0, win, 9, keep)
        href[s] = np.maximum(np.where(m0, 2.0 * x, 0.0) @ W1.astype(np.float64) + b1, 0.0)
        m1 = uncertainty.dropout_keep(SEED, s0 + s, 1, win, 6, keep)
        zref[s] = np.where(m1, 2.0 * href[s], 0.0) @ W2.astype(np.float64) + b2
    assert_exact('ops.fc_forward_dropout site 0', h, href)
    assert_exact('ops.fc_forward_dropout site 1', z, zref)
    with pytest.raises(ValueError, match='win'):
        ops.fc_forward_dropout(xd, _dev(W1), _dev(b1), True, wind[:4], S, s0, 0, SEED, T, inv)
    with pytest.raises(ValueError, match='outside the range'):
        ops.fc_forward_dropout(torch.zeros((512, 8), device=DEV), torch.zeros((8, 512), device=DEV), torch.zeros(512, device=DEV), True,
                               torch.zeros(512, dtype=torch.int32, device=DEV), 5, 0, 0, SEED, T, inv)


# ------------------------------------------------------------------------------------------------------------ mc_reduce

def mc_logits(S, B, C):
    """Logits [S, B, C], multiples of 1/8 in [-3, 3], with planted rows: window 0 has two identical columns above all others
    (a tie of the mean probabilities that is exact by symmetry); with B > 1, window 3 is saturated at +-80, window 5 has its
    classes tied in every sample, window 7 holds one NaN.  Then the top class of a window whose top-2 gap of the float64 mean
    probabilities is neither 0 nor above 1e-3 is raised by 1 in every sample until every window is decided."""
    rs = np.random.RandomState(1000 * S + 10 * B + C)
    z = rs.randint(-24, 25, (S, B, C)) / 8.0
    if C >= 2:
        z[:, 0, C - 1] = z[:, 0, C // 2 - (C == 2)] = 4.0 + rs.randint(0, 8, S) / 8.0
    if B > 1:
        z[:, 3] = -80.0
        z[np.arange(S), 3, np.arange(S) % C] = 80.0
        z[:, 5] = 1.25
        z[S - 1, 7, C // 2] = np.nan
    nan = np.isnan(z).any(axis=(0, 2))
    for _ in range(8):
        p = uncertainty.mc_measures(z)['probabilities']
        if C < 2:
            break
        top = np.sort(np.where(np.isnan(p), 0.0, p), axis=1)[:, -2:]
        gap = top[:, 1] - top[:, 0]
        bad = ~nan & (gap != 0) & (gap <= 1e-3)
        if not bad.any():
            break
        for w in np.nonzero(bad)[0]:
            z[:, w, np.argmax(p[w])] += 1.0
    else:
        raise AssertionError('undecided windows remain')
    assert np.array_equal(z[~np.isnan(z)] * 8, np.round(z[~np.isnan(z)] * 8))
    return z.astype(np.float32), nan


def _guarded_int(n):
    whole = torch.full((n + 512,), -77, dtype=torch.int32, device=DEV)
    return whole, whole[256:256 + n]


@pytest.mark.parametrize('C', [1, 2, 22, 64])
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('S', [1, 2, 33])
def test_mc_reduce_vs_float64(lib, S, B, C):
    assert lib.chebgcn_mc_reduce_supported(S, C) == 1
    z, nan = mc_logits(S, B, C)
    want = uncertainty.mc_measures(z)
    zd = _dev(z)
    runs = []
    for _ in range(2):
        f = {k: Guarded(B, n) for k, n in (('probabilities', C), ('entropy', 1), ('expected_entropy', 1), ('mutual_information', 1),
                                           ('agreement', 1))}
        lw, lab = _guarded_int(B)
        vw, votes = _guarded_int(B * C)
        _lib.check(lib.chebgcn_mc_reduce(_P(zd), S, B, C, _P(f['probabilities'].t), _P(f['entropy'].t), _P(f['expected_entropy'].t),
                                         _P(f['mutual_information'].t), _P(lab), _P(votes), _P(f['agreement'].t), _stream()), 'mc_reduce')
        assert _lib.last_dispatch() == 'mc_reduce_kernel'
        torch.cuda.synchronize()
        for k, g in f.items():
            g.check('mc_reduce ' + k)
        for whole, n in ((lw, B), (vw, B * C)):
            assert bool((whole[:256] == -77).all()) and bool((whole[256 + n:] == -77).all()), 'mc_reduce: an int store left its buffer'
        out = {k: g.t.cpu().numpy().reshape(B, -1) for k, g in f.items()}
        out.update(labels=lab.cpu().numpy(), votes=votes.cpu().numpy().reshape(B, C))
        runs.append(out)
    got, again = runs
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), 'mc_reduce %s: two runs differ' % k
    # exact: votes, agreement, labels
    assert np.array_equal(got['votes'], want['votes']) and (got['votes'].sum(axis=1) == S).all()
    assert np.array_equal(got['agreement'][:, 0], (want['votes'][np.arange(B), want['labels']] / np.float32(S)).astype(np.float32))
    assert np.array_equal(got['labels'], want['labels']), (got['labels'], want['labels'])
    if C >= 2:
        assert got['labels'][0] == min(C - 1, C // 2 - (C == 2)), 'the tie of two identical columns goes to the first'
    # within the parity bound: the mean probabilities and the entropies; NaN exactly where the logits hold one
    tol = 1e-5 * max(1.0, np.log(C))
    errs = {}
    for k, t in (('probabilities', 1e-5), ('entropy', tol), ('expected_entropy', tol), ('mutual_information', tol)):
        g, w = got[k].reshape(B, -1).astype(np.float64), np.asarray(want[k]).reshape(B, -1)
        assert np.array_equal(np.isnan(g).any(axis=1), nan) and np.array_equal(np.isnan(w).any(axis=1), nan), k
        errs[k] = float(np.abs(g[~nan] - w[~nan]).max()) if (~nan).any() else 0.0
        print('mc_reduce S%d B%d C%d %s: max err %.3e (bound %.1e)' % (S, B, C, k, errs[k], t))
        assert errs[k] <= t, (k, errs[k], t)
    ok = ~nan
    assert (got['entropy'][ok] >= 0).all() and (got['mutual_information'][ok] >= 0).all()
    if S == 1:
        assert (got['agreement'][ok, 0] == 1).all()             # (the NaN window votes for its NaN's class, its label is class 0)
    if B > 1:
        assert got['entropy'][3, 0] < 1e-30 + (np.log(min(S, C)) + 1e-5 if S > 1 else 0) and got['expected_entropy'][3, 0] == 0.0
    record_measured('mc_reduce_vs_float64[S%d-B%d-C%d]' % (S, B, C), **errs)


def test_ops_mc_reduce_refuses_large_sizes(lib):
    with pytest.raises(ValueError, match='mc_reduce'):
        ops.mc_reduce(torch.zeros((1025, 1, 2), device=DEV))
    with pytest.raises(ValueError, match='mc_reduce'):
        ops.mc_reduce(torch.zeros((2, 1, 65), device=DEV))
    out = ops.mc_reduce(torch.zeros((2, 3, 4), device=DEV))
    assert out['labels'].tolist() == [0, 0, 0] and out['votes'].tolist() == [[2, 0, 0, 0]] * 3
    assert np.allclose(out['entropy'].cpu().numpy(), np.log(4), atol=1e-6)
