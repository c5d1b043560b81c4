"""Parcellation, the parts that need no device: the bookkeeping of ``Parcellation``, every refusal, the float32 NumPy twin
``reduce_host`` against a float64 restatement of the reference (``model.py:47-53``: sorted unique positive labels, then
``np.mean(x[:, ind], axis=1)`` per label; weighted: ``np.average``), ``expand``, and the C entry points' presence and argument
checks.  ``ref64`` / ``bound`` / ``make_labels`` / ``make_series`` are what tests/test_gpu_parcellation.py compares against.

The bound is derived, not measured: a region of n members summed sequentially in float32 (one rounded product per weighted
term, n - 1 rounded adds, one rounded division, unit roundoff 2^-24) is within  (n + 2) * 2^-24 * sum|w x| / sum w  of the exact
mean; any other fixed order is tighter.  SUM mode is the numerator alone: (n + 2) * 2^-24 * sum|w x|."""
import numpy as np
import pytest

from gcn_fmri_decoding_amd import Parcellation, _lib, parcellation

U = 2.0 ** -24


def ref64(labels, x, weights=None, mode='mean'):
    """The reference's reduction in float64, per label."""
    labels = np.asarray(labels).reshape(-1)
    x = np.asarray(x, np.float32).astype(np.float64)
    cols = []
    for i in [i for i in np.unique(labels) if i > 0]:
        ind = np.nonzero(labels == i)[0]
        if weights is None:
            cols.append(np.mean(x[:, ind], axis=1) if mode == 'mean' else np.sum(x[:, ind], axis=1))
        else:
            w = np.asarray(weights, np.float32).astype(np.float64)[ind]
            s = (x[:, ind] * w).sum(axis=1)
            cols.append(s / w.sum() if mode == 'mean' else s)
    return np.stack(cols, axis=1)


def bound(labels, x, weights=None, mode='mean'):
    """[T, R] float64: (n + 2) 2^-24 sum|w x| / sum w  (SUM: without the denominator)."""
    labels = np.asarray(labels).reshape(-1)
    x = np.abs(np.asarray(x, np.float32).astype(np.float64))
    cols = []
    for i in [i for i in np.unique(labels) if i > 0]:
        ind = np.nonzero(labels == i)[0]
        w = np.ones(len(ind)) if weights is None else np.asarray(weights, np.float32).astype(np.float64)[ind]
        s = (x[:, ind] * w).sum(axis=1)
        cols.append((len(ind) + 2) * U * (s / w.sum() if mode == 'mean' else s))
    return np.stack(cols, axis=1)


def make_labels(V, R, chunk, seed=0):
    """Labels over V vertices with R regions (ids with gaps, compacted by Parcellation) built to reach the kernel's edges:
    background at both ends of V (from V >= 8), region A with a member on either side of EVERY chunk boundary and, where V
    allows, more than half of V; region B wholly inside one chunk; single-vertex regions; everything else scattered."""
    rs = np.random.RandomState(seed * 1000003 + V * 31 + R)
    R = min(R, V)
    ids = np.sort(rs.choice(np.arange(1, 3 * R + 5), size=R, replace=False))
    lab = np.zeros(V, np.int64)
    lo, hi = (2, V - 3) if V >= R + 8 else (0, V)               # background [0, 2) and [V - 3, V)
    free = np.arange(lo, hi)
    rs.shuffle(free)
    lab[free[:R]] = ids                                         # every region has a member
    rest = free[R:]
    if R == 1:
        lab[rest] = ids[0]
        return lab
    nbig = V // 2 if len(rest) >= V // 2 else len(rest) // 3     # region A: with its first member, more than half of V
    lab[rest[:nbig]] = ids[0]
    rest = rest[nbig:]
    singles = max(1, R // 8) if R >= 3 else 0                   # the last `singles` regions keep their single vertex
    middle = ids[1:R - singles]
    lab[rest] = middle[rs.randint(0, len(middle), size=len(rest))] if len(middle) else ids[0]
    for b in range(chunk, V, chunk):                            # A has a member on either side of every chunk boundary
        for v in (b - 1, b):
            if lo <= v < hi and (lab == lab[v]).sum() > 1:
                lab[v] = ids[0]
    if len(middle):                                             # region B: wholly inside the chunk of its first member
        home = int(free[1]) // chunk
        away = np.nonzero((lab == ids[1]) & (np.arange(V) // chunk != home))[0]
        lab[away] = ids[0]
    assert len(np.unique(lab[lab > 0])) == R
    return lab


def make_series(T, V, seed=0):
    """Mixed sign and magnitude: a normal plus a per-vertex offset of up to +-100, so that a wrong member moves a mean by far
    more than the bound."""
    rs = np.random.RandomState(seed * 7919 + T * 13 + V)
    return (rs.randn(T, V) + 100.0 * rs.uniform(-1, 1, size=V)[None, :]).astype(np.float32)


def make_weights(labels, seed=0):
    rs = np.random.RandomState(seed + 17)
    w = rs.uniform(0.05, 3.0, size=len(labels)).astype(np.float32)
    w[::7] = 0.0                                                # zero weights are allowed ...
    for i in np.unique(labels[labels > 0]):                     # ... as long as a region keeps a positive sum
        ind = np.nonzero(labels == i)[0]
        if w[ind].sum() == 0:
            w[ind[0]] = 1.0
    return w


def test_bookkeeping_gaps_background_and_shapes():
    lab = np.array([0, 7, 7, -3, 2, 0, 900, 2, 7, -1])
    P = Parcellation(lab)
    assert (P.V, P.R) == (10, 3)
    assert np.array_equal(P.regions, [2, 7, 900]) and np.array_equal(P.counts, [2, 3, 1])
    assert P.region_of.dtype == np.int32 and np.array_equal(P.region_of, [-1, 1, 1, -1, 0, -1, 2, 0, 1, -1])
    assert np.array_equal(P.ptr, [0, 2, 5, 6]) and np.array_equal(P.idx, [4, 7, 1, 2, 8, 6])
    assert P.regions.tolist() == [i for i in np.unique(lab) if i > 0]         # the reference's RegionLabels
    P2 = Parcellation(lab[None, :].astype(np.int16))                          # [1, V], as nibabel gives
    assert np.array_equal(P2.region_of, P.region_of) and P2.V == 10
    P1 = Parcellation(np.full(5, 4))                                          # R = 1, no background
    assert (P1.R, P1.counts.tolist(), P1.region_of.tolist()) == (1, [5], [0] * 5)
    Ps = Parcellation([3])                                                    # V = 1: a single-vertex region
    assert (Ps.V, Ps.R, Ps.counts.tolist()) == (1, 1, [1])
    x = make_series(4, 10)
    assert np.array_equal(Ps.reduce_host(x[:, :1]), x[:, :1])


def test_value_errors_without_a_device(monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(torch.cuda, 'current_device', boom)
    monkeypatch.setattr(torch.Tensor, 'to', boom)
    lab = np.array([1, 1, 2, 0, 2, 3])
    for bad in (lab.astype(np.float32), lab > 1, np.zeros(6, np.int64), -lab, lab.reshape(2, 3), np.zeros((0,), np.int64),
                np.arange(1, 65537 + 1)):
        with pytest.raises(ValueError):
            Parcellation(bad)
    Parcellation(np.arange(1, 65536))                                         # R = 65535 is served
    for w in (np.ones(5), np.ones((6, 1)), [1, 1, 1, np.nan, 1, 1], [1, 1, 1, 1, np.inf, 1], [1, -1, 1, 1, 1, 1],
              [0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 0]):
        with pytest.raises(ValueError):
            Parcellation(lab, weights=w)
    Parcellation(lab, weights=[1, 0, 1, 0, 1, 1])                             # zero on the background or on part of a region
    P = Parcellation(lab)
    x = np.zeros((3, 6), np.float32)
    for call in (P.reduce, P.reduce_host):
        with pytest.raises(ValueError):
            call(x, mode='median')
        with pytest.raises(ValueError):
            call(x[:, :5])
        with pytest.raises(ValueError):
            call(x[0])
        with pytest.raises(ValueError):
            call([])
        with pytest.raises(ValueError):
            call([x, 'run'])
    with pytest.raises(ValueError):
        P.reduce(x, chunk_rows=0)
    with pytest.raises(ValueError):
        P.expand(np.zeros(4))
    with pytest.raises(ValueError):
        P.expand(np.zeros((2, 2, 3)))


CASES = [(1, 1, 3), (63, 5, 4), (700, 40, 9), (1500, 1, 2), (1500, 360, 3), (2100, 65, 5)]


@pytest.mark.parametrize('V,R,T', CASES)
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('mode', ['mean', 'sum'])
def test_reduce_host_within_the_bound_of_float64(V, R, T, weighted, mode):
    lab = make_labels(V, R, chunk=512)
    w = make_weights(lab) if weighted else None
    P = Parcellation(lab, weights=w)
    x = make_series(T, V)
    got = P.reduce_host(x, mode=mode)
    assert got.dtype == np.float32 and got.shape == (T, P.R)
    want, b = ref64(lab, x, w, mode), bound(lab, x, w, mode)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= b).all(), (err / np.maximum(b, 1e-300)).max()
    # any numeric dtype, tensors, lists
    assert np.array_equal(P.reduce_host(x.astype(np.float64), mode=mode), got)
    import torch
    outs = P.reduce_host([torch.as_tensor(x), x[:1]], mode=mode)
    assert isinstance(outs, list) and np.array_equal(outs[0], got) and np.array_equal(outs[1], got[:1])


def test_sequential_order_is_the_stated_one():
    """The twin against a scalar loop that states the order literally: acc = 0; acc = fl(acc + fl(w x)) member by member."""
    lab = make_labels(300, 7, chunk=64)
    w = make_weights(lab)
    x = make_series(3, 300)
    for weights in (None, w):
        P = Parcellation(lab, weights=weights)
        want = np.zeros((3, P.R), np.float32)
        for r in range(P.R):
            for t in range(3):
                acc, den = np.float32(0), np.float32(0)
                for v in P.idx[P.ptr[r]:P.ptr[r + 1]]:
                    acc = np.float32(acc + (x[t, v] if weights is None else np.float32(weights[v] * x[t, v])))
                    den = np.float32(den + (np.float32(1) if weights is None else weights[v]))
                want[t, r] = np.float32(acc / den)
        assert np.array_equal(P.reduce_host(x), want)


def test_a_swapped_pair_moves_a_mean_by_more_than_the_bound():
    V, T = 2100, 4
    lab = make_labels(V, 65, chunk=512)
    P = Parcellation(lab)
    x = make_series(T, V)
    a = int(P.idx[P.ptr[0]])                                    # a member of the largest region (the hardest to move)
    others = np.nonzero((lab > 0) & (lab != lab[a]))[0]
    b = int(others[np.argmax(np.abs(x[0, others] - x[0, a]))])
    y = x.copy()
    y[:, [a, b]] = y[:, [b, a]]
    moved = np.abs(P.reduce_host(y).astype(np.float64) - P.reduce_host(x))
    bd = bound(lab, x)
    for r in (P.region_of[a], P.region_of[b]):
        assert (moved[:, r] > 4 * bd[:, r]).all(), (moved[:, r], bd[:, r])


def test_expand_is_constant_inside_regions_and_fill_outside():
    lab = make_labels(700, 40, chunk=512)
    P = Parcellation(lab)
    red = P.reduce_host(make_series(5, 700))
    for fill in (0.0, -7.5, np.nan):
        out = P.expand(red, fill=fill)
        assert out.dtype == np.float32 and out.shape == (5, 700)
        for r in range(P.R):
            assert np.array_equal(out[:, P.region_of == r], np.repeat(red[:, r:r + 1], P.counts[r], axis=1))
        bg = out[:, P.region_of < 0]
        assert bg.size and (np.isnan(bg).all() if np.isnan(fill) else (bg == np.float32(fill)).all())
    assert np.array_equal(P.expand(red[2]), P.expand(red)[2]) and P.expand(red[2]).shape == (700,)
    import torch
    t = P.expand(torch.as_tensor(red))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), P.expand(red))


def test_abi_symbols_and_geometry():
    lib = _lib.lib()
    for name in ('chebgcn_parcellate', 'chebgcn_parcel_expand', 'chebgcn_parcellate_query'):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert (_lib.PARCEL_MEAN, _lib.PARCEL_SUM) == (0, 1) and parcellation.MODES == ('mean', 'sum')
    from gcn_fmri_decoding_amd import ops
    g = ops.parcellate_geometry()
    assert g['tile'] % (4 * g['rows']) == 0 and g['rows'] > 1 and g['wide_T'] >= g['rows'] and g['regions_per_pass'] >= 64
    assert all(v > 0 for v in g.values()) and lib.chebgcn_parcellate_query(99) == -1


ONE = 16        # any non-NULL value: a refused call dereferences nothing


@pytest.mark.parametrize('args', [
    dict(x=None), dict(ptr=None), dict(idx=None), dict(out=None), dict(T=0), dict(V=0), dict(R=0), dict(ldx=99), dict(ldo=9),
    dict(R=65536, ldo=70000), dict(mode=2), dict(mode=-1), dict(nnz=101), dict(x=ONE + 2)])
def test_parcellate_refuses_arguments_before_any_launch(args):
    a = dict(x=ONE, ldx=100, ptr=ONE, idx=ONE, nnz=50, w=None, out=ONE, ldo=10, T=5, V=100, R=10, mode=0)
    a.update(args)
    lib = _lib.lib()
    rc = lib.chebgcn_parcellate(a['x'], a['ldx'], a['ptr'], a['idx'], a['nnz'], a['w'], a['out'], a['ldo'], a['T'], a['V'], a['R'],
                                a['mode'], None)
    assert rc == -1, (rc, lib.chebgcn_last_error())
    assert b'parcellate' in lib.chebgcn_last_error()


@pytest.mark.parametrize('args', [dict(maps=None), dict(region_of=None), dict(out=None), dict(B=0), dict(R=0), dict(V=0),
                                  dict(R=65536), dict(region_of=ONE + 4)])
def test_parcel_expand_refuses_arguments_before_any_launch(args):
    a = dict(maps=ONE, region_of=ONE, out=ONE, B=2, R=10, V=100)
    a.update(args)
    lib = _lib.lib()
    rc = lib.chebgcn_parcel_expand(a['maps'], a['region_of'], a['out'], a['B'], a['R'], a['V'], 0.0, None)
    assert rc == -1, (rc, lib.chebgcn_last_error())
    assert b'parcel_expand' in lib.chebgcn_last_error()
