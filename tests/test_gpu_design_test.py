"""``chebgcn_perm_glm_t`` against its NumPy restatement ``stats.perm_t_host`` at the edges of the kernel (bit for bit), and
``stats.design_test`` on the device against ``stats.design_test_host`` (exact in every field).  Shapes come from
``ops.perm_glm_geometry()`` and ``ops.cluster_geometry()``."""
import ctypes

import numpy as np
import pytest

import map_test_cases as cases
from gcn_fmri_decoding_amd import _lib, stats

pytestmark = pytest.mark.gpu

KERNEL = 'perm_glm_t_kernel<'


def assert_same(a, b):
    assert type(a) is type(b) and a._fields == b._fields
    for name, u, v in zip(a._fields, a, b):
        if isinstance(u, np.ndarray):
            assert u.dtype == v.dtype and u.shape == v.shape, name
            assert np.array_equal(u, v), '%s differs at %d places' % (name, int((u != v).sum()))
        else:
            assert u == v, name


def both(x, A, D, c, **kw):
    """Device result (twice: identical) against the host twin; every t launch is the new kernel's."""
    _lib.dispatch_log = log = []
    try:
        dev = stats.design_test(x, A, D, c, **kw)
    finally:
        _lib.dispatch_log = None
    took = [d for what, d in log if what == 'perm_glm_t']
    assert took and all(d.startswith(KERNEL) for d in took), took
    assert not [d for what, d in log if what == 'signflip_t' or 'signflip' in d]
    assert len(took) + sum(what == 'cluster_enhance' for what, d in log) == len(log)
    assert_same(dev, stats.design_test(x, A, D, c, **kw))
    assert_same(dev, stats.design_test_host(x.cpu().numpy() if hasattr(x, 'cpu') else x, A, D, c, **kw))
    assert dev.exact is False
    return dev


def kernel_case(S, r, M, P, flips, seed):
    """Inputs of the stated arithmetic: an orthonormal Uf whose first column is constant, any u, e with a vertex of zeros
    (vertex 0) and one that is constant across subjects, hence inside the span of Uf (vertex 1), where M allows."""
    rs = np.random.RandomState(seed)
    Uf = np.ascontiguousarray(np.linalg.qr(np.column_stack([np.ones(S), rs.randn(S, r - 1)]))[0])
    u = rs.randn(r)
    e = rs.randn(S, M).astype(np.float32)
    if M >= 3:
        e[:, 0] = 0.0
        e[:, 1] = 0.75
    ed = e.astype(np.float64)
    q = np.zeros(M)
    for j in range(S):
        q = q + ed[j] * ed[j]
    return e, q, Uf, u, 0.3 + rs.rand(), S - r, stats.permutations(S, P, seed, flips=flips)


def on_device(e, q, Uf, u, unorm2, dof, rows):
    import torch
    from gcn_fmri_decoding_amd import ops
    dev = torch.device('cuda')
    t = ops.perm_glm_t(*(torch.as_tensor(a).to(dev) for a in (e, q, Uf, u)), unorm2, dof,
                       torch.as_tensor(np.ascontiguousarray(rows).view(np.int32)).to(dev))
    assert _lib.last_dispatch().startswith(KERNEL)
    return t.cpu().numpy()


@pytest.mark.parametrize('r', [1, 2, 16, 17, 33])
def test_kernel_at_its_edges(r):
    """Every vertex tail, subject count, permutation tail and panel count of the kernel against the stated arithmetic."""
    from gcn_fmri_decoding_amd import ops
    geo = ops.perm_glm_geometry(r)
    VB, PT = geo['vertices'], geo['perms']
    assert VB >= 2 and PT >= 2 and geo['panel'] == 16
    n = 0
    for S in (r + 1, 37):
        for M in (1, 63, VB - 1, VB, VB + 1):
            for flips in (False, True):
                args = kernel_case(S, r, M, 2 * PT + 3, flips, seed=S + M)
                want = stats.perm_t_host(*args)
                for Pb in (1, PT - 1, PT, PT + 1, 2 * PT + 3):
                    got = on_device(*args[:6], args[6][:Pb])
                    assert got.dtype == np.float32 and got.shape == (Pb, M)
                    assert np.array_equal(got, want[:Pb]), (S, M, flips, Pb, int((got != want[:Pb]).sum()))
                    n += 1
                if M >= 3:
                    assert (want[:, 0] == 0).all()                  # constant (zero) across subjects: t = 0
                    if not flips:
                        assert (want[:, 1] == 0).all()              # inside the span of the design: rss under the floor, t = 0
                    assert (want[:, 2:] != 0).any()
    assert n == 100


def test_batches_and_a_table_that_starts_later():
    """Permutations [0, 11) in one call, in calls of 1, 4 and 6, and as rows [5, 11) of the table alone: the same bits."""
    args = kernel_case(23, 5, 300, 11, True, seed=3)
    whole = on_device(*args)
    assert np.array_equal(whole, stats.perm_t_host(*args))
    rows = args[6]
    parts = [on_device(*args[:6], rows[a:b]) for a, b in ((0, 1), (1, 5), (5, 11))]
    assert np.array_equal(np.concatenate(parts), whole)
    e2 = np.ascontiguousarray(args[0][:, :77])                      # ... and whatever M holds
    assert np.array_equal(on_device(e2, args[1][:77].copy(), *args[2:]), whole[:, :77])


def test_a_row_number_beyond_the_design_is_clamped():
    args = kernel_case(9, 3, 130, 6, False, seed=1)
    rows = args[6].copy()
    rows[2, 4] = np.uint32(9)
    rows[3, 0] = np.uint32(0x7FFFFFFF)
    rows[5, 8] = np.uint32(0x80000000 | 4000)
    got = on_device(*args[:6], rows)
    assert np.array_equal(got, stats.perm_t_host(*args[:6], rows))
    assert np.array_equal(got[:2], stats.perm_t_host(*args)[:2])


def group_design(S):
    g = (np.arange(S) % 2).astype(np.float64)
    return np.stack([g, 1 - g], 1), [1.0, -1.0]


@pytest.mark.parametrize('stat', ['max', 'extent', 'tfce'])
@pytest.mark.parametrize('tail', [1, -1, 0])
def test_every_statistic_and_tail(stat, tail):
    M, S = 63, 11
    A = cases.random_graph(M, 3, M)
    x = cases.smooth_maps(S, M, seed=7, A=A)
    D, c = group_design(S)
    x[::2, :M // 2] += 0.7
    kw = {'threshold': 0.8} if stat == 'extent' else {}
    res = both(x, A, D, c, stat=stat, tail=tail, n_perm=30, seed=5, **kw)
    assert res.n_perm == 30 and res.dof == S - 2 and res.p.min() >= 1 / 30
    assert (res.labels is not None) == (stat == 'extent')


def test_streamed_arm():
    from gcn_fmri_decoding_amd import ops
    M = ops.cluster_geometry()['onchip_M'] + 1
    S = 8
    A = cases.random_graph(M, 3, 1)
    x = cases.smooth_maps(S, M, seed=2, A=A)
    D = np.column_stack([np.ones(S), np.linspace(-1, 1, S), np.cos(np.arange(S))])
    _lib.dispatch_log = log = []
    try:
        stats.design_test(x, A, D, [0, 1, 0], stat='tfce', tail=1, n_perm=5, step=0.35, seed=1)
    finally:
        _lib.dispatch_log = None
    assert all(d.startswith('cluster_prep_kernel') for what, d in log if what == 'cluster_enhance')
    res = both(x, A, D, [0, 1, 0], stat='tfce', tail=1, n_perm=5, step=0.35, seed=1)
    assert res.dof == S - 3 and res.stat.max() > 0


def test_blocks_flips_and_classes():
    import torch
    M, S = 63, 12
    A = cases.random_graph(M, 3, 9)
    pair = np.repeat(np.arange(6), 2)
    cond = np.tile([1.0, -1.0], 6)
    D = np.column_stack([cond, (pair[:, None] == np.arange(6)[None, :]).astype(float)])
    c = [1.0] + [0.0] * 6
    x = cases.smooth_maps(S, M, seed=3, A=A)
    x[::2, :20] += 0.6
    res = both(x, A, D, c, stat='tfce', tail=0, n_perm=30, blocks=pair, seed=2)
    assert res.dof == S - 7                                          # the condition and six subject columns
    both(x, A, D, c, stat='tfce', tail=0, n_perm=30, blocks=pair, flips=True, seed=2)
    ones = both(x, A, np.ones((S, 1)), [1.0], stat='max', tail=1, n_perm=30, flips=True, seed=2)
    assert ones.dof == S - 1
    xs = np.stack([x, cases.smooth_maps(S, M, seed=4, A=A)], 1)      # [S, 2, M]: the classes share the table
    D2, c2 = group_design(S)
    two = both(xs, A, D2, c2, stat='tfce', tail=1, n_perm=30, seed=6)
    assert two.t.shape == (2, M) and two.null.shape == (2, 30) and two.step.shape == (2,)
    for k in range(2):
        one = stats.design_test(xs[:, k], A, D2, c2, stat='tfce', tail=1, n_perm=30, seed=6)
        assert np.array_equal(one.stat, two.stat[k]) and np.array_equal(one.null, two.null[k]) and np.array_equal(one.p, two.p[k])
    assert_same(two, both(torch.as_tensor(xs).cuda(), A, D2, c2, stat='tfce', tail=1, n_perm=30, seed=6))


def test_sizes_beyond_the_limits_are_refused_before_any_launch():
    """By argument only: the entry answers CHEBGCN_EUNSUPPORTED (-4) or CHEBGCN_EINVAL (-1) and enqueues nothing."""
    import torch
    from gcn_fmri_decoding_amd import ops
    geo = ops.perm_glm_geometry()
    assert geo == dict(geo, max_r=64, max_S=4096, max_M=1 << 24, max_perms=65535)
    assert [ops.perm_glm_geometry(r)['perms'] <= geo['perms'] for r in (1, 4, 5, 64)] == [True] * 4
    lib = _lib.lib()
    assert lib.chebgcn_perm_glm_query(99) == -1 and lib.chebgcn_perm_glm_query(100) == -1 and lib.chebgcn_perm_glm_query(165) == -1
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = ctypes.c_void_p(buf.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(S=8, M=8, r=2, Pb=1, e=p, q=p, Uf=p, u=p, rows=p, t=p, unorm2=1.0, dof=None):
        return lib.chebgcn_perm_glm_t(e, q, Uf, u, unorm2, S - r if dof is None else dof, rows, t, S, M, r, Pb, stream)
    assert call(S=geo['max_S'] + 1) == -4
    assert call(M=geo['max_M'] + 1) == -4
    assert call(Pb=geo['max_perms'] + 1) == -4
    assert call(S=100, r=geo['max_r'] + 1) == -4
    assert b'served' in lib.chebgcn_last_error()
    for name in ('e', 'q', 'Uf', 'u', 'rows', 't'):
        assert call(**{name: None}) == -1, name
    odd4, odd2 = ctypes.c_void_p(buf.data_ptr() + 4), ctypes.c_void_p(buf.data_ptr() + 2)
    for name in ('q', 'Uf', 'u'):
        assert call(**{name: odd4}) == -1, name
    for name in ('e', 'rows', 't'):
        assert call(**{name: odd2}) == -1, name
    assert b'unaligned' in lib.chebgcn_last_error()
    assert call(S=4, r=4) == -1 and call(dof=0) == -1 and call(unorm2=0.0) == -1 and call(Pb=0) == -1 and call(r=0) == -1
    torch.cuda.synchronize()
    assert (buf == 0).all()
    with pytest.raises(_lib.ChebgcnError):
        ops.perm_glm_t(buf[:16].float().reshape(4, 4), buf[:4], buf[:8].reshape(4, 2), buf[:2], 1.0, 2,
                       torch.zeros((3, 5), dtype=torch.int32, device='cuda'))
