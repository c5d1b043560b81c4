"""The Chebyshev recurrence kernels on operators with rows of 21 ... 140 entries, BY NAME, against float64.  The GPU part needs an
MI355X (``-m gpu``); the two host tests at the top run anywhere (``bank_order`` needs the library, not a device).

Every recurrence kernel gathers a row of L~ in record classes: 8 entries always, a third quad for 9-10 (its ids ride in the value
record) and 11-12 entries, and beyond 12 a loop over the variable-stride image (csrc/recurrence.hip ``len > 4*QMAX``,
csrc/recurrence4.hip ``mC``, csrc/recurrence_ord_kernel.h ``mC`` / ``mC_hi``).  The graphs of the other GPU tests (cube kNN with
k <= 8, five random neighbours) have rows of at most 18 entries: that loop never took more than two turns, no wave ever had all its
slots long, and slots 32..39 of the ordered kernels (the shortest rows of a sorted graph) never had a bit set.  A kNN connectivity
graph with k = 32 (``graph.connectivity_graph``) has 33 ... 56 entries in EVERY row; that is also where the fused atlas layer
declines (rows beyond 20 entries) and these kernels take over.

Three seeded operator families (host, below):

* ``hubs(n_active, n_iso, seed)``   five random neighbours per vertex, symmetrised, plus nine hub vertices with 21 ... 130 extra
                                     neighbours (a few long rows at the sorted front), then isolated vertices; normalised Laplacian
* ``dense(n_active, n_iso, seed, deg)``   ``deg`` random neighbours per vertex: every active row longer than 12 entries
                                     (deg = 32: rows of 45 ... 82; deg = 13 for the large sizes: 13 ... ~45)
* ``directed(n, seed, transposed)``  NON-symmetric L = A + I (L~ = A): the first 160 rows have exactly 0, 1, 7, 8, 9, 10, 11, 12, 13,
                                     16, 17, 20, 21, 24, 25, 32, 33, 64, 65, 130 entries (cycling), the rest 3 ... 11; rows scaled to
                                     abs-sum 1, then columns to abs-sum <= 1 (so ||A||_2 <= 1); forward and adjoint images have
                                     different profiles, and there are vertices with an empty row and a non-empty column, the
                                     reverse, and neither.

Kernel families covered (``CASES``; each template asserted through ``chebgcn_last_dispatch()``, taken from the dispatch rule of
csrc/recurrence.hip ``dispatch_onchip``, csrc/recurrence4.hip ``shape4``, csrc/recurrence_ord.hip ``ordered_shape``):

* ``cheb_onchip_kernel<4,..,256,*>``        hubs / dense / directed / directed^T at M = 360, hubs and dense near 2000
* ``cheb_onchip_kernel<2,..>`` (planes = 2)  256 threads (M = 360), 512 threads (M = 2070), 768 threads (M = 4160)
* ``cheb4_kernel`` (planes = 4)              10 rows per thread (2600 active) and 20 (6000 active), isolated vertices in registers
                                             (``ISOREG`` true) and not (2100 isolated vertices), directed at 2600
* ``cheb_ord_kernel<..,256,false>``          1500 active vertices in ``length_order`` (adjoint: the on-chip kernel)
* ``cheb_ord_kernel<..,512,*>``              2600 active; once with 3600 isolated vertices (``+ cheb_ord_tail_kernel``)
* ``cheb_ord2_kernel``                       11000 active (hubs); 16500 active with deg = 13 (NG = 9: slots 32..35 exist and are long)
* ``cheb_step_global_kernel``                M = 21000 (no LDS image), hubs

Every case: 14 planes for four-plane kernels, 15 for two-plane ones (a partial last group); K = 5, and K = 2 once per family; x
and G non-zero at isolated vertices, pads NaN, outputs pre-filled with NaN; EVERY plane of every order of the stack and every
plane of dx against the float64 recurrence and Clenshaw adjoint (``torch.sparse`` on the device, L~ and L~^T from the CSR the
library was given; tied to SciPy on the host on three planes at 1e-12); in place == copying forward bit for bit; a second call
bit-identical.  Then the atlas case end to end: ``connectivity_graph`` (M = 360, k = 32) -> ``adjacency`` -> ``laplacian``, every row
beyond 20 entries, the fused layer declines, one layer (``ops.cheb_conv``) and a two-layer cgcnn against oracle/layers_ref.py in
float64, the dispatch log naming the recurrence kernel of M = 360 and no ``fused_layer_*`` kernel.

Bounds -- the project's own, PER PLANE: ``REL = 1e-5`` of the plane's maximum for the stack, ``GREL = 2e-5`` for dx.  Not tuned to
these kernels: the same recurrences in NumPy fp32 against float64 (K = 5, 15 planes, on the host: ``_fp32_host_errors`` below, the
families at M = 360 / 1040 / 2660, directed and its transpose at 360 / 2600) give worst-plane errors of

    family      forward (fp32 vs float64)    Clenshaw adjoint (fp32 vs float64)
    hubs        1.7e-7 ... 3.0e-7            1.0e-7 ... 2.4e-7
    dense       3.0e-7 ... 3.7e-7            0.9e-7 ... 1.1e-7
    directed    1.4e-7 ... 2.7e-7            1.1e-7 ... 1.4e-7

which leaves a factor above 25 (forward, 1e-5 / 3.7e-7) and above 80 (adjoint, 2e-5 / 2.4e-7) for the kernels' other summation
order.  The network bounds are those of test_gpu_finetune.py: logits 1e-5, gradients 2e-4 of their largest element.

Measured on the MI355X (profiles/r08_long_rows_measured.jsonl, 31 kernel cases): every case within 4.3e-7 (stack; the largest at
``cheb_ord_kernel<4112,2,2,512,false>`` on dense rows of 45 ... 82) and 1.7e-7 (dx; ``cheb_onchip_kernel<2,2,1,256,true>`` on the
directed operator) -- the size of the fp32 host figures above; longest row 141 entries.  Atlas layer: out 1.3e-7, dx 1.7e-7, dW
1.3e-7, dbias 5.7e-8; two-layer cgcnn: logits 3.5e-7, gradients at most 3.1e-7.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import record_measured

REL, GREL = 1e-5, 2e-5
gpu = pytest.mark.gpu

HUB_EXTRA = (21, 24, 25, 32, 33, 48, 64, 65, 130)
DIRECTED_LENGTHS = (0, 1, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 24, 25, 32, 33, 64, 65, 130)
# directed: vertices no row points at (an empty COLUMN): row 3 has 8 entries, row 20 none (isolated), the last row 3 ... 11
DIRECTED_NO_COLUMN = lambda n: (3, 20, n - 1)


# ------------------------------------------------------------------------------------
# the operator families (host)
# ------------------------------------------------------------------------------------

def _weights(rs, n):
    return np.exp(-rs.rand(n) * 2).astype(np.float32)


def _base(n, deg, rs):
    """``deg`` random neighbours per vertex, Gaussian weights, symmetrised (the base of ``_random_graph`` in
    test_gpu_recurrence_shapes.py, there with deg = 5)."""
    rows = np.repeat(np.arange(n), deg)
    cols = rs.randint(0, n, rows.size)
    keep = rows != cols
    W = sp.coo_matrix((_weights(rs, int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    return W.maximum(W.T)


def _laplacian_with_isolated(W, n_iso):
    from gcn_fmri_decoding_amd import graph
    W = sp.block_diag([W, sp.csr_matrix((n_iso, n_iso), dtype=np.float32)], format='csr')      # empty rows and columns
    return graph.laplacian(W.astype(np.float32), normalized=True)


@functools.lru_cache(maxsize=None)
def hubs(n_active, n_iso, seed):
    rs = np.random.RandomState(seed)
    W = _base(n_active, 5, rs)
    hub = 7 + (n_active - 20) // len(HUB_EXTRA) * np.arange(len(HUB_EXTRA))          # spread over the caller's order
    others = np.setdiff1d(np.arange(n_active), hub)
    r = np.concatenate([np.full(e, h) for h, e in zip(hub, HUB_EXTRA)])
    c = np.concatenate([rs.choice(others, e, replace=False) for e in HUB_EXTRA])
    E = sp.coo_matrix((_weights(rs, r.size), (r, c)), shape=W.shape).tocsr()
    W = W.maximum(E.maximum(E.T))
    return _laplacian_with_isolated(W, n_iso)


@functools.lru_cache(maxsize=None)
def dense(n_active, n_iso, seed, deg):
    return _laplacian_with_isolated(_base(n_active, deg, np.random.RandomState(seed)), n_iso)


@functools.lru_cache(maxsize=None)
def directed(n, seed, transposed=False):
    rs = np.random.RandomState(seed)
    lengths = np.concatenate([np.resize(DIRECTED_LENGTHS, 160), rs.randint(3, 12, n - 160)])
    targets = np.setdiff1d(np.arange(n), DIRECTED_NO_COLUMN(n))
    r = np.repeat(np.arange(n), lengths)
    c = np.concatenate([rs.choice(targets[targets != v], l, replace=False) for v, l in enumerate(lengths)])
    A = sp.coo_matrix(((0.05 + rs.rand(r.size)) * rs.choice([-1.0, 1.0], r.size), (r, c)), shape=(n, n)).tocsr()
    assert np.array_equal(np.diff(A.indptr), lengths)
    A = sp.diags(1.0 / np.maximum(np.asarray(abs(A).sum(axis=1)).ravel(), 1e-30)) @ A             # rows: abs-sum 1
    A = A @ sp.diags(1.0 / np.maximum(np.asarray(abs(A).sum(axis=0)).ravel(), 1.0))               # columns: abs-sum <= 1
    A = sp.csr_matrix(A.T if transposed else A).astype(np.float32)
    return (A + sp.identity(n, dtype=np.float32, format='csr')).tocsr()


FAMILIES = {'hubs': hubs, 'dense': dense, 'directed': directed}


def profile(L):
    """(row lengths of L~, row lengths of L~^T) of what the library is given."""
    from gcn_fmri_decoding_amd import graph
    indptr, indices, _ = graph.rescaled_laplacian_csr(L)
    return np.diff(indptr), np.bincount(indices, minlength=L.shape[0])


CLASSES = {'<=8': (1, 8), '9-10': (9, 10), '11-12': (11, 12), '13-16': (13, 16), '17-20': (17, 20), '21-24': (21, 24),
           '>=25': (25, 1 << 30), '>=64': (64, 1 << 30), '>=128': (128, 1 << 30)}


def classes_of(lengths):
    return {name for name, (lo, hi) in CLASSES.items() if bool(((lengths >= lo) & (lengths <= hi)).any())}


# ------------------------------------------------------------------------------------
# host tests (no marker)
# ------------------------------------------------------------------------------------

def test_operator_families_are_what_they_are_meant_to_be():
    from gcn_fmri_decoding_amd import graph
    seen_rows, seen_cols = set(), set()
    for L in (hubs(350, 10, 1), hubs(2600, 8, 5), dense(350, 10, 2, 32), dense(2600, 8, 6, 32), dense(16500, 8, 16, 13)):
        rows, cols = profile(L)
        # symmetric in structure; in value up to the rounding of (D^-1/2 W) D^-1/2 (the adjoint reference transposes the CSR)
        assert np.array_equal(rows, cols) and abs(L - L.T).max() <= 1e-7
        seen_rows |= classes_of(rows)
        seen_cols |= classes_of(cols)
        # length_order + permute leave L~ and L~^T sorted by descending length, isolated vertices last
        Lp = graph.permute(L, graph.length_order(L))
        for lens in profile(Lp):
            assert bool((np.diff(lens) <= 0).all())
    for n, e in zip(np.sort(profile(hubs(350, 10, 1))[0])[::-1], sorted(HUB_EXTRA, reverse=True)):
        assert e <= n <= e + 20                                                         # the hubs: extra + the base's 5 ... ~16
    assert profile(hubs(350, 10, 1))[0].max() >= 130
    for L, n_active in ((dense(350, 10, 2, 32), 350), (dense(2600, 8, 6, 32), 2600), (dense(16500, 8, 16, 13), 16500),
                        (dense(6000, 8, 10, 13), 6000)):
        rows, _ = profile(L)
        assert rows[:n_active].min() > 12 and not rows[n_active:].any()                 # no active row of 12 entries or fewer
    assert profile(dense(2600, 8, 6, 32))[0].max() >= 64
    for n in (360, 2600):
        rows, cols = profile(directed(n, 3))
        rt, ct = profile(directed(n, 3, True))
        assert np.array_equal(rows, ct) and np.array_equal(cols, rt)
        assert np.array_equal(rows[:160], np.resize(DIRECTED_LENGTHS, 160)) and 3 <= rows[160:].min() and rows[160:].max() <= 11
        assert classes_of(rows) == set(CLASSES)                                         # every record class, forward
        assert cols.max() < 64 and cols.max() != rows.max()                             # another profile in the adjoint image
        assert rows[0] == 0 and cols[0] > 0                                             # empty row, non-empty column
        assert rows[3] == 8 and cols[3] == 0 and rows[n - 1] > 0 and cols[n - 1] == 0   # the reverse
        assert rows[20] == 0 and cols[20] == 0                                          # isolated
        At = sp.csr_matrix(directed(n, 3) - sp.identity(n, dtype=np.float32))
        assert abs(At).sum(axis=1).max() <= 1 + 1e-6 and abs(At).sum(axis=0).max() <= 1 + 1e-6
        seen_rows |= classes_of(rows) | classes_of(rt)
        seen_cols |= classes_of(cols) | classes_of(ct)
    assert seen_rows == set(CLASSES) and seen_cols == set(CLASSES), (seen_rows, seen_cols)


@pytest.mark.parametrize('family,args', [('hubs', (2600, 8, 5)), ('dense', (2600, 8, 6, 32)), ('hubs', (1500, 40, 4))],
                         ids=['hubs2608', 'dense2608', 'hubs1540'])
def test_bank_order_on_long_rows(family, args):
    """``graph.bank_order`` (chebgcn_bank_order, host only) on long rows: a permutation, still sorted by descending length, and
    the fullest-bank sum no larger than before."""
    from gcn_fmri_decoding_amd import graph
    L = FAMILIES[family](*args)
    stats = []
    order = graph.bank_order(L, stats=stats)
    M = L.shape[0]
    assert np.array_equal(np.sort(order), np.arange(M))
    rows, cols = profile(graph.permute(L, order))
    assert bool((np.diff(rows) <= 0).all()) and bool((np.diff(cols) <= 0).all())
    assert np.array_equal(rows, profile(graph.permute(L, graph.length_order(L)))[0])
    assert stats[0] > 0 and stats[1] <= stats[0], stats


def _fp32_host_errors(K=5, nplanes=15):
    """The numbers of the docstring: the forward recurrence and the Clenshaw adjoint in NumPy fp32 against float64, worst plane.
    ``python -c "import test_gpu_long_rows as t; print(t._fp32_host_errors())"`` in tests/."""
    from gcn_fmri_decoding_amd import graph
    out = {}
    for name, Ls in (('hubs', [hubs(350, 10, 1), hubs(1000, 40, 4), hubs(2600, 60, 5)]),
                     ('dense', [dense(350, 10, 2, 32), dense(1000, 40, 4, 32), dense(2600, 60, 6, 32)]),
                     ('directed', [directed(360, 3), directed(360, 3, True), directed(2600, 3), directed(2600, 3, True)])):
        ef, ea = [], []
        for L in Ls:
            M = L.shape[0]
            indptr, indices, data = graph.rescaled_laplacian_csr(L)
            A32 = sp.csr_matrix((data, indices, indptr), shape=(M, M))
            A64, At32 = A32.astype(np.float64), sp.csr_matrix(A32.T)
            At64 = At32.astype(np.float64)
            rs = np.random.RandomState(M)
            x = rs.randn(M, nplanes).astype(np.float32)
            G = rs.randn(K, M, nplanes).astype(np.float32)
            res = {}
            for A, At, dt in ((A32, At32, np.float32), (A64, At64, np.float64)):
                T = [x.astype(dt), A @ x.astype(dt)]
                for _ in range(2, K):
                    T.append(2 * (A @ T[-1]) - T[-2])
                c2, c1 = np.zeros_like(T[0]), G[K - 1].astype(dt)
                for j in range(K - 2, 0, -1):
                    c2, c1 = c1, G[j].astype(dt) + 2 * (At @ c1) - c2
                res[dt] = (T, G[0].astype(dt) + At @ c1 - c2)
            (T32, dx32), (T, dx) = res[np.float32], res[np.float64]
            ef.append(max(float((np.abs(a.astype(np.float64) - b).max(0) / np.abs(b).max(0)).max()) for a, b in zip(T32, T)))
            ea.append(float((np.abs(dx32.astype(np.float64) - dx).max(0) / np.abs(dx).max(0)).max()))
        out[name] = dict(forward=(min(ef), max(ef)), adjoint=(min(ea), max(ea)))
    return out


# ------------------------------------------------------------------------------------
# every recurrence kernel family by name
# ------------------------------------------------------------------------------------

ONCHIP = 'cheb_onchip_kernel<%d,%d,%d,%d,%s>'
CHEB4 = 'cheb4_kernel<%d,%d,%d,512,%s,%s>'


def _onchip(*shape):
    return ONCHIP % (shape + ('false',)), ONCHIP % (shape + ('true',))


def _cheb4(ent, nj, nq, isoreg):
    return CHEB4 % (ent, nj, nq, 'false', 'true' if isoreg else 'false'), CHEB4 % (ent, nj, nq, 'true', 'false')


def _ord(family, ent, nq, ng, nt, tail=False):
    f, a = ['%s<%d,%d,%d,%d,%s>' % (family, ent, nq, ng, nt, adj) for adj in ('false', 'true')]
    return (f + ' + cheb_ord_tail_kernel<false>', a + ' + cheb_ord_tail_kernel<true>') if tail else (f, a)


# id -> (family, arguments, planes asked for (0: automatic), vertices in length_order, (forward template, adjoint template)).
# The templates follow from the sizes alone (active vertices, M, planes): tools/shape_names.py prints the rule's choice.
CASES = {
    # cheb_onchip_kernel<4,..,256,*>: at most 2048 active rows and 768 linear pieces, the caller's order
    'onchip4_hubs360': ('hubs', (350, 10, 1), 0, False, _onchip(4, 2, 1, 256)),
    'onchip4_dense360': ('dense', (350, 10, 2, 32), 0, False, _onchip(4, 2, 1, 256)),
    'onchip4_directed360': ('directed', (360, 3), 0, False, _onchip(4, 2, 1, 256)),
    'onchip4_directedT360': ('directed', (360, 3, True), 0, False, _onchip(4, 2, 1, 256)),
    'onchip4_hubs2000': ('hubs', (1990, 10, 7), 0, False, _onchip(4, 8, 2, 256)),
    'onchip4_dense2070': ('dense', (1990, 80, 8, 32), 0, False, _onchip(4, 8, 3, 256)),          # 520 linear pieces: three per thread
    # cheb_onchip_kernel<2,..>, planes = 2: every vertex is a row; 256 / 512 / 768 threads
    'onchip2_hubs360': ('hubs', (350, 10, 1), 2, False, _onchip(2, 2, 1, 256)),
    'onchip2_directed360': ('directed', (360, 3), 2, False, _onchip(2, 2, 1, 256)),
    'onchip2_dense2070': ('dense', (2060, 10, 9, 32), 2, False, _onchip(2, 8, 3, 512)),
    'onchip2_hubs4160': ('hubs', (4150, 10, 11), 2, False, _onchip(2, 8, 3, 768)),
    'onchip2_dense4160': ('dense', (4150, 10, 12, 13), 2, False, _onchip(2, 8, 3, 768)),         # (deg = 13: the large sizes)
    # cheb4_kernel, planes = 4: 10 / 20 rows per thread; 2100 isolated vertices: more than four per thread (ISOREG false)
    'cheb4_dense2608': ('dense', (2600, 8, 6, 32), 4, False, _cheb4(5120, 10, 3, True)),
    'cheb4_hubs4700': ('hubs', (2600, 2100, 13), 4, False, _cheb4(5120, 10, 3, False)),
    'cheb4_directed2600': ('directed', (2600, 3), 4, False, _cheb4(5120, 10, 3, True)),
    'cheb4_dense6008': ('dense', (6000, 8, 10, 13), 4, False, _cheb4(10240, 20, 6, True)),
    'cheb4_hubs8100': ('hubs', (6000, 2100, 14), 4, False, _cheb4(10240, 20, 6, False)),
    # cheb_ord_kernel<..,256,false>: 1025 ... 2048 vertices in length order; the adjoint of such a graph is the on-chip kernel
    'ord256_hubs1540': ('hubs', (1500, 40, 4), 0, True, (_ord('cheb_ord_kernel', 2064, 2, 2, 256)[0], _onchip(4, 8, 2, 256)[1])),
    'ord256_dense1540': ('dense', (1500, 40, 15, 32), 0, True, (_ord('cheb_ord_kernel', 2064, 2, 2, 256)[0], _onchip(4, 8, 2, 256)[1])),
    # cheb_ord_kernel<..,512,*>; 3600 isolated vertices are more than one quad level: the streamed tail
    'ord512_hubs2608': ('hubs', (2600, 8, 5), 0, True, _ord('cheb_ord_kernel', 4112, 2, 2, 512)),
    'ord512_dense2608': ('dense', (2600, 8, 6, 32), 0, True, _ord('cheb_ord_kernel', 4112, 2, 2, 512)),
    'ord512_dense6200_tail': ('dense', (2600, 3600, 17, 32), 0, True, _ord('cheb_ord_kernel', 4112, 3, 2, 512, tail=True)),
    # cheb_ord2_kernel; 16500 active vertices: NG = 9, the slots 32..35 of a wave hold rows, and every row is long
    'ord2_hubs11008': ('hubs', (11000, 8, 18), 0, True, _ord('cheb_ord2_kernel', 12304, 6, 6, 512)),
    'ord2_dense16508': ('dense', (16500, 8, 16, 13), 0, True, _ord('cheb_ord2_kernel', 18448, 9, 9, 512)),
    # no LDS image beyond 20480 vertices: one launch per step
    'global_hubs21000': ('hubs', (20990, 10, 19), 0, False, ('cheb_step_global_kernel', 'cheb_step_global_kernel')),
}
K2_CASES = ('onchip4_dense360', 'onchip2_dense2070', 'cheb4_dense2608', 'ord256_dense1540', 'ord512_dense6200_tail', 'ord2_dense16508',
            'global_hubs21000')
RUNS = [(c, 5) for c in CASES] + [(c, 2) for c in K2_CASES]


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _sparse64(indptr, indices, data, M, dev):
    import torch
    return torch.sparse_csr_tensor(torch.as_tensor(indptr.astype(np.int64)), torch.as_tensor(indices.astype(np.int64)),
                                   torch.as_tensor(data.astype(np.float64)), size=(M, M)).to(dev)


def _same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@gpu
@pytest.mark.parametrize('case,K', RUNS, ids=['%s_K%d' % r for r in RUNS])
def test_long_rows_every_plane(dev, case, K):
    import torch
    from gcn_fmri_decoding_amd import _lib, graph, ops
    lib = _lib.lib()
    family, args, planes, ordered, (name_f, name_a) = CASES[case]
    L0 = FAMILIES[family](*args)
    M = L0.shape[0]
    if ordered:
        order = graph.length_order(L0)
        g = ops.Graph(L0, dev, order=order)
        L = graph.permute(L0, order)
        assert g.ordered, 'no ordered kernel shape for M = %d' % M
        PL = g.query(16)
        assert g.query(17) == (int(name_f.split(',')[1]) * 4 * int(name_f.split(',')[3]) if 'tail' in name_f else 0)
    else:
        g, L = ops.Graph(L0, dev, planes=planes), L0
        assert not g.ordered
        PL = g.query(6)
        assert planes in (0, PL)
    assert g.on_chip == (not name_f.startswith('cheb_step_global'))
    assert PL == (0 if not g.on_chip else 2 if name_f.startswith(('cheb_onchip_kernel<2', 'cheb_ord2')) else 4), PL
    indptr, indices, data = graph.rescaled_laplacian_csr(L)
    rows = np.diff(indptr)
    assert rows.max() > 20                                     # beyond what the fused atlas layer and the other tests' graphs have
    if case == 'ord2_dense16508':
        nactive = int((rows > 0).sum())
        assert nactive > 16384 and rows[:nactive].min() > 12   # NG = 9: the slots behind 32 hold rows, the shortest active row is long
    Mp = g.Mp
    B, Fin = (2, 7) if PL == 4 else (3, 5)                      # 14 / 15 planes: a partial last plane group
    nplanes = B * Fin
    assert PL == 0 or nplanes % PL != 0
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * K + M)
    x = torch.randn((B, Fin, Mp), generator=gen, device=dev)    # (non-zero at isolated vertices too)
    x[:, :, M:] = float('nan')
    G = torch.randn((K, B, Fin, Mp), generator=gen, device=dev)
    G[:, :, :, M:] = float('nan')
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    stacks = []
    for _ in range(2):
        stack = torch.full((K, B, Fin, Mp), float('nan'), device=dev)
        _lib.check(lib.chebgcn_recurrence_fwd(g.handle, P(x), P(stack), B, Fin, K, st), 'fwd copy')
        assert _lib.last_dispatch() == name_f, (_lib.last_dispatch(), name_f)
        stacks.append(stack)
    stack = stacks[0]
    assert bool(torch.isfinite(stack[..., :M]).all()), '%s: NaN / not written in the stack' % name_f
    assert _same_bits(stack[..., :M], stacks[1][..., :M]), '%s: two forward calls differ' % name_f
    assert _same_bits(stack[0][..., :M], x[..., :M]), 'slab 0 is a copy of x'
    stack2 = torch.full((K, B, Fin, Mp), float('nan'), device=dev)
    stack2[0].copy_(x)
    _lib.check(lib.chebgcn_recurrence_fwd(g.handle, P(stack2), P(stack2), B, Fin, K, st), 'fwd in place')
    assert _lib.last_dispatch() == name_f
    assert _same_bits(stack[..., :M], stack2[..., :M]), '%s: in place and copied T_0 differ' % name_f
    del stacks, stack2

    A64 = sp.csr_matrix((data.astype(np.float64), indices, indptr), shape=(M, M))
    At64 = sp.csr_matrix(A64.T)
    At64.sort_indices()
    Ld, LTd = _sparse64(indptr, indices, data, M, dev), _sparse64(At64.indptr, At64.indices, At64.data, M, dev)
    X = x[:, :, :M].double().reshape(nplanes, M).t().contiguous()
    T64 = [X, torch.sparse.mm(Ld, X)]
    for k in range(2, K):
        T64.append(2 * torch.sparse.mm(Ld, T64[-1]) - T64[-2])
    Gk = lambda k: G[k, :, :, :M].double().reshape(nplanes, M).t().contiguous()
    c2, c1 = torch.zeros_like(X), Gk(K - 1)
    for j in range(K - 2, 0, -1):
        c2, c1 = c1, Gk(j) + 2 * torch.sparse.mm(LTd, c1) - c2
    dref = Gk(0) + torch.sparse.mm(LTd, c1) - c2
    for pl in (0, nplanes // 2, nplanes - 1):                   # the device's float64 against SciPy's on the host
        t0, t1 = X[:, pl].cpu().numpy(), A64 @ X[:, pl].cpu().numpy()
        for k in range(2, K):
            t0, t1 = t1, 2 * (A64 @ t1) - t0
        assert np.abs(T64[K - 1][:, pl].cpu().numpy() - t1).max() <= 1e-12 * np.abs(t1).max()
        gs = [Gk(k)[:, pl].cpu().numpy() for k in range(K)]
        d2, d1 = np.zeros(M), gs[K - 1]
        for j in range(K - 2, 0, -1):
            d2, d1 = d1, gs[j] + 2 * (At64 @ d1) - d2
        dh = gs[0] + At64 @ d1 - d2
        assert np.abs(dref[:, pl].cpu().numpy() - dh).max() <= 1e-12 * np.abs(dh).max()

    worst_f, where = 0.0, None
    for k in range(K):
        got = stack[k, :, :, :M].reshape(nplanes, M).double().t()
        scale = T64[k].abs().amax(dim=0)
        assert bool((scale > 0).all())
        per_plane = (got - T64[k]).abs().amax(dim=0) / scale
        if float(per_plane.max()) > worst_f:
            pl = int(per_plane.argmax())
            v = int((got - T64[k])[:, pl].abs().argmax())
            worst_f, where = float(per_plane.max()), (k, pl, v, int(rows[v]))
    print('%s K=%d %s: stack worst plane %.3e at (order, plane, vertex, row length) %s' % (case, K, name_f, worst_f, where))

    dxs = []
    for _ in range(2):
        dx = torch.full((B, Fin, Mp), float('nan'), device=dev)
        _lib.check(lib.chebgcn_recurrence_bwd(g.handle, P(G), P(dx), B, Fin, K, st), 'bwd')
        assert _lib.last_dispatch() == name_a, (_lib.last_dispatch(), name_a)
        dxs.append(dx)
    assert bool(torch.isfinite(dxs[0][..., :M]).all()), '%s: NaN / not written in dx' % name_a
    assert _same_bits(dxs[0][..., :M], dxs[1][..., :M]), '%s: two adjoint calls differ' % name_a
    gotx = dxs[0][:, :, :M].reshape(nplanes, M).double().t()
    per_plane = (gotx - dref).abs().amax(dim=0) / dref.abs().amax(dim=0)
    worst_a = float(per_plane.max())
    pl = int(per_plane.argmax())
    v = int((gotx - dref)[:, pl].abs().argmax())
    cols = np.diff(At64.indptr)
    print('%s K=%d %s: dx worst plane %.3e at (plane, vertex, column length) %s' % (case, K, name_a, worst_a, (pl, v, int(cols[v]))))
    record_measured('long_rows[%s_K%d]' % (case, K), fwd=name_f, bwd=name_a, longest_row=int(rows.max()), longest_column=int(cols.max()),
                    stack=worst_f, dx=worst_a)
    assert worst_f <= REL, '%s: stack %.3e from float64 at (order, plane, vertex, row length) %s' % (name_f, worst_f, where)
    assert worst_a <= GREL, '%s: dx plane %d is %.3e from float64 (vertex %d, column of %d entries)' % (name_a, pl, worst_a, v, cols[v])


# ------------------------------------------------------------------------------------
# the atlas case end to end: a k = 32 connectivity graph on 360 regions
# ------------------------------------------------------------------------------------

ATLAS_M, ATLAS_K = 360, 32
ATLAS_NAMES = _onchip(4, 2, 1, 256)
_atlas = {}


def atlas_laplacian(dev):
    """``connectivity_graph`` on seeded latent-factor runs (two runs of 150 time points, 12 factors + noise), then ``adjacency``
    and ``laplacian``: the reference's RSFC graph construction, neighbour search on the device."""
    from gcn_fmri_decoding_amd import graph
    if 'L' not in _atlas:
        rs = np.random.RandomState(32)
        mix = rs.randn(12, ATLAS_M)
        runs = [(rs.randn(150, 12) @ mix + 2.0 * rs.randn(150, ATLAS_M)).astype(np.float32) for _ in range(2)]
        d, idx = graph.connectivity_graph(runs, k=ATLAS_K, device=dev)
        assert d.shape == idx.shape == (ATLAS_M, ATLAS_K)
        d = np.maximum(d, 0)                      # (1 - r of two all but identical series may round below 0; none here)
        _atlas['L'] = graph.laplacian(graph.adjacency(d, idx).astype(np.float32), normalized=True)
    return _atlas['L']


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


@gpu
def test_atlas_graph_rows_and_fused_layer_declines(dev):
    from gcn_fmri_decoding_amd import _lib, ops
    L = atlas_laplacian(dev)
    rows, cols = profile(L)
    assert rows.min() > 20 and np.array_equal(rows, cols), (rows.min(), rows.max())       # k = 32 neighbours at least, everywhere
    assert rows.min() >= ATLAS_K
    g = ops.Graph(L, dev)
    assert g.Mp <= 384 and g.query(5) == rows.max() and g.query(6) == 4 and not g.ordered
    for B, Fin, K, Fout in ((8, 3, 4, 8), (8, 8, 4, 16), (300, 16, 4, 16)):
        assert _lib.lib().chebgcn_fused_layer_supported(g.handle, B, Fin, K, Fout) == 0


@gpu
def test_atlas_one_layer_vs_float64(dev):
    """One graph-convolution layer through ``ops.cheb_conv`` (B = 8, Fin = 12, K = 4, Fout = 8, per-filter bias, ReLU) against
    ``oracle/layers_ref`` in float64: out at REL of the pre-activation's scale per plane, dx at GREL per plane, dW and dbias at
    GREL of their largest element (the bounds of test_gpu_fused_layer_arms.test_through_cheb_conv); the ReLU gate of the reference
    is the kernel's own ``out > 0``.  The dispatch log names the M = 360 recurrence kernels (the input gradient in Clenshaw form:
    the forward form of ``ops.dx_by_forward`` is for graphs in length order) and no fused one."""
    import torch
    from gcn_fmri_decoding_amd import _lib, ops
    from oracle import layers_ref as R
    L = atlas_laplacian(dev)
    g = ops.Graph(L, dev)
    M, Mp, B, Fin, K, Fout = ATLAS_M, g.Mp, 8, 12, 4, 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(360)
    x = torch.randn((B, Fin, Mp), generator=gen, device=dev)
    gout = torch.randn((B, Fout, Mp), generator=gen, device=dev)
    x[..., M:] = 0.0
    gout[..., M:] = 0.0
    W = (torch.randn((Fin * K, Fout), generator=gen, device=dev) * (0.5 / np.sqrt(Fin * K))).requires_grad_(True)
    bias = (torch.randn((Fout,), generator=gen, device=dev) * 0.3).requires_grad_(True)
    x.requires_grad_(True)
    _lib.dispatch_log = log = []
    try:
        out = ops.cheb_conv(x, W, bias, g, K, relu=True, bias_kind=_lib.BIAS_FILTER)
        out.backward(gout)
    finally:
        _lib.dispatch_log = None
    torch.cuda.synchronize()
    assert not any('fused_layer' in w or 'fused_layer' in n for w, n in log), log
    assert ('recurrence_fwd', ATLAS_NAMES[0]) in log, log
    assert ('recurrence_bwd', ATLAS_NAMES[1]) in log, log
    to_ref = lambda t: np.ascontiguousarray(t.detach()[..., :M].cpu().numpy().astype(np.float64).transpose(0, 2, 1))     # [B, M, F]
    L64 = L.astype(np.float64)
    W64, b64 = W.detach().cpu().numpy().astype(np.float64), bias.detach().cpu().numpy().astype(np.float64)
    y, T = R.chebyshev5_fwd(to_ref(x), L64, W64, K, return_stack=True)
    y = y + b64
    got = to_ref(out)
    e_out = float((np.abs(got - np.maximum(y, 0)).max(axis=1) / np.abs(y).max(axis=1)).max())
    dy = to_ref(gout) * (got > 0)
    dx, dW = R.chebyshev5_bwd(dy, L64, W64, K, T)
    e_dx = float((np.abs(to_ref(x.grad) - dx).max(axis=1) / np.abs(dx).max(axis=1)).max())
    e_dW = _rel(W.grad.cpu().numpy().astype(np.float64), dW)
    e_db = _rel(bias.grad.cpu().numpy().astype(np.float64), dy.sum(axis=(0, 1)))
    print('atlas layer: out %.3e dx %.3e dW %.3e dbias %.3e' % (e_out, e_dx, e_dW, e_db))
    record_measured('long_rows[atlas_layer]', out=e_out, dx=e_dx, dW=e_dW, dbias=e_db)
    assert e_out <= REL and e_dx <= GREL and e_dW <= GREL and e_db <= GREL, (e_out, e_dx, e_dW, e_db)


@gpu
def test_atlas_small_cgcnn_vs_float64(dev):
    """A cgcnn of two conv layers (K = 4, F = 8 and 16, per-vertex bias, no pooling), FC 12 - 5, three input channels, batch 8,
    exact fp32 products (``contraction = 'f32'``): logits within 1e-5 of the largest and every gradient of one step within 2e-4 of
    its largest element of ``oracle/layers_ref.Net`` in float64 -- the bounds of test_gpu_finetune.py.  Every recurrence launch
    of the step is the M = 360 generic kernel; no fused atlas-layer kernel runs."""
    import torch
    from gcn_fmri_decoding_amd import _lib, models_gcn, ops
    from oracle import layers_ref as R
    L = atlas_laplacian(dev)
    M, B, C, reg = ATLAS_M, 8, 3, 5e-4
    F, K, p, Mfc = [8, 16], [4, 4], [1, 1], [12, 5]
    onet = R.Net([L.astype(np.float64)], F, K, p, Mfc, channel=C, brelu='b2relu', regularization=reg, dtype=np.float64)
    rs = np.random.RandomState(8)
    params = {}
    for k, s in onet.param_shapes().items():
        params[k] = ((0.2 + 0.05 * rs.randn(*s)) if k.endswith('bias') else rs.randn(*s) * np.sqrt(2.0 / s[0])).astype(np.float32)
    x = rs.randn(B, M, C).astype(np.float32)
    labels = rs.randint(0, Mfc[-1], B)
    net = models_gcn.cgcnn({'device': dev}, [L] * 2, F, K, p, Mfc, filter='chebyshev5', brelu='b2relu', pool='mpool1', initial='he',
                           channel=C, regularization=reg, dropout=1, batch_size=B, verbose=False)
    net.contraction = 'f32'
    net.enable_step_graph(False)
    for k, v in params.items():
        net.set_variable(k, v)
    xs = torch.full((B, C, ops.plane_stride(M)), float('nan'), device=dev)
    xs[:, :, :M] = torch.as_tensor(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    ld = torch.as_tensor(labels).to(dev)
    _lib.dispatch_log = log = []
    try:
        with torch.no_grad():
            logits = net._inference_storage(xs, 1).cpu().numpy().astype(np.float64)
        net.train_step(xs, ld)
        torch.cuda.synchronize()
    finally:
        _lib.dispatch_log = None
    assert not any('fused_layer' in w or 'fused_layer' in n for w, n in log), log
    rec = [(w, n) for w, n in log if w.startswith('recurrence')]
    assert ('recurrence_fwd', ATLAS_NAMES[0]) in rec and all(n in ATLAS_NAMES for _, n in rec), rec
    assert any(w in ('recurrence_bwd', 'recurrence_fwd_t') for w, _ in rec), rec          # layer 2's input gradient
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    ref_logits, cache = onet.forward(p64, x.astype(np.float64))
    _, dlogits = onet.loss(p64, ref_logits, labels)
    grads = onet.backward(p64, cache, dlogits)
    e_logits = _rel(logits, ref_logits)
    measured = {'logits': e_logits}
    worst = 0.0
    for k in params:
        ref = grads[k] - (reg * p64[k] if onet.regularized(k) else 0)           # net.gradient: without the L2 term (test_gpu_dispatch.py)
        measured['grad_' + k] = e = _rel(net.gradient(k).cpu().numpy().astype(np.float64), ref)
        worst = max(worst, e)
    print('atlas cgcnn: %s' % measured)
    record_measured('long_rows[atlas_cgcnn]', **measured)
    assert e_logits <= 1e-5, e_logits
    assert worst <= 2e-4, measured
