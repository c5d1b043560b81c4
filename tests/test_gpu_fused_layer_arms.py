"""Every arm of the fused atlas-layer kernels (csrc/fused_small.hip), BY NAME, against float64 at their edges.  Needs an
MI355X: ``-m gpu``.

``fs_dispatch`` instantiates sixteen kernels ``fused_layer_kernel<NW,PL,ADJ,ML>``: NW = 8 / 12 waves by the plane stride
(<= 256 / <= 384), PL = 8 / 16 planes per lane by the batch (a window split between two workgroups while
``2 B <= 1.5 x CUs``), ADJ = the layer / its gradient wrt the input, ML = 16 / 20 operator entries per row held in registers by
the longest row of the operator the launch reads (L~ forward, L~^T backward).  Plain tensors through the C ABI
(``chebgcn_fused_layer_supported / _workspace / _fwd / _bwd_x``); every case

* asserts the host-side longest row before it trusts a name, then names its kernel through ``chebgcn_last_dispatch()``,
* compares EVERY element of every output with a float64 restatement of the header comment of fused_small.hip (``ref_forward``,
  ``ref_backward`` below: torch float64, on the device here; tests/test_fused_layer_refs.py ties both to literal nested-loop
  transcriptions on a machine without a GPU).  The operator is what the library gets: ``graph.rescaled_laplacian_csr(L)``
  values (fp32) cast to float64 (scattered into a dense matrix: no two entries of a row share a column, and a float64 sum over
  a row does not depend on the entries' order at the bounds asserted here),
* poisons the pad [M, Mp) of every input plane with NaN (the dout pad of a backward without a mask is 0, as
  test_fused_atlas_layer_vs_oracle documents), pre-fills every output and the workspace with a sentinel and surrounds each
  with a sentinel margin ("not written" and "written outside" are both visible),
* checks the ReLU bit mask against ``out > 0`` of the kernel's OWN output bit for bit, pad bits 0,
* gates the backward with a RANDOM mask (not the forward's: no ReLU within round-off of zero can enter, and the gate is tested
  on its own),
* calls twice and asserts bit-identical results, and asserts the inference form (no stack, no mask) gives the same ``out``.

Bounds -- the project's own (REL, GREL of test_gpu_dispatch.py / test_gpu_recurrence_shapes.py), applied PER PLANE:
``max|got - ref| <= 1e-5 max|ref|`` for ``out`` (scale: the plane's pre-activation |y|) and for each plane of the stack, 2e-5 for
``dx``.  Not tuned to the kernel: the same recurrence and contraction in NumPy fp32 against float64 stays at or below 1.4e-6
(out), 4.8e-7 (stack) and 7.5e-7 (dx) per plane on these graphs up to K = 25, Fin = 32; the kernel's other summation order
(fmaf chains, matrix-core k order) has a factor of 7 to spend.  Copies (slab 0 of the stack, ``stack == x``) are bit-exact.

Measured on the MI355X (profiles/r07_fused_layer_arms_measured.jsonl): every case within 2.1e-6 (out), 7.2e-7 (stack), 1.8e-6
(dx); the largest of each at K = 31, eight waves, one workgroup per window -- the launch that asks for all 163 840 bytes of a
CU's LDS succeeds, as does K = 26 at twelve waves.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import record_measured

pytestmark = pytest.mark.gpu
REL, GREL = 1e-5, 2e-5
F64 = torch.float64
EUNSUPPORTED = -4
FS_MAXLEN = 20
BIAS = {'none': 0, 'filter': 1, 'vertex': 2}


def plane_stride(M):
    return (int(M) + 31) & ~31


# ------------------------------------------------------------------------------------
# operators (host)
# ------------------------------------------------------------------------------------

class Operator:
    """A matrix L as the library receives it: CSR of ``rescaled_laplacian_csr(L)``; the longest row of L~ and of L~^T."""

    def __init__(self, L):
        from gcn_fmri_decoding_amd import graph
        self.L = sp.csr_matrix(L)
        self.M = int(self.L.shape[0])
        self.Mp = plane_stride(self.M)
        self.indptr, self.indices, self.data = graph.rescaled_laplacian_csr(self.L)
        self.rows = np.diff(self.indptr)
        self.cols = np.bincount(self.indices, minlength=self.M)
        self.len_fwd, self.len_adj = int(self.rows.max()), int(self.cols.max())

    def dense(self, device='cpu'):
        return dense_operator(self.indptr, self.indices, self.data, self.M).to(device)

    @property
    def nw(self):
        return 8 if self.Mp <= 256 else 12 if self.Mp <= 384 else 0

    @staticmethod
    def ml(longest):
        assert 0 < longest <= FS_MAXLEN
        return 16 if longest <= 16 else FS_MAXLEN


@functools.lru_cache(maxsize=None)
def synthetic(N, k):
    """``graph.synthetic_graph(N, k, levels=1)``: kNN graph + one coarsening level (its fake vertices are isolated: empty rows
    that carry data in every test here)."""
    from gcn_fmri_decoding_amd import graph
    return Operator(graph.synthetic_graph(N, k=k, levels=1)[0][0])


@functools.lru_cache(maxsize=None)
def knn(M, k, isolated=()):
    """The normalised Laplacian of a symmetrised kNN graph on exactly M vertices (no coarsening: M is what the test asks for),
    the vertices ``isolated`` cut off (empty rows and columns)."""
    from gcn_fmri_decoding_amd import graph
    z = np.random.RandomState(0).rand(M, 3).astype(np.float32)
    d, idx = graph.distance_sklearn_metrics(z, k=k)
    A = graph.adjacency(d, idx).astype(np.float32).tolil()
    for v in isolated:
        A[v, :] = 0
        A[:, v] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    return Operator(graph.laplacian(A, normalized=True))


@functools.lru_cache(maxsize=None)
def ring(M, transposed):
    """A NON-symmetric operator: L = A + I (rescale_L subtracts the identity again: L~ = A), A = a ring of 4 neighbours
    (v +- 1, v +- 2) plus 15 rows (10, 20, .., 150) that also point at vertex 0; every value drawn on its own.  Rows of A have
    4 or 5 entries, column 0 has 19; ``transposed``: A^T instead."""
    rs = np.random.RandomState(M)
    r = np.repeat(np.arange(M), 4)
    c = (r + np.tile([-2, -1, 1, 2], M)) % M
    extra = 10 * np.arange(1, 16)
    r, c = np.concatenate([r, extra]), np.concatenate([c, np.zeros(15, np.int64)])
    A = sp.coo_matrix(((0.05 + 0.2 * rs.rand(r.size)).astype(np.float32), (r, c)), shape=(M, M)).tocsr()
    assert A.nnz == 4 * M + 15                                            # no duplicates
    if transposed:
        A = sp.csr_matrix(A.T)
    return Operator((A + sp.identity(M, dtype=np.float32, format='csr')).tocsr())


def dense_operator(indptr, indices, data, M):
    """CSR (fp32 values) -> dense float64 [M, M]."""
    rows = np.repeat(np.arange(M), np.diff(indptr))
    D = np.zeros((M, M), np.float64)
    assert len(set(zip(rows.tolist(), np.asarray(indices).tolist()))) == len(data)
    D[rows, indices] = np.asarray(data, np.float32).astype(np.float64)
    return torch.as_tensor(D)


# ------------------------------------------------------------------------------------
# the references: torch float64 (any device)
# ------------------------------------------------------------------------------------

def ref_forward(D, x, W, K, bias=None, relu=False):
    """x [B, Fin, M], W [Fin*K, Fout], bias None / [Fout] / [Fout, M] -> (y before the activation [B, Fout, M], out, stack
    [K, B, Fin, M]):  T_0 = x, T_1 = L~ T_0, T_k = 2 L~ T_{k-1} - T_{k-2};  y[b,o,m] = sum_{fin,k} W[fin*K+k, o] T_k[b,fin,m] + bias."""
    B, Fin, M = x.shape
    T = [x]
    if K > 1:
        T.append(torch.matmul(x, D.T))                              # (L~ t)[m] = sum_n D[m, n] t[n]
    for _ in range(2, K):
        T.append(2 * torch.matmul(T[-1], D.T) - T[-2])
    stack = torch.stack(T)
    y = torch.einsum('fko,kbfm->bom', W.reshape(Fin, K, -1), stack)
    if bias is not None:
        y = y + (bias[None, :, None] if bias.dim() == 1 else bias[None])
    return y, (torch.clamp(y, min=0) if relu else y), stack


def ref_backward(D, dy, gate, W, Fin, K):
    """dy [B, Fout, M], gate None / bool [B, Fout, M] -> dx [B, Fin, M]:  G_j[b,fin,m] = sum_o W[fin*K+j, o] (gate dy)[b,o,m];
    c_{K-1} = G_{K-1}, c_j = G_j + 2 L~^T c_{j+1} - c_{j+2}, dx = G_0 + L~^T c_1 - c_2."""
    if gate is not None:
        dy = torch.where(gate, dy, torch.zeros_like(dy))
    W3 = W.reshape(Fin, K, -1)
    G = lambda j: torch.einsum('fo,bom->bfm', W3[:, j], dy)
    c1 = c2 = None                                                   # c_{j+1}, c_{j+2}
    for j in range(K - 1, 0, -1):
        c = G(j)
        if c1 is not None:
            c = c + 2 * torch.matmul(c1, D)                          # (L~^T c)[m] = sum_n D[n, m] c[n]
        if c2 is not None:
            c = c - c2
        c1, c2 = c, c1
    dx = G(0)
    if c1 is not None:
        dx = dx + torch.matmul(c1, D)
    if c2 is not None:
        dx = dx - c2
    return dx


def mask_bits(mask, Mp):
    """[.., Mp/4] bytes -> [.., Mp] bool: vertex m is bit (m & 3) of byte m / 4; the upper four bits of a byte must be 0."""
    assert not bool((mask >> 4).any()), 'mask byte with a bit above the four vertex bits'
    return torch.stack([(mask >> r) & 1 for r in range(4)], -1).reshape(mask.shape[:-1] + (Mp,)).bool()


def launch_geometry(nw, pl, K, B, cus):
    """fs_lds / the slot count of fs_launch (csrc/fused_small.hip), restated: (LDS bytes, workgroup slots, workgroups wanted)."""
    lds = (32 * nw * (2 * pl + 4) + K * 1024) * 4
    slots = cus * min(2, max(1, (160 * 1024) // lds))
    ns = 16 // pl
    return lds, slots - slots % ns, B * ns


# ------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from gcn_fmri_decoding_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


_graphs = {}


def device_graph(op, dev):
    from gcn_fmri_decoding_amd import ops
    if id(op) not in _graphs:
        g = ops.Graph(op.L, dev)
        assert (g.M, g.Mp) == (op.M, op.Mp)
        assert not g.on_chip or g.query(5) == op.len_fwd             # the library's longest forward row = the host's
        _graphs[id(op)] = (g, op)
    return _graphs[id(op)][0]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _named(name):
    from gcn_fmri_decoding_amd import _lib
    assert _lib.last_dispatch() == name, (_lib.last_dispatch(), name)


class Guarded:
    """An output of ``shape`` filled with a sentinel (NaN; 0xA5 for bytes), inside one allocation with a sentinel margin of at
    least one row (a multiple of 32 elements: the output keeps the allocation's alignment) in front and behind."""

    def __init__(self, shape, dtype, dev):
        self.fill = float('nan') if dtype.is_floating_point else 0xA5
        n = int(np.prod(shape))
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        self.m = max(32, (row + 31) // 32 * 32)
        self.full = torch.full((self.m + n + self.m,), self.fill, dtype=dtype, device=dev)
        self.t = self.full[self.m:self.m + n].view(shape)

    def refill(self):
        self.full.fill_(self.fill)

    def _is_fill(self, t):
        return bool(torch.isnan(t).all()) if self.fill != self.fill else bool((t == self.fill).all())

    def margins_intact(self):
        return self._is_fill(torch.cat([self.full[:self.m], self.full[self.full.numel() - self.m:]]))

    def untouched(self):
        return self._is_fill(self.full)


def same_bits(a, b):
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def plane_error(got, ref, scale_ref, bound, what):
    """Every plane (last axis): finite and max|got - ref| <= bound * max|scale_ref|; returns the worst plane's ratio
    max|got - ref| / max|scale_ref|."""
    assert got.shape == ref.shape == scale_ref.shape, (what, got.shape, ref.shape)
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), '%s: %d of %d elements not written or not finite' % (what, int(bad.sum()), got.numel())
    err = (got.to(F64) - ref).abs().amax(-1)
    scale = scale_ref.abs().amax(-1)
    assert bool((scale > 0).all()), '%s: a reference plane is identically zero (the case does not test it)' % what
    ratio = err / scale
    worst = float(ratio.max())
    print('%s: worst plane %.3e (bound %.1e)' % (what, worst, bound))
    assert worst <= bound, '%s: %d of %d planes beyond %.1e, worst %.3e' % (what, int((ratio > bound).sum()), ratio.numel(), bound, worst)
    return worst


class Layer:
    """One (operator, B, Fin, K, Fout, bias, relu) case: inputs with poisoned pads on the device, the float64 references, and
    the guarded launches."""

    def __init__(self, dev, lib, cus, op, B, Fin, K, Fout, bias_kind='none', relu=False, seed=0):
        self.dev, self.lib, self.op, self.g = dev, lib, op, device_graph(op, dev)
        self.B, self.Fin, self.K, self.Fout, self.bias_kind, self.relu = B, Fin, K, Fout, bias_kind, bool(relu)
        M, Mp = op.M, op.Mp
        self.split = 2 if 2 * B <= cus + cus // 2 else 1                # fs_split: two workgroups per window while CUs would idle
        self.pl = 16 // self.split
        self.cus = cus
        gen = torch.Generator(device=dev)
        gen.manual_seed(1000003 * seed + 7919 * B + 131 * Fin + 17 * K + Fout + M)
        rnd = lambda *s: torch.randn(s, generator=gen, device=dev)
        self.x = rnd(B, Fin, Mp)
        self.x[..., M:] = float('nan')
        self.W = rnd(Fin * K, Fout) * (0.5 / np.sqrt(Fin * K))
        self.bias = None
        if bias_kind == 'filter':
            self.bias = rnd(Fout) * 0.3
        elif bias_kind == 'vertex':
            self.bias = rnd(Fout, Mp) * 0.3
            self.bias[:, M:] = float('nan')
        self.dout = rnd(B, Fout, Mp)
        self.dout[..., M:] = float('nan') if self.relu else 0.0
        # the backward's gate: random bits, random in the pad as well
        self.gate = torch.randint(0, 16, (B, Fout, Mp // 4), generator=gen, device=dev, dtype=torch.uint8) if self.relu else None
        self.nws = lib.chebgcn_fused_layer_workspace(self.g.handle, B, Fin, K, Fout)
        self.D = op.dense(dev)

    # names ---------------------------------------------------------------------------------------------------------------------
    def fwd_name(self):
        return 'fused_layer_kernel<%d,%d,false,%d>' % (self.op.nw, self.pl, Operator.ml(self.op.len_fwd)) + (
            ' + fused_combine_kernel' if self.split == 2 else '')

    def bwd_name(self):
        return 'fused_layer_kernel<%d,%d,true,%d>' % (self.op.nw, self.pl, Operator.ml(self.op.len_adj))

    # launches ------------------------------------------------------------------------------------------------------------------
    def forward(self, stack, out, mask, ws, x=None):
        return self.lib.chebgcn_fused_layer_fwd(self.g.handle, _p(self.x if x is None else x), _p(self.W), _p(self.bias), BIAS[self.bias_kind],
                                                _p(stack), _p(out), _p(mask), _p(ws), self.nws, self.B, self.Fin, self.K, self.Fout,
                                                int(self.relu), _s())

    def backward(self, dx):
        return self.lib.chebgcn_fused_layer_bwd_x(self.g.handle, _p(self.dout), _p(self.gate), _p(self.W), _p(dx), self.B, self.Fin, self.K,
                                                  self.Fout, _s())

    def check(self, tag, alias=False):
        """Forward (training form twice, inference form, optionally ``stack == x``) and backward (twice), everything compared;
        returns the measured errors."""
        from gcn_fmri_decoding_amd import _lib
        dev, op, B, Fin, K, Fout = self.dev, self.op, self.B, self.Fin, self.K, self.Fout
        M, Mp = op.M, op.Mp
        assert self.lib.chebgcn_fused_layer_supported(self.g.handle, B, Fin, K, Fout) == 1
        assert self.nws == (2 * B * 32 * Mp * 4 if self.split == 2 else 0)
        stack, out = Guarded((K, B, Fin, Mp), torch.float32, dev), Guarded((B, Fout, Mp), torch.float32, dev)
        mask = Guarded((B, Fout, Mp // 4), torch.uint8, dev) if self.relu else None
        ws = Guarded((max(self.nws // 4, 1),), torch.float32, dev)
        all_out = [t for t in (stack, out, mask, ws) if t is not None]
        runs = []
        for _ in range(2):
            for t in all_out:
                t.refill()
            _lib.check(self.forward(stack.t, out.t, mask.t if mask else None, ws.t), 'fused_layer_fwd')
            _named(self.fwd_name())
            assert all(t.margins_intact() for t in all_out), tag + ': forward wrote outside an output'
            runs.append((out.t.clone(), stack.t.clone(), mask.t.clone() if mask else None))
        assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), tag + ': two forward runs differ'
        assert mask is None or torch.equal(runs[0][2], runs[1][2]), tag + ': two forward runs differ in the mask'
        got_out, got_stack, got_mask = runs[0]
        x64, W64 = self.x[..., :M].to(F64), self.W.to(F64)
        b64 = None if self.bias is None else (self.bias.to(F64) if self.bias.dim() == 1 else self.bias[:, :M].to(F64))
        y, act, T = ref_forward(self.D, x64, W64, K, b64, self.relu)
        got = {}
        got['out'] = plane_error(got_out[..., :M], act, y, REL, tag + ' out')
        got['stack'] = plane_error(got_stack[..., :M], T, T, REL, tag + ' stack')
        assert same_bits(got_stack[0][..., :M], self.x[..., :M]), tag + ': slab 0 of the stack is a copy of x'
        del T, y, act
        if mask:
            bits = mask_bits(got_mask, Mp)
            assert torch.equal(bits[..., :M], got_out[..., :M] > 0), tag + ': ReLU bit mask disagrees with the output'
            assert not bool(bits[..., M:].any()), tag + ': mask bits set in the pad'
        # inference form: no stack is written, no mask; the same output bits
        out.refill()
        ws.refill()
        _lib.check(self.forward(None, out.t, None, ws.t), 'fused_layer_fwd')
        _named(self.fwd_name())
        assert out.margins_intact() and ws.margins_intact()
        assert same_bits(out.t[..., :M], got_out[..., :M]), tag + ': inference form differs'
        if alias:
            # slab 0 IS the input (``stack == x``): T_0 stays in place, the rest of the stack and `out` as in the copying call
            for t in all_out:
                t.refill()
            stack.t[0].copy_(self.x)
            _lib.check(self.forward(stack.t, out.t, mask.t if mask else None, ws.t, x=stack.t), 'fused_layer_fwd')
            _named(self.fwd_name())
            assert all(t.margins_intact() for t in all_out)
            assert same_bits(stack.t[0], self.x), tag + ': stack == x: slab 0 changed'
            assert same_bits(stack.t[1:], got_stack[1:]) and same_bits(out.t, got_out), tag + ': stack == x differs from the copying call'
            assert mask is None or torch.equal(mask.t, got_mask)
        del stack, runs, got_stack
        # gradient wrt the input
        dx = Guarded((B, Fin, Mp), torch.float32, dev)
        druns = []
        for _ in range(2):
            dx.refill()
            _lib.check(self.backward(dx.t), 'fused_layer_bwd_x')
            _named(self.bwd_name())
            assert dx.margins_intact(), tag + ': backward wrote outside dx'
            druns.append(dx.t.clone())
        assert same_bits(druns[0], druns[1]), tag + ': two backward runs differ'
        gate = mask_bits(self.gate, Mp)[..., :M] if self.relu else None
        dref = ref_backward(self.D, self.dout[..., :M].to(F64), gate, W64, Fin, K)
        got['dx'] = plane_error(druns[0][..., :M], dref, dref, GREL, tag + ' dx')
        record_measured('fused_layer_arms[%s]' % tag, fwd=self.fwd_name(), bwd=self.bwd_name(), **got)
        return got

    def _refs_with(self, D):
        """(out, pre-activation, dx) in float64 for the operator D -- for the test that compares with ANOTHER operator's."""
        M = self.op.M
        b64 = None if self.bias is None else (self.bias.to(F64) if self.bias.dim() == 1 else self.bias[:, :M].to(F64))
        y, act, _ = ref_forward(D, self.x[..., :M].to(F64), self.W.to(F64), self.K, b64, self.relu)
        gate = mask_bits(self.gate, self.op.Mp)[..., :M] if self.relu else None
        return act, y, ref_backward(D, self.dout[..., :M].to(F64), gate, self.W.to(F64), self.Fin, self.K)

    def declined(self, tag):
        """A shape the fused kernels do not serve: _supported and _workspace 0, _fwd and _bwd_x EUNSUPPORTED, nothing written."""
        dev, B, Fin, K, Fout, Mp = self.dev, self.B, self.Fin, self.K, self.Fout, self.op.Mp
        assert self.lib.chebgcn_fused_layer_supported(self.g.handle, B, Fin, K, Fout) == 0, tag
        assert self.nws == 0, tag
        stack, out = Guarded((K, B, Fin, Mp), torch.float32, dev), Guarded((B, Fout, Mp), torch.float32, dev)
        mask, dx = Guarded((B, Fout, Mp // 4), torch.uint8, dev), Guarded((B, Fin, Mp), torch.float32, dev)
        ws = Guarded((2 * B * 32 * Mp,), torch.float32, dev)
        self.nws = ws.t.numel() * 4
        rc = self.forward(stack.t, out.t, mask.t if self.relu else None, ws.t)
        assert rc == EUNSUPPORTED and 'not served' in self.lib.chebgcn_last_error().decode(), (tag, rc)
        rc = self.backward(dx.t)
        assert rc == EUNSUPPORTED and 'not served' in self.lib.chebgcn_last_error().decode(), (tag, rc)
        torch.cuda.synchronize()
        assert all(t.untouched() for t in (stack, out, mask, dx, ws)), tag + ': a declined call wrote something'


# ------------------------------------------------------------------------------------
# all sixteen instantiations by name
# ------------------------------------------------------------------------------------

# (N, k) of graph.synthetic_graph(N, k, levels=1) -> (M, longest row), computed on the CPU; the kernel family they select
SYNTHETIC = {(360, 8): (376, 15), (246, 8): (260, 15), (100, 8): (108, 14),               # ML 16
             (330, 10): (342, 19), (224, 8): (234, 18), (150, 10): (156, 20), (30, 8): (32, 18),      # ML 20 (156: the limit)
             (200, 12): (204, 21), (360, 12): (374, 23)}                                # declined
B_SPLIT, B_WHOLE = 5, 200                                # 2 B <= 1.5 CUs: two workgroups per window (PL 8); above: one (PL 16)


def synthetic_checked(N, k):
    op = synthetic(N, k)
    assert (op.M, op.len_fwd, op.len_adj) == SYNTHETIC[(N, k)] + (SYNTHETIC[(N, k)][1],), (N, k, op.M, op.len_fwd, op.len_adj)
    assert int((op.rows == 0).sum()) > 0                 # isolated vertices (the coarsening's fake ones): they carry data here
    return op


def instantiation_names():
    """The names the table below asserts, from the host-side figures alone (tests/test_fused_layer_refs.py: sixteen)."""
    names = set()
    for (N, k), (M, longest) in SYNTHETIC.items():
        if longest <= FS_MAXLEN:
            for pl in (8, 16):
                for adj in ('false', 'true'):
                    names.add('fused_layer_kernel<%d,%d,%s,%d>' % (8 if plane_stride(M) <= 256 else 12, pl, adj, Operator.ml(longest)))
    return names


@pytest.mark.parametrize('B', [B_SPLIT, B_WHOLE], ids=['split', 'whole'])
@pytest.mark.parametrize('N,k', [nk for nk, (_, n) in SYNTHETIC.items() if n <= FS_MAXLEN], ids=lambda v: str(v))
def test_every_instantiation_by_name(dev, lib, cus, N, k, B):
    """NW by the plane stride, PL by the batch, ML by the longest row (15, 15, 14 -> 16; 19, 18, 20, 18 -> 20): with ADJ, all 16
    kernels of fs_dispatch, each asserted by its exact name in Layer.check; M = 32 = Mp (one wave of eight with a vertex), 156
    (rows of 20 entries: FS_MAXLEN itself), 260 -> 288 (twelve waves, three without a vertex)."""
    op = synthetic_checked(N, k)
    case = Layer(dev, lib, cus, op, B, 20, 4, 24, 'vertex', True, seed=1)
    assert case.split == (2 if B == B_SPLIT else 1)
    case.check('inst_N%d_k%d_B%d' % (N, k, B))


@pytest.mark.parametrize('N,k', [(200, 12), (360, 12)])
def test_rows_beyond_twenty_entries_are_declined(dev, lib, cus, N, k):
    op = synthetic_checked(N, k)
    assert op.len_fwd > FS_MAXLEN and op.nw
    for B in (B_SPLIT, B_WHOLE):
        Layer(dev, lib, cus, op, B, 5, 3, 6, 'vertex', True).declined('rows_N%d_B%d' % (N, B))


def test_more_than_384_vertices_declined(dev, lib, cus):
    op = knn(400, 6)
    assert op.Mp == 416 and op.len_fwd <= 16
    Layer(dev, lib, cus, op, 4, 5, 3, 6).declined('M400')


# ------------------------------------------------------------------------------------
# a second window in the same workgroup (the persistent loop's second turn)
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,k,B,Fin,K,Fout', [
    (360, 8, 515, 8, 3, 8),           # NW 12, PL 16, two workgroups per CU: 512 slots, three workgroups take a second window
    (360, 8, 515, 32, 10, 32),        # NW 12, PL 16, one workgroup per CU: 256 slots, two full rounds and three windows more
    (100, 8, 515, 32, 3, 32),         # NW 8
    (224, 8, 515, 16, 10, 16),        # NW 8, ML 20
    (360, 8, 150, 32, 16, 32),        # split, K = 16: 96 256 bytes of LDS, one workgroup per CU: 256 slots for 300 half-windows
    (150, 10, 150, 17, 16, 9),        # ... NW 8, ML 20
], ids=lambda v: str(v))
def test_second_window_per_workgroup(dev, lib, cus, N, k, B, Fin, K, Fout):
    """``for (b = blockIdx.x / NS; b < B; b += gridDim.x / NS)`` taking a second (and third) turn: the LDS image, the register-held
    operator row and Ws re-used by the next window.  Every window compared; random data, so windows b and b + gridDim / NS
    differ."""
    op = synthetic_checked(N, k)
    case = Layer(dev, lib, cus, op, B, Fin, K, Fout, 'vertex', True, seed=2)
    lds, slots, want = launch_geometry(op.nw, case.pl, K, B, cus)
    assert lds <= 160 * 1024 and want > slots, 'a single-turn launch: %d workgroups wanted, %d slots' % (want, slots)
    case.check('second_N%d_B%d_K%d' % (N, B, K))


# ------------------------------------------------------------------------------------
# a non-symmetric operator: L~ forward, L~^T backward, ML of each
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [B_SPLIT, B_WHOLE], ids=['split', 'whole'])
@pytest.mark.parametrize('transposed', [False, True], ids=['A', 'At'])
@pytest.mark.parametrize('M', [200, 300])
def test_non_symmetric_operator(dev, lib, cus, M, transposed, B):
    """The forward reads fwd.fs_rec and takes ML from the longest ROW, the backward adj.fs_rec and the longest COLUMN: rows of
    5 (ML 16) against a column of 19 (ML 20), and the transpose.  A symmetric Laplacian cannot tell them apart; this one does
    (the float64 result of the transposed operator is farther than 1e-3 of the scale from what the kernels return)."""
    op = ring(M, transposed)
    want = (19, 5) if transposed else (5, 19)
    assert (op.len_fwd, op.len_adj) == want and op.data.size == 4 * M + 15, (op.len_fwd, op.len_adj, op.data.size)
    Lt = sp.csr_matrix((op.data, op.indices, op.indptr), shape=(M, M))
    assert abs(Lt - Lt.T).max() > 0.05
    case = Layer(dev, lib, cus, op, B, 6, 4, 7, 'filter', True, seed=3)
    assert case.fwd_name().startswith('fused_layer_kernel<%d,%d,false,%d>' % (8 if M == 200 else 12, case.pl, 20 if transposed else 16))
    assert case.bwd_name() == 'fused_layer_kernel<%d,%d,true,%d>' % (8 if M == 200 else 12, case.pl, 16 if transposed else 20)
    case.check('ring_M%d_%s_B%d' % (M, 'At' if transposed else 'A', B))
    # the test can tell the operator from its transpose
    out = Guarded((B, 7, op.Mp), torch.float32, dev)
    dx = Guarded((B, 6, op.Mp), torch.float32, dev)
    ws = Guarded((max(case.nws // 4, 1),), torch.float32, dev)
    assert case.forward(None, out.t, None, ws.t) == 0 and case.backward(dx.t) == 0
    act_t, y_t, dx_t = case._refs_with(case.D.T.contiguous())
    assert float((out.t[..., :M].to(F64) - act_t).abs().max()) > 1e-3 * float(y_t.abs().max())
    assert float((dx.t[..., :M].to(F64) - dx_t).abs().max()) > 1e-3 * float(dx_t.abs().max())


# ------------------------------------------------------------------------------------
# K edges
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [3, B_WHOLE], ids=['split', 'whole'])
@pytest.mark.parametrize('N,k', [(100, 8), (330, 10)], ids=['nw8', 'nw12'])
@pytest.mark.parametrize('K', [1, 2, 3])
def test_small_K(dev, lib, cus, K, N, k, B):
    """K = 1: no step, the image is written and never read (out = W_0 x, dx = W_0 dy); K = 2: the first step is the last;
    K = 3: one step of each kind."""
    Layer(dev, lib, cus, synthetic_checked(N, k), B, 9, K, 10, 'vertex', True, seed=4).check('K%d_N%d_B%d' % (K, N, B), alias=True)


@pytest.mark.parametrize('N,k,K', [(360, 8, 27), (224, 8, 32)])
def test_K_beyond_the_lds_limit_is_declined(dev, lib, cus, N, k, K):
    op = synthetic_checked(N, k)
    assert launch_geometry(op.nw, 16, K - 1, 1, cus)[0] <= 160 * 1024 < launch_geometry(op.nw, 16, K, 1, cus)[0]
    for B in (3, B_WHOLE):
        Layer(dev, lib, cus, op, B, 4, K, 4, 'none', False).declined('K%d_B%d' % (K, B))


@pytest.mark.parametrize('B', [B_WHOLE, 3], ids=['whole', 'split'])
@pytest.mark.parametrize('N,k,K', [(360, 8, 26), (224, 8, 31)], ids=['nw12_K26', 'nw8_K31'])
def test_lds_limit(dev, lib, cus, N, k, K, B):
    """The largest K that ``fs_lds(nw, 16, K) <= 160 KB`` admits: K = 26 at twelve waves (161 792 bytes), K = 31 at eight, where
    the one-workgroup launch asks for all 163 840 bytes of a CU's LDS.  Served shapes, launched once each."""
    op = synthetic_checked(N, k)
    case = Layer(dev, lib, cus, op, B, 32, K, 32, 'vertex', True, seed=5)
    lds = launch_geometry(op.nw, 16, K, B, cus)[0]
    assert lds == (161792 if K == 26 else 163840)
    case.check('ldslimit_N%d_K%d_B%d' % (N, K, B))


# ------------------------------------------------------------------------------------
# filter edges: the plane-prefix counts nacc_fout / nst_fin, the half of a split window that owns no input plane
# ------------------------------------------------------------------------------------

FILTERS = [(1, 1), (1, 32), (32, 1), (3, 17), (4, 4), (5, 3), (16, 16), (17, 8), (31, 31), (32, 32), (8, 15), (15, 5)]


@pytest.mark.parametrize('B', [4, 193], ids=['split', 'whole'])
@pytest.mark.parametrize('N,k', [(246, 8), (224, 8)], ids=['nw12_ml16', 'nw8_ml20'])
@pytest.mark.parametrize('Fin,Fout', FILTERS, ids=['%dx%d' % f for f in FILTERS])
def test_filter_edges(dev, lib, cus, Fin, Fout, N, k, B):
    """Fin / Fout of 1, 3, 4, 5, 8, 15, 16, 17, 31, 32: with PL = 8 workgroup sp owns the planes 4 sp + {0..3, 8..11, 16..19,
    24..27}: Fin <= 4 leaves sp = 1 with no input plane at all, Fin = 5 with one; accumulator rows pu(r) + 4 h past Fout are
    neither biased, stored nor masked.  193: the smallest batch that is not split on 256 CUs."""
    case = Layer(dev, lib, cus, synthetic_checked(N, k), B, Fin, 3, Fout, 'vertex', True, seed=6)
    assert case.split == (2 if B == 4 else 1)
    case.check('filters_%dx%d_N%d_B%d' % (Fin, Fout, N, B))


@pytest.mark.parametrize('Fin,Fout', [(33, 8), (8, 33)])
def test_more_than_32_filters_declined(dev, lib, cus, Fin, Fout):
    for B in (4, 193):
        Layer(dev, lib, cus, synthetic_checked(246, 8), B, Fin, 3, Fout, 'filter', True).declined('filters_%dx%d_B%d' % (Fin, Fout, B))


# ------------------------------------------------------------------------------------
# vertex edges
# ------------------------------------------------------------------------------------

VERTICES = [(32, 8, 16), (64, 8, 16), (256, 8, 16), (384, 8, 16), (384, 10, 20), (257, 8, 16), (353, 10, 20)]


@pytest.mark.parametrize('B', [B_SPLIT, B_WHOLE], ids=['split', 'whole'])
@pytest.mark.parametrize('M,k,ml', VERTICES, ids=['M%d_k%d_ml%d' % v for v in VERTICES])
def test_vertex_edges(dev, lib, cus, M, k, ml, B):
    """M == Mp (no pad) at 32, 64, 256 (eight full waves), 384 (twelve); M = Mp - 31 at Mp = 288 and 384 (the last wave holds one
    vertex); three isolated vertices (1, M / 2 and the LAST one) with data in x and dout."""
    op = knn(M, k, isolated=(1, M // 2, M - 1))
    assert op.Mp == (M if M % 32 == 0 else M + 31)
    assert Operator.ml(op.len_fwd) == ml == Operator.ml(op.len_adj), (op.len_fwd, op.len_adj)
    assert all(op.rows[v] == 0 and op.cols[v] == 0 for v in (1, M // 2, M - 1)) and int((op.rows == 0).sum()) == 3
    Layer(dev, lib, cus, op, B, 12, 4, 20, 'vertex', True, seed=7).check('vertices_M%d_k%d_B%d' % (M, k, B))


# ------------------------------------------------------------------------------------
# epilogues
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [B_SPLIT, B_WHOLE], ids=['combine', 'one_workgroup'])
@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('bias_kind', ['none', 'filter', 'vertex'])
def test_epilogues(dev, lib, cus, bias_kind, relu, B):
    """bias none / per filter / per vertex x ReLU off / on, in fused_combine_kernel and in the one-workgroup epilogue (ballot
    mask bytes); each also with ``stack == x``."""
    Layer(dev, lib, cus, synthetic_checked(360, 8), B, 10, 3, 13, bias_kind, relu, seed=8).check(
        'epilogue_%s_relu%d_B%d' % (bias_kind, relu, B), alias=True)


# ------------------------------------------------------------------------------------
# through ops.cheb_conv
# ------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,bias_kind', [(300, 'vertex'), (8, 'filter')])
def test_through_cheb_conv(dev, lib, cus, B, bias_kind):
    """Autograd forward + backward of ops.cheb_conv on an ML 20 graph reach the fused kernels (dispatch log): B = 300 takes a
    second window per workgroup (K = 10: one workgroup per CU), B = 8 the split path.  out, dx against float64 at the bounds
    above; dW and dbias (the library's separate gradient kernels, fed by the fused forward's stack and mask) at GREL of their
    largest element, the project's bound for gradients (fp32 sums of B M terms of either sign: a few 2^-24 of their scale).
    The ReLU gate of the reference is the kernel's own ``out > 0`` (a pre-activation within round-off of 0 must not enter)."""
    from gcn_fmri_decoding_amd import _lib, ops
    op = synthetic_checked(330, 10)
    g = device_graph(op, dev)
    M, Mp, Fin, K, Fout = op.M, op.Mp, 15, 10, 32
    case = Layer(dev, lib, cus, op, B, Fin, K, Fout, bias_kind, True, seed=9)
    if B == 300:
        _, slots, want = launch_geometry(op.nw, 16, K, B, cus)
        assert case.split == 1 and want > slots
    x = case.x.clone()
    x[..., M:] = 0.0
    bias = case.bias.clone()
    if bias_kind == 'vertex':
        bias[:, M:] = 0.0
    gout = case.dout.clone()
    gout[..., M:] = 0.0
    x.requires_grad_(True)
    W = case.W.clone().requires_grad_(True)
    bias.requires_grad_(True)
    _lib.dispatch_log = log = []
    try:
        out = ops.cheb_conv(x, W, bias, g, K, relu=True, bias_kind=BIAS[bias_kind])
        out.backward(gout)
    finally:
        _lib.dispatch_log = None
    torch.cuda.synchronize()
    assert ('fused_layer_fwd', case.fwd_name()) in log and ('fused_layer_bwd_x', case.bwd_name()) in log, log
    assert not any(w.startswith('recurrence') for w, _ in log), log
    x64, W64 = x.detach()[..., :M].to(F64), W.detach().to(F64)
    b64 = bias.detach().to(F64) if bias_kind == 'filter' else bias.detach()[:, :M].to(F64)
    y, act, T = ref_forward(case.D, x64, W64, K, b64, True)
    got = {'out': plane_error(out.detach()[..., :M], act, y, REL, 'cheb_conv out')}
    gate = out.detach()[..., :M] > 0
    dy = torch.where(gate, gout[..., :M].to(F64), torch.zeros((), dtype=F64, device=dev))
    dref = ref_backward(case.D, dy, None, W64, Fin, K)
    got['dx'] = plane_error(x.grad[..., :M], dref, dref, GREL, 'cheb_conv dx')
    dW = torch.einsum('kbfm,bom->fko', T, dy).reshape(Fin * K, Fout)
    db = dy.sum((0, 2)) if bias_kind == 'filter' else dy.sum(0)
    gb = bias.grad if bias_kind == 'filter' else bias.grad[:, :M]
    for name, g_, r_ in (('dW', W.grad, dW), ('dbias', gb, db)):
        assert bool(torch.isfinite(g_).all())
        got[name] = float((g_.to(F64) - r_).abs().max() / r_.abs().max())
        print('cheb_conv %s: %.3e' % (name, got[name]))
        assert got[name] <= GREL, '%s: %.3e' % (name, got[name])
    record_measured('fused_layer_arms[cheb_conv_B%d]' % B, **got)
