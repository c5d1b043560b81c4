"""PyTorch-ROCm face of libchebgcn.so: device graph handles, plane-layout helpers and the
``torch.autograd.Function`` wrappers around the HIP kernels.  PyTorch supplies device
memory, streams and autograd bookkeeping; every arithmetic op of the graph-convolution
path runs in the library (there is no torch / CPU fallback -- a missing library or a
failing call raises).

Plane layout: the reference's activation ``x[N, M, F]`` (models_gcn.py:588) is kept as a
contiguous *storage* tensor ``[N, F, Mp]`` (vertex axis fastest, ``Mp = plane_stride(M)``).
``plane_view(storage, M)`` exposes it with the reference's logical shape ``[N, M, F]``
without copying; ``plane_storage(x)`` goes back (zero-copy when ``x`` is such a view).
"""
import collections
import ctypes as C
import os
import weakref

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from . import graph as _graph
from ._lib import BIAS_FILTER, BIAS_NONE, BIAS_VERTEX, POOL_AVG, POOL_MAX, plane_stride


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class KernelTimers:
    """Optional per-launch HIP-event timing of the hot kernels (used by bench.py for the
    roofline line).  Events are recorded on the stream the kernel is launched on; nothing
    is synchronised until ``summary()``.  Disabled (``timers is None``) by default."""

    def __init__(self, every=1, by_dispatch=False):
        self.records = {}           # name -> list of (start, end, algorithmic bytes, flops)
        # by_dispatch: one entry per (op, kernel template chebgcn_last_dispatch() reported) instead of one per op -- a
        # network whose layers differ in size runs the same op on different kernels
        self.by_dispatch = bool(by_dispatch)
        # An event pair per launch costs ~5 % of a training step (the markers keep consecutive
        # kernels from overlapping): with ``every = n`` only every n-th step is instrumented.
        # The caller announces steps with ``next_step()``.
        self.every = max(1, int(every))
        self.steps = 0
        self.sampled_steps = 0
        self.active = True

    def next_step(self):
        self.active = self.steps % self.every == 0
        self.sampled_steps += int(self.active)
        self.steps += 1

    def launch(self, name, nbytes, flops, fn):
        if not self.active:
            return fn()
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        rc = fn()
        end.record()
        if self.by_dispatch:
            name = '%s | %s' % (name, _lib.last_dispatch())
        self.records.setdefault(name, []).append((start, end, nbytes, flops))
        return rc

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _, _ in recs]
            out[name] = {'launches': len(recs), 'total_ms': float(sum(ms)), 'avg_ms': float(sum(ms) / len(ms)),
                         'bytes': float(sum(r[2] for r in recs)), 'flops': float(sum(r[3] for r in recs))}
        return out


timers = None
bf16_dy16 = True             # 'bf16' wide layers: dy handed to the two contraction gradients as bf16 (chebgcn_relu_grad_bf16); same results
fold_relu_grad = True        # pool == 1 layers: ReluGrad inside chebgcn_contract_bwd_*_relu (False: separate brelu_pool_bwd pass)
# atlas-sized graphs: recurrence + contraction (and the gradient wrt the input) as one on-chip launch per layer
fused_small = os.environ.get('CHEBGCN_FUSED_SMALL', '1') != '0' 
# contract_bwd_w on a second stream beside contract_bwd_x / recurrence_bwd (dW feeds neither).  'auto' (default since round 6):
# only for layers of more than 32 filters (both gradients are long matrix-bound kernels that share a CU well -- config-4 /
# config-5 layer 2 % faster with it in split bf16, 8 % in fp32).  For 32-filter layers the weight gradient cannot start
# beside the recurrence (one 160 KB workgroup per CU) and then shares HBM with the input gradient's contraction: measured in
# round 6 with the weight gradient on two workgroups per CU, same box -- configs[1] 3.14 ms with the second stream, 3.08 without;
# the captured atlas step (N = 360) 0.82 -> 0.76 ms, N = 1000 1.95 -> 1.88 ms (EXPERIMENTS 8.6).  True / False force it.
# Never on instrumented steps, whose per-kernel event times must not include a neighbour.
overlap_bwd_w = {'1': True, '0': False}.get(os.environ.get('CHEBGCN_OVERLAP_BWD_W', 'auto'), 'auto')
# d(loss)/dx of a layer with Fout <= Fin as  sum_k [T_k(L~^T) dy] W_k^T  -- the FORWARD recurrence on the planes of dy
# (chebgcn_recurrence_fwd_t, in place in slab 0 of the gradient stack), then the forward contraction kernel with the re-indexed
# weights -- instead of chebgcn_contract_bwd_x + chebgcn_recurrence_bwd (the same sum in Clenshaw form): as many bytes, on the two
# faster kernels (the stack of dy is written by a recurrence at 0.49 and read by a contraction at 0.64 of the HBM roofline
# instead of written by one at 0.55 and read by one at 0.43); False keeps the Clenshaw form everywhere
dx_by_forward = os.environ.get('CHEBGCN_DX_BY_FORWARD', '1') != '0'
bias_side_small = True       # fused atlas-size layers: the bias reduction on the second stream as well
_side_streams = {}


def _side_stream(dev):
    key = torch.device(dev).index
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=dev)
    return _side_streams[key]


def _launch(name, nbytes, flops, fn):
    """Run one C-ABI call, optionally bracketed by HIP events."""
    if timers is None:
        return fn()
    return timers.launch(name, nbytes, flops, fn)


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.ChebgcnError('chebgcn ops need ROCm device tensors; got a %s tensor '
                                    '(there is no CPU path)' % t.device)


# ------------------------------------------------------------------------------------
# device graph
# ------------------------------------------------------------------------------------

class Graph:
    """Device image of one Laplacian: ``rescale_L(L, lmax=2)`` and its transpose, as the
    constant sparse operand of the recurrence (models_gcn.py:590-596)."""

    def __init__(self, L, device=None, planes=0, order=None):
        """``planes``: planes a recurrence workgroup carries on chip -- 0 = automatic, 2 or 4
        (chebgcn_graph_create_planes; a choice of speed, not of results).  ``order``: relabel the vertices first
        (``graph.permute(L, order)``; with ``graph.length_order(L)`` the library runs its ordered recurrence kernels,
        ``query(12) == 1``): every plane this graph is used with is then in that vertex order."""
        self.M = int(L.shape[0])
        self.Mp = plane_stride(self.M)
        if not planes:
            planes = int(os.environ.get('CHEBGCN_PLANES', '0'))      # A/B experiments (tools/ab_bench.sh): 2 or 4 for every graph
        if order is not None:
            L = _graph.permute(L, np.asarray(order, np.int64))
        indptr, indices, data = _graph.rescaled_laplacian_csr(L)
        self.nnz = int(len(data))
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = _lib.lib().chebgcn_graph_create_planes(self.M, self.nnz, indptr.ctypes.data_as(C.c_void_p),
                                                        indices.ctypes.data_as(C.c_void_p),
                                                        data.ctypes.data_as(C.c_void_p), int(planes), C.byref(handle))
        _lib.check(rc, 'graph_create')
        self.handle = handle
        self._ordered = None
        self._finalizer = weakref.finalize(self, _lib.lib().chebgcn_graph_destroy, handle)

    def query(self, what):
        v = C.c_int64()
        _lib.check(_lib.lib().chebgcn_graph_query(self.handle, what, C.byref(v)), 'graph_query')
        return v.value

    @property
    def on_chip(self):
        return bool(self.query(3))

    @property
    def ordered(self):
        """Rows sorted by descending length and a kernel shape that serves the graph: the recurrence runs on the ordered
        kernels (csrc/recurrence_ord_kernel.h)."""
        if self._ordered is None:
            self._ordered = bool(self.query(12))
        return self._ordered


_graph_cache = weakref.WeakValueDictionary()


def graph_for(L, device=None):
    """Cache of device graphs keyed by the identity of the SciPy matrix and the device."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    key = (id(L), dev)
    g = _graph_cache.get(key)
    if g is None or g.M != L.shape[0]:
        g = Graph(L, torch.device('cuda', dev))
        _graph_cache[key] = g
        # keep the graph alive as long as the matrix object is
        try:
            L._chebgcn_graphs = getattr(L, '_chebgcn_graphs', {})
            L._chebgcn_graphs[dev] = g
        except AttributeError:
            pass
    return g


# ------------------------------------------------------------------------------------
# plane layout helpers
# ------------------------------------------------------------------------------------

def plane_empty(B, F, M, device, zero=False):
    Mp = plane_stride(M)
    return (torch.zeros if zero else torch.empty)((B, F, Mp), dtype=torch.float32, device=device)


def plane_view(storage, M):
    """[B, F, Mp] storage -> logical [B, M, F] view (no copy)."""
    return storage[:, :, :M].permute(0, 2, 1)


def _is_plane_view(x):
    if x.dim() != 3 or x.dtype != torch.float32:
        return False
    B, M, F = x.shape
    Mp = plane_stride(M)
    if x.stride() != (F * Mp, 1, Mp):
        return False
    need = (x.storage_offset() + B * F * Mp) * 4
    return x.untyped_storage().nbytes() >= need


def plane_storage(x):
    """Logical [B, M, F] tensor -> contiguous [B, F, Mp] storage.  Zero-copy for tensors
    produced by ``plane_view``; otherwise one layout-change kernel (to_plane)."""
    _require_cuda(x)
    B, M, F = x.shape
    Mp = plane_stride(M)
    if _is_plane_view(x):
        return x.as_strided((B, F, Mp), (F * Mp, Mp, 1))
    return ToPlane.apply(x)


class ToPlane(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous().float()
        B, M, F = x.shape
        out = plane_empty(B, F, M, x.device)
        _lib.check(_lib.lib().chebgcn_to_plane(_p(x), _p(out), B, M, F, _stream()), 'to_plane')
        ctx.shape = (B, M, F)
        return out

    @staticmethod
    def backward(ctx, g):
        B, M, F = ctx.shape
        g = g.contiguous()
        out = torch.empty((B, M, F), dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().chebgcn_from_plane(_p(g), _p(out), B, M, F, _stream()), 'from_plane')
        return out


def from_plane(storage, M):
    """[B, F, Mp] storage -> contiguous [B, M, F] tensor in the reference layout."""
    storage = storage.contiguous()
    B, F, Mp = storage.shape
    out = torch.empty((B, M, F), dtype=torch.float32, device=storage.device)
    _lib.check(_lib.lib().chebgcn_from_plane(_p(storage), _p(out), B, M, F, _stream()), 'from_plane')
    return out


def perm_data(x, perm, sample=None, out=None):
    """GPU ``coarsening.perm_data_3d`` (+ batch gather): x[S_total, N, F] (device, row
    layout), perm int32 [M] on device, optional sample indices -> storage [S, F, Mp]."""
    _require_cuda(x, perm, sample)
    x = x.contiguous()
    S_total, N, F = x.shape
    M = int(perm.numel())
    S = S_total if sample is None else int(sample.numel())
    if out is None:
        out = plane_empty(S, F, M, x.device)
    _lib.check(_lib.lib().chebgcn_perm_data(_p(x), _p(perm), _p(sample), _p(out), S, N, M, F, _stream()), 'perm_data')
    return out


def _windows_out(out, n, sample, C, planes):
    """``(B, out)`` of a gather of ``sample`` (None: all ``n``) windows: ``out`` where it is contiguous ``[B, C, Mp]``, else new."""
    shape = (int(n if sample is None else sample.numel()), C, planes.shape[1])
    if out is None or tuple(out.shape) != shape or not out.is_contiguous():
        out = torch.empty(shape, dtype=torch.float32, device=planes.device)
    return shape[0], out


def _mix_tables(tab, cnt, what, name):
    """``(S', smax)`` of the tables of a plan: ``tab`` contiguous int64 ``[S', smax]``, ``cnt`` int32 ``[S']``."""
    if tab.dim() != 2 or cnt.dim() != 1 or tab.shape[0] != cnt.shape[0] or tab.dtype != torch.int64 \
            or cnt.dtype != torch.int32 or not tab.is_contiguous() or not cnt.is_contiguous():
        raise _lib.ChebgcnError('%s: %s must be contiguous int64 [S, smax] and cnt int32 [S]' % (what, name))
    return int(tab.shape[0]), int(tab.shape[1])


def _stats_launch(what, planes, M, C, nbytes, traffic, entry, *head):
    """What the statistics entries share: the outputs ``mean, var`` float64 and ``scale, shift`` float32, ``[C, Mp]`` each, the
    workspace, and the launch ``entry(*head, mean, var, scale, shift, M, C, workspace, its bytes, stream)``."""
    kinds = (torch.float64, torch.float64, torch.float32, torch.float32)
    outs = tuple(torch.empty((C, planes.shape[1]), dtype=dt, device=planes.device) for dt in kinds)
    ws = _workspace(int(nbytes), planes.device, what)
    _lib.check(_launch(what, traffic, 0.0, lambda: entry(*head, *map(_p, outs), M, C, _p(ws), ws.numel(), _stream())), what)
    return outs


def gather_windows(planes, rows, M, C, sample=None, scale=None, shift=None, out=None):
    """Windows of a staged series (chebgcn_gather_windows): ``planes`` [Ttot, Mp] fp32 (internal vertex order, zero pad),
    ``rows`` int64 device table of the windows' first rows, ``sample`` int32 device indices into it (None: all of them, in
    order) -> storage [B, C, Mp]; ``scale`` / ``shift`` [C, Mp]: ``x * scale + shift`` in two roundings.  ``out``: a buffer of
    that shape."""
    _require_cuda(planes, rows, sample, scale, shift, out)
    Ttot, Mp = planes.shape
    B, out = _windows_out(out, rows.numel(), sample, C, planes)
    _lib.check(_launch('gather_windows', 8.0 * B * C * Mp, 0.0, lambda: _lib.lib().chebgcn_gather_windows(
        _p(planes), Ttot, _p(rows), _p(sample), _p(scale), _p(shift), _p(out), B, M, C, _stream())), 'gather_windows')
    return out


def gather_windows_mix(planes, rows, cnt, M, C, sample=None, scale=None, shift=None, out=None, sources=None):
    """Windows that are means of source windows (chebgcn_gather_windows_mix): ``rows`` int64 [S', smax] and ``cnt`` int32 [S']
    device tables (window ``w`` is the mean of the ``cnt[w]`` windows that start at ``rows[w, :cnt[w]]``: float32 adds in that
    order, one rounded division, then the tables), otherwise ``gather_windows``.  ``sources``: the mean ``cnt`` of the
    windows gathered, for the launch log's byte count (None: ``smax``)."""
    _require_cuda(planes, rows, cnt, sample, scale, shift, out)
    Ttot, Mp = planes.shape
    W, smax = _mix_tables(rows, cnt, 'gather_windows_mix', 'rows')
    B, out = _windows_out(out, W, sample, C, planes)
    nsrc = float(smax if sources is None else sources)
    _lib.check(_launch('gather_windows_mix', 4.0 * (nsrc + 1) * B * C * Mp, 0.0, lambda: _lib.lib().chebgcn_gather_windows_mix(
        _p(planes), Ttot, _p(rows), _p(cnt), smax, _p(sample), _p(scale), _p(shift), _p(out), B, M, C, _stream())),
        'gather_windows_mix')
    return out


def window_stats(planes, rows, M, C):
    """Per (channel, vertex) statistics over the windows ``rows`` of a staged series (chebgcn_window_stats), none of them
    built: ``(mean, var)`` float64 and ``(scale, shift)`` float32, all [C, Mp] on the device, internal vertex order."""
    _require_cuda(planes, rows)
    Ttot, Mp = planes.shape
    lib = _lib.lib()
    return _stats_launch('window_stats', planes, M, C, lib.chebgcn_window_stats_workspace(Ttot, M, C), 4.0 * Ttot * Mp,
                         lib.chebgcn_window_stats, _p(planes), Ttot, _p(rows), int(rows.numel()))


def _index_table(idx, M, C, fold, what):
    if idx.dim() != 2 or idx.dtype != torch.int64 or not idx.is_contiguous() or idx.shape[0] < 1 \
            or isinstance(fold, bool) or not isinstance(fold, (int, np.integer)) or not 1 <= fold <= 16 \
            or idx.shape[1] != int(C) * int(fold):
        raise _lib.ChebgcnError('%s: idx must be contiguous int64 [S, C * fold] with fold in [1, 16] (C = %r, fold = %r, got %s %s)'
                                % (what, C, fold, idx.dtype, tuple(idx.shape)))
    return int(idx.shape[0]), int(idx.shape[1])


def gather_windows_indexed(planes, idx, M, C, fold=1, src=None, cnt=None, sample=None, scale=None, shift=None, out=None,
                           sources=None):
    """Windows that are lists of rows (chebgcn_gather_windows_indexed): ``idx`` int64 [S, C * fold] device table of rows of
    ``planes`` (channel ``c`` of window ``s`` is the float32 mean of the rows ``idx[s, f * C + c]``), ``src`` int64 [S', smax] /
    ``cnt`` int32 [S'] (both or neither): output window ``w`` is the mean of the ``cnt[w]`` windows ``src[w, :cnt[w]]`` of
    ``idx``; ``sample`` int32 device indices (None: all, in order) -> storage [B, C, Mp], then the tables like
    ``gather_windows``.  ``sources``: the mean ``cnt`` of the windows gathered, for the launch log's byte count."""
    _require_cuda(planes, idx, src, cnt, sample, scale, shift, out)
    Ttot, Mp = planes.shape
    S, Cin = _index_table(idx, M, C, fold, 'gather_windows_indexed')
    if (src is None) != (cnt is None):
        raise _lib.ChebgcnError('gather_windows_indexed: src and cnt come together (both or neither)')
    W, smax = (S, 1) if src is None else _mix_tables(src, cnt, 'gather_windows_indexed', 'src')
    B, out = _windows_out(out, W, sample, C, planes)
    nsrc = float(fold) * float((smax if src is not None else 1) if sources is None else sources)
    _lib.check(_launch('gather_windows_indexed', 4.0 * (nsrc + 1) * B * C * Mp, 0.0,
                       lambda: _lib.lib().chebgcn_gather_windows_indexed(
                           _p(planes), Ttot, _p(idx), S, Cin, int(fold), _p(src), _p(cnt), W, smax, _p(sample), _p(scale),
                           _p(shift), _p(out), B, M, C, _stream())), 'gather_windows_indexed')
    return out


def window_stats_indexed(planes, idx, M, C, fold=1):
    """``window_stats`` over windows that are lists of rows (chebgcn_window_stats_indexed; ``idx`` as in
    ``gather_windows_indexed``): the statistics of the folded float32 values the gather forms."""
    _require_cuda(planes, idx)
    Ttot, Mp = planes.shape
    S, Cin = _index_table(idx, M, C, fold, 'window_stats_indexed')
    lib = _lib.lib()
    return _stats_launch('window_stats_indexed', planes, M, C, lib.chebgcn_window_stats_indexed_workspace(S, M, C),
                         4.0 * S * Cin * Mp, lib.chebgcn_window_stats_indexed, _p(planes), Ttot, _p(idx), S, Cin, int(fold))


def gather_windows_reflect(planes, rows, tshift, M, C, sample=None, scale=None, shift=None, out=None):
    """``gather_windows`` with a time shift per window (chebgcn_gather_windows_reflect): ``tshift`` int32 device table indexed
    like ``rows`` (None: no shift), channel ``c`` of window ``w`` is plane ``rho(c + tshift[w])`` of the window's ``C`` planes,
    ``rho`` the symmetric reflection (``series.reflect_channels``); the tables are those of the output channel."""
    _require_cuda(planes, rows, tshift, sample, scale, shift, out)
    Ttot, Mp = planes.shape
    if tshift is not None and (tshift.dtype != torch.int32 or tshift.dim() != 1 or tshift.numel() != rows.numel()
                               or not tshift.is_contiguous()):
        raise _lib.ChebgcnError('gather_windows_reflect: tshift must be contiguous int32, one entry per row of the table')
    B, out = _windows_out(out, rows.numel(), sample, C, planes)
    _lib.check(_launch('gather_windows_reflect', 8.0 * B * C * Mp, 0.0, lambda: _lib.lib().chebgcn_gather_windows_reflect(
        _p(planes), Ttot, _p(rows), _p(tshift), _p(sample), _p(scale), _p(shift), _p(out), B, M, C, _stream())),
        'gather_windows_reflect')
    return out


def window_drop(x, win, M, D, seed, refill, pos=None, scale=None, shift=None, drop_value=1.0):
    """Vertex dropout in place on a gathered batch (chebgcn_window_drop): ``x`` contiguous storage [B, C, Mp], ``win`` int32
    device [B] the augmented-set index of every row, ``D`` draws per window out of the ``M`` vertices
    (``series.drop_vertices(seed, refill, win[b], D, M)``), ``pos`` int32 device [M] caller vertex -> position in ``x`` (None:
    the identity).  The drawn vertices take ``drop_value`` in every channel, seen through ``scale`` / ``shift`` [C, Mp] where
    given (a rounded product, then a rounded sum).  Writes ``B * D * C`` floats and nothing else; returns ``x``."""
    _require_cuda(x, win, pos, scale, shift)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[2] != plane_stride(M):
        raise _lib.ChebgcnError('window_drop: x must be contiguous float32 plane storage [B, C, Mp(M = %d)], got %s %s'
                                % (M, x.dtype, tuple(x.shape)))
    B, C, Mp = x.shape
    if win.dtype != torch.int32 or win.dim() != 1 or win.numel() != B or not win.is_contiguous():
        raise _lib.ChebgcnError('window_drop: win must be contiguous int32 [B = %d]' % B)
    if pos is not None and (pos.dtype != torch.int32 or pos.dim() != 1 or pos.numel() != M or not pos.is_contiguous()):
        raise _lib.ChebgcnError('window_drop: pos must be contiguous int32 [M = %d]' % M)
    for t in (scale, shift):
        if t is not None and (tuple(t.shape) != (C, Mp) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.ChebgcnError('window_drop: scale and shift must be contiguous float32 [C, Mp]')
    _lib.check(_launch('window_drop', 4.0 * B * int(D) * C, 0.0, lambda: _lib.lib().chebgcn_window_drop(
        _p(x), _p(win), B, M, C, int(D), int(seed), int(refill), _p(pos), _p(scale), _p(shift), float(drop_value), _stream())),
        'window_drop')
    return x


def knn(planes, N, k, metric):
    """The k nearest other vertices of every vertex (chebgcn_knn): ``planes`` [D, Np] fp32 feature-major planes on the device
    (zero pad), ``metric`` one of ``_lib.KNN_*`` -> ``(dist float32 [N, k] ascending, idx int32 [N, k])`` on the device.  The
    N x N matrix is never formed."""
    _require_cuda(planes)
    D, Np = planes.shape
    if Np != plane_stride(N) or planes.dtype != torch.float32 or not planes.is_contiguous():
        raise _lib.ChebgcnError('knn: planes must be contiguous float32 [D, plane_stride(N)]')
    dev = planes.device
    nbytes = int(_lib.lib().chebgcn_knn_workspace(N, D, k))
    ws = _workspace(nbytes, dev, 'knn')
    dist = torch.empty((N, k), dtype=torch.float32, device=dev)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    _lib.check(_launch('knn', 4.0 * D * Np + 8.0 * N * k, 2.0 * N * N * D, lambda: _lib.lib().chebgcn_knn(
        _p(planes), N, D, k, int(metric), _p(dist), _p(idx), _p(ws), ws.numel(), _stream())), 'knn')
    return dist, idx


def _staged_runs(planes, run_offsets, M, what):
    """``(Ttot, Mp, R)`` of staged runs: ``planes`` contiguous float32 [Ttot, plane_stride(M)], ``run_offsets`` int64 [R + 1]."""
    if planes.dim() != 2 or planes.shape[1] != plane_stride(M) or planes.dtype != torch.float32 or not planes.is_contiguous():
        raise _lib.ChebgcnError('%s: planes must be contiguous float32 [Ttot, plane_stride(M)]' % what)
    R = int(run_offsets.numel()) - 1
    if run_offsets.dtype != torch.int64 or run_offsets.dim() != 1 or R < 1 or not run_offsets.is_contiguous():
        raise _lib.ChebgcnError('%s: run_offsets must be a contiguous int64 vector of R + 1 entries' % what)
    return int(planes.shape[0]), int(planes.shape[1]), R


def series_normalise(planes, run_offsets, M, scale=1.0, out=None):
    """Every run of a staged series centred and scaled to norm ``scale`` per vertex inside that run
    (chebgcn_series_normalise): ``planes`` [Ttot, Mp] fp32, ``run_offsets`` int64 [R + 1] on the device (run r = rows
    [run_offsets[r], run_offsets[r + 1]), checked by the caller) -> [Ttot, Mp]; a vertex constant in a run is zero there."""
    _require_cuda(planes, run_offsets, out)
    Ttot, Mp, R = _staged_runs(planes, run_offsets, M, 'series_normalise')
    o = run_offsets.cpu().numpy()           # one small download: the kernel trusts the table, so it is checked here
    if o[0] != 0 or o[-1] != Ttot or (np.diff(o) < 1).any():
        raise _lib.ChebgcnError('series_normalise: run_offsets must ascend from 0 to Ttot')
    if out is None:
        out = torch.empty_like(planes)
    elif (out.shape != planes.shape or out.dtype != torch.float32 or not out.is_contiguous()
          or out.data_ptr() == planes.data_ptr()):
        raise _lib.ChebgcnError('series_normalise: out must be a contiguous float32 tensor shaped like planes, not planes itself')
    _lib.check(_launch('series_normalise', 16.0 * Ttot * Mp, 0.0, lambda: _lib.lib().chebgcn_series_normalise(
        _p(planes), Ttot, _p(run_offsets), R, M, float(scale), _p(out), _stream())), 'series_normalise')
    return out


def parcellate_geometry():
    """The constants of the parcellation kernels (chebgcn_parcellate_query), so that callers and tests follow the tile:
    ``tile`` floats of x a workgroup holds per chunk (a chunk is ``tile // rows`` vertices of every row), ``rows`` the row tile of
    the rows4 arm, ``wide_T`` the rows from which it runs, ``regions_per_pass``, ``max_grid`` workgroups of a launch,
    ``expand_grid_rows`` and ``expand_vec`` of the expand kernel."""
    q = _lib.lib().chebgcn_parcellate_query
    return {'tile': q(0), 'rows': q(1), 'wide_T': q(2), 'regions_per_pass': q(3), 'max_grid': q(4), 'expand_grid_rows': q(5),
            'expand_vec': q(6)}


def _rows_of(t, n, what):
    """Row stride (elements) of a 2-D float32 device tensor whose rows are contiguous over ``n`` values."""
    if t.dim() != 2 or t.shape[1] != n or t.dtype != torch.float32 or (n > 1 and t.stride(1) != 1):
        raise _lib.ChebgcnError('%s must be float32 [rows, %d] with contiguous rows' % (what, n))
    ld = int(t.stride(0)) if t.shape[0] > 1 else n
    if ld < n:
        raise _lib.ChebgcnError('%s: a row stride of %d elements is less than the %d values of a row' % (what, ld, n))
    return ld


def parcellate(x, ptr, idx, R, w=None, mode=_lib.PARCEL_MEAN, out=None):
    """A vertex-level run reduced to regions (chebgcn_parcellate): ``x`` float32 [T, V] on the device, rows contiguous (any row
    stride >= V: a view of some columns of a wider tensor is taken as it is), ``ptr`` int32 [R + 1] / ``idx`` int32 [nnz] the
    regions' member lists on the device (ascending inside a region; the caller checks them, the kernel trusts them), ``w``
    float32 [V] or None -> ``out`` float32 [T, R] (given: any row stride >= R).  Sums run in ascending member order, one
    rounded division: see include/chebgcn.h."""
    _require_cuda(x, ptr, idx, w, out)
    if x.dim() != 2:
        raise _lib.ChebgcnError('parcellate: x must be [T, V]')
    T, V = int(x.shape[0]), int(x.shape[1])
    ldx = _rows_of(x, V, 'parcellate: x')
    if (ptr.dtype != torch.int32 or idx.dtype != torch.int32 or ptr.dim() != 1 or idx.dim() != 1 or ptr.numel() != R + 1
            or not ptr.is_contiguous() or not idx.is_contiguous()):
        raise _lib.ChebgcnError('parcellate: ptr / idx must be contiguous int32 vectors of R + 1 / nnz entries')
    if w is not None and (w.dtype != torch.float32 or w.shape != (V,) or not w.is_contiguous()):
        raise _lib.ChebgcnError('parcellate: w must be a contiguous float32 vector of V entries')
    if out is None:
        out = torch.empty((T, R), dtype=torch.float32, device=x.device)
    elif out.shape[0] != T:
        raise _lib.ChebgcnError('parcellate: out has %d rows, x has %d' % (out.shape[0], T))
    ldo = _rows_of(out, R, 'parcellate: out')
    if T == 0:
        return out
    _lib.check(_launch('parcellate', 4.0 * T * V + 4.0 * T * R, float(T) * idx.numel(), lambda: _lib.lib().chebgcn_parcellate(
        _p(x), ldx, _p(ptr), _p(idx), idx.numel(), _p(w), _p(out), ldo, T, V, int(R), int(mode), _stream())), 'parcellate')
    return out


def parcel_expand(maps, region_of, fill=0.0, out=None):
    """Region maps back on the vertices (chebgcn_parcel_expand): ``maps`` float32 [B, R] and ``region_of`` int32 [V] (-1:
    background) on the device, both contiguous -> ``out`` float32 [B, V], ``out[b, v] = maps[b, region_of[v]]`` or ``fill``."""
    _require_cuda(maps, region_of, out)
    if maps.dim() != 2 or maps.dtype != torch.float32 or not maps.is_contiguous():
        raise _lib.ChebgcnError('parcel_expand: maps must be contiguous float32 [B, R]')
    if region_of.dim() != 1 or region_of.dtype != torch.int32 or not region_of.is_contiguous():
        raise _lib.ChebgcnError('parcel_expand: region_of must be a contiguous int32 vector')
    B, R = maps.shape
    V = int(region_of.numel())
    if out is None:
        out = torch.empty((B, V), dtype=torch.float32, device=maps.device)
    elif out.shape != (B, V) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.ChebgcnError('parcel_expand: out must be contiguous float32 [B, V]')
    if B == 0:
        return out
    _lib.check(_launch('parcel_expand', 4.0 * B * V + 4.0 * V + 4.0 * B * R, 0.0, lambda: _lib.lib().chebgcn_parcel_expand(
        _p(maps), _p(region_of), _p(out), B, R, V, float(fill), _stream())), 'parcel_expand')
    return out


def cheb_filter_workspace(graph, nplanes, K, J, arm=_lib.FILTER_AUTO):
    """Bytes of scratch ``cheb_filter`` takes for this launch (chebgcn_cheb_filter_workspace): two slabs of ``nplanes`` planes
    in the rolling arm, K in the stack arm; ``arm = 0`` answers for the arm the library would choose."""
    return int(_lib.lib().chebgcn_cheb_filter_workspace(graph.handle, int(nplanes), int(K), int(J), int(arm)))


def cheb_filter(graph, x, coeff, arm=_lib.FILTER_AUTO, out=None):
    """``y[j] = sum_k coeff[j, k] T_k(L~) x`` (chebgcn_cheb_filter): ``x`` contiguous float32 plane storage ``[..., Mp]`` in the
    graph's vertex order (every leading axis counts planes), ``coeff`` float32 ``[J, K]`` on the device, 1 <= J <= 8,
    1 <= K <= 256 -> ``out`` float32 ``[J, ..., Mp]``.  ``arm``: 0 automatic, 1 rolling (two work slabs, any graph), 2 stack (K
    slabs, the on-chip / ordered recurrence kernels).  x is not written; the pad of ``out`` is scratch."""
    _require_cuda(x, coeff, out)
    Mp = graph.Mp
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] != Mp or not x.is_contiguous() or x.numel() == 0:
        raise _lib.ChebgcnError('cheb_filter: x must be contiguous float32 planes [..., %d]' % Mp)
    if coeff.dtype != torch.float32 or coeff.dim() != 2 or not coeff.is_contiguous():
        raise _lib.ChebgcnError('cheb_filter: coeff must be a contiguous float32 [J, K] device tensor')
    J, K = int(coeff.shape[0]), int(coeff.shape[1])
    nplanes = x.numel() // Mp
    shape = (J,) + tuple(x.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.ChebgcnError('cheb_filter: out must be contiguous float32 %r' % (shape,))
    lib = _lib.lib()
    nws = int(lib.chebgcn_cheb_filter_workspace(graph.handle, nplanes, K, J, int(arm)))
    ws = _workspace(nws, x.device, 'cheb_filter') if nws else None
    slab = 4.0 * nplanes * Mp
    steps = max(K - 1, 1)
    _lib.check(_launch('cheb_filter', slab * (steps * (3 + 2 * J) + 1), 2.0 * nplanes * (graph.nnz * (K - 1) + graph.M * K * J),
                       lambda: lib.chebgcn_cheb_filter(graph.handle, _p(x), _p(coeff), _p(out), _p(ws), nplanes, K, J, int(arm),
                                                       _stream())), 'cheb_filter')
    return out


def cluster_geometry():
    """The limits of the permutation-inference kernels (chebgcn_cluster_query): ``onchip_M`` the largest M of the on-chip arm of
    ``cluster_enhance`` (LDS of a workgroup / ``state_bytes`` per vertex), ``max_S`` subjects, ``max_M`` vertices, ``max_heights``,
    ``max_perms`` permutations of one call, ``state_bytes`` of state per (permutation, vertex)."""
    q = _lib.lib().chebgcn_cluster_query
    return {'onchip_M': q(0), 'max_S': q(1), 'max_M': q(2), 'max_heights': q(3), 'max_perms': q(4), 'state_bytes': q(5)}


def _vec(t, dtype, n, what):
    if t.dtype != dtype or t.dim() != 1 or t.numel() < n or not t.is_contiguous():
        raise _lib.ChebgcnError('%s must be a contiguous %s vector of at least %d entries' % (what, str(dtype).split('.')[-1], n))


def signflip_t(x, q, p0, Pb, seed, bits=None, out=None):
    """The sign-flip t maps of permutations ``p0 .. p0 + Pb - 1`` (chebgcn_signflip_t): ``x`` float32 [S, M] and ``q`` float64 [M]
    on the device -> float32 [Pb, M].  ``bits``: int32 [Pb, ceil(S / 32)] packed signs (bit set: negated), or None: the
    signs are drawn from ``(seed, permutation)`` and permutation 0 is the identity.  The arithmetic: include/chebgcn.h."""
    _require_cuda(x, q, bits, out)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.ChebgcnError('signflip_t: x must be contiguous float32 [S, M]')
    S, M = int(x.shape[0]), int(x.shape[1])
    _vec(q, torch.float64, M, 'signflip_t: q')
    Pb = int(Pb)
    if bits is not None and (bits.dtype != torch.int32 or tuple(bits.shape) != (Pb, (S + 31) // 32) or not bits.is_contiguous()):
        raise _lib.ChebgcnError('signflip_t: bits must be contiguous int32 words [%d, %d]' % (Pb, (S + 31) // 32))
    if out is None:
        out = torch.empty((Pb, M), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (Pb, M) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.ChebgcnError('signflip_t: out must be contiguous float32 [%d, %d]' % (Pb, M))
    _lib.check(_launch('signflip_t', 4.0 * Pb * M + 4.0 * S * M, 2.0 * Pb * M * S, lambda: _lib.lib().chebgcn_signflip_t(
        _p(x), _p(q), _p(bits), _p(out), S, M, int(p0) & 0xFFFFFFFF, Pb, int(seed) & 0xFFFFFFFF, _stream())), 'signflip_t')
    return out


def perm_glm_geometry(r=None):
    """The constants of ``perm_glm_t`` (chebgcn_perm_glm_query), so that callers and tests follow the tile: ``vertices`` and
    ``perms`` of a workgroup (at rank ``r``; None: the most at any rank), ``panel`` columns of Uf of one pass over e, ``max_r``
    / ``max_S`` / ``max_M`` served, ``max_perms`` of one call."""
    q = _lib.lib().chebgcn_perm_glm_query
    return {'vertices': q(0), 'perms': q(1 if r is None else 100 + int(r)), 'panel': q(2), 'max_r': q(3), 'max_S': q(4),
            'max_M': q(5), 'max_perms': q(6)}


def perm_glm_t(e, q, Uf, u, unorm2, dof, rows, out=None):
    """The t maps of one contrast under the permutations of a table (chebgcn_perm_glm_t): ``e`` float32 [S, M], ``q`` float64
    [M], ``Uf`` float64 [S, r], ``u`` float64 [r] and ``rows`` int32 [Pb, S] (the uint32 entries of ``stats.permutations``,
    reinterpreted) on the device, ``unorm2`` and ``dof`` numbers -> float32 [Pb, M].  The arithmetic: include/chebgcn.h."""
    _require_cuda(e, q, Uf, u, rows, out)
    if e.dim() != 2 or e.dtype != torch.float32 or not e.is_contiguous():
        raise _lib.ChebgcnError('perm_glm_t: e must be contiguous float32 [S, M]')
    S, M = int(e.shape[0]), int(e.shape[1])
    _vec(q, torch.float64, M, 'perm_glm_t: q')
    if Uf.dim() != 2 or Uf.dtype != torch.float64 or int(Uf.shape[0]) != S or not Uf.is_contiguous() or Uf.numel() == 0:
        raise _lib.ChebgcnError('perm_glm_t: Uf must be contiguous float64 [%d, r]' % S)
    r = int(Uf.shape[1])
    _vec(u, torch.float64, r, 'perm_glm_t: u')
    if rows.dim() != 2 or rows.dtype != torch.int32 or int(rows.shape[1]) != S or not rows.is_contiguous() or rows.numel() == 0:
        raise _lib.ChebgcnError('perm_glm_t: rows must be contiguous int32 words [Pb, %d]' % S)
    Pb = int(rows.shape[0])
    if out is None:
        out = torch.empty((Pb, M), dtype=torch.float32, device=e.device)
    elif tuple(out.shape) != (Pb, M) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.ChebgcnError('perm_glm_t: out must be contiguous float32 [%d, %d]' % (Pb, M))
    _lib.check(_launch('perm_glm_t', 4.0 * Pb * M + 4.0 * S * M, 4.0 * Pb * M * S * r, lambda: _lib.lib().chebgcn_perm_glm_t(
        _p(e), _p(q), _p(Uf), _p(u), float(unorm2), int(dof), _p(rows), _p(out), S, M, r, Pb, _stream())), 'perm_glm_t')
    return out


def cluster_enhance_workspace(Pb, M, mode, arm=_lib.CLUSTER_AUTO):
    """Bytes of scratch ``cluster_enhance`` takes (chebgcn_cluster_enhance_workspace): 0 on chip, ``state_bytes`` per
    (permutation, vertex) streamed."""
    return int(_lib.lib().chebgcn_cluster_enhance_workspace(int(Pb), int(M), int(mode), int(arm)))


def cluster_check(status):
    """Read the status word of ``cluster_enhance`` calls (synchronises) and raise what it reports."""
    code = int(status.item())
    if code:
        raise _lib.ChebgcnError('cluster_enhance: %s' % {
            _lib.CLUSTER_EHEIGHTS: 'a permutation has more heights than the tables hold',
            _lib.CLUSTER_ELOOP: 'a union-find loop ran past its bound'}.get(code, 'status %d' % code))


def cluster_enhance(t, mode, ptr=None, idx=None, hf=None, hw=None, ep=None, step=1.0, NH=1, negate=False, want_out=True,
                    want_labels=False, want_max=True, arm=_lib.CLUSTER_AUTO, status=None):
    """Cluster enhancement of a batch of t maps (chebgcn_cluster_enhance): ``t`` float32 [Pb, M] on the device, the graph as
    int32 CSR ``ptr`` [M + 1] / ``idx`` on the device, the tables ``hf`` float32 / ``hw`` float64 (at least NH + 1 entries) and
    ``ep`` float64 [M + 1].  Returns ``(out float64 [Pb, M] | None, labels int32 [Pb, M] | None, pmax float64 [Pb] | None)``.
    ``status``: an int32 [1] device tensor the caller zeroed and reads later with ``cluster_check`` (one synchronisation for many
    calls); None: the call checks its own and synchronises."""
    _require_cuda(t, ptr, idx, hf, hw, ep, status)
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
        raise _lib.ChebgcnError('cluster_enhance: t must be contiguous float32 [Pb, M]')
    Pb, M = int(t.shape[0]), int(t.shape[1])
    mode, NH = int(mode), int(NH)
    own = None
    if mode != _lib.CLUSTER_MAX:
        if NH < 1:
            raise _lib.ChebgcnError('cluster_enhance: NH = %d heights' % NH)
        _vec(ptr, torch.int32, M + 1, 'cluster_enhance: ptr')
        _vec(idx, torch.int32, 0, 'cluster_enhance: idx')
        _vec(hf, torch.float32, NH + 1, 'cluster_enhance: hf')
        _vec(hw, torch.float64, NH + 1, 'cluster_enhance: hw')
        _vec(ep, torch.float64, M + 1, 'cluster_enhance: ep')
        if status is None:
            status = own = torch.zeros(1, dtype=torch.int32, device=t.device)
        _vec(status, torch.int32, 1, 'cluster_enhance: status')
    lib = _lib.lib()
    nws = int(lib.chebgcn_cluster_enhance_workspace(Pb, M, mode, int(arm)))
    ws = _workspace(nws, t.device, 'cluster_enhance') if nws else None
    out = torch.empty((Pb, M), dtype=torch.float64, device=t.device) if want_out else None
    labels = torch.empty((Pb, M), dtype=torch.int32, device=t.device) if want_labels else None
    pmax = torch.empty((Pb,), dtype=torch.float64, device=t.device) if want_max else None
    nnz = int(idx.numel()) if idx is not None else 0
    _lib.check(_launch('cluster_enhance', 4.0 * Pb * M, 0.0, lambda: lib.chebgcn_cluster_enhance(
        _p(ptr), _p(idx), nnz, _p(t), int(bool(negate)), _p(hf), _p(hw), NH, _p(ep), float(step), _p(out), _p(labels), _p(pmax),
        _p(status), _p(ws), nws, Pb, M, mode, int(arm), _stream())), 'cluster_enhance')
    if own is not None:
        cluster_check(own)
    return out, labels, pmax


def glm_geometry():
    """The constants of the GLM kernels (chebgcn_glm_query), so that callers and tests follow the tile: ``vertices`` of a
    project workgroup, ``panel`` columns of Q of one pass over the scan, ``max_k`` / ``max_C`` / ``max_P`` served, ``split`` the
    run length from which the time loop is cut into slices, ``slice`` the least rows of a slice, ``slices`` at most, ``max_runs``
    of one call."""
    q = _lib.lib().chebgcn_glm_query
    return {'vertices': q(0), 'panel': q(1), 'max_k': q(2), 'max_C': q(3), 'split': q(4), 'slice': q(5), 'slices': q(6),
            'max_P': q(7), 'max_runs': q(8)}


def _dense(t, dtype, shape, what):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.ChebgcnError('%s must be a contiguous %s tensor %r, got %s %r' % (
            what, str(dtype).split('.')[-1], tuple(shape), str(t.dtype).split('.')[-1], tuple(t.shape)))


def glm_project(planes, run_offsets, M, Q):
    """The projections of every run on its design's orthonormal basis (chebgcn_glm_project): ``planes`` float32 [Ttot, Mp],
    ``run_offsets`` int64 [R + 1] and ``Q`` float64 [Ttot, k] on the device -> ``(a float64 [R, k, Mp], yy float64 [R, Mp])``
    in one workspace (the next call on the stream reuses it).  float64 FMA chains in ascending t: include/chebgcn.h."""
    _require_cuda(planes, run_offsets, Q)
    Ttot, Mp, R = _staged_runs(planes, run_offsets, M, 'glm_project')
    if Q.dim() != 2:
        raise _lib.ChebgcnError('glm_project: Q must be float64 [Ttot, k]')
    k = int(Q.shape[1])
    _dense(Q, torch.float64, (Ttot, k), 'glm_project: Q')
    lib = _lib.lib()
    nbytes = int(lib.chebgcn_glm_workspace(R, M, k))
    ws = _workspace(max(nbytes, 8) + 8, planes.device, 'glm')
    ws = ws[(-ws.data_ptr()) % 8:]
    a = ws[:8 * R * k * Mp].view(torch.float64).view(R, k, Mp) if nbytes else None
    yy = ws[8 * R * k * Mp:8 * R * (k + 1) * Mp].view(torch.float64).view(R, Mp) if nbytes else None
    panels = -(-k // max(glm_geometry()['panel'], 1))
    _lib.check(_launch('glm_project', 4.0 * Ttot * Mp * panels + 8.0 * R * (k + 1) * Mp, 2.0 * Ttot * Mp * (k + 1),
                       lambda: lib.chebgcn_glm_project(_p(planes), Ttot, _p(run_offsets), R, int(M), _p(Q), k, _p(a), _p(yy),
                                                       _stream())), 'glm_project')
    return a, yy


def _finish_tables(what, R, k, Mp, U, B, out64, want32, dev):
    """What the two finish kernels share: ``U`` float64 [R, C, k] and ``B`` float64 [R, P, k] or None checked, ``out64`` (a pair
    of float64 [R, C, Mp], or None) checked, and the float32 outputs allocated:
    ``(C, P, e64, v64, e32, v32, t32 (None without want32), beta [R, P, Mp] or None)``."""
    if U.dim() != 3:
        raise _lib.ChebgcnError('%s: U must be float64 [R, C, k]' % what)
    C_ = int(U.shape[1])
    _dense(U, torch.float64, (R, C_, k), what + ': U')
    P = 0
    beta = None
    if B is not None:
        if B.dim() != 3:
            raise _lib.ChebgcnError('%s: B must be float64 [R, P, k]' % what)
        P = int(B.shape[1])
        _dense(B, torch.float64, (R, P, k), what + ': B')
        beta = torch.empty((R, P, Mp), dtype=torch.float32, device=dev)
    e64 = v64 = None
    if out64 is not None:
        e64, v64 = out64
        _require_cuda(e64, v64)
        _dense(e64, torch.float64, (R, C_, Mp), what + ': out64[0]')
        _dense(v64, torch.float64, (R, C_, Mp), what + ': out64[1]')
    e32 = v32 = t32 = None
    if want32:
        e32, v32, t32 = (torch.empty((R, C_, Mp), dtype=torch.float32, device=dev) for _ in range(3))
    return C_, P, e64, v64, e32, v32, t32, beta


def glm_finish(a, yy, run_offsets, Ttot, rank, U, unorm2, M, B=None, out64=None, want32=False):
    """Residual variance and contrasts of every (run, vertex) (chebgcn_glm_finish) from what ``glm_project`` returned: ``rank``
    int32 [R], ``U`` float64 [R, C, k], ``unorm2`` float64 [R, C], ``B`` float64 [R, P, k] or None, all on the device.
    ``out64``: a pair of float64 [R, C, Mp] tensors that receive effect and variance (for ``glm_combine``).  Returns
    ``(effect, variance, t)`` float32 [R, C, Mp] (``want32``, else None) and ``beta`` float32 [R, P, Mp] or None."""
    _require_cuda(a, yy, run_offsets, rank, U, unorm2, B)
    R, k, Mp = (int(v) for v in a.shape)
    if Mp != plane_stride(M):
        raise _lib.ChebgcnError('glm_finish: a must be [R, k, plane_stride(M)]')
    _dense(a, torch.float64, (R, k, Mp), 'glm_finish: a')
    _dense(yy, torch.float64, (R, Mp), 'glm_finish: yy')
    _dense(run_offsets, torch.int64, (R + 1,), 'glm_finish: run_offsets')
    _dense(rank, torch.int32, (R,), 'glm_finish: rank')
    C_, P, e64, v64, e32, v32, t32, beta = _finish_tables('glm_finish', R, k, Mp, U, B, out64, want32, a.device)
    _dense(unorm2, torch.float64, (R, C_), 'glm_finish: unorm2')
    _lib.check(_launch('glm_finish', 8.0 * R * Mp * (k * (1 + C_ + P) + 1), 2.0 * R * Mp * k * (1 + C_ + P),
                       lambda: _lib.lib().chebgcn_glm_finish(
                           _p(a), _p(yy), _p(run_offsets), int(Ttot), _p(rank), _p(U), _p(unorm2), _p(B), R, int(M), k, C_, P,
                           _p(e64), _p(v64), _p(e32), _p(v32), _p(t32), _p(beta), _stream())), 'glm_finish')
    return e32, v32, t32, beta


def glm_combine(e64, v64, group_ptr, group_runs, M):
    """Fixed effects over the runs of every group (chebgcn_glm_combine): ``e64`` / ``v64`` float64 [R, C, Mp] from ``glm_finish``,
    ``group_ptr`` int32 [S + 1] / ``group_runs`` int32 [nruns] on the device -> ``(effect, variance, t)`` float32 [S, C, M]."""
    _require_cuda(e64, v64, group_ptr, group_runs)
    R, C_, Mp = (int(v) for v in e64.shape)
    if Mp != plane_stride(M):
        raise _lib.ChebgcnError('glm_combine: the maps must be [R, C, plane_stride(M)]')
    _dense(e64, torch.float64, (R, C_, Mp), 'glm_combine: effects')
    _dense(v64, torch.float64, (R, C_, Mp), 'glm_combine: variances')
    S = int(group_ptr.numel()) - 1
    n = int(group_runs.numel())
    if S < 1 or n < 1:
        raise _lib.ChebgcnError('glm_combine: no groups')
    _dense(group_ptr, torch.int32, (S + 1,), 'glm_combine: group_ptr')
    _dense(group_runs, torch.int32, (n,), 'glm_combine: group_runs')
    out = tuple(torch.empty((S, C_, M), dtype=torch.float32, device=e64.device) for _ in range(3))
    _lib.check(_launch('glm_combine', 16.0 * n * C_ * M + 12.0 * S * C_ * M, 2.0 * n * C_ * M, lambda: _lib.lib().chebgcn_glm_combine(
        _p(e64), _p(v64), _p(group_ptr), _p(group_runs), n, R, S, C_, int(M), _p(out[0]), _p(out[1]), _p(out[2]), _stream())),
        'glm_combine')
    return out


def glm_ar1_geometry(k=None):
    """The constants of the AR(1) finish kernel (chebgcn_glm_ar1_query): ``waves`` of a workgroup, ``solve`` contrasts per forward
    solve; with a rank ``k`` also its ``bucket`` (the ``KB`` of ``glm_finish_ar1_kernel<KB>``) and the ``vertices`` of a
    workgroup at that rank."""
    q = _lib.lib().chebgcn_glm_ar1_query
    out = {'waves': q(0), 'solve': q(1)}
    if k is not None:
        out.update(bucket=q(100 + int(k)), vertices=q(200 + int(k)))
    return out


def glm_project_ar1(planes, run_offsets, M, W):
    """The sums of the AR(1) fit (chebgcn_glm_project_ar1): ``planes`` float32 [Ttot, Mp], ``run_offsets`` int64 [R + 1] and
    ``W = [Q | Qs]`` float64 [Ttot, 2k] on the device -> ``(ah float64 [R, 2k, Mp], s0, s1 float64 [R, Mp])`` in one workspace
    (the next call on the stream reuses it)."""
    _require_cuda(planes, run_offsets, W)
    Ttot, Mp, R = _staged_runs(planes, run_offsets, M, 'glm_project_ar1')
    if W.dim() != 2 or W.shape[1] % 2:
        raise _lib.ChebgcnError('glm_project_ar1: W must be float64 [Ttot, 2k]')
    k = int(W.shape[1]) // 2
    _dense(W, torch.float64, (Ttot, 2 * k), 'glm_project_ar1: W')
    lib = _lib.lib()
    nbytes = int(lib.chebgcn_glm_ar1_workspace(R, M, k))
    ws = _workspace(max(nbytes, 8) + 8, planes.device, 'glm')
    ws = ws[(-ws.data_ptr()) % 8:]
    n = 8 * R * Mp
    ah = ws[:2 * k * n].view(torch.float64).view(R, 2 * k, Mp) if nbytes else None
    s0 = ws[2 * k * n:(2 * k + 1) * n].view(torch.float64).view(R, Mp) if nbytes else None
    s1 = ws[(2 * k + 1) * n:(2 * k + 2) * n].view(torch.float64).view(R, Mp) if nbytes else None
    panels = -(-2 * k // max(glm_geometry()['panel'], 1))
    _lib.check(_launch('glm_project_ar1', 4.0 * Ttot * Mp * panels + 8.0 * R * (2 * k + 2) * Mp, 2.0 * Ttot * Mp * (2 * k + 2),
                       lambda: lib.chebgcn_glm_project_ar1(_p(planes), Ttot, _p(run_offsets), R, int(M), _p(W), k, _p(ah), _p(s0),
                                                           _p(s1), _stream())), 'glm_project_ar1')
    return ah, s0, s1


def glm_finish_ar1(ah, s0, s1, planes, W, run_offsets, rank, D, E, U, M, rho=None, B=None, out64=None, want32=False):
    """The AR(1) generalised least-squares fit of every (run, vertex) (chebgcn_glm_finish_ar1) from what ``glm_project_ar1``
    returned: ``D``, ``E`` float64 [R, k, k], ``U`` float64 [R, C, k], ``B`` float64 [R, P, k] or None, ``rank`` int32 [R].
    ``rho``: None estimates a coefficient per (run, vertex), a float applies it everywhere.  Returns ``(effect, variance, t)``
    float32 [R, C, Mp] (``want32``, else None), ``beta`` float32 [R, P, Mp] or None, and ``rho`` float32 [R, Mp]."""
    _require_cuda(ah, s0, s1, planes, W, run_offsets, rank, D, E, U, B)
    R, k2, Mp = (int(v) for v in ah.shape)
    k = k2 // 2
    if Mp != plane_stride(M) or k2 % 2:
        raise _lib.ChebgcnError('glm_finish_ar1: ah must be [R, 2k, plane_stride(M)]')
    Ttot = int(planes.shape[0])
    _dense(ah, torch.float64, (R, 2 * k, Mp), 'glm_finish_ar1: ah')
    _dense(s0, torch.float64, (R, Mp), 'glm_finish_ar1: s0')
    _dense(s1, torch.float64, (R, Mp), 'glm_finish_ar1: s1')
    _dense(planes, torch.float32, (Ttot, Mp), 'glm_finish_ar1: planes')
    _dense(W, torch.float64, (Ttot, 2 * k), 'glm_finish_ar1: W')
    _dense(run_offsets, torch.int64, (R + 1,), 'glm_finish_ar1: run_offsets')
    _dense(rank, torch.int32, (R,), 'glm_finish_ar1: rank')
    _dense(D, torch.float64, (R, k, k), 'glm_finish_ar1: D')
    _dense(E, torch.float64, (R, k, k), 'glm_finish_ar1: E')
    C_, P, e64, v64, e32, v32, t32, beta = _finish_tables('glm_finish_ar1', R, k, Mp, U, B, out64, want32, ah.device)
    rho_out = torch.empty((R, Mp), dtype=torch.float32, device=ah.device)
    flops = 2.0 * R * Mp * (k * k * k / 6.0 + k * k * (1 + C_) / 2.0 + k * (4 + P))
    _lib.check(_launch('glm_finish_ar1', 8.0 * R * Mp * (2 * k + 2 + 2 * C_) + 4.0 * R * Mp * (1 + P), flops,
                       lambda: _lib.lib().chebgcn_glm_finish_ar1(
                           _p(ah), _p(s0), _p(s1), _p(planes), _p(W), _p(run_offsets), Ttot, _p(rank), _p(D), _p(E), _p(U), _p(B),
                           R, int(M), k, C_, P, int(rho is not None), float(rho) if rho is not None else 0.0,
                           _p(e64), _p(v64), _p(e32), _p(v32), _p(t32), _p(beta), _p(rho_out), _stream())), 'glm_finish_ar1')
    return e32, v32, t32, beta, rho_out


def glm_trials_geometry():
    """The constants of the single-trial kernel (chebgcn_glm_trials_query): ``vertices`` of a workgroup, ``panel`` trial columns of
    one pass over the scan, ``max_G1`` columns of a trial's model besides the nuisance (itself and the others), ``max_k`` planes of
    common sums (q + G), ``max_trials`` of one run, ``max_runs`` of one call."""
    q = _lib.lib().chebgcn_glm_trials_query
    return {'vertices': q(0), 'panel': q(1), 'max_G1': q(2), 'max_k': q(3), 'max_trials': q(4), 'max_runs': q(5)}


def glm_trials_model(Ttot, Mp, R, k, nmax, N, G1, nout):
    """``(bytes, flops)`` of one ``glm_trials`` call as ``_launch`` counts them: per panel of trial columns the scan read once and
    the ``k + 1`` planes of common sums read once, the ``nout`` float32 maps written once; one multiply-add per (row, vertex,
    trial column) of the pass and the ``(1 + G)^2``-sized epilogue per (trial, vertex)."""
    panels = -(-nmax // max(glm_trials_geometry()['panel'], 1))
    nbytes = 4.0 * Ttot * Mp * panels + 8.0 * R * (k + 1) * Mp * panels + 4.0 * N * Mp * nout
    return nbytes, 2.0 * Ttot * Mp * nmax + 2.0 * N * Mp * (G1 * G1 + 2 * G1 + 4)


def glm_trials(planes, run_offsets, M, Z, trial_offsets, a, yy, q_rank, own, rank, w, F, outputs=('beta', 't')):
    """The single-trial fits of every (run, trial, vertex) (chebgcn_glm_trials): ``planes`` float32 [Ttot, Mp], ``run_offsets``
    int64 [R + 1], ``Z`` float64 [Ttot, nmax] the projected trial columns, ``trial_offsets`` int64 [R + 1], ``a`` float64
    [R, k, Mp] / ``yy`` float64 [R, Mp] from ``glm_project`` over ``[Qn | Z_S]``, ``q_rank`` int32 [R], and the flat per-trial
    tables ``own`` / ``rank`` int32 [N], ``w`` float64 [N, G1], ``F`` float64 [N, G1, G1], all on the device.  Returns
    ``(beta, variance, t)`` float32 [N, Mp], None for what ``outputs`` does not name.  The byte model counts every panel over
    every run's rows, which is exact when the runs have equally many trials."""
    _require_cuda(planes, run_offsets, Z, trial_offsets, a, yy, q_rank, own, rank, w, F)
    Ttot, Mp, R = _staged_runs(planes, run_offsets, M, 'glm_trials')
    if Z.dim() != 2 or a.dim() != 3 or w.dim() != 2:
        raise _lib.ChebgcnError('glm_trials: Z [Ttot, nmax], a [R, k, Mp] and w [N, G1] are expected')
    nmax, k = int(Z.shape[1]), int(a.shape[1])
    N, G1 = int(w.shape[0]), int(w.shape[1])
    _dense(trial_offsets, torch.int64, (R + 1,), 'glm_trials: trial_offsets')
    _dense(Z, torch.float64, (Ttot, nmax), 'glm_trials: Z')
    _dense(a, torch.float64, (R, k, Mp), 'glm_trials: a')
    _dense(yy, torch.float64, (R, Mp), 'glm_trials: yy')
    _dense(q_rank, torch.int32, (R,), 'glm_trials: q_rank')
    _dense(own, torch.int32, (N,), 'glm_trials: own')
    _dense(rank, torch.int32, (N,), 'glm_trials: rank')
    _dense(w, torch.float64, (N, G1), 'glm_trials: w')
    _dense(F, torch.float64, (N, G1, G1), 'glm_trials: F')
    unknown = set(outputs) - {'beta', 'variance', 't'}
    if unknown or not outputs:
        raise _lib.ChebgcnError("glm_trials: outputs must name some of 'beta', 'variance', 't', got %r" % (outputs,))
    out = [torch.empty((N, Mp), dtype=torch.float32, device=planes.device) if name in outputs else None
           for name in ('beta', 'variance', 't')]
    nbytes, flops = glm_trials_model(Ttot, Mp, R, k, nmax, N, G1, len(set(outputs)))
    _lib.check(_launch('glm_trials', nbytes, flops, lambda: _lib.lib().chebgcn_glm_trials(
        _p(planes), Ttot, _p(run_offsets), R, int(M), _p(Z), nmax, _p(trial_offsets), _p(a), _p(yy), k, _p(q_rank), _p(own), _p(rank),
        _p(w), _p(F), G1, N, _p(out[0]), _p(out[1]), _p(out[2]), _stream())), 'glm_trials')
    return tuple(out)


def searchlight_geometry():
    """The constants of the searchlight kernels (chebgcn_searchlight_query), so that callers and tests follow the tile: ``tile``
    lanes of a score wave, ``centres`` of a score workgroup, ``max_C`` classes served, ``vertices`` of a spread / fit workgroup,
    ``max_models`` of one call, ``max_tiles`` of a model's test samples, ``max_groups``; ``buckets``: the class bucket (the ``NC``
    of ``searchlight_score_kernel<NC>``) of every class count 2 .. ``max_C``; and per bucket ``per_lane`` -- the test samples of
    a lane: a workgroup covers ``tile * per_lane`` consecutive test samples of a model -- and ``unroll``, its neighbours in
    flight."""
    q = _lib.lib().chebgcn_searchlight_query
    buckets = {c: q(100 + c) for c in range(2, q(3) + 1)}
    widths = sorted(set(buckets.values()))
    return {'tile': q(0), 'centres': q(1), 'max_C': q(3), 'vertices': q(4), 'max_models': q(5), 'max_tiles': q(6), 'max_groups': q(7),
            'buckets': buckets, 'per_lane': {b: q(9) if b <= q(8) else 1 for b in widths},
            'unroll': {b: q(10) if b <= q(8) else q(2) for b in widths}}


def _sl_patterns(Xt, S, what):
    if Xt.dim() != 2 or Xt.shape[1] != plane_stride(S) or Xt.dtype != torch.float32 or not Xt.is_contiguous():
        raise _lib.ChebgcnError('%s: Xt must be contiguous float32 [M, plane_stride(S)]' % what)
    return int(Xt.shape[0])


def _sl_lists(ptr, idx, n, what):
    if idx.dim() != 1 or idx.numel() < 1:
        raise _lib.ChebgcnError('%s: empty sample lists' % what)
    _dense(ptr, torch.int32, (n + 1,), what + ': list pointers')
    _dense(idx, torch.int32, (int(idx.numel()),), what + ': list entries')
    return int(idx.numel())


def _sl_rows(rowptr, colidx, what):
    """``(U, nnz)`` of the int32 CSR rows of all neighbourhoods."""
    U = int(rowptr.numel()) - 1
    return U, _sl_lists(rowptr, colidx, U, what)


def _sl_index(t, name, what):
    """The length of the int32 list ``t`` of the ``name`` (centres, models) of one launch."""
    n = int(t.numel())
    if n < 1:
        raise _lib.ChebgcnError('%s: no %s' % (what, name))
    _dense(t, torch.int32, (n,), '%s: %s' % (what, name))
    return n


def _sl_tables(S, C, U, sgroup, slabel, sorig, correct, scores, predictions, what):
    """``G`` of ``correct`` int32 [G, C, U], after the sample tables int32 [S] and ``scores`` / ``predictions`` where given."""
    for t, name in ((sgroup, 'sgroup'), (slabel, 'slabel'), (sorig, 'sorig')):
        _dense(t, torch.int32, (S,), '%s: %s' % (what, name))
    if correct.dim() != 3 or correct.shape[1] != C or correct.shape[2] != U:
        raise _lib.ChebgcnError('%s: correct must be int32 [G, C, U]' % what)
    G = int(correct.shape[0])
    _dense(correct, torch.int32, (G, C, U), what + ': correct')
    if scores is not None:
        _dense(scores, torch.float64, (S, C, U), what + ': scores')
    if predictions is not None:
        _dense(predictions, torch.uint8, (S, U), what + ': predictions')
    return G


def searchlight_spread(Xt, S, list_ptr, list_idx):
    """The variance of the whole training set of every model at every vertex (chebgcn_searchlight_spread): ``Xt`` float32
    [M, plane_stride(S)] vertex-major patterns, ``list_ptr`` int32 [NM + 1] / ``list_idx`` int32 the models' training samples,
    on the device -> float64 [NM, M].  Two-pass float64 moments in list order: include/chebgcn.h."""
    _require_cuda(Xt, list_ptr, list_idx)
    M = _sl_patterns(Xt, S, 'searchlight_spread')
    NM = int(list_ptr.numel()) - 1
    n = _sl_lists(list_ptr, list_idx, NM, 'searchlight_spread')
    spread = torch.empty((NM, M), dtype=torch.float64, device=Xt.device)
    _lib.check(_launch('searchlight_spread', 8.0 * n * M + 8.0 * NM * M, 4.0 * n * M, lambda: _lib.lib().chebgcn_searchlight_spread(
        _p(Xt), int(S), M, _p(list_ptr), _p(list_idx), n, NM, _p(spread), _stream())), 'searchlight_spread')
    return spread


def searchlight_fit(Xt, S, class_ptr, class_idx, C, eps, pooled=False):
    """The naive-Bayes tables of every (model, vertex) (chebgcn_searchlight_fit): ``class_ptr`` int32 [NM * C + 1] /
    ``class_idx`` int32 the training samples of every (model, class), ``eps`` float64 [NM] the smoothing added to every variance
    -> ``(par float64 [NM, M, NC, 2] = (mu, 1 / (2 var)), lg float64 [NM, M, NC] = log(2 pi var) / 2)``, ``NC`` the class bucket
    of ``C``; ``pooled``: one variance for all classes."""
    _require_cuda(Xt, class_ptr, class_idx, eps)
    M = _sl_patterns(Xt, S, 'searchlight_fit')
    NM = int(eps.numel())
    _dense(eps, torch.float64, (NM,), 'searchlight_fit: eps')
    n = _sl_lists(class_ptr, class_idx, NM * int(C), 'searchlight_fit')
    NC = int(_lib.lib().chebgcn_searchlight_query(100 + int(C)))
    if NC < int(C):
        raise _lib.ChebgcnError('searchlight_fit: C = %r classes are not served' % (C,))
    par = torch.empty((NM, M, NC, 2), dtype=torch.float64, device=Xt.device)
    lg = torch.empty((NM, M, NC), dtype=torch.float64, device=Xt.device)
    _lib.check(_launch('searchlight_fit', 8.0 * n * M + 24.0 * NM * M * NC, 4.0 * n * M, lambda: _lib.lib().chebgcn_searchlight_fit(
        _p(Xt), int(S), M, _p(class_ptr), _p(class_idx), n, NM, int(C), int(bool(pooled)), _p(eps), _p(par), _p(lg), _stream())),
        'searchlight_fit')
    return par, lg


def searchlight_score(Xt, S, rowptr, colidx, u0, Ub, test_ptr, tmax, C, par, lg, logprior, sgroup, slabel, sorig, correct,
                      scores=None, predictions=None):
    """Score the centres ``[u0, u0 + Ub)`` (chebgcn_searchlight_score): ``rowptr`` / ``colidx`` int32 CSR of all U neighbourhoods,
    ``test_ptr`` int32 [NM + 1] the (contiguous) test samples of every model, ``tmax`` the most of one model, ``par`` / ``lg``
    from ``searchlight_fit``, ``logprior`` float64 [NM, NC], ``sgroup`` / ``slabel`` / ``sorig`` int32 [S].  ADDS the hits to
    ``correct`` int32 [G, C, U] and fills ``scores`` float64 [S, C, U] / ``predictions`` uint8 [S, U] where given.  float64 in
    the centred form, a fixed order per centre: include/chebgcn.h."""
    _require_cuda(Xt, rowptr, colidx, test_ptr, par, lg, logprior, sgroup, slabel, sorig, correct, scores, predictions)
    M = _sl_patterns(Xt, S, 'searchlight_score')
    S, C, u0, Ub = int(S), int(C), int(u0), int(Ub)
    U, nnz = _sl_rows(rowptr, colidx, 'searchlight_score')
    NM = int(test_ptr.numel()) - 1
    _dense(test_ptr, torch.int32, (NM + 1,), 'searchlight_score: test_ptr')
    NC = int(_lib.lib().chebgcn_searchlight_query(100 + C))
    _dense(par, torch.float64, (NM, M, NC, 2), 'searchlight_score: par')
    _dense(lg, torch.float64, (NM, M, NC), 'searchlight_score: lg')
    _dense(logprior, torch.float64, (NM, NC), 'searchlight_score: logprior')
    G = _sl_tables(S, C, U, sgroup, slabel, sorig, correct, scores, predictions, 'searchlight_score')
    if not 0 <= u0 <= U - Ub or Ub < 1:
        raise _lib.ChebgcnError('searchlight_score: centres [%d, %d) outside the %d rows' % (u0, u0 + Ub, U))
    nbytes = max(8 * NM * Ub * NC, 8)
    ws = _workspace(nbytes + 8, Xt.device, 'searchlight')
    ws = ws[(-ws.data_ptr()) % 8:]
    base = ws[:nbytes].view(torch.float64)
    terms = float(S) * float(nnz) * Ub / max(U, 1)
    _lib.check(_launch('searchlight_score', 4.0 * terms + 16.0 * NM * NC * float(nnz) * Ub / max(U, 1), 4.0 * terms * C,
                       lambda: _lib.lib().chebgcn_searchlight_score(
                           _p(Xt), S, M, _p(rowptr), _p(colidx), nnz, U, u0, Ub, _p(test_ptr), int(tmax), NM, C, _p(par), _p(lg),
                           _p(logprior), _p(sgroup), _p(slabel), _p(sorig), G, _p(base), _p(correct), _p(scores), _p(predictions),
                           _stream())), 'searchlight_score')


def searchlight_lda_geometry():
    """The constants of the LDA searchlight kernel (chebgcn_searchlight_lda_query): ``threads`` of a workgroup (the test samples
    of one scoring pass), ``max_P`` the longest row served, ``tile`` training samples of a residual tile, ``max_C``, ``blocks``
    along a side of the covariance triangle, ``max_models``, ``max_tiles``, ``max_groups``, ``narrow`` -- the class count up to
    which the class tables on chip are narrow -- and ``buckets``: the ball bucket (the ``PB`` of ``searchlight_lda_kernel<PB>``)
    of every row length 1 .. ``max_P``."""
    q = _lib.lib().chebgcn_searchlight_lda_query
    return {'threads': q(0), 'max_P': q(1), 'tile': q(2), 'max_C': q(3), 'blocks': q(4), 'max_models': q(5), 'max_tiles': q(6),
            'max_groups': q(7), 'narrow': q(8), 'buckets': {P: q(100 + P) for P in range(1, q(1) + 1)}}


def searchlight_lda(Xt, S, rowptr, colidx, centres, bucket, class_ptr, class_idx, test_ptr, tmax, C, par, logprior, shrinkage, sgroup,
                    slabel, sorig, correct, scores=None, predictions=None, gamma_out=None):
    """Shrinkage LDA at the rows ``centres`` (int32 [Ub], all of at most ``bucket`` vertices) for every model
    (chebgcn_searchlight_lda): one workgroup per (centre, model) forms the pooled within-class covariance of the ball, shrinks
    it (``shrinkage`` in [1e-6, 1], or negative for Ledoit-Wolf), factorises it and scores the model's test samples.  ``par``
    float64 [NM, M, NC, 2] from ``searchlight_fit`` with ``eps = 0``; the other tables as ``searchlight_score``.  ADDS the hits
    to ``correct`` int32 [G, C, U]; fills ``scores`` float64 [S, C, U] / ``predictions`` uint8 [S, U] / ``gamma_out`` float64
    [NM, U] (the shrinkage used) where given.  The model and its orders: include/chebgcn.h."""
    _require_cuda(Xt, rowptr, colidx, centres, class_ptr, class_idx, test_ptr, par, logprior, sgroup, slabel, sorig, correct, scores,
                  predictions, gamma_out)
    M = _sl_patterns(Xt, S, 'searchlight_lda')
    S, C, bucket = int(S), int(C), int(bucket)
    U, nnz = _sl_rows(rowptr, colidx, 'searchlight_lda')
    NM = int(test_ptr.numel()) - 1
    _dense(test_ptr, torch.int32, (NM + 1,), 'searchlight_lda: test_ptr')
    nidx = _sl_lists(class_ptr, class_idx, NM * C, 'searchlight_lda')
    Ub = _sl_index(centres, 'centres', 'searchlight_lda')
    NC = int(_lib.lib().chebgcn_searchlight_query(100 + C))
    _dense(par, torch.float64, (NM, M, NC, 2), 'searchlight_lda: par')
    _dense(logprior, torch.float64, (NM, NC), 'searchlight_lda: logprior')
    G = _sl_tables(S, C, U, sgroup, slabel, sorig, correct, scores, predictions, 'searchlight_lda')
    if gamma_out is not None:
        _dense(gamma_out, torch.float64, (NM, U), 'searchlight_lda: gamma_out')
    tri = 0.5 * bucket * (bucket + 1)
    _lib.check(_launch('searchlight_lda', 4.0 * float(nidx) * bucket * Ub + 4.0 * float(S) * bucket * Ub, float(nidx) * tri * Ub,
                       lambda: _lib.lib().chebgcn_searchlight_lda(
                           _p(Xt), S, M, _p(rowptr), _p(colidx), nnz, U, _p(centres), Ub, bucket, _p(class_ptr), _p(class_idx), nidx,
                           _p(test_ptr), int(tmax), NM, C, _p(par), _p(logprior), float(shrinkage), _p(sgroup), _p(slabel), _p(sorig), G,
                           _p(correct), _p(scores), _p(predictions), _p(gamma_out), _stream())), 'searchlight_lda')


def searchlight_rdm_geometry():
    """The constants of the RSA searchlight kernel (chebgcn_searchlight_rdm_query): ``threads`` of a workgroup, ``max_P`` the
    longest row served, ``tile`` samples of a residual tile, ``max_C``, ``max_pairs`` of classes (two per thread beyond
    ``threads``), ``max_cells`` of one call, ``narrow`` -- the class count up to which the class tables on chip are narrow -- and
    ``buckets``: the ball bucket (the ``PB`` of ``searchlight_rdm_kernel<PB>``) of every row length 1 .. ``max_P``."""
    q = _lib.lib().chebgcn_searchlight_rdm_query
    return {'threads': q(0), 'max_P': q(1), 'tile': q(2), 'max_C': q(3), 'max_pairs': q(4), 'max_cells': q(5), 'narrow': q(6),
            'buckets': {P: q(100 + P) for P in range(1, q(1) + 1)}}


def searchlight_rdm(Xt, S, rowptr, colidx, centres, bucket, cell_ptr, class_ptr, class_idx, C, par, shrinkage, rdm, gamma_out=None):
    """Crossnobis distances at the rows ``centres`` (int32 [Ub], all of at most ``bucket`` vertices) for every group
    (chebgcn_searchlight_rdm): one workgroup per (centre, group) forms the covariance of the residuals about the cell means over
    all cells of the group, shrinks it (``shrinkage`` in [1e-6, 1], or negative for Ledoit-Wolf), factorises it, whitens every
    cell's class patterns and takes the cross-validated distances.  ``cell_ptr`` int32 [G + 1]: the contiguous cells of every
    group; ``class_ptr`` int32 [NM * C + 1] / ``class_idx`` int32 the samples of every (cell, class); ``par`` float64
    [NM, M, NC, 2] from ``searchlight_fit`` with one model per cell and ``eps = 0``.  Fills ``rdm`` float64 [G, C (C - 1) / 2, U]
    and ``gamma_out`` float64 [G, U] (the shrinkage used; -1 where the ball is degenerate) at these rows.  The quantity and its
    orders: include/chebgcn.h."""
    _require_cuda(Xt, rowptr, colidx, centres, cell_ptr, class_ptr, class_idx, par, rdm, gamma_out)
    M = _sl_patterns(Xt, S, 'searchlight_rdm')
    S, C, bucket = int(S), int(C), int(bucket)
    U, nnz = _sl_rows(rowptr, colidx, 'searchlight_rdm')
    G = int(cell_ptr.numel()) - 1
    if G < 1:
        raise _lib.ChebgcnError('searchlight_rdm: no groups')
    _dense(cell_ptr, torch.int32, (G + 1,), 'searchlight_rdm: cell_ptr')
    if par.dim() != 4:
        raise _lib.ChebgcnError('searchlight_rdm: par must be float64 [NM, M, NC, 2]')
    NM = int(par.shape[0])
    nidx = _sl_lists(class_ptr, class_idx, NM * C, 'searchlight_rdm')
    Ub = _sl_index(centres, 'centres', 'searchlight_rdm')
    NC = int(_lib.lib().chebgcn_searchlight_query(100 + C))
    _dense(par, torch.float64, (NM, M, NC, 2), 'searchlight_rdm: par')
    npairs = C * (C - 1) // 2
    _dense(rdm, torch.float64, (G, npairs, U), 'searchlight_rdm: rdm')
    if gamma_out is not None:
        _dense(gamma_out, torch.float64, (G, U), 'searchlight_rdm: gamma_out')
    tri = 0.5 * bucket * (bucket + 1)
    _lib.check(_launch('searchlight_rdm', 4.0 * float(nidx) * bucket * Ub + 16.0 * NM * bucket * C * Ub, float(nidx) * tri * Ub,
                       lambda: _lib.lib().chebgcn_searchlight_rdm(
                           _p(Xt), S, M, _p(rowptr), _p(colidx), nnz, U, _p(centres), Ub, bucket, _p(cell_ptr), _p(class_ptr),
                           _p(class_idx), nidx, NM, C, _p(par), float(shrinkage), G, _p(rdm), _p(gamma_out), _stream())),
               'searchlight_rdm')


def searchlight_svm_geometry():
    """The constants of the SVM searchlight kernel (chebgcn_searchlight_svm_query): ``threads`` of a workgroup, ``max_n`` the
    largest training set served, ``tile`` vertices of a tile, ``max_C``, ``chunk`` test samples of a scoring chunk,
    ``max_models``, ``max_tiles``, ``max_groups``, ``max_iter`` the largest sweep cap, ``super_tile`` vertices whose means are
    formed at once, and ``buckets``: the sample bucket (the ``NB`` of ``searchlight_svm_kernel<NB>``) of every training-set size
    1 .. ``max_n``."""
    q = _lib.lib().chebgcn_searchlight_svm_query
    return {'threads': q(0), 'max_n': q(1), 'tile': q(2), 'max_C': q(3), 'chunk': q(4), 'max_models': q(5), 'max_tiles': q(6),
            'max_groups': q(7), 'max_iter': q(8), 'super_tile': q(9), 'buckets': {n: q(100 + n) for n in range(1, q(1) + 1)}}


SVM_LOSSES = {'squared_hinge': 0, 'hinge': 1}


def searchlight_svm(Xt, S, rowptr, colidx, centres, models, bucket, list_ptr, list_idx, test_ptr, tmax, C, Creg, loss, tol, max_iter,
                    sgroup, slabel, sorig, correct, scores=None, predictions=None, sweeps=None, residual=None):
    """A one-vs-rest linear SVM at the rows ``centres`` (int32 [Ub], of any length) for the models ``models`` (int32 [NMb], all
    with training sets of at most ``bucket`` samples) (chebgcn_searchlight_svm): one workgroup per (centre, model) forms the
    Gram matrix of the centred training samples, solves the dual of every class by coordinate descent (``Creg`` the SVM's ``C``,
    ``loss`` ``'squared_hinge'`` or ``'hinge'``, at most ``max_iter`` sweeps, stopped at ``max |PG| <= tol``) and scores the
    model's test samples.  ``list_ptr`` int32 [NM + 1] / ``list_idx`` int32: the training samples of every model; the other
    tables as ``searchlight_score``.  ADDS the hits to ``correct`` int32 [G, C, U]; fills ``scores`` float64 [S, C, U] /
    ``predictions`` uint8 [S, U] / ``sweeps`` int32 [NM, U] / ``residual`` float64 [NM, U] where given.  The model and its orders:
    include/chebgcn.h."""
    _require_cuda(Xt, rowptr, colidx, centres, models, list_ptr, list_idx, test_ptr, sgroup, slabel, sorig, correct, scores, predictions,
                  sweeps, residual)
    if loss not in SVM_LOSSES:
        raise _lib.ChebgcnError("searchlight_svm: loss must be 'squared_hinge' or 'hinge', got %r" % (loss,))
    M = _sl_patterns(Xt, S, 'searchlight_svm')
    S, C, bucket = int(S), int(C), int(bucket)
    U, nnz = _sl_rows(rowptr, colidx, 'searchlight_svm')
    NM = int(test_ptr.numel()) - 1
    _dense(test_ptr, torch.int32, (NM + 1,), 'searchlight_svm: test_ptr')
    nidx = _sl_lists(list_ptr, list_idx, NM, 'searchlight_svm')
    Ub, NMb = _sl_index(centres, 'centres', 'searchlight_svm'), _sl_index(models, 'models', 'searchlight_svm')
    G = _sl_tables(S, C, U, sgroup, slabel, sorig, correct, scores, predictions, 'searchlight_svm')
    if sweeps is not None:
        _dense(sweeps, torch.int32, (NM, U), 'searchlight_svm: sweeps')
    if residual is not None:
        _dense(residual, torch.float64, (NM, U), 'searchlight_svm: residual')
    terms = float(nnz) * Ub / max(U, 1) * NMb                  # (vertex, model) pairs of the launch
    tri = 0.5 * bucket * (bucket + 1)
    _lib.check(_launch('searchlight_svm', 8.0 * terms * bucket + 4.0 * float(S) * float(nnz) * Ub / max(U, 1), 2.0 * terms * tri,
                       lambda: _lib.lib().chebgcn_searchlight_svm(
                           _p(Xt), S, M, _p(rowptr), _p(colidx), nnz, U, _p(centres), Ub, _p(models), NMb, bucket, _p(list_ptr),
                           _p(list_idx), nidx, _p(test_ptr), int(tmax), NM, C, float(Creg), SVM_LOSSES[loss], float(tol), int(max_iter),
                           _p(sgroup), _p(slabel), _p(sorig), G, _p(correct), _p(scores), _p(predictions), _p(sweeps), _p(residual),
                           _stream())), 'searchlight_svm')


# ------------------------------------------------------------------------------------
# the graph-convolution layer
# ------------------------------------------------------------------------------------

_workspaces = {}
# set by cgcnn._capture_step around a capture: scratch allocated while capturing comes from THAT graph's private pool and is
# never handed to another graph (or to eager code on a stream with the same handle)
capture_tag = None


def _cap():
    return capture_tag if (capture_tag is not None and torch.cuda.is_current_stream_capturing()) else None


def connectome_geometry():
    """The constants of the connectome kernels (chebgcn_connectome_query), so that callers and tests follow their edges:
    ``max_regions``, ``max_runs`` of one call, ``tile`` the side of a covariance / gram tile, ``rows`` of a tile's operands in LDS
    at once, ``panel`` the columns of a Cholesky panel, ``stage`` the finished columns staged at once, ``threads`` of a finish
    workgroup, ``classes`` the row classes of beta_."""
    q = _lib.lib().chebgcn_connectome_query
    return {'max_regions': q(0), 'max_runs': q(1), 'tile': q(2), 'rows': q(3), 'panel': q(4), 'stage': q(5), 'threads': q(6),
            'classes': q(7)}


def connectome_cov(planes, run_offsets, R):
    """Means, beta_ and the biased covariance of every staged run (chebgcn_connectome_cov): ``planes`` float32 [Ttot, Rp],
    ``run_offsets`` int64 [S + 1] on the device -> the float64 workspace ``connectome_finish`` consumes (the next call on the
    stream reuses it).  The arithmetic and the order of every sum: include/chebgcn.h."""
    _require_cuda(planes, run_offsets)
    Ttot, Rp, S = _staged_runs(planes, run_offsets, R, 'connectome_cov')
    lib = _lib.lib()
    nbytes = int(lib.chebgcn_connectome_workspace(S, int(R)))
    ws = _workspace(max(nbytes, 16) + 16, planes.device, 'connectome')
    ws = ws[(-ws.data_ptr()) % 16:]
    _lib.check(_launch('connectome_cov', 4.0 * Ttot * Rp * 3 + 8.0 * S * Rp * Rp, 1.0 * Ttot * R * (R + 1),
                       lambda: lib.chebgcn_connectome_cov(_p(planes), Ttot, _p(run_offsets), S, int(R), _p(ws), nbytes, _stream())),
               'connectome_cov')
    return ws


def connectome_finish(ws, run_offsets, Ttot, R, kind, shrinkage, matrices, shrinkage_out, degenerate):
    """Shrinkage and the matrices of one kind (chebgcn_connectome_finish) from what ``connectome_cov`` left in ``ws``, which it
    overwrites: ``kind`` an index into ``_lib.CONNECTOME_KINDS``, ``shrinkage`` in [0, 1] or negative for Ledoit-Wolf.  Fills
    ``matrices`` float32 [S, R, R], ``shrinkage_out`` float64 [S] and ``degenerate`` int32 [S], all on the device."""
    _require_cuda(ws, run_offsets, matrices, shrinkage_out, degenerate)
    S = int(run_offsets.numel()) - 1
    _dense(run_offsets, torch.int64, (S + 1,), 'connectome_finish: run_offsets')
    _dense(matrices, torch.float32, (S, R, R), 'connectome_finish: matrices')
    _dense(shrinkage_out, torch.float64, (S,), 'connectome_finish: shrinkage_out')
    _dense(degenerate, torch.int32, (S,), 'connectome_finish: degenerate')
    lib = _lib.lib()
    nbytes = int(lib.chebgcn_connectome_workspace(S, int(R)))
    inverse = int(kind) >= 2
    _lib.check(_launch('connectome_finish', 8.0 * S * R * R * (6 if inverse else 3), (2.0 if inverse else 0.0) * S * R * R * R,
                       lambda: lib.chebgcn_connectome_finish(_p(ws), min(nbytes, ws.numel()), _p(run_offsets), int(Ttot), S, int(R), int(kind),
                                                             float(shrinkage), _p(matrices), _p(shrinkage_out), _p(degenerate),
                                                             _stream())), 'connectome_finish')


def connectome_mean(matrices, degenerate):
    """The mean over the runs that are not flagged (chebgcn_connectome_mean): ``matrices`` float32 [S, R, R], ``degenerate`` int32
    [S] -> float32 [R, R]; a float64 sum in ascending run order, rounded once; zeros where every run is flagged."""
    _require_cuda(matrices, degenerate)
    if matrices.dim() != 3 or matrices.shape[1] != matrices.shape[2]:
        raise _lib.ChebgcnError('connectome_mean: matrices must be float32 [S, R, R]')
    S, R = int(matrices.shape[0]), int(matrices.shape[1])
    _dense(matrices, torch.float32, (S, R, R), 'connectome_mean: matrices')
    _dense(degenerate, torch.int32, (S,), 'connectome_mean: degenerate')
    mean = torch.empty((R, R), dtype=torch.float32, device=matrices.device)
    _lib.check(_launch('connectome_mean', 4.0 * (S + 1) * R * R, 1.0 * S * R * R, lambda: _lib.lib().chebgcn_connectome_mean(
        _p(matrices), _p(degenerate), S, R, _p(mean), _stream())), 'connectome_mean')
    return mean


def tangent_geometry():
    """The constants of the tangent kernels (chebgcn_tangent_query): ``max_regions``, ``max_matrices`` of one call, ``block`` the
    columns of a Jacobi block, ``threads`` of a step workgroup (a thread's second row starts there), ``sweeps`` the cap,
    ``tile`` the side of a product tile, ``rows`` of a tile's operands in LDS at once, ``inner`` the sweeps inside a block pair."""
    q = _lib.lib().chebgcn_tangent_query
    return {'max_regions': q(0), 'max_matrices': q(1), 'block': q(2), 'threads': q(3), 'sweeps': q(4), 'tile': q(5), 'rows': q(6),
            'inner': q(7)}


def _sym_stack(m, what, S=None, R=None):
    if m.dim() != 3 or m.shape[1] != m.shape[2]:
        raise _lib.ChebgcnError('%s must be float64 [S, R, R]' % what)
    S, R = int(m.shape[0]) if S is None else S, int(m.shape[1]) if R is None else R
    _dense(m, torch.float64, (S, R, R), what)
    return S, R


def connectome_sigma(ws, run_offsets, Ttot, R, shrinkage, sigma, shrinkage_out):
    """The shrunk covariance of every run in float64 (chebgcn_connectome_sigma) from what ``connectome_cov`` left in ``ws``, which
    it overwrites: fills ``sigma`` float64 [S, R, R] and ``shrinkage_out`` float64 [S]."""
    _require_cuda(ws, run_offsets, sigma, shrinkage_out)
    S = int(run_offsets.numel()) - 1
    _dense(run_offsets, torch.int64, (S + 1,), 'connectome_sigma: run_offsets')
    _dense(sigma, torch.float64, (S, R, R), 'connectome_sigma: sigma')
    _dense(shrinkage_out, torch.float64, (S,), 'connectome_sigma: shrinkage_out')
    lib = _lib.lib()
    nbytes = int(lib.chebgcn_connectome_workspace(S, int(R)))
    _lib.check(_launch('connectome_sigma', 8.0 * S * R * R * 4, 0.0, lambda: lib.chebgcn_connectome_sigma(
        _p(ws), min(nbytes, ws.numel()), _p(run_offsets), int(Ttot), S, int(R), float(shrinkage), _p(sigma), _p(shrinkage_out),
        _stream())), 'connectome_sigma')


def sym_eigh(matrices):
    """Eigendecompositions of symmetric matrices (chebgcn_sym_eigh): ``matrices`` float64 [S, R, R] on the device ->
    ``(w [S, R] in no particular order, Vt [S, R, R] with row p the eigenvector of w[p], sweeps int32 [S], converged int32
    [S])``.  The call reads one int32 back per sweep.  The method and the order of every sum: include/chebgcn.h."""
    _require_cuda(matrices)
    S, R = _sym_stack(matrices, 'sym_eigh: matrices')
    lib = _lib.lib()
    nbytes = int(lib.chebgcn_tangent_workspace(S, R))
    ws = _workspace(max(nbytes, 8) + 8, matrices.device, 'tangent_eigh')
    ws = ws[(-ws.data_ptr()) % 8:]
    w = torch.empty((S, R), dtype=torch.float64, device=matrices.device)
    Vt = torch.empty((S, R, R), dtype=torch.float64, device=matrices.device)
    sweeps = torch.empty((S,), dtype=torch.int32, device=matrices.device)
    converged = torch.empty((S,), dtype=torch.int32, device=matrices.device)
    _lib.check(_launch('sym_eigh', 8.0 * S * R * R * 4, 0.0, lambda: lib.chebgcn_sym_eigh(
        _p(matrices), S, R, _p(w), _p(Vt), _p(sweeps), _p(converged), _p(ws), nbytes, _stream())), 'sym_eigh')
    return w, Vt, sweeps, converged


def sym_function(w, Vt, func, a=1.0, flags=None, float32=False, out=None):
    """``V diag(f(a w)) V^T`` per matrix (chebgcn_sym_function) from what ``sym_eigh`` returned; ``func`` one of
    ``_lib.SYM_FUNCTIONS``.  ``flags`` int32 [S] (default: fresh zeros) is set where a matrix has an eigenvalue the function cannot
    take; flagged matrices come out as zeros.  -> ``(out float64 or float32 [S, R, R], flags)``."""
    _require_cuda(w, Vt, flags, out)
    S, R = _sym_stack(Vt, 'sym_function: Vt')
    _dense(w, torch.float64, (S, R), 'sym_function: w')
    if func not in _lib.SYM_FUNCTIONS:
        raise _lib.ChebgcnError('sym_function: func must be one of %r, got %r' % (_lib.SYM_FUNCTIONS, func))
    if flags is None:
        flags = torch.zeros((S,), dtype=torch.int32, device=Vt.device)
    _dense(flags, torch.int32, (S,), 'sym_function: flags')
    dtype = torch.float32 if float32 else torch.float64
    if out is None:
        out = torch.empty((S, R, R), dtype=dtype, device=Vt.device)
    _dense(out, dtype, (S, R, R), 'sym_function: out')
    fvals = _workspace(8 * S * R + 8, Vt.device, 'tangent_fvals')
    fvals = fvals[(-fvals.data_ptr()) % 8:]
    _lib.check(_launch('sym_function', 8.0 * S * R * R * 2, 1.0 * S * R * R * (R + 1), lambda: _lib.lib().chebgcn_sym_function(
        _p(w), _p(Vt), S, R, _lib.SYM_FUNCTIONS.index(func), float(a), _p(out), int(bool(float32)), _p(flags), _p(fvals), _stream())),
        'sym_function')
    return out, flags


def sym_congruence(W, matrices, out=None):
    """``W A_s W`` for one symmetric ``W`` float64 [R, R] and symmetric ``matrices`` float64 [S, R, R] (chebgcn_sym_congruence) ->
    float64 [S, R, R], each symmetric bit for bit."""
    _require_cuda(W, matrices, out)
    S, R = _sym_stack(matrices, 'sym_congruence: matrices')
    _dense(W, torch.float64, (R, R), 'sym_congruence: W')
    if out is None:
        out = torch.empty_like(matrices)
    _dense(out, torch.float64, (S, R, R), 'sym_congruence: out')
    scratch = _workspace(8 * S * R * R + 8, matrices.device, 'tangent_congruence')
    scratch = scratch[(-scratch.data_ptr()) % 8:]
    _lib.check(_launch('sym_congruence', 8.0 * S * R * R * 4, 3.0 * S * R * R * R, lambda: _lib.lib().chebgcn_sym_congruence(
        _p(W), _p(matrices), S, R, _p(out), _p(scratch), _stream())), 'sym_congruence')
    return out


def sym_mean(matrices, flags, acc, first=True, n_total=0):
    """The running sum of the unflagged matrices in ascending order (chebgcn_sym_mean): ``acc`` float64 [R, R] is started
    (``first``) or continued; with ``n_total`` > 0 the call ends the mean -> ``(mean float64 [R, R], norm float64 [1])``, its
    Frobenius norm; else ``None``."""
    _require_cuda(matrices, flags, acc)
    S, R = _sym_stack(matrices, 'sym_mean: matrices')
    _dense(flags, torch.int32, (S,), 'sym_mean: flags')
    _dense(acc, torch.float64, (R, R), 'sym_mean: acc')
    mean = norm = None
    if n_total > 0:
        mean = torch.empty((R, R), dtype=torch.float64, device=matrices.device)
        norm = torch.empty((1,), dtype=torch.float64, device=matrices.device)
    _lib.check(_launch('sym_mean', 8.0 * (S + 2) * R * R, 1.0 * S * R * R, lambda: _lib.lib().chebgcn_sym_mean(
        _p(matrices), _p(flags), S, R, int(bool(first)), int(n_total), _p(acc), _p(mean), _p(norm), _stream())), 'sym_mean')
    return (mean, norm) if n_total > 0 else None


def ridge_geometry():
    """The constants of the ridge kernels (chebgcn_ridge_query): ``tile`` the vertices of a workgroup, ``block`` the outputs of a
    register block, ``max_F`` / ``max_A`` served, ``max_runs`` of one list, ``max_models`` of one call, ``threads`` of a
    workgroup, ``buckets`` the buckets of F the score kernel is built for."""
    q = _lib.lib().chebgcn_ridge_query
    return {'tile': q(0), 'block': q(1), 'max_F': q(2), 'max_A': q(3), 'max_runs': q(4), 'max_models': q(5), 'threads': q(6),
            'buckets': sorted({q(100 + F) for F in range(1, q(2) + 1)})}


def _ridge_tables(what, c, list_ptr, list_runs, E, F):
    """``c`` float64 [R, F, Mp] and the run lists of E models checked -> ``(R, Mp, nlist)``."""
    if c.dim() != 3:
        raise _lib.ChebgcnError('%s: c must be float64 [R, F, Mp]' % what)
    R, Mp = int(c.shape[0]), int(c.shape[2])
    _dense(c, torch.float64, (R, F, Mp), what + ': c')
    _dense(list_ptr, torch.int32, (2 * E + 1,), what + ': list_ptr')
    nlist = int(list_runs.numel())
    _dense(list_runs, torch.int32, (nlist,), what + ': list_runs')
    return R, Mp, nlist


def ridge_workspace(E, F, M, device):
    """The float64 workspace [E, 2, F, Mp] of the ridge kernels as ``(tensor, bytes)`` (chebgcn_ridge_workspace), kept per device
    and stream like every scratch."""
    nbytes = int(_lib.lib().chebgcn_ridge_workspace(int(E), int(F), int(M)))
    ws = _workspace(max(nbytes, 8) + 8, device, 'ridge')
    return ws[(-ws.data_ptr()) % 8:], nbytes


def ridge_rotate(c, list_ptr, list_runs, V, M, ws=None):
    """The run sums of every model's two lists, rotated into its eigenbasis (chebgcn_ridge_rotate): ``c`` float64 [R, F, Mp],
    ``list_ptr`` int32 [2 E + 1] / ``list_runs`` int32 [nlist] (list 2 e the training runs of model e, 2 e + 1 its held-out
    runs), ``V`` float64 [E, F, F] on the device -> the workspace ``(ws, bytes)`` that ``ridge_score`` and ``ridge_weights``
    read (``ws``: one given by the caller, at least that large).  The chains: include/chebgcn.h."""
    _require_cuda(c, list_ptr, list_runs, V, ws)
    if V.dim() != 3:
        raise _lib.ChebgcnError('ridge_rotate: V must be float64 [E, F, F]')
    E, F = int(V.shape[0]), int(V.shape[1])
    _dense(V, torch.float64, (E, F, F), 'ridge_rotate: V')
    R, Mp, nlist = _ridge_tables('ridge_rotate', c, list_ptr, list_runs, E, F)
    if Mp != plane_stride(M):
        raise _lib.ChebgcnError('ridge_rotate: c must be [R, F, plane_stride(M)]')
    lib = _lib.lib()
    if ws is None:
        ws, nbytes = ridge_workspace(E, F, M, c.device)
    else:
        nbytes = min(int(lib.chebgcn_ridge_workspace(E, F, int(M))), ws.numel() * ws.element_size())
    _lib.check(_launch('ridge_rotate', 8.0 * E * F * Mp * 3, 4.0 * E * F * F * Mp, lambda: lib.chebgcn_ridge_rotate(
        _p(c), R, _p(list_ptr), _p(list_runs), nlist, _p(V), E, F, int(M), _p(ws), nbytes, _stream())), 'ridge_rotate')
    return ws, nbytes


def ridge_score(ws, nbytes, tss, list_ptr, list_runs, H, d, fold_ptr, M, Ef, kind='r2', scores=False):
    """Every fold model scored at every penalty and the folds of every subject averaged (chebgcn_ridge_score): ``ws`` from
    ``ridge_rotate`` over E >= ``Ef`` models, ``tss`` float64 [R, Mp], ``H`` float64 [E, F, F] (symmetric bit for bit), ``d``
    float64 [E, A, F], ``fold_ptr`` int32 [S + 1] (the folds of subject s are the models fold_ptr[s] .. fold_ptr[s + 1] - 1) ->
    ``(score float32 [S, M], alpha_index int32 [S, M], scores float32 [S, A, M] or None, fold_scores float64 [Ef, A, Mp])``."""
    _require_cuda(ws, tss, list_ptr, list_runs, H, d, fold_ptr)
    if H.dim() != 3 or d.dim() != 3:
        raise _lib.ChebgcnError('ridge_score: H must be float64 [E, F, F] and d float64 [E, A, F]')
    E, F, A = int(H.shape[0]), int(H.shape[1]), int(d.shape[1])
    _dense(H, torch.float64, (E, F, F), 'ridge_score: H')
    _dense(d, torch.float64, (E, A, F), 'ridge_score: d')
    if kind not in _lib.RIDGE_SCORES:
        raise _lib.ChebgcnError('ridge_score: kind must be one of %r, got %r' % (_lib.RIDGE_SCORES, kind))
    Mp = plane_stride(M)
    R = int(tss.shape[0]) if tss.dim() == 2 else 0
    _dense(tss, torch.float64, (R, Mp), 'ridge_score: tss')
    _dense(list_ptr, torch.int32, (2 * E + 1,), 'ridge_score: list_ptr')
    nlist = int(list_runs.numel())
    _dense(list_runs, torch.int32, (nlist,), 'ridge_score: list_runs')
    S = int(fold_ptr.numel()) - 1
    _dense(fold_ptr, torch.int32, (S + 1,), 'ridge_score: fold_ptr')
    dev = tss.device
    Ef = int(Ef)
    fold = torch.empty((max(Ef, 1), A, Mp), dtype=torch.float64, device=dev)
    score = torch.empty((S, int(M)), dtype=torch.float32, device=dev)
    index = torch.empty((S, int(M)), dtype=torch.int32, device=dev)
    table = torch.empty((S, A, int(M)), dtype=torch.float32, device=dev) if scores else None
    _lib.check(_launch('ridge_score', 8.0 * Ef * Mp * (2 * F + A), 2.0 * Ef * A * F * (F + 2) * Mp, lambda: _lib.lib().chebgcn_ridge_score(
        _p(ws), nbytes, _p(tss), R, _p(list_ptr), _p(list_runs), nlist, _p(H), _p(d), _p(fold_ptr), E, Ef, S, F, A, int(M),
        _lib.RIDGE_SCORES.index(kind), _p(fold), _p(score), _p(index), _p(table), _stream())), 'ridge_score')
    return score, index, table, fold


def ridge_weights(ws, nbytes, Vt, d, all_model, alpha_index, M):
    """The refit of every subject at its selected penalties (chebgcn_ridge_weights): ``ws`` from ``ridge_rotate``, ``Vt`` float64
    [E, F, F] (V transposed), ``d`` float64 [E, A, F], ``all_model`` int32 [S] the model trained on all the subject's runs,
    ``alpha_index`` int32 [S, M] -> float32 [S, F, M]."""
    _require_cuda(ws, Vt, d, all_model, alpha_index)
    if Vt.dim() != 3 or d.dim() != 3:
        raise _lib.ChebgcnError('ridge_weights: Vt must be float64 [E, F, F] and d float64 [E, A, F]')
    E, F, A = int(Vt.shape[0]), int(Vt.shape[1]), int(d.shape[1])
    _dense(Vt, torch.float64, (E, F, F), 'ridge_weights: Vt')
    _dense(d, torch.float64, (E, A, F), 'ridge_weights: d')
    S = int(all_model.numel())
    _dense(all_model, torch.int32, (S,), 'ridge_weights: all_model')
    _dense(alpha_index, torch.int32, (S, int(M)), 'ridge_weights: alpha_index')
    weights = torch.empty((S, F, int(M)), dtype=torch.float32, device=Vt.device)
    _lib.check(_launch('ridge_weights', 8.0 * S * F * plane_stride(M) + 4.0 * S * F * M, 2.0 * S * F * (F + 1) * M,
                       lambda: _lib.lib().chebgcn_ridge_weights(_p(ws), nbytes, _p(Vt), _p(d), _p(all_model), _p(alpha_index), E, S, F,
                                                                A, int(M), _p(weights), _stream())), 'ridge_weights')
    return weights


def _workspace(nbytes, device, tag=''):
    """Scratch of a library call, kept per device, stream and use: launches on one stream are ordered, so the buffer of the
    previous call of the same kind is free by the time the next one runs."""
    key = (device.index, torch.cuda.current_stream().cuda_stream, tag, _cap())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


_mean_grad_buffers = {}


def _mean_grad_buffer(B, Mp, device):
    """[B, Mp] scratch of the fused last layer's backward; columns beyond M stay zero (only [:, :M] is ever written)."""
    key = (B, Mp, device.index, torch.cuda.current_stream().cuda_stream, _cap())
    buf = _mean_grad_buffers.get(key)
    if buf is None:
        buf = _mean_grad_buffers[key] = torch.zeros((B, Mp), dtype=torch.float32, device=device)
    return buf


def softmax_xent(logits, labels):
    """Mean softmax cross-entropy of ``logits [B, C]`` against ``labels [B]`` (int32 or int64) and its gradient wrt the
    logits, one launch (tf.nn.sparse_softmax_cross_entropy_with_logits + tf.reduce_mean, models_gcn.py:257-259).  Returns
    (loss: 0-d tensor, dlogits [B, C]); the caller seeds autograd with ``logits.backward(dlogits)``."""
    _require_cuda(logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32 or labels.dim() != 1 or labels.numel() != logits.shape[0]:
        raise ValueError('softmax_xent: logits [B, C] float32 and labels [B]')
    if labels.dtype not in (torch.int32, torch.int64):
        labels = labels.long()
    z = logits.detach().contiguous()
    labels = labels.contiguous()
    B, C = z.shape
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    _lib.check(_lib.lib().chebgcn_softmax_xent(_p(z), _p(labels), int(labels.dtype == torch.int64), _p(loss), _p(dz), B, C,
                                               _stream()), 'softmax_xent')
    return loss, dz


def cache_keys():
    """Keys of the per-stream scratch caches above (workspaces, the fused last layer's gradient buffer)."""
    return {('ws',) + k for k in _workspaces} | {('mg',) + k for k in _mean_grad_buffers}


def drop_cache_keys(keys):
    """Forget scratch buffers -- those a captured step allocated from its graph's private pool on its capture streams
    (cgcnn.enable_step_graph records them): kept here they would pin that pool after the graph is gone, and a later capture
    on the same stream would be handed a buffer of a destroyed graph."""
    for k in keys:
        (_workspaces if k[0] == 'ws' else _mean_grad_buffers).pop(tuple(k[1:]), None)


def _brelu_bwd_ws(B, M, F, pool, bias_kind, device):
    """Scratch of chebgcn_brelu_pool_bwd: the per-workgroup partials of a per-filter (b1relu) bias gradient."""
    n = _lib.lib().chebgcn_brelu_pool_bwd_workspace(B, M, F, pool, bias_kind)
    if n == 0:
        return None, 0
    ws = torch.empty(n, dtype=torch.uint8, device=device)
    return ws, n


def _check_grad_buffer(buf, shape, what):
    if tuple(buf.shape) != tuple(shape) or not buf.is_contiguous() or buf.dtype != torch.float32 or not buf.is_cuda:
        raise ValueError('%s buffer must be a contiguous float32 device tensor of shape %s' % (what, tuple(shape)))


PRECISIONS = {'f32': 0, 'bf16': 1, 'bf16x3': 3}     # contraction arithmetic -> passes of chebgcn_contract_fwd_bf16
FP32_MFMA_BALANCE = 19.6        # flop per HBM byte at which the fp32-input matrix cores (157 TFLOP/s) meet 8 TB/s


def resolve_precision(precision, Fin, K, Fout):
    """'auto' -> the arithmetic a layer of this shape computes in: 'f32' (fp32-input matrix instructions, exact products)
    where the contraction is HBM-bound anyway (what BASELINE configs[1] runs: 32 filters), 'bf16x3' where fp32 matrix
    work would bound it -- more than 32 filters and an arithmetic intensity 2*Fin*K*Fout / (4*(Fin*K + Fout)) above the
    machine balance of the fp32 matrix cores.  'bf16x3' splits each fp32 operand into two bf16 and accumulates
    hi*hi + hi*lo + lo*hi in fp32: 3e-6 ... 6e-6 of the tensor's scale from the fp32 layer (tests/test_gpu_dispatch.py holds
    every arm to 1e-5 against float64), at a third of the time.  Anything else is returned unchanged."""
    if precision != 'auto':
        return precision
    ai = float(Fin) * K * Fout / (2.0 * (Fin * K + Fout))
    return 'bf16x3' if (Fout > 32 and ai > FP32_MFMA_BALANCE) else 'f32'


def contract_fwd_into(stack, W, bias, bias_kind, out, argmax, B, M, Fin, K, Fout, pool, pool_kind, relu, precision='f32',
                      what='contract_fwd', gate=None):
    """Launches the forward contraction (models_gcn.py:611-648) into ``out``.

    precision 'f32' = chebgcn_contract_fwd (exact fp32 MFMA); 'bf16' / 'bf16x3' =
    chebgcn_contract_fwd_bf16 with 1 / 3 passes (wide layers, BASELINE config 5).
    ``gate``: a ReLU mask [B, Fout, Mp/4]; the result is stored gated by it (chebgcn_contract_fwd_gated: fp32, no bias / ReLU /
    pooling -- the input gradient in forward form with the ReluGrad of the layer below in its epilogue)."""
    lib = _lib.lib()
    if precision not in PRECISIONS:
        raise ValueError('precision must be one of %s' % sorted(PRECISIONS))
    Mo = M // pool
    nbytes, flops = 4.0 * B * (M * Fin * K + Mo * Fout), 2.0 * B * M * Fin * K * Fout
    if gate is not None:
        if precision != 'f32' or bias is not None or pool != 1 or relu or argmax is not None:
            raise ValueError('contract_fwd_into(gate=...): fp32, no bias, no ReLU, no pooling')
        _lib.check(_launch(what, nbytes + 0.25 * B * M * Fout, flops,
                           lambda: lib.chebgcn_contract_fwd_gated(_p(stack), _p(W), _p(gate), _p(out), B, M, Fin, K, Fout,
                                                                  _stream())), what)
        return
    if precision == 'f32':
        _lib.check(_launch(what, nbytes, flops,
                           lambda: lib.chebgcn_contract_fwd(_p(stack), _p(W), _p(bias), bias_kind, _p(out), _p(argmax), B, M,
                                                            Fin, K, Fout, pool, pool_kind, int(relu), _stream())),
                   what)
        return
    nws = lib.chebgcn_contract_fwd_bf16_workspace(Fin, K, Fout)
    ws = _workspace(nws, stack.device, 'fwd_bf16')
    _lib.check(_launch(what + '_' + precision, nbytes, flops,
                       lambda: lib.chebgcn_contract_fwd_bf16(_p(stack), _p(W), _p(bias), bias_kind, _p(out), _p(argmax), B, M,
                                                             Fin, K, Fout, pool, pool_kind, int(relu), PRECISIONS[precision],
                                                             _p(ws), nws, _stream())),
               what + '_bf16')


def _detached(t):
    """``t`` as a kernel operand: detached and contiguous (None stays None)."""
    return None if t is None else t.detach().contiguous()


def _out_buffer(out, B, F, M, device):
    """The caller's ``out``, checked, or new planes ``[B, F, stride(M)]``."""
    if out is None:
        return plane_empty(B, F, M, device)
    if tuple(out.shape) != (B, F, plane_stride(M)) or not out.is_contiguous():
        raise ValueError('out buffer has the wrong shape')
    return out


def _contract_cost(B, M, Fin, K, Fout, planes=None):
    """(algorithmic bytes, flops) of a contraction or one of its gradients, for ``_launch``: the compulsory
    traffic is the stack, 4*M*Fin*K per window, and ``planes`` planes of M vertices (the layer's Fout; 1 under the fused
    feature mean)."""
    return 4.0 * B * M * (Fin * K + (Fout if planes is None else planes)), 2.0 * B * M * Fin * K * Fout


def _pool_gather(y, maps, out, sel, B, M, Fout, pool, pool_kind, relu):
    """Pooling between two vertex orders: gathers the clusters of the unpooled ``y`` (source order) through LDS into ``out``
    (csrc/pointwise.hip pool_gather_fwd_kernel); ``sel``: the selection bytes a backward pass reads, or None."""
    Mo = M // pool
    _lib.check(_launch('pool_gather_fwd', B * Fout * (4.0 * (M + Mo) + Mo), 0.0, lambda: _lib.lib().chebgcn_pool_gather_fwd(
        _p(y), _p(maps[0]), _p(out), _p(sel), B, M, Fout, pool, pool_kind, int(relu), _stream())), 'pool_gather_fwd')


def dx_by_forward_shape(graph, Fin, K, Fout, precision):
    """Does a layer of this shape form its input gradient by the forward recurrence on dy (``dx_by_forward``)?  THE rule:
    ``ChebConv.backward`` takes that form, and ``ChebConv.forward`` offers its mask to the layer above (``GateLink``), where
    this holds and their own conditions do; the models pre-index the weights of such layers, which read
    W'[fo*K + k][fin] = W[fin*K + k][fo].
    On graphs in length order only: there the forward recurrence kernel is the faster of the two (0.49 against 0.43 of the
    HBM roofline in the step).  In the caller's order the Clenshaw kernels are as fast or faster -- measured: the reference's
    own shape at N = 1000 / 2000 (batch 128, K = 10) 1.93 / 3.32 ms this way against 1.89 / 3.16 ms; the level-0 layers of
    the pooling network run their forward recurrence on two planes, the adjoint on four (common.h pick_ell)."""
    return bool(dx_by_forward and K > 1 and Fout <= Fin and resolve_precision(precision, Fin, K, Fout) != 'bf16' and graph.ordered)


# What one backward pass of ChebConv runs, decided before anything is launched (_bwd_choose):
#   dy     how dy and the bias gradient are obtained (_bwd_dy): 'mean_gate', 'fold', 'dy16', 'link' or 'plain'
#   grads  which contraction gradients read it (_BWD_W, _BWD_X): 'dy16', 'bf16', 'relu_mean', 'relu_bias', 'relu' or 'plain'
#   by_fwd the input gradient by the forward recurrence on dy;  merge_bias: dbias rides in the weight gradient's launch;
#   defer_bias: the bias reduction is enqueued behind the layer's other gradients;  side: the weight gradient on a second stream
_BwdChoice = collections.namedtuple('_BwdChoice', 'dy grads by_fwd merge_bias defer_bias side')

# One arm of a contraction gradient, by ``grads``: its entry point and what that takes besides the operands every arm has.
# mask: reads the ReLU mask;  dbias: writes the bias gradient too;  passes: takes the number of bf16 passes;  what: the name
# _lib.check reports (None: the launch's name);  planes: planes of dy per window (None: Fout).  A new arm is one row here.
_Arm = collections.namedtuple('_Arm', 'entry mask dbias passes what planes', defaults=(False, False, False, None, None))
_BWD_W = {                                     # the weight gradient
    'dy16': _Arm('chebgcn_contract_bwd_w_bf16_dy16'),
    'bf16': _Arm('chebgcn_contract_bwd_w_bf16', passes=True),
    'relu_mean': _Arm('chebgcn_contract_bwd_w_relu_mean', mask=True),
    'relu_bias': _Arm('chebgcn_contract_bwd_w_relu_bias', mask=True, dbias=True),
    'relu': _Arm('chebgcn_contract_bwd_w_relu', mask=True),
    'plain': _Arm('chebgcn_contract_bwd_w'),
}
_BWD_X = {                                     # the input gradient in Clenshaw form
    'dy16': _Arm('chebgcn_contract_bwd_x_bf16_dy16'),
    'bf16': _Arm('chebgcn_contract_bwd_x_bf16', passes=True),
    'relu_mean': _Arm('chebgcn_contract_bwd_x_relu_mean', mask=True, what='contract_bwd_x_relu_mean', planes=1),
    'relu': _Arm('chebgcn_contract_bwd_x_relu', mask=True, what='contract_bwd_x_relu'),
    'plain': _Arm('chebgcn_contract_bwd_x', what='contract_bwd_x'),
}
_BWD_X['relu_bias'] = _BWD_X['relu']           # (the merged bias gradient is the weight gradient's business)


def _bwd_choose(ctx, gout, argmax, dbias):
    """The ``_BwdChoice`` of one backward pass: reads the module switches, launches nothing."""
    lib = _lib.lib()
    B, M, Fin, K, Fout, pool, pool_kind, relu, bias_kind = ctx.cfg
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    # gradient wrt the input by the forward recurrence on dy (dx_by_forward_shape): dy is then materialised (slab 0 of the stack
    # the recurrence fills), so the ReluGrad is not folded into the contraction gradients of this layer.  Under the fused
    # feature mean only where one pass can gate the mean's gradient AND reduce the bias gradient (relu_grad_mean)
    by_fwd = bool(need_x and not ctx.fused and dx_by_forward_shape(ctx.graph, Fin, K, Fout, ctx.precision)
                  and (not ctx.mean or (ctx.fold and dbias is not None)))
    fold = ctx.fold and not by_fwd
    dy16 = bool(bf16_dy16 and not fold and ctx.precision == 'bf16' and pool == 1 and relu and argmax is not None
                and lib.chebgcn_bf16_dy16_supported(B, M, Fin, K, Fout))
    link, merge_bias = ctx.link_out, False
    if by_fwd and ctx.mean:
        dy = 'mean_gate'             # leaves an ordinary materialised dy: the contraction gradients below are not the mean's
    elif fold:
        dy = 'fold'
        # small launches (atlas-sized layers): the per-vertex bias gradient rides in the launch that adds the weight gradient's
        # partials (chebgcn_contract_bwd_w_relu_bias) -- one ~5 us launch less per layer
        merge_bias = bool(merge_bias_small and dbias is not None and bias_kind == BIAS_VERTEX and not ctx.mean
                          and need_w and not PRECISIONS[ctx.precision]
                          and lib.chebgcn_contract_bwd_w_relu_bias_merged(B, M, Fin, K, Fout))
    elif dy16:
        dy = 'dy16'
    elif (by_fwd and link is not None and link.gstack is not None and link.gstack.data_ptr() == gout.data_ptr()
          and tuple(gout.shape) == (B, Fout, ctx.graph.Mp)):
        dy = 'link'                  # the slab the layer above stored its gated input gradient in, recognised by address
    else:
        dy = 'plain'
    grads = ('dy16' if dy16 else 'bf16' if PRECISIONS[ctx.precision] else 'plain' if not fold
             else 'relu_mean' if ctx.mean else 'relu_bias' if merge_bias else 'relu')
    # the weight gradient on a second stream (see overlap_bwd_w); never on instrumented steps
    want_side = (Fout > 32) if overlap_bwd_w == 'auto' else bool(overlap_bwd_w)
    side = bool(need_w and want_side and need_x and (timers is None or not timers.active))
    return _BwdChoice(dy, grads, by_fwd, merge_bias, dy == 'fold' and dbias is not None and not merge_bias, side)


def _bwd_dy(ctx, ch, gout, out, argmax, dbias):
    """dy and the bias gradient.  Returns (dy, mask, gstack, bias job): ``mask`` where the contraction gradients gate dy
    themselves, ``gstack`` the [K, B, Fout, Mp] stack whose slab 0 dy is (``ch.by_fwd``), the job a bias reduction still to
    be enqueued."""
    lib = _lib.lib()
    B, M, Fin, K, Fout, pool, pool_kind, relu, bias_kind = ctx.cfg
    g, dev = ctx.graph, gout.device
    if ch.dy == 'mean_gate':
        # the last layer under the fused feature mean: every filter's gradient is the plane gout / Fout; one pass gates it
        # with the ReLU mask into slab 0 of the stack the recurrence fills and reduces the bias gradient
        gstack = torch.empty((K, B, Fout, g.Mp), dtype=torch.float32, device=dev)
        dy = gstack[0]
        bws, nbws = _brelu_bwd_ws(B, M, Fout, 1, bias_kind, dev)
        _lib.check(_launch('relu_grad_mean', B * M * (4.0 + Fout * 4.25), 0.0, lambda: lib.chebgcn_relu_grad_mean(
            _p(gout), _p(argmax), _p(dy), _p(dbias), bias_kind, B, M, Fout, _p(bws), nbws, _stream())), 'relu_grad_mean')
        return dy, None, gstack, None
    if ch.dy == 'fold':
        # ReluGrad folded into the two contraction gradients (chebgcn_contract_bwd_*_relu read gout and the
        # mask); what is left of this pass is the bias reduction, which writes nothing but dbias
        if not ch.defer_bias:
            return gout, argmax, None, None

        # feeds nothing in backward: enqueued BEHIND contract_bwd_x / recurrence_bwd (the chain the next layer waits
        # for) -- 3.88 against 3.93 ms per step at the bench shape; on the second stream it costs 4 %
        def bias_job():
            bws, nbws = _brelu_bwd_ws(B, M, Fout, 1, bias_kind, dev)
            if ctx.mean:
                _lib.check(_launch('bias_grad', B * M * (4.0 + Fout * 0.25), 0.0, lambda: lib.chebgcn_bias_grad_relu_mean(
                    _p(gout), _p(argmax), _p(dbias), bias_kind, B, M, Fout, _p(bws), nbws, _stream())), 'bias_grad_relu_mean')
                return
            _lib.check(_launch('bias_grad', B * Fout * M * (4.0 + 0.25), 0.0, lambda: lib.chebgcn_brelu_pool_bwd(
                _p(gout), None, _p(argmax), None, _p(dbias), bias_kind, B, M, Fout, 1, pool_kind, 1, _p(bws), nbws,
                _stream())), 'brelu_pool_bwd')
        return gout, argmax, None, bias_job
    bk = bias_kind if dbias is not None else BIAS_NONE
    if ch.dy == 'dy16':
        # one-pass bf16 gradients of a wide layer: the ReluGrad pass writes dy as bf16 -- what the matrix cores would round it
        # to anyway (bit-identical results), half the bytes of the largest operand of both gradients
        dy = torch.empty((B, Fout, g.Mp), dtype=torch.bfloat16, device=dev)
        bws, nbws = _brelu_bwd_ws(B, M, Fout, 1, bk, dev)
        _lib.check(_launch('relu_grad_bf16', B * Fout * M * (6.0 + 0.25), 0.0, lambda: lib.chebgcn_relu_grad_bf16(
            _p(gout), _p(argmax), _p(dy), _p(dbias), bk, B, M, Fout, _p(bws), nbws, _stream())), 'relu_grad_bf16')
        return dy, None, None, None
    if ch.dy == 'link':
        # the layer above stored its input gradient gated by this layer's mask, straight into slab 0 of this stack
        # (GateLink): what is left of the ReluGrad pass is the bias reduction, a plain sum of gated values over the windows
        gstack, ctx.link_out.gstack = ctx.link_out.gstack, None
        dy = gstack[0]
        if dbias is not None:
            # at once, not behind the layer's other gradients like the bias reduction of the 'fold' arm: dy was written
            # by the kernel in front of this one (2.95 against 2.97-3.01 ms per step at the bench shape, same box)
            bws, nbws = _brelu_bwd_ws(B, M, Fout, 1, bias_kind, dev)
            _lib.check(_launch('bias_grad', B * Fout * M * 4.0, 0.0, lambda: lib.chebgcn_brelu_pool_bwd(
                _p(dy), None, None, None, _p(dbias), bias_kind, B, M, Fout, 1, pool_kind, 0, _p(bws), nbws,
                _stream())), 'brelu_pool_bwd')
        return dy, None, gstack, None
    # 'plain': one pass over gout materialises dy (un-pooling, ReluGrad) and reduces the bias gradient
    if ctx.link_out is not None:
        ctx.link_out.gstack = None
    gstack = None
    if ch.by_fwd:
        gstack = torch.empty((K, B, Fout, g.Mp), dtype=torch.float32, device=dev)
        dy = gstack[0]                      # T_0 of the recurrence on dy: written in place
    else:
        dy = torch.empty((B, Fout, g.Mp), dtype=torch.float32, device=dev)
    Mo = M // pool
    if ctx.pool_maps is not None:
        # pooled between two vertex orders: the forward's selection bytes carry the ReLU of the maximum as well
        nbws = lib.chebgcn_pool_scatter_bwd_workspace(B, M, Fout, pool, bk)
        bws = torch.empty(nbws, dtype=torch.uint8, device=dev) if nbws else None
        _lib.check(_launch('pool_scatter_bwd', B * Fout * (4.0 * M + 5.0 * Mo), 0.0, lambda: lib.chebgcn_pool_scatter_bwd(
            _p(gout), _p(argmax), _p(ctx.pool_maps[1]), _p(dy), _p(dbias), bk, B, M, Fout, pool, pool_kind, relu,
            _p(bws), nbws, _stream())), 'pool_scatter_bwd')
    else:
        # with the ReLU mask of a pool == 1 layer `out` is not read (a byte per four vertices instead)
        nbytes = B * Fout * M * (8.0 + 0.25) if out is None else 4.0 * B * Fout * (2 * Mo + M)
        bws, nbws = _brelu_bwd_ws(B, M, Fout, pool, bk, dev)
        _lib.check(_launch('brelu_pool_bwd', nbytes, 0.0, lambda: lib.chebgcn_brelu_pool_bwd(
            _p(gout), _p(out), _p(argmax), _p(dy), _p(dbias), bk, B, M, Fout,
            pool, pool_kind, relu, _p(bws), nbws, _stream())), 'brelu_pool_bwd')
    return dy, None, gstack, None


def _bwd_w(ctx, ch, stack, dy, mask, dbias, dW_buf, bias_job):
    """The weight gradient, on the second stream where ``ch.side``.  Returns (dW, that stream or None -- the caller joins it --,
    the bias job if it is still to be enqueued)."""
    lib = _lib.lib()
    B, M, Fin, K, Fout = ctx.cfg[:5]
    dev = dy.device
    passes = PRECISIONS[ctx.precision]
    ws = _workspace((lib.chebgcn_contract_bwd_w_bf16_workspace if passes else lib.chebgcn_contract_bwd_w_workspace)(
        B, M, Fin, K, Fout), dev)
    if dW_buf is not None:
        _check_grad_buffer(dW_buf, (Fin * K, Fout), 'dW')
        dW = dW_buf                       # written, not accumulated: one use per step
    else:
        dW = torch.empty((Fin * K, Fout), dtype=torch.float32, device=dev)
    arm = _BWD_W[ch.grads]
    args = ([_p(stack), _p(dy)] + ([_p(mask)] if arm.mask else []) + [_p(dW)] + ([_p(dbias)] if arm.dbias else [])
            + [_p(ws), ws.numel(), B, M, Fin, K, Fout] + ([passes] if arm.passes else []))
    what = 'contract_bwd_w' + ('_' + ctx.precision if passes else '')

    def launch():
        _lib.check(_launch(what, *_contract_cost(B, M, Fin, K, Fout), lambda: getattr(lib, arm.entry)(*args, _stream())), what)

    if not ch.side:
        launch()
        return dW, None, bias_job
    # dW does not feed dx: it runs beside contract_bwd_x / recurrence_bwd on a second stream
    side = _side_stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch()
        if bias_job is not None and ctx.fused and bias_side_small:
            # atlas-sized layers: the main stream is the critical path of a chain of short launches and the second
            # stream has slack -- the bias reduction goes there too (on the benchmark graph that costs 4 %: it stays
            # behind contract_bwd_x / recurrence_bwd on the main stream)
            bias_job()
            bias_job = None
    return dW, side, bias_job


def _bwd_x(ctx, ch, Wc, dy, mask, gstack):
    """The input gradient: fused on chip, by the forward recurrence on dy (``ch.by_fwd``; ``gstack``: the stack whose slab 0 dy
    is), or in Clenshaw form."""
    lib = _lib.lib()
    B, M, Fin, K, Fout = ctx.cfg[:5]
    g, dev = ctx.graph, dy.device
    if ctx.fused:
        # G_j = dy W_j^T on the matrix cores feeding the adjoint recurrence on chip: no gradient stack in memory
        dx = torch.empty((B, Fin, g.Mp), dtype=torch.float32, device=dev)
        _lib.check(_launch('fused_layer_bwd_x', 4.0 * B * M * (Fin + Fout), 2.0 * B * M * Fin * K * Fout,
                           lambda: lib.chebgcn_fused_layer_bwd_x(g.handle, _p(dy), _p(mask), _p(Wc), _p(dx), B, Fin, K, Fout,
                                                                 _stream())), 'fused_layer_bwd_x')
        return dx
    if ch.by_fwd:
        _lib.check(_launch('recurrence_fwd_t', 4.0 * B * M * Fout * K, 0.0, lambda: lib.chebgcn_recurrence_fwd_t(
            g.handle, _p(dy), _p(gstack), B, Fout, K, _stream())), 'recurrence_fwd_t')
        Wt = ctx.Wt                                                                        # W'[fo*K + k][fin] = W[fin*K + k][fo]
        if Wt is None or tuple(Wt.shape) != (Fout * K, Fin):
            Wt = torch.empty((Fout * K, Fin), dtype=torch.float32, device=dev)
            _lib.check(lib.chebgcn_reindex_weights(_p(Wc), _p(Wt), Fin, K, Fout, _stream()), 'reindex_weights')
        li, gate = ctx.link_in, None
        if (li is not None and li.mask is not None and ctx.precision == 'f32' and li.shape[1:] == (B, Fin, g.Mp)
                and lib.chebgcn_contract_fwd_gated_supported(B, M, Fout, K, Fin)):
            # the layer below wants its dy as slab 0 of a gradient stack: this contraction stores it there, gated by that
            # layer's ReLU mask
            li.gstack = torch.empty(li.shape, dtype=torch.float32, device=dev)
            dx, gate = li.gstack[0], li.mask
        else:
            dx = torch.empty((B, Fin, g.Mp), dtype=torch.float32, device=dev)
        contract_fwd_into(gstack, Wt, None, BIAS_NONE, dx, None, B, M, Fout, K, Fin, 1, POOL_MAX, False, ctx.precision,
                          what='contract_bwd_x', gate=gate)
        return dx
    gstack = torch.empty((K, B, Fin, g.Mp), dtype=torch.float32, device=dev)
    arm = _BWD_X[ch.grads]
    passes = PRECISIONS[ctx.precision]
    name = 'contract_bwd_x' + ('_' + ctx.precision if passes else '')
    args = [_p(dy)] + ([_p(mask)] if arm.mask else []) + [_p(Wc), _p(gstack), B, M, Fin, K, Fout] + ([passes] if arm.passes else [])
    if passes:
        nws = lib.chebgcn_contract_bwd_x_bf16_workspace(Fin, K, Fout)
        args += [_p(_workspace(nws, dev, 'bwd_x_bf16')), nws]                  # its own: bwd_w may be running beside it
    _lib.check(_launch(name, *_contract_cost(B, M, Fin, K, Fout, arm.planes), lambda: getattr(lib, arm.entry)(*args, _stream())),
               arm.what or name)
    dx = torch.empty((B, Fin, g.Mp), dtype=torch.float32, device=dev)
    _lib.check(_launch('recurrence_bwd', 4.0 * B * M * Fin * (K + 1), 0.0, lambda: lib.chebgcn_recurrence_bwd(
        g.handle, _p(gstack), _p(dx), B, Fin, K, _stream())), 'recurrence_bwd')
    return dx


class ChebConv(torch.autograd.Function):
    """y = pool(act(sum_k T_k(L~) x W_k + bias)) on plane storage tensors.

    forward : recurrence_fwd (models_gcn.py:598-610) + contract_fwd (:611-648); four exits -- the fused atlas layer, the fused
              feature mean, pooling between two vertex orders, the plain one -- which all end in ``_keep``
    backward: ``_bwd_choose`` decides, then ``_bwd_dy`` (brelu_pool_bwd and its kin), ``_bwd_w`` (contract_bwd_w*) and
              ``_bwd_x`` (contract_bwd_x* + recurrence_bwd, or recurrence_fwd_t + contract_fwd) only launch; for pool == 1
              layers with ReLU the ReluGrad runs inside contract_bwd_w_relu / contract_bwd_x_relu on the bit mask the
              forward left, and brelu_pool_bwd only reduces the bias gradient
    ``bufs`` is a ``Buffers`` holder (kept out of autograd's sight): ``bufs.stack`` is an
    optional preallocated [K, B, Fin, Mp] buffer -- when ``x`` already is its slab 0 no copy
    of T_0 is made; ``bufs.out`` optionally receives the result, e.g. slab 0 of the next
    layer's stack.
    """

    @staticmethod
    def _keep(ctx, bufs, graph, cfg, bias, saved, fold=False, mean=False, fused=False, precision='f32', pool_maps=None, Wt=None,
              link_in=None, link_out=None):
        """Everything ``backward`` reads, in one place: what differs between the forward's exits is passed in, the rest comes
        from ``bufs``.  ``saved``: (stack, W, out, mask / argmax / selection bytes)."""
        ctx.save_for_backward(*saved)
        ctx.fold, ctx.mean, ctx.fused = fold, mean, fused
        ctx.graph, ctx.cfg = graph, cfg
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        ctx.grad_bufs = (bufs.dW, bufs.dbias)
        ctx.done = bufs.done
        ctx.precision = precision
        ctx.pool_maps = pool_maps
        ctx.Wt = Wt
        ctx.link_in, ctx.link_out = link_in, link_out

    @staticmethod
    def forward(ctx, x, W, bias, graph, K, pool, pool_kind, relu, bias_kind, bufs):
        _require_cuda(x, W, bias)
        if bufs is None:
            # a bare ChebConv.apply without buffers: the caller's grad mode counts as on (grad mode is always off in here, and
            # that is what a Buffers() made here would record)
            bufs = Buffers()
            bufs.grad_mode = True
        stack = bufs.stack
        given = None if bufs.out is None else bufs.out.detach()                # fresh alias: an output, not an input, for autograd
        lib = _lib.lib()
        x = x if x.is_contiguous() else x.contiguous()
        B, Fin, Mp = x.shape
        M = graph.M
        if Mp != graph.Mp:
            raise ValueError('activation plane stride %d does not match the graph (%d vertices)' % (Mp, M))
        FinK, Fout = W.shape
        if FinK != Fin * K:
            raise ValueError('weight rows %d != Fin*K = %d' % (FinK, Fin * K))
        Wc = W.detach().contiguous()
        b = _detached(bias)
        Mo = M // pool
        mean, precision = bool(bufs.mean), bufs.precision
        need_w = ctx.needs_input_grad[1]
        wants_grad = bufs.grad_mode and any(ctx.needs_input_grad[:3])         # inference: no mask is written
        # atlas-sized graphs (<= 384 vertices, Fin, Fout <= 32, no pooling): the whole layer in one on-chip launch
        # (csrc/fused_small.hip); the stack is written only when a weight gradient will read it
        if (fused_small and pool == 1 and precision == 'f32' and not mean
                and lib.chebgcn_fused_layer_supported(graph.handle, B, Fin, K, Fout)):
            if not (bufs.grad_mode and need_w):
                stack = None                      # nothing will read it (inference, frozen weights): it is never written
            elif stack is None:
                stack = torch.empty((K, B, Fin, Mp), dtype=torch.float32, device=x.device)
            out = _out_buffer(given, B, Fout, M, x.device)
            mask = torch.empty((B, Fout, Mp // 4), dtype=torch.uint8, device=x.device) if (relu and wants_grad) else None
            nws = lib.chebgcn_fused_layer_workspace(graph.handle, B, Fin, K, Fout)
            ws = _workspace(nws, x.device, 'fused_fwd') if nws else None
            nbytes = 4.0 * B * M * (Fin + Fout + (Fin * (K - 1) if stack is not None else 0))
            _lib.check(_launch('fused_layer_fwd', nbytes, 2.0 * B * M * Fin * K * Fout, lambda: lib.chebgcn_fused_layer_fwd(
                graph.handle, _p(x), _p(Wc), _p(b), bias_kind, _p(stack), _p(out), _p(mask), _p(ws), nws, B, Fin, K, Fout,
                int(relu), _stream())), 'fused_layer_fwd')
            # (its backward never takes the forward form: no re-indexed weights, no links)
            ChebConv._keep(ctx, bufs, graph, (B, M, Fin, K, Fout, 1, POOL_MAX, int(relu), bias_kind), bias,
                           (stack, Wc, None if relu else out, mask), fold=bool(relu), fused=True)
            return out
        if stack is None:
            stack = torch.empty((K, B, Fin, Mp), dtype=torch.float32, device=x.device)
        # algorithmic bytes: recurrence 4*M*Fin*K per window; the contraction: _contract_cost
        _lib.check(_launch('recurrence_fwd', 4.0 * M * Fin * K * B, 0.0, lambda: lib.chebgcn_recurrence_fwd(
            graph.handle, _p(x), _p(stack), B, Fin, K, _stream())), 'recurrence_fwd')
        cfg = (B, M, Fin, K, Fout, pool, pool_kind, int(relu), bias_kind)
        # the stack feeds the weight gradient alone: without one (saliency passes) it is not kept alive until the backward
        kept = stack if need_w else None
        if mean:
            if not conv_mean_supported(B, M, Fin, K, Fout, pool, relu, precision):
                raise ValueError('cheb_conv(mean=True): layer not served (ops.conv_mean_supported)')
            mask = torch.empty((B, Fout, Mp // 4), dtype=torch.uint8, device=x.device) if wants_grad else None
            y = torch.empty((B, Mp), dtype=torch.float32, device=x.device)
            _lib.check(_launch('contract_fwd', *_contract_cost(B, M, Fin, K, Fout, 1),
                               lambda: lib.chebgcn_contract_fwd_mean(_p(stack), _p(Wc), _p(b), bias_kind, _p(y), _p(mask), B, M,
                                                                     Fin, K, Fout, _stream())), 'contract_fwd_mean')
            ChebConv._keep(ctx, bufs, graph, cfg, bias, (kept, Wc, None, mask), fold=True, mean=True, Wt=bufs.Wt,
                           link_in=bufs.link_in)
            return y[:, :M]                   # the logical [B, M] mean (row stride Mp): its gradient arrives dense
        out = _out_buffer(given, B, Fout, Mo, x.device)
        maps = bufs.pool_maps if pool > 1 else None
        if maps is not None:
            # pooling between two vertex orders: the contraction (bias, ReLU) leaves the unpooled result in the source order,
            # one more pass gathers the clusters (_pool_gather)
            y_full = plane_empty(B, Fout, M, x.device)
            contract_fwd_into(stack, Wc, b, bias_kind, y_full, None, B, M, Fin, K, Fout, 1, pool_kind, relu, precision)
            sel = torch.empty(out.shape, dtype=torch.uint8, device=x.device) if wants_grad else None
            _pool_gather(y_full, maps, out, sel, B, M, Fout, pool, pool_kind, relu)
            ChebConv._keep(ctx, bufs, graph, cfg, bias, (kept, Wc, None, sel), precision=precision, pool_maps=maps, Wt=bufs.Wt,
                           link_in=bufs.link_in)
            return out
        argmax = None
        if pool > 1 and (pool_kind == POOL_MAX or relu):
            argmax = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
        # pool == 1 with ReLU: contract_fwd leaves a bit per vertex (the ReLU mask) and the gradients of the
        # contraction gate the incoming gradient themselves -- no dy tensor, no pass over `out` in backward
        fold = bool(fold_relu_grad and pool == 1 and relu and precision == 'f32')
        if pool == 1 and relu and wants_grad:
            # the mask also serves the separate ReluGrad pass (bf16 gradients): a byte per four vertices instead of `out`
            argmax = torch.empty((B, Fout, Mp // 4), dtype=torch.uint8, device=x.device)
        contract_fwd_into(stack, Wc, b, bias_kind, out, argmax, B, M, Fin, K, Fout, pool, pool_kind, relu, precision)
        link = bufs.link_out
        if link is not None:
            # where this layer's backward will take its gated dy as slab 0 of the stack its recurrence_fwd_t fills (by_fwd in
            # _bwd_choose; of the four exits this one alone makes the offer), the layer above gets the mask to gate with
            link.gstack = None
            ok = bool(gate_links and pool == 1 and relu and wants_grad and argmax is not None and ctx.needs_input_grad[0]
                      and dx_by_forward_shape(graph, Fin, K, Fout, precision))
            link.mask, link.shape = (argmax, (K, B, Fout, Mp)) if ok else (None, None)
        ChebConv._keep(ctx, bufs, graph, cfg, bias, (kept, Wc, None if (pool == 1 and relu) else out, argmax), fold=fold,
                       precision=precision, Wt=bufs.Wt, link_in=bufs.link_in, link_out=link)
        return out

    @staticmethod
    def backward(ctx, gout):
        stack, Wc, out, argmax = ctx.saved_tensors
        dW_buf, dbias_buf = ctx.grad_bufs
        B, M, Fin, K, Fout, pool, pool_kind, relu, bias_kind = ctx.cfg
        if ctx.mean:
            # every filter's dy is gout / Fout, one plane [B][Mp] per window, zero in the padding: scaled into a buffer whose
            # padding was zeroed once (one kernel per step instead of autograd's zero-fill + copy of a sliced output)
            gm = _mean_grad_buffer(B, ctx.graph.Mp, gout.device)
            torch.mul(gout, 1.0 / Fout, out=gm[:, :M])
            gout = gm
        else:
            gout = gout.contiguous()
        dev = gout.device
        dbias = None
        if bias_kind != BIAS_NONE and ctx.needs_input_grad[2]:
            if dbias_buf is not None:
                _check_grad_buffer(dbias_buf, ctx.bias_shape, 'dbias')
                dbias = dbias_buf                 # overwritten, like dW: one use per step
            else:
                dbias = torch.zeros(ctx.bias_shape, dtype=torch.float32, device=dev)
        ch = _bwd_choose(ctx, gout, argmax, dbias)
        dy, mask, gstack, bias_job = _bwd_dy(ctx, ch, gout, out, argmax, dbias)
        dW = side = dx = None
        if ctx.needs_input_grad[1]:
            dW, side, bias_job = _bwd_w(ctx, ch, stack, dy, mask, dbias, dW_buf, bias_job)
        if ctx.needs_input_grad[0]:
            dx = _bwd_x(ctx, ch, Wc, dy, mask, gstack)
        if bias_job is not None:
            bias_job()
        if side is not None:
            # joined before this layer's buffers (stack, dy, workspace) can be reused and before
            # anything consumes dW
            torch.cuda.current_stream(dev).wait_stream(side)
        if ctx.done is not None:
            ctx.done()                            # e.g. dist.DataParallel.layer_done: this layer's gradients are enqueued
        # gradients written into the caller's buffers are not handed to autograd a second time
        return (dx, None if dW_buf is not None else dW, None if dbias_buf is not None else dbias,
                None, None, None, None, None, None, None)


class Buffers:
    """Preallocated buffers for ``cheb_conv`` (plain object, not a tensor).  ``stack`` / ``out``:
    see ChebConv.  ``dW`` / ``dbias``: gradient buffers the backward pass WRITES (overwrites, it
    does not accumulate: one use of a variable per step) in place of returning the gradients to
    autograd -- the model hands over views of its flat gradient buffer and saves an add per
    variable and step.  ``done``: called at the end of the layer's backward, once its gradient
    kernels are enqueued (dist.DataParallel starts the layer's all-reduce from it).  ``mean``: the
    layer is followed by ``tf.reduce_mean(x, -1)`` (models_gcn.py:673) and returns that mean, storage
    [B, Mp], instead of its output (chebgcn_contract_fwd_mean; the gradients read one plane per window)."""
    __slots__ = ('stack', 'out', 'dW', 'dbias', 'precision', 'done', 'mean', 'grad_mode', 'pool_maps', 'Wt', 'link_in', 'link_out')

    def __init__(self, stack=None, out=None, dW=None, dbias=None, precision='f32', done=None, mean=False, pool_maps=None, Wt=None,
                 link_in=None, link_out=None):
        # ``GateLink`` objects shared with the layer below (link_in) / above (link_out) when this layer's input IS that layer's
        # output and nothing else reads it: the upper layer's input gradient is then stored gated by the lower layer's ReLU mask
        self.link_in, self.link_out = link_in, link_out
        # the layer's weights already re-indexed for the forward form of the input gradient (reindex_weights_batch: the model
        # does every layer in one launch in front of the backward pass); None: the backward pass re-indexes them itself
        self.Wt = Wt
        self.stack, self.out, self.dW, self.dbias, self.precision, self.done = stack, out, dW, dbias, precision, done
        # a pooled layer whose input and / or output vertices are not in the coarsening's tree order: (pmap, smap), int32 device
        # tensors of M entries each (``pool_maps``); the layer then pools through them (chebgcn_pool_gather_fwd / _scatter_bwd)
        self.pool_maps = pool_maps
        self.mean = mean          # the layer returns the mean over its filters, [B, Mp] (see conv_mean_supported)
        # the caller's grad mode: inside Function.forward grad mode is always off, and ``ctx.needs_input_grad`` is True for a
        # Parameter even under torch.no_grad() -- with this off nothing that only a backward pass would read is written
        # (the ReLU mask; in the fused atlas layer the whole K-slab stack)
        self.grad_mode = torch.is_grad_enabled()


class GateLink:
    """What two consecutive ``cheb_conv`` layers share so that the ReluGrad of the lower one runs in the epilogue of the upper
    one's input gradient (TF autodiff chains exactly these two ops: models_gcn.py:616 -> :625/:629 of the previous layer).

    The caller creates one per pair -- ``Buffers(link_out=l)`` for the lower layer, ``Buffers(link_in=l)`` for the upper -- and
    thereby states that the lower layer's output feeds the upper layer and NOTHING else.  The lower layer's forward fills
    ``mask`` / ``shape`` when its own backward will want its dy as slab 0 of a gradient stack; the upper layer's backward then
    allocates that stack, stores its gated input gradient there (``gstack``) and returns the slab to autograd; the lower layer's
    backward recognises the slab BY ADDRESS (anything else -- a copy, a sum with another gradient -- takes the ordinary pass, and
    gating a gated gradient again changes nothing) and only reduces its bias gradient."""
    __slots__ = ('mask', 'shape', 'gstack')

    def __init__(self):
        self.mask = self.shape = self.gstack = None


gate_links = os.environ.get('CHEBGCN_GATE_LINKS', '1') != '0'
merge_bias_small = os.environ.get('CHEBGCN_MERGE_BIAS_SMALL', '1') != '0'     # the bias gradient in the weight gradient's reduce launch (small launches)


def conv_mean_supported(B, M, Fin, K, Fout, pool, relu, precision='f32'):
    """Can ``cheb_conv(..., mean=True)`` serve this layer?  (pool 1, ReLU, fp32 contraction, a shape of the ring kernel.)"""
    precision = resolve_precision(precision, Fin, K, Fout)
    return bool(fold_relu_grad and pool == 1 and relu and precision == 'f32'
                and _lib.lib().chebgcn_contract_fwd_mean_supported(B, M, Fin, K, Fout))


def pool_maps(pool, src_order, dst_order, M, device):
    """Index maps of a pooled layer between two vertex orders (include/chebgcn.h, chebgcn_pool_gather_fwd): the reference pools
    the consecutive vertices ``pool*j .. pool*j + pool - 1`` of its (tree) order into vertex ``j`` (models_gcn.py:631-648).
    ``src_order[v']`` = reference vertex at position ``v'`` of the source level's internal order (None: identity), ``dst_order``
    likewise for the pooled level.  Returns (pmap, smap) int32 device tensors:
    ``pmap[j'*pool + i]`` = source position of member i of pooled position j'; ``smap[v']`` = ``j'*pool + i``."""
    M = int(M)
    Mo = M // pool
    src = np.arange(M, dtype=np.int64) if src_order is None else np.asarray(src_order, np.int64)
    dst = np.arange(Mo, dtype=np.int64) if dst_order is None else np.asarray(dst_order, np.int64)
    if src.shape != (M,) or dst.shape != (Mo,):
        raise ValueError('pool_maps: orders of %d / %d vertices expected' % (M, Mo))
    inv_src = np.empty(M, np.int64)
    inv_src[src] = np.arange(M)
    pmap = inv_src[(pool * dst[:, None] + np.arange(pool)[None, :]).reshape(-1)]
    smap = np.empty(M, np.int64)
    smap[pmap] = np.arange(M)
    dev = torch.device(device)
    return (torch.as_tensor(pmap.astype(np.int32)).to(dev), torch.as_tensor(smap.astype(np.int32)).to(dev))


def reindex_weights_batch(Ws, shapes):
    """``[W'_l]`` for the layers ``Ws`` ([Fin*K, Fout] each, ``shapes`` = [(Fin, K, Fout)]) in ONE launch
    (chebgcn_reindex_weights_batch): W'[fo*K + k][fin] = W[fin*K + k][fo]."""
    n = len(Ws)
    if n == 0:
        return []
    if n > 16:
        return reindex_weights_batch(Ws[:16], shapes[:16]) + reindex_weights_batch(Ws[16:], shapes[16:])
    _require_cuda(*Ws)
    Ws = [w.detach() if w.is_contiguous() else w.detach().contiguous() for w in Ws]
    total = sum(fi * k * fo for fi, k, fo in shapes)
    flat = torch.empty(total, dtype=torch.float32, device=Ws[0].device)
    outs, at = [], 0
    for fi, k, fo in shapes:
        outs.append(flat[at:at + fi * k * fo].view(fo * k, fi))
        at += fi * k * fo
    arr_p = (C.c_void_p * n)
    arr_i = (C.c_int * n)
    _lib.check(_lib.lib().chebgcn_reindex_weights_batch(
        n, arr_p(*[w.data_ptr() for w in Ws]), arr_p(*[o.data_ptr() for o in outs]), arr_i(*[s[0] for s in shapes]),
        arr_i(*[s[1] for s in shapes]), arr_i(*[s[2] for s in shapes]), _stream()), 'reindex_weights_batch')
    return outs


def cheb_conv(x, W, bias, graph, K, pool=1, pool_kind=POOL_MAX, relu=False, bias_kind=BIAS_NONE, stack=None, out=None,
              dW=None, dbias=None, precision='f32', done=None, mean=False, pool_maps=None, Wt=None, link_in=None, link_out=None):
    """``precision``: arithmetic of the contraction and of its two gradients ('auto': resolve_precision; 'f32', 'bf16', 'bf16x3':
    chebgcn_contract_fwd_bf16 / _bwd_x_bf16 / _bwd_w_bf16 with 1 or 3 passes); storage, the recurrence, its adjoint
    and the bias / ReLU / pooling gradients stay fp32.  ``link_in`` / ``link_out``: ``GateLink``."""
    precision = resolve_precision(precision, x.shape[1], K, W.shape[1])
    bufs = Buffers(stack, out, dW, dbias, precision, done, mean, pool_maps if pool > 1 else None, Wt, link_in, link_out)
    return ChebConv.apply(x, W, bias, graph, K, pool, pool_kind, relu, bias_kind, bufs)


def conv_windows(win, W, bias, graph, K, C, pool=1, pool_kind=POOL_MAX, relu=True, bias_kind=BIAS_NONE, out=None, pool_maps=None):
    """The first conv layer of a batch of windows of ONE longer series (``decode.Windows``: the series' Chebyshev stack
    ``[K, T, Mp]`` and the batch's window starts), forward only: chebgcn_contract_fwd_windows in place of ``cheb_conv``'s
    recurrence + contraction -- the same products in the same order.  ``out`` / ``pool_maps``: as ``cheb_conv``."""
    lib = _lib.lib()
    _require_cuda(win.stack, win.starts, W, bias)
    B, M, Mp = win.B, graph.M, graph.Mp
    Fout = int(W.shape[1])
    if tuple(win.stack.shape) != (K, win.T, Mp) or not win.stack.is_contiguous() or win.starts.dtype != torch.int32:
        raise ValueError('conv_windows: stack [K, T, Mp] float32 and int32 starts expected')
    if W.shape[0] != C * K:
        raise ValueError('weight rows %d != C*K = %d' % (W.shape[0], C * K))
    W, b = _detached(W), _detached(bias)
    maps = pool_maps if pool > 1 else None
    cp = 1 if maps is not None else pool
    out = _out_buffer(out, B, Fout, M // pool, W.device)
    y = plane_empty(B, Fout, M, W.device) if maps is not None else out
    _lib.check(_launch('contract_fwd_windows', 4.0 * B * M * (C * K + Fout / cp), 2.0 * B * M * C * K * Fout,
                       lambda: lib.chebgcn_contract_fwd_windows(_p(win.stack), win.T, _p(win.starts), _p(W), _p(b), bias_kind, _p(y),
                                                                None, B, M, C, K, Fout, cp, pool_kind, int(relu), _stream())),
               'contract_fwd_windows')
    if maps is not None:
        _pool_gather(y, maps, out, None, B, M, Fout, pool, pool_kind, relu)
    return out


class BiasReluPool(torch.autograd.Function):
    """Standalone bias + ReLU + pooling (b1relu / b2relu / mpool1 / apool1 called on their
    own, models_gcn.py:619-648) on plane storage tensors."""

    @staticmethod
    def forward(ctx, x, bias, M, pool, pool_kind, relu, bias_kind):
        _require_cuda(x, bias)
        x = x if x.is_contiguous() else x.contiguous()
        B, F, Mp = x.shape
        out = plane_empty(B, F, M // pool, x.device)
        argmax = None
        if pool > 1 and (pool_kind == POOL_MAX or relu):
            argmax = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
        b = bias.detach().contiguous() if bias is not None else None
        _lib.check(_lib.lib().chebgcn_brelu_pool_fwd(_p(x), _p(b), bias_kind, _p(out), _p(argmax), B, M, F, pool,
                                                     pool_kind, int(relu), _stream()), 'brelu_pool_fwd')
        ctx.save_for_backward(out, argmax)
        ctx.cfg = (B, M, F, pool, pool_kind, int(relu), bias_kind, Mp)
        ctx.bias_shape = None if bias is None else tuple(bias.shape)
        return out

    @staticmethod
    def backward(ctx, gout):
        out, argmax = ctx.saved_tensors
        B, M, F, pool, pool_kind, relu, bias_kind, Mp = ctx.cfg
        gout = gout.contiguous()
        dy = torch.empty((B, F, Mp), dtype=torch.float32, device=gout.device)
        dbias = None
        if bias_kind != BIAS_NONE and ctx.needs_input_grad[1]:
            dbias = torch.zeros(ctx.bias_shape, dtype=torch.float32, device=gout.device)
        bk = bias_kind if dbias is not None else BIAS_NONE
        bws, nbws = _brelu_bwd_ws(B, M, F, pool, bk, gout.device)
        _lib.check(_lib.lib().chebgcn_brelu_pool_bwd(_p(gout), _p(out), _p(argmax), _p(dy), _p(dbias), bk, B, M, F, pool,
                                                     pool_kind, relu, _p(bws), nbws, _stream()), 'brelu_pool_bwd')
        return dy, dbias, None, None, None, None, None


# ------------------------------------------------------------------------------------
# spectral filters (filter = 'fourier' / 'spline', models_gcn.py:512-556)
# ------------------------------------------------------------------------------------

def spectral_basis(U, device):
    """The Fourier basis ``U[vertex, frequency]`` (``graph.fourier``) as the device operand of the spectral kernels:
    ``[Mp, Mp]`` fp32, zero-padded."""
    U = np.asarray(U, np.float32)
    M = U.shape[0]
    Mp = plane_stride(M)
    host = np.zeros((Mp, Mp), np.float32)
    host[:M, :M] = U
    return torch.as_tensor(host).to(device)


def _spectral_flops(R, Mp):
    return 2.0 * R * Mp * Mp


def spectral_transform(x, basis, M, transpose):
    """Planes ``x[B, F, Mp]`` -> ``out[r][j] = sum_m x[r][m] U[m][j]`` (analysis) or ``sum_m x[r][m] U[j][m]``
    (synthesis, ``transpose``) on the matrix cores (chebgcn_spectral_transform)."""
    _require_cuda(x, basis)
    x = x if x.is_contiguous() else x.contiguous()
    B, F, Mp = x.shape
    out = torch.empty_like(x)
    R = B * F
    _launch('spectral_synthesis' if transpose else 'spectral_analysis', 4.0 * (2 * R * Mp + Mp * Mp), _spectral_flops(R, Mp),
            lambda: _lib.check(_lib.lib().chebgcn_spectral_transform(_p(x), _p(basis), _p(out), R, M, int(bool(transpose)),
                                                                     _stream()), 'spectral_transform'))
    return out


def _spectral_operands(what, **tensors):
    """The shared entry checks of the spectral wrappers below: device tensors, fp32, of the stated rank, contiguous (a view is
    copied, as in spectral_transform).  ``tensors``: name -> (tensor, rank).  Returns the contiguous tensors in order."""
    _require_cuda(*(t for t, _ in tensors.values()))
    out = []
    for name, (t, rank) in tensors.items():
        if t.dtype != torch.float32 or t.dim() != rank:
            raise ValueError('%s: %s must be a %d-D fp32 tensor, got %s %s' % (what, name, rank, t.dtype, tuple(t.shape)))
        out.append(t if t.is_contiguous() else t.contiguous())
    return out


def spectral_mix(xh, W, M, transpose=False):
    """The per-frequency filter: ``y[b][o][m] = sum_i W[m][o][i] xh[b][i][m]`` (``transpose``: ``sum_o W[m][o][i] dy[b][o][m]``,
    its input gradient); ``W`` is ``[M, Fout, Fin]``, ``xh`` planes ``[B, Fin, Mp]`` (``transpose``: ``[B, Fout, Mp]``)."""
    what = 'spectral_mix_bwd_x' if transpose else 'spectral_mix_fwd'
    xh, W = _spectral_operands(what, planes=(xh, 3), W=(W, 3))
    B, Ni, Mp = xh.shape
    _, Fout, Fin = W.shape
    No = Fin if transpose else Fout
    if Mp != plane_stride(M) or W.shape[0] != M or Ni != (Fout if transpose else Fin):
        raise ValueError('%s: planes %s and W %s do not agree at M = %d' % (what, tuple(xh.shape), tuple(W.shape), M))
    out = torch.empty((B, No, Mp), dtype=torch.float32, device=xh.device)
    fn = _lib.lib().chebgcn_spectral_mix_bwd_x if transpose else _lib.lib().chebgcn_spectral_mix_fwd
    _launch(what, 4.0 * (B * (Ni + No) * Mp + W.numel()), 2.0 * B * M * Fin * Fout,
            lambda: _lib.check(fn(_p(xh), _p(W), _p(out), B, M, Fin, Fout, _stream()), what))
    return out


def spectral_mix_bwd_w(dyh, xh, M):
    """``dW[m][o][fin] = sum_b dyh[b][o][m] xh[b][fin][m]``, summed over the windows in a fixed order."""
    what = 'spectral_mix_bwd_w'
    dyh, xh = _spectral_operands(what, dyh=(dyh, 3), xh=(xh, 3))
    B, Fout, Mp = dyh.shape
    Fin = xh.shape[1]
    if Mp != plane_stride(M) or xh.shape[0] != B or xh.shape[2] != Mp:
        raise ValueError('%s: dyh %s and xh %s do not agree at M = %d' % (what, tuple(dyh.shape), tuple(xh.shape), M))
    dW = torch.empty((M, Fout, Fin), dtype=torch.float32, device=dyh.device)
    _launch(what, 4.0 * (B * (Fin + Fout) * Mp + dW.numel()), 2.0 * B * M * Fin * Fout,
            lambda: _lib.check(_lib.lib().chebgcn_spectral_mix_bwd_w(_p(dyh), _p(xh), _p(dW), B, M, Fin, Fout, _stream()), what))
    return dW


def spline_expand(Bs, Wk, transpose=False):
    """``W = Bs @ Wk`` ([M, K] x [K, C]); ``transpose``: ``dWk = Bs^T @ dW`` (``Wk`` is then dW [M, C])."""
    what = 'spectral_spline_expand_bwd' if transpose else 'spectral_spline_expand'
    Bs, Wk = _spectral_operands(what, Bs=(Bs, 2), Wk=(Wk, 2))
    M, K = Bs.shape
    C = Wk.shape[1]
    if Wk.shape[0] != (M if transpose else K):
        raise ValueError('%s: Bs %s and %s %s do not agree' % (what, tuple(Bs.shape), 'dW' if transpose else 'Wk', tuple(Wk.shape)))
    if transpose:
        out = torch.empty((K, C), dtype=torch.float32, device=Wk.device)
        fn = _lib.lib().chebgcn_spectral_spline_expand_bwd
    else:
        out = torch.empty((M, C), dtype=torch.float32, device=Wk.device)
        fn = _lib.lib().chebgcn_spectral_spline_expand
    _launch(what, 4.0 * (M * K + (M + K) * C), 2.0 * M * K * C,
            lambda: _lib.check(fn(_p(Bs), _p(Wk), _p(out), M, K, C, _stream()), what))
    return out


class SpectralConv(torch.autograd.Function):
    """``filter_in_fourier`` (models_gcn.py:512-528) on plane storage: analysis, the per-frequency ``[Fout x Fin]`` mix,
    synthesis.  ``W``: ``[M, Fout, Fin]`` (``fourier``, :530-538), or, with the spline basis ``Bs [M, K]`` given, the
    ``[K, Fout*Fin]`` control weights the filter is expanded from (``spline``, :540-556).  Saves the analysed input for
    the weight gradient where one is wanted; returns no input gradient where the input needs none."""

    @staticmethod
    def forward(ctx, x, W, basis, Bs, M, Fout):
        _require_cuda(x, W, basis, Bs)
        x = x if x.is_contiguous() else x.contiguous()
        B, Fin, Mp = x.shape
        if basis.shape != (Mp, Mp):
            raise ValueError('spectral conv: basis %s for planes of %d vertices' % (tuple(basis.shape), M))
        Wd = W.detach().contiguous()
        Wf = (spline_expand(Bs, Wd) if Bs is not None else Wd).view(M, Fout, Fin)
        xh = spectral_transform(x, basis, M, False)
        y = spectral_transform(spectral_mix(xh, Wf, M), basis, M, True)
        ctx.save_for_backward(xh if ctx.needs_input_grad[1] else None, Wf, basis, Bs)
        ctx.M = M
        return y

    @staticmethod
    def backward(ctx, gy):
        xh, Wf, basis, Bs = ctx.saved_tensors
        M = ctx.M
        gy = gy if gy.is_contiguous() else gy.contiguous()
        dyh = spectral_transform(gy, basis, M, False)          # the adjoint of synthesis is analysis
        dx = dW = None
        if ctx.needs_input_grad[1]:
            dW = spectral_mix_bwd_w(dyh, xh, M)
            if Bs is not None:
                dW = spline_expand(Bs, dW.view(M, -1), transpose=True)
        if ctx.needs_input_grad[0]:
            dx = spectral_transform(spectral_mix(dyh, Wf, M, transpose=True), basis, M, True)
        return dx, dW, None, None, None, None


class FeatureMean(torch.autograd.Function):
    """tf.reduce_mean(x, -1) (models_gcn.py:673): storage [B, F, Mp] -> dense [B, M]."""

    @staticmethod
    def forward(ctx, x, M):
        _require_cuda(x)
        x = x if x.is_contiguous() else x.contiguous()
        B, F, Mp = x.shape
        y = torch.empty((B, M), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().chebgcn_feature_mean_fwd(_p(x), _p(y), B, M, F, _stream()), 'feature_mean_fwd')
        ctx.cfg = (B, M, F, Mp)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, M, F, Mp = ctx.cfg
        gy = gy.contiguous()
        dx = torch.empty((B, F, Mp), dtype=torch.float32, device=gy.device)
        _lib.check(_lib.lib().chebgcn_feature_mean_bwd(_p(gy), _p(dx), B, M, F, _stream()), 'feature_mean_bwd')
        return dx, None


FC_BWD_MAX_INNER = int(os.environ.get('CHEBGCN_FC_BWD_MAX_INNER', 4096))      # beyond: the gradients stay on the vendor GEMMs (tools/probes/fc_small_probe.py)
FC_FWD_MAX_INNER = int(os.environ.get('CHEBGCN_FC_FWD_MAX_INNER', 1 << 20))     # A/B knob for bench runs


def _fc_fwd(rows, ld, W, b, relu, timer_name):
    """The one launch of chebgcn_fc_fwd: ``act(rows @ W + b)``, float32 ``[B, O]``.  ``rows``: ``B`` rows of row stride ``ld``
    floats, the first ``I = W.shape[0]`` of each the input; ``W`` and ``b`` contiguous.  The caller has asked
    chebgcn_fc_fwd_supported.  ``timer_name``: the entry of ``ops.timers`` the launch is counted under, None for none."""
    B, (I, O) = rows.shape[0], W.shape
    L = _lib.lib()
    y = torch.empty((B, O), dtype=torch.float32, device=rows.device)
    nws = L.chebgcn_fc_fwd_workspace(B, I, O)
    ws = _workspace(nws, rows.device, 'fc_fwd') if nws else None
    call = lambda: L.chebgcn_fc_fwd(_p(rows), ld, _p(W), _p(b), _p(y), _p(ws), nws, B, I, O, 1 if relu else 0, _stream())
    _lib.check(_launch(timer_name, 4.0 * (B * I + I * O + B * O), 2.0 * B * I * O, call) if timer_name else call(), 'fc_fwd')
    return y


def _fc_bwd(rows, ld, W, g, y, dW, db, dx, lddx, timer_name):
    """The one launch of chebgcn_fc_bwd for ``rows`` as in ``_fc_fwd``: WRITES the weight and bias gradients into ``dW`` / ``db``
    and the input gradient into ``dx`` (row stride ``lddx``), each where given; ReluGrad on ``y`` where given.  ``timer_name``
    as in ``_fc_fwd``, and what a failure is reported as ('fc_bwd' without one)."""
    B, (I, O) = rows.shape[0], W.shape
    need_w, need_x = dW is not None, dx is not None
    call = lambda: _lib.lib().chebgcn_fc_bwd(_p(rows), ld, _p(W), _p(g), _p(y), _p(dW), _p(db), _p(dx), lddx, B, I, O, _stream())
    # 'fc_bwd' counts the rows as read whichever gradients are formed; 'fc_bwd_x' (no dW: the rows are not read) does not
    nbytes = 4.0 * (B * I * ((timer_name != 'fc_bwd_x') + need_x) + I * O * (1 + need_w) + B * O)
    _lib.check(_launch(timer_name, nbytes, 2.0 * B * I * O * (need_w + need_x), call) if timer_name else call(),
               timer_name or 'fc_bwd')


def fc_forward(x, W, b, relu):
    """``act(x @ W + b)`` of the head's FC layers (models_gcn.py:650-656) by the library's small-product kernel, or None
    where the product is outside its range (large or odd inner size: the caller uses the vendor GEMM).  x may be a
    [B, M] view of a [B, Mp] buffer."""
    if not (x.is_cuda and x.dtype == torch.float32 and W.dtype == torch.float32 and x.dim() == 2 and W.is_contiguous()
            and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0):
        return None
    B, I = x.shape
    if I > FC_FWD_MAX_INNER or not _lib.lib().chebgcn_fc_fwd_supported(B, I, W.shape[1]):
        return None
    return _fc_fwd(x, x.stride(0), W, b, relu, None)       # (outside ops.timers: the 'fc_fwd' entry is the native callers' alone)


def fc_backward(x, W, g, y, dW, db, need_dx):
    """The three gradients of ``act(x @ W + b)`` (ReluGrad on ``y`` where given) by the library kernels: dW and db are
    WRITTEN into the given buffers.  Returns ``(dx,)`` (``(None,)`` unless ``need_dx``), or None where fc_forward would
    decline and nothing was launched."""
    B, I = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.stride(1) == 1 and W.is_contiguous() and g.is_contiguous()
            and dW.is_contiguous() and db.is_contiguous() and (y is None or y.is_contiguous())
            and I <= FC_BWD_MAX_INNER and _lib.lib().chebgcn_fc_fwd_supported(B, I, W.shape[1])):
        return None
    dx = torch.empty((B, I), dtype=torch.float32, device=x.device) if need_dx else None
    _fc_bwd(x, x.stride(0), W, g, y, dW, db, dx, I, None)
    return (dx,)


def _optimizer_step(entry, p, g, m, v, n_reg, lr_t, sq_partials, beta1, beta2, eps, grad_scale, l2, timer_name=None):
    """The checks and the call of every optimizer entry point chebgcn_<entry> on flat fp32 buffers.  ``lr_t``: a Python float,
    or a one-element float32 DEVICE tensor read when the kernel runs (the form a captured step graph replays).  ``n_reg``: None
    for the entries without that argument.  ``sq_partials``: None for plain ``adam_step``, whose two C entry points take the
    step size one way each and which alone accepts no elements; else the buffer of the partial sums of squares, and the number
    of partials written is returned."""
    sq = sq_partials is not None
    _require_cuda(p, g, m, v, sq_partials)
    n = p.numel()
    if not (g.numel() == m.numel() == v.numel() == n) or (sq and n == 0) or not (n_reg is None or 0 <= n_reg <= n):
        raise ValueError('%s: size mismatch' % entry)
    lib = _lib.lib()
    nparts = lib.chebgcn_adam_partials(n) if sq else None
    if sq and (sq_partials.dtype != torch.float32 or sq_partials.numel() < nparts):
        raise ValueError('%s: sq_partials needs %d float32' % (entry, nparts))
    dev_lr = isinstance(lr_t, torch.Tensor)
    if dev_lr:
        if not sq:
            _require_cuda(lr_t)
        if lr_t.dtype != torch.float32 or lr_t.numel() != 1 or not lr_t.is_cuda:
            raise ValueError('%s: a device lr_t must be one float32' % entry)
    if sq:
        lr = (0.0 if dev_lr else float(lr_t), _p(lr_t) if dev_lr else None)
    else:
        entry, lr = (entry + '_dev', (_p(lr_t),)) if dev_lr else (entry, (float(lr_t),))
    args = ((_p(p), _p(g), _p(m), _p(v), n) + (() if n_reg is None else (int(n_reg),)) + lr
            + (float(beta1), float(beta2), float(eps), float(grad_scale), float(l2)) + ((_p(sq_partials),) if sq else ())
            + (_stream(),))
    call = lambda: getattr(lib, 'chebgcn_' + entry)(*args)
    _lib.check(_launch(timer_name, 28.0 * n, 0.0, call) if timer_name else call(), entry)     # reads p, g, m, v; writes p, m, v
    return nparts


def adam_step(p, g, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
    """In-place TF-form Adam on flat fp32 buffers (models_gcn.py:296).  ``lr_t``: a Python float (chebgcn_adam_step), or a
    one-element fp32 DEVICE tensor read when the kernel runs (chebgcn_adam_step_dev)."""
    _optimizer_step('adam_step', p, g, m, v, None, lr_t, None, beta1, beta2, eps, grad_scale, l2)


def adam_step_sq(p, g, m, v, lr_t, sq_partials, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
    """``adam_step`` that also leaves the per-workgroup partial sums of squares of the PRE-update ``p`` in ``sq_partials``
    (float32, at least ``adam_partials(n)`` elements): the L2 term of the loss without a pass of its own.  Returns the
    number of partials written."""
    return _optimizer_step('adam_step_sq', p, g, m, v, None, lr_t, sq_partials, beta1, beta2, eps, grad_scale, l2)


def adam_step_sq_all(p, g, m, v, n_reg, lr_t, sq_partials, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
    """``adam_step_sq`` over ALL variables in one launch: the first ``n_reg`` elements are regularised (L2 term in the gradient,
    counted in the partial sums of squares), the rest -- the biases -- take plain Adam.  Returns the number of partials."""
    return _optimizer_step('adam_step_sq_all', p, g, m, v, n_reg, lr_t, sq_partials, beta1, beta2, eps, grad_scale, l2)


def nadam_step_sq_all(p, g, m, v, n_reg, lr_t, sq_partials, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, l2=0.0):
    """Nadam -- tf.contrib.opt.NadamOptimizer, TF's ApplyAdam with use_nesterov (finetuning_cgcnn, models_gcn.py:895-933) --
    over ``p`` in one launch (chebgcn_nadam_step_sq_all): the first ``n_reg`` elements take the L2 term and leave the partial
    sums of squares of their PRE-update values in ``sq_partials``, the rest plain Nadam.  Returns the number of partials."""
    return _optimizer_step('nadam_step_sq_all', p, g, m, v, n_reg, lr_t, sq_partials, beta1, beta2, eps, grad_scale, l2, 'nadam')


def planes_to_rows(planes, M, order=None, ld=None, out=None):
    """``tf.reshape(conv, [N, M*F])`` (models_gcn.py:805-806) of plane storage ``[B, F, Mp]``: ``[B, ld]`` rows (``ld``
    defaults to M*F rounded up to 4; the columns past M*F are left unwritten), element ``m*F + f`` = vertex m (the caller's
    order), filter f.  ``order``: int32 device tensor, internal position -> reference vertex, or None (planes in the caller's
    order).  ``out``: float32 ``[B, >= M*F]`` with contiguous rows (any row stride) to write into instead of a new tensor."""
    _require_cuda(planes, out)
    B, F, Mp = planes.shape
    if Mp != plane_stride(M) or not planes.is_contiguous():
        raise ValueError('planes_to_rows: planes of %d vertices expected' % M)
    if out is not None:
        if out.dim() != 2 or out.shape[0] != B or out.shape[1] < M * F or out.dtype != torch.float32:
            raise ValueError('planes_to_rows: out must be float32 [%d, >= %d]' % (B, M * F))
        ld = _rows_of(out, int(out.shape[1]), 'planes_to_rows: out')
        rows = out
    else:
        ld = ld or ((M * F + 3) & ~3)
        rows = torch.empty((B, ld), dtype=torch.float32, device=planes.device)
    _lib.check(_launch('planes_to_rows', 8.0 * B * M * F, 0.0, lambda: _lib.lib().chebgcn_planes_to_rows(
        _p(planes), _p(rows), _p(order), B, M, F, ld, _stream())), 'planes_to_rows')
    return rows


def rows_to_planes(rows, M, F, order=None):
    """The adjoint of ``planes_to_rows``: ``[B, >= M*F]`` rows -> plane storage ``[B, F, Mp]``, zero in the pad."""
    _require_cuda(rows)
    B, ld = rows.shape
    if ld < M * F or rows.stride(1) != 1 or rows.stride(0) != ld:
        raise ValueError('rows_to_planes: rows of at least %d floats expected' % (M * F))
    planes = torch.empty((B, F, plane_stride(M)), dtype=torch.float32, device=rows.device)
    _lib.check(_launch('rows_to_planes', 8.0 * B * M * F, 0.0, lambda: _lib.lib().chebgcn_rows_to_planes(
        _p(rows), _p(planes), _p(order), B, M, F, ld, _stream())), 'rows_to_planes')
    return planes


class FlatFC(torch.autograd.Function):
    """The first head layer of ``finetuning_cgcnn``: ``act(reshape(x, [B, M*F]) @ W + b)`` on plane storage ``x`` [B, F, Mp]
    of the top conv layer (models_gcn.py:805-806 and :744-750).  The flatten is chebgcn_planes_to_rows; the product runs on
    the library's FC kernels at every inner size they serve (chebgcn_fc_fwd / chebgcn_fc_bwd called directly: the inner
    size M*F is far beyond FC_BWD_MAX_INNER, which keeps cgcnn's own head where it is).  Backward WRITES dW / db into
    ``gW`` / ``gb`` when they are given; the input gradient, where wanted, goes back to planes (chebgcn_rows_to_planes)."""

    @staticmethod
    def forward(ctx, x, W, b, order, M, relu, gW, gb):
        _require_cuda(x, W, b)
        B, F, Mp = x.shape
        I, O = M * F, W.shape[1]
        if tuple(W.shape) != (I, O) or tuple(b.shape) != (O,):
            raise ValueError('FlatFC: weights [%d, O] and bias [O] expected' % I)
        if not _lib.lib().chebgcn_fc_fwd_supported(B, I, O):
            raise ValueError('FlatFC: %d x %d x %d is outside the range of chebgcn_fc_fwd' % (B, I, O))
        rows = planes_to_rows(x.contiguous(), M, order)
        Wc = W.detach().contiguous()
        y = _fc_fwd(rows, rows.shape[1], Wc, b.detach().contiguous(), relu, 'fc_fwd')
        ctx.save_for_backward(rows, Wc, y if relu else None)
        ctx.cfg, ctx.order, ctx.bufs = (B, M, F, I, O), order, (gW, gb)
        return y

    @staticmethod
    def backward(ctx, g):
        rows, Wc, y = ctx.saved_tensors
        B, M, F, I, O = ctx.cfg
        gW, gb = ctx.bufs
        g = g.contiguous()
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dW = db = drows = None
        if need_w:
            dW = gW if gW is not None else torch.empty((I, O), dtype=torch.float32, device=g.device)
            db = gb if gb is not None else torch.empty((O,), dtype=torch.float32, device=g.device)
            _check_grad_buffer(dW, (I, O), 'dW')
            _check_grad_buffer(db, (O,), 'db')
        if ctx.needs_input_grad[0]:
            drows = torch.empty(rows.shape, dtype=torch.float32, device=g.device)
        if need_w or drows is not None:
            _fc_bwd(rows, rows.shape[1], Wc, g, y, dW, db, drows, rows.shape[1], 'fc_bwd')
        dx = rows_to_planes(drows, M, F, ctx.order) if drows is not None else None
        return (dx, None if gW is not None else dW, None if gb is not None else db, None, None, None, None, None)


def loss_bookkeeping(cross_entropy, sq_partials, nparts, half_reg, ema, corr, decay=0.9):
    """loss = cross_entropy + half_reg * sum(sq_partials[:nparts]); ema <- ema + (1 - decay)(loss - ema) in place;
    returns loss_average = ema * corr (``corr``: float, or one-element device tensor read when the kernel runs)."""
    _require_cuda(cross_entropy, ema)
    out = torch.empty((), dtype=torch.float32, device=ema.device)
    dev_c = isinstance(corr, torch.Tensor)
    _lib.check(_lib.lib().chebgcn_loss_bookkeeping(_p(cross_entropy), _p(sq_partials) if nparts else None, int(nparts), float(half_reg),
                                                   _p(ema), float(decay), 0.0 if dev_c else float(corr), _p(corr) if dev_c else None,
                                                   None, _p(out), _stream()), 'loss_bookkeeping')
    return out


# ------------------------------------------------------------------------------------
# saliency maps (base_model.saliency): the head without weight gradients and the three kernels of csrc/saliency.hip
# ------------------------------------------------------------------------------------

SCORES = {'logit': 0, 'logprob': 1}
SALIENCY_METHODS = {'gradient': 0, 'grad_x_input': 1, 'integrated': 2}


def _fc_rows(x):
    """``x`` [B, I] as rows the library's FC kernels take (row stride a multiple of 4 floats, 16-byte aligned): itself where it
    is such a view, else a copy into a buffer of that stride."""
    B, I = x.shape
    if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.stride(0) >= I and x.data_ptr() % 16 == 0:
        return x
    buf = torch.empty((B, (I + 3) & ~3), dtype=torch.float32, device=x.device)
    buf[:, :I].copy_(x)
    return buf[:, :I]


class FCInputGrad(torch.autograd.Function):
    """``act(x @ W + b)`` of the head whose backward forms the input gradient only (chebgcn_fc_bwd with dW = NULL): what a
    saliency pass runs in place of the layer.  Both directions are the library's kernels at every size chebgcn_fc_fwd serves;
    a size it does not serve raises."""

    @staticmethod
    def forward(ctx, x, W, b, relu):
        _require_cuda(x, W, b)
        B, I = x.shape
        O = W.shape[1]
        if not _lib.lib().chebgcn_fc_fwd_supported(B, I, O):
            raise ValueError('saliency: the FC layer %d x %d x %d is outside the range of chebgcn_fc_fwd' % (B, I, O))
        rows = _fc_rows(x.detach())
        Wc = W.detach().contiguous()
        y = _fc_fwd(rows, rows.stride(0), Wc, b.detach().contiguous(), relu, 'fc_fwd')
        ctx.save_for_backward(rows, Wc, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        rows, Wc, y = ctx.saved_tensors
        dx = torch.empty(rows.shape, dtype=torch.float32, device=g.device)
        _fc_bwd(rows, rows.stride(0), Wc, g.contiguous(), y, None, None, dx, rows.shape[1], 'fc_bwd_x')
        return dx, None, None, None


def saliency_seed(logits, targets, rep, nvalid, score, cls_out=None, want_grad=True):
    """d score / d logits of ``logits [B, C]`` (chebgcn_saliency_seed): row r attributes ``targets[r // rep]`` (int64 device
    tensor) or, with ``targets`` None, its own argmax; rows from ``nvalid`` get zeros.  Writes the attributed class of the
    windows into ``cls_out`` (int64) when given.  Returns dlogits (None unless ``want_grad``)."""
    _require_cuda(logits, targets, cls_out)
    z = logits.detach().contiguous()
    B, C = z.shape
    for t, what in ((targets, 'targets'), (cls_out, 'cls_out')):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < (nvalid + rep - 1) // rep):
            raise ValueError('saliency_seed: %s must be contiguous int64 with a value per window' % what)
    dz = torch.empty_like(z) if want_grad else None
    _lib.check(_launch('saliency_seed', 4.0 * 2 * B * C, 0.0, lambda: _lib.lib().chebgcn_saliency_seed(
        _p(z), _p(targets), int(rep), int(nvalid), SCORES[score], _p(dz), _p(cls_out), B, C, _stream())), 'saliency_seed')
    return dz


def saliency_path(data, order, sample, baseline, R, steps, M):
    """Plane storage ``[R, F, Mp]`` of the integrated-gradients path (chebgcn_saliency_path): row ``w*steps + j`` =
    ``baseline + (j + 1/2)/steps * (data[sample[w]] - baseline)`` in the internal vertex order ``order`` (int32 device,
    internal position -> vertex of ``data``, or None); zero rows behind the windows."""
    _require_cuda(data, order, sample, baseline)
    S, N, F = data.shape
    nw = int(sample.numel())
    out = torch.empty((int(R), F, plane_stride(M)), dtype=torch.float32, device=data.device)
    _lib.check(_launch('saliency_path', 4.0 * F * (nw * N * (1 + (baseline is not None)) + R * plane_stride(M)), 0.0,
                       lambda: _lib.lib().chebgcn_saliency_path(_p(data), _p(order), _p(sample), _p(baseline), _p(out), nw,
                                                                int(steps), int(R), N, int(M), F, _stream())), 'saliency_path')
    return out


def saliency_reduce(dx, data, order, sample, baseline, steps, method, absolute, out, cls=None, acc=None):
    """Input-gradient planes ``dx`` [>= nw*steps, F, Mp] (internal order) -> ``out`` [nw, M, F] in the caller's order (times
    1, x or (x - x0)/steps; ``absolute``: |.|), and with ``acc`` (float64 [C, M, F]) the per-class sums of those rows over
    the windows' classes ``cls`` (int64 [nw]) added to it (chebgcn_saliency_reduce)."""
    _require_cuda(dx, data, order, sample, baseline, out, cls, acc)
    nw, M, F = out.shape
    if not out.is_contiguous() or dx.shape[1] != F or dx.shape[0] < nw * steps or not dx.is_contiguous():
        raise ValueError('saliency_reduce: shapes of dx %s and out %s do not match' % (tuple(dx.shape), tuple(out.shape)))
    if acc is not None and (acc.dtype != torch.float64 or not acc.is_contiguous() or tuple(acc.shape[1:]) != (M, F)
                            or cls is None or cls.dtype != torch.int64 or cls.numel() != nw):
        raise ValueError('saliency_reduce: acc float64 [C, %d, %d] with int64 cls [%d]' % (M, F, nw))
    m = SALIENCY_METHODS[method]
    # dx (the steps of every window), the rows written, x where the method reads it; the class sums read the rows again and
    # update the float64 accumulator
    nbytes = 4.0 * nw * M * F * (steps + 1 + (m > 0) + (m == 2 and baseline is not None))
    if acc is not None:
        nbytes += 4.0 * nw * M * F + 16.0 * acc.shape[0] * M * F
    _lib.check(_launch('saliency_reduce', nbytes, 0.0, lambda: _lib.lib().chebgcn_saliency_reduce(
        _p(dx), _p(data), _p(order), _p(sample), _p(baseline), nw, int(steps), M, F, m, int(bool(absolute)), _p(out), _p(cls),
        int(acc.shape[0]) if acc is not None else 0, _p(acc), _stream())), 'saliency_reduce')
    return out


# ------------------------------------------------------------------------------------
# occlusion maps (base_model.occlusion): the kernels of csrc/occlusion.hip around the inference layers
# ------------------------------------------------------------------------------------

def occlusion_rows(data, order, gid, baseline, r0, R, G, M):
    """Plane storage ``[R, F, Mp]`` of rows ``r0 .. r0 + R - 1`` of an occlusion run (chebgcn_occlusion_rows): row r is window
    ``r // (G + 1)`` of ``data`` with the vertices of group ``r % (G + 1) - 1`` set to ``baseline`` (slot 0: none), in the
    internal vertex order ``order`` (int32 device, internal position -> vertex of ``data``, or None); ``gid``: int32 device
    group of each internal position; zero rows past the last window."""
    _require_cuda(data, order, gid, baseline)
    S, N, F = data.shape
    G1, Mp = int(G) + 1, plane_stride(M)
    out = torch.empty((int(R), F, Mp), dtype=torch.float32, device=data.device)
    windows = max(0, min(S - 1, (int(r0) + int(R) - 1) // G1) - int(r0) // G1 + 1)
    nbytes = 4.0 * (F * (windows * N + (baseline is not None) * N + R * Mp) + M)
    _lib.check(_launch('occlusion_rows', nbytes, 0.0, lambda: _lib.lib().chebgcn_occlusion_rows(
        _p(data), _p(order), _p(gid), _p(baseline), _p(out), int(r0), int(R), S, int(G), N, int(M), F, _stream())),
        'occlusion_rows')
    return out


def occlusion_score(logits, r0, G, cls, score, ref, drop):
    """``drop[w, g]`` (float32 ``[S, G]``) of the rows whose logits ``[R, C]`` a pass from row ``r0`` formed, for the windows'
    classes ``cls`` (int64 ``[S]``); ``ref`` (float32 ``[S]``) carries a window's own score to the passes after the one that
    holds its row (chebgcn_occlusion_score)."""
    _require_cuda(logits, cls, ref, drop)
    z = logits.detach().contiguous()
    R, C = z.shape
    S = drop.shape[0]
    if not (drop.is_contiguous() and drop.dtype == torch.float32 and drop.shape[1] == G and cls.dtype == torch.int64
            and cls.is_contiguous() and cls.numel() == S and ref.dtype == torch.float32 and ref.numel() == S):
        raise ValueError('occlusion_score: drop float32 [S, %d], cls int64 [S] and ref float32 [S]' % G)
    _lib.check(_launch('occlusion_score', 4.0 * R * (2 * C + 2), 0.0, lambda: _lib.lib().chebgcn_occlusion_score(
        _p(z), int(r0), R, S, int(G), C, _p(cls), SCORES[score], _p(ref), _p(drop), _stream())), 'occlusion_score')


def occlusion_class_sums(drop, cls, acc):
    """``acc[k] += `` the sum, windows in order, of the rows of ``drop`` [S, G] whose window has class k (``cls`` int64 [S],
    ``acc`` float64 [C, G]; chebgcn_occlusion_class_sums)."""
    _require_cuda(drop, cls, acc)
    S, G = drop.shape
    if not (drop.is_contiguous() and acc.is_contiguous() and acc.dtype == torch.float64 and acc.shape[1] == G
            and cls.dtype == torch.int64 and cls.numel() == S):
        raise ValueError('occlusion_class_sums: drop float32 [S, G], cls int64 [S], acc float64 [C, G]')
    C = acc.shape[0]
    _lib.check(_launch('occlusion_class_sums', 4.0 * S * G + 8.0 * C * S + 16.0 * C * G, 0.0,
                       lambda: _lib.lib().chebgcn_occlusion_class_sums(_p(drop), _p(cls), S, G, C, _p(acc), _stream())),
               'occlusion_class_sums')
    return acc


# ------------------------------------------------------------------------------------
# Shapley maps (base_model.shapley): the kernels of csrc/shapley.hip around the inference layers
# ------------------------------------------------------------------------------------

# The score table [windows, P, G + 1] of a shapley call stays on the device until its windows are reduced; a call whose table
# would be larger than this is run over as many windows at a time as fit (one window at the least).
SHAPLEY_TABLE_BYTES = 64 << 20


def shapley_rows(data, order, gid, rank, baseline, r0, R, M):
    """Plane storage ``[R, F, Mp]`` of rows ``r0 .. r0 + R - 1`` of a Shapley run (chebgcn_shapley_rows): with ``rank`` int32
    device ``[P, G]`` (``rank[p, g]`` the position of group g in permutation p), row r is window ``r // (P (G + 1))`` of
    ``data`` with its own values on the groups whose rank in permutation ``(r // (G + 1)) % P`` is below ``r % (G + 1)`` and on
    the positions of no group, and ``baseline`` elsewhere; ``order``, ``gid``: as for ``occlusion_rows``; zero rows past the
    last window."""
    _require_cuda(data, order, gid, rank, baseline)
    S, N, F = data.shape
    if rank.dtype != torch.int32 or rank.dim() != 2 or not rank.is_contiguous():
        raise ValueError('shapley_rows: rank must be a contiguous int32 [P, G] tensor')
    P, G = rank.shape
    Mp = plane_stride(M)
    out = torch.empty((int(R), F, Mp), dtype=torch.float32, device=data.device)
    # the rows written; per workgroup of 16 rows its window's tile (and the baseline's) read once
    nbytes = 4.0 * (F * (R * Mp + (int(R) + 15) // 16 * N * (1 + (baseline is not None))) + M)
    _lib.check(_launch('shapley_rows', nbytes, 0.0, lambda: _lib.lib().chebgcn_shapley_rows(
        _p(data), _p(order), _p(gid), _p(rank), _p(baseline), _p(out), int(r0), int(R), S, P, G, N, int(M), F, _stream())),
        'shapley_rows')
    return out


def shapley_score(logits, r0, cls, score, table):
    """The scores of the rows whose logits ``[R, C]`` a pass from row ``r0`` formed, written to ``table`` (float32
    ``[S, P, G + 1]``, flat index = the row) for the windows' classes ``cls`` (int64 ``[S]``; chebgcn_shapley_score)."""
    _require_cuda(logits, cls, table)
    z = logits.detach().contiguous()
    R, C = z.shape
    if not (table.dim() == 3 and table.is_contiguous() and table.dtype == torch.float32 and cls.dtype == torch.int64
            and cls.is_contiguous() and cls.numel() == table.shape[0]):
        raise ValueError('shapley_score: table float32 [S, P, G + 1] and cls int64 [S]')
    S, P, G1 = table.shape
    _lib.check(_launch('shapley_score', 4.0 * R * (C + 1), 0.0, lambda: _lib.lib().chebgcn_shapley_score(
        _p(z), int(r0), R, S, P, G1 - 1, C, _p(cls), SCORES[score], _p(table), _stream())), 'shapley_score')


def shapley_reduce(table, rank, phi):
    """``phi[w, g]`` (float32 ``[S, G]``) = the mean over the permutations of group g's marginal contribution in the score
    ``table`` (float32 ``[S, P, G + 1]``), summed in float64 in the order of p (chebgcn_shapley_reduce)."""
    _require_cuda(table, rank, phi)
    S, P, G1 = table.shape
    if not (table.is_contiguous() and table.dtype == torch.float32 and rank.dtype == torch.int32 and rank.is_contiguous()
            and tuple(rank.shape) == (P, G1 - 1) and phi.dtype == torch.float32 and phi.is_contiguous()
            and tuple(phi.shape) == (S, G1 - 1)):
        raise ValueError('shapley_reduce: table float32 [S, P, G + 1], rank int32 [P, G], phi float32 [S, G]')
    G = G1 - 1
    _lib.check(_launch('shapley_reduce', 4.0 * (2 * S * P * G + P * G + S * G), 0.0, lambda: _lib.lib().chebgcn_shapley_reduce(
        _p(table), _p(rank), S, P, G, _p(phi), _stream())), 'shapley_reduce')
    return phi


# ------------------------------------------------------------------------------------
# Grad-CAM maps (base_model.gradcam): the two kernels of csrc/gradcam.hip behind the pass that stops at a layer
# ------------------------------------------------------------------------------------

GRADCAM_METHODS = {'gradcam': 0, 'grad_x_activation': 1}


def gradcam_map(A, G, method, order, nw, N, P, relu, out):
    """Rows ``out`` [nw, N*P] (float32, the caller's input vertex order) of the windows' maps from a layer's activation ``A`` and
    its gradient ``G`` (plane storage [>= nw, F, Mp(N)] in the level's internal order ``order``: int32 device, internal position
    -> reference vertex, or None): 'gradcam' weighs the filters by the mean of G over the level's vertices
    (chebgcn_gradcam_weights), 'grad_x_activation' takes G itself; chebgcn_gradcam_map sums over the filters, applies ReLU and
    writes each level vertex to its P input vertices."""
    _require_cuda(A, G, order, out)
    A = A.detach()
    G = G.detach()
    A = A if A.is_contiguous() else A.contiguous()
    G = G if G.is_contiguous() else G.contiguous()
    B, F, Mp = A.shape
    if (tuple(G.shape) != (B, F, Mp) or Mp != plane_stride(N) or B < nw or out.dtype != torch.float32
            or not out.is_contiguous() or tuple(out.shape) != (nw, N * P)
            or (order is not None and (order.dtype != torch.int32 or order.numel() != N))):
        raise ValueError('gradcam_map: A and G [>= %d, F, %d], out float32 [%d, %d], order int32 [%d]'
                         % (nw, plane_stride(N), nw, N * P, N))
    L = _lib.lib()
    alpha = None
    if GRADCAM_METHODS[method] == 0:
        alpha = torch.empty((nw, F), dtype=torch.float32, device=A.device)
        _lib.check(_launch('gradcam_weights', 4.0 * nw * F * (N + 1), 0.0, lambda: L.chebgcn_gradcam_weights(
            _p(G), nw, F, N, _p(alpha), _stream())), 'gradcam_weights')
    # A (and G per vertex) over the level's vertices, the order table, the rows written
    nbytes = 4.0 * (nw * F * N * (1 + (alpha is None)) + (N if order is not None else 0) + nw * N * P)
    _lib.check(_launch('gradcam_map', nbytes, 2.0 * nw * F * N, lambda: L.chebgcn_gradcam_map(
        _p(A), _p(G) if alpha is None else None, _p(alpha), _p(order), nw, F, N, P, int(bool(relu)), _p(out), N * P,
        _stream())), 'gradcam_map')
    return out


# ------------------------------------------------------------------------------------ Monte-Carlo dropout (uncertainty.py)

MC_SAMPLES_MAX = 1024        # chebgcn_mc_reduce_supported
MC_CLASSES_MAX = 64


def fc_forward_native(x, W, b, relu, who):
    """``act(x @ W + b)`` on chebgcn_fc_fwd at every size it serves; a size it does not serve raises (``who`` names the caller):
    never the vendor GEMM.  ``x`` [B, I] may be any view (ops._fc_rows copies rows the kernel cannot take)."""
    _require_cuda(x, W, b)
    B, I = x.shape
    O = W.shape[1]
    if not _lib.lib().chebgcn_fc_fwd_supported(B, I, O):
        raise ValueError('%s: the FC layer %d x %d x %d is outside the range of chebgcn_fc_fwd' % (who, B, I, O))
    rows = _fc_rows(x.detach())
    return _fc_fwd(rows, rows.stride(0), W.detach().contiguous(), b.detach().contiguous(), relu, 'fc_fwd')


def _fc_sample_rows(x):
    """``x`` [S, B, I] as sample matrices the dropout FC kernel takes (unit stride along I, row and sample strides multiples of 4
    floats, 16-byte aligned): itself where it is such a tensor, else a copy with rows padded by zeros."""
    S, B, I = x.shape
    if (x.stride(2) == 1 and x.stride(1) % 4 == 0 and x.stride(1) >= I and x.stride(0) % 4 == 0
            and x.stride(0) >= (B - 1) * x.stride(1) + I and x.data_ptr() % 16 == 0):
        return x
    buf = torch.zeros((S, B, (I + 3) & ~3), dtype=torch.float32, device=x.device)
    buf[:, :, :I].copy_(x)
    return buf[:, :, :I]


def fc_forward_dropout(x, W, b, relu, win, S, s0, layer, seed, threshold, inv_keep):
    """``S`` Monte-Carlo dropout samples of one FC layer (chebgcn_fc_fwd_dropout): ``y[s] = act((mask_s * x_s / keep) @ W + b)``,
    float32 ``[S, B, O]``.  ``x``: ``[B, I]``, one input shared by every sample, or ``[S, B, I]``; ``win``: int32 device ``[B]``, the
    window number of every row; ``s0``: the number of the first sample; ``layer``: the dropout site; ``threshold`` / ``inv_keep``:
    ``uncertainty.dropout_threshold``.  A size the kernel does not serve raises: there is no other path."""
    _require_cuda(x, W, b, win)
    shared = x.dim() == 2
    rows = _fc_rows(x.detach()) if shared else _fc_sample_rows(x.detach())
    B, I = rows.shape[-2:]
    O = W.shape[1]
    S = int(S)
    if not shared and rows.shape[0] != S:
        raise ValueError('fc_forward_dropout: x holds %d samples, S = %d' % (rows.shape[0], S))
    if win.dtype != torch.int32 or not win.is_contiguous() or win.numel() != B:
        raise ValueError('fc_forward_dropout: win must be a contiguous int32 vector with a window number per row')
    L = _lib.lib()
    if not L.chebgcn_fc_fwd_dropout_supported(S, B, I, O):
        raise ValueError('fc_forward_dropout: %d samples of the FC layer %d x %d x %d are outside the range of '
                         'chebgcn_fc_fwd_dropout' % (S, B, I, O))
    Wc, bc = W.detach().contiguous(), b.detach().contiguous()
    y = torch.empty((S, B, O), dtype=torch.float32, device=rows.device)
    nws = L.chebgcn_fc_fwd_dropout_workspace(S, B, I, O)
    ws = _workspace(nws, rows.device, 'fc_fwd_dropout') if nws else None
    ldx, sx = (rows.stride(0), 0) if shared else (rows.stride(1), rows.stride(0))
    _lib.check(_launch('fc_fwd_dropout', 4.0 * ((1 if shared else S) * B * I + I * O + S * B * O), 2.0 * S * B * I * O,
                       lambda: L.chebgcn_fc_fwd_dropout(_p(rows), ldx, sx, _p(Wc), _p(bc), _p(y), _p(ws), nws, _p(win), S, B, I, O,
                                                        1 if relu else 0, int(seed), int(s0), int(layer), int(threshold),
                                                        float(inv_keep), _stream())), 'fc_fwd_dropout')
    return y


def mc_reduce(logits):
    """The uncertainty measures of sampled logits float32 ``[S, B, C]`` (chebgcn_mc_reduce), as device tensors: ``probabilities``
    ``[B, C]``, ``entropy``, ``expected_entropy``, ``mutual_information``, ``agreement`` float32 ``[B]``, ``labels`` int32 ``[B]``,
    ``votes`` int32 ``[B, C]``."""
    _require_cuda(logits)
    z = logits.detach().contiguous()
    S, B, C = z.shape
    if z.dtype != torch.float32 or not _lib.lib().chebgcn_mc_reduce_supported(S, C):
        raise ValueError('mc_reduce: float32 logits of 1 <= S <= %d samples and 1 <= C <= %d classes, got %s [%d, %d, %d]'
                         % (MC_SAMPLES_MAX, MC_CLASSES_MAX, z.dtype, S, B, C))
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=z.device)
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=z.device)
    out = dict(probabilities=f(B, C), entropy=f(B), expected_entropy=f(B), mutual_information=f(B), labels=i(B), votes=i(B, C),
               agreement=f(B))
    _lib.check(_launch('mc_reduce', 4.0 * (S * B * C + 2 * B * C + 5 * B), 0.0, lambda: _lib.lib().chebgcn_mc_reduce(
        _p(z), S, B, C, _p(out['probabilities']), _p(out['entropy']), _p(out['expected_entropy']), _p(out['mutual_information']),
        _p(out['labels']), _p(out['votes']), _p(out['agreement']), _stream())), 'mc_reduce')
    return out
