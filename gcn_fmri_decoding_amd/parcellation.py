"""Parcellation: vertex- or grayordinate-level scans ``[T, V]`` reduced to the regions of an atlas on the device, and region maps
put back on the vertices.

The reference does the reduction on the host, per label (``model.py:47-53``: ``RegionLabels = [i for i in np.unique(atlas) if
i > 0]``, then ``np.mean(conn[:, ind], axis=1)`` for every label) or as a pandas group-by (``model.py:85-91``), and stores the
result.  Here ``Parcellation(labels).reduce(runs)`` gives the ``[T, R]`` series as float32 device tensors, which
``stage_windows``, ``fit_series``, ``fit_events``, ``stage_events``, ``decode_series`` and ``graph.connectivity_graph`` take as
they are; host input is uploaded a bounded slice of rows at a time, so the vertex-level run never exists on the device as a whole.

The arithmetic is stated, not left to the launch: float32, every region's members added one after the other in ascending vertex
order from 0, a weighted term rounded as a product before it is added, the weighted denominator summed in the same order, one
rounded division.  ``reduce_host`` performs the same operations in float32 NumPy and gives the same bits.
"""
import numpy as np

from .runs import cuda_device, is_tensor

MODES = ('mean', 'sum')
RMAX = 65535
CHUNK_BYTES = 256 << 20         # a slice of host rows on the device at most


class Parcellation:
    """The regions of an atlas over V vertices.

    ``labels``: integer ``[V]`` (a ``[1, V]`` array, as nibabel gives for a dlabel file, is accepted).  Regions are the sorted
    unique labels > 0, compacted to 0 .. R - 1; labels <= 0 are background.  ``weights``: optional per-vertex ``[V]`` (vertex
    areas, a soft atlas' membership), finite, >= 0, with a positive sum inside every region.

    Attributes: ``V``, ``R``, ``regions`` (the original ids, int64 [R]), ``counts`` (int64 [R]), ``region_of`` (int32 [V], -1 for
    background), ``ptr`` / ``idx`` (int32: the members of region r are ``idx[ptr[r]:ptr[r + 1]]``, ascending), ``weights``
    (float32 [V] or None).  Bad arguments raise ``ValueError`` before the device is touched."""

    def __init__(self, labels, weights=None):
        lab = np.asarray(labels)
        if lab.ndim == 2 and lab.shape[0] == 1:
            lab = lab[0]
        if lab.ndim != 1 or lab.size < 1:
            raise ValueError('Parcellation: labels must be [V] (or [1, V]), got shape %r' % (np.shape(labels),))
        if lab.dtype == bool or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError('Parcellation: labels must be integers, got %s' % lab.dtype)
        self.V = int(lab.size)
        if self.V > 1 << 30:
            raise ValueError('Parcellation: %d vertices, at most 2^30' % self.V)
        lab = lab.astype(np.int64)
        regions = np.unique(lab)
        regions = regions[regions > 0]
        if regions.size == 0:
            raise ValueError('Parcellation: no positive label')
        if regions.size > RMAX:
            raise ValueError('Parcellation: %d regions, at most %d' % (regions.size, RMAX))
        self.R = int(regions.size)
        self.regions = regions
        pos = np.searchsorted(regions, lab)
        pos[pos == self.R] = 0
        member = regions[pos] == lab
        self.region_of = np.where(member, pos, -1).astype(np.int32)
        order = np.argsort(self.region_of, kind='stable')          # background first, then region by region, ascending vertex
        self.idx = order[self.V - int(member.sum()):].astype(np.int32)
        self.counts = np.bincount(self.region_of[member], minlength=self.R).astype(np.int64)
        self.ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.weights = None
        if weights is not None:
            w = np.asarray(weights)
            if w.shape != (self.V,):
                raise ValueError('Parcellation: weights must be [%d], got shape %r' % (self.V, w.shape))
            try:
                w = w.astype(np.float32)
            except (TypeError, ValueError):
                raise ValueError('Parcellation: weights must be numbers')
            if not np.isfinite(w).all():
                raise ValueError('Parcellation: weights hold non-finite values')
            if (w < 0).any():
                raise ValueError('Parcellation: negative weights')
            if (self._sum_in_order(w[None, :], None)[0] <= 0).any():
                raise ValueError('Parcellation: the weights of a region sum to zero')
            self.weights = w
        self._dev = {}

    # ---- the stated order, in NumPy ---------------------------------------------------------------------------------------------
    def _sum_in_order(self, x, w):
        """float32 [T, R]: per region acc = 0, then acc = acc + (w[v] * x[:, v]) member by member in ascending order -- a loop
        over member rank, vectorised over rows and regions."""
        acc = np.zeros((x.shape[0], self.R), np.float32)
        start = self.ptr[:-1].astype(np.int64)
        for k in range(int(self.counts.max())):
            sel = np.nonzero(self.counts > k)[0]
            v = self.idx[start[sel] + k]
            term = x[:, v]
            if w is not None:
                term = term * w[v]                                 # float32 product, rounded on its own
            acc[:, sel] = acc[:, sel] + term
        return acc

    def reduce_host(self, series, mode='mean'):
        """``reduce`` in float32 NumPy: the same adds in the same order (ascending members, sequential), the same single
        division -- the bits of the device kernel.  One ``[T, V]`` run or a list of runs -> float32 ``[T, R]`` arrays."""
        if mode not in MODES:
            raise ValueError('Parcellation: mode must be one of %s, not %r' % (MODES, mode))
        runs, single = self._runs(series)
        out = []
        for r in runs:
            x = r.detach().cpu().numpy() if is_tensor(r) else np.asarray(r)
            x = x.astype(np.float32, copy=False)
            with np.errstate(invalid='ignore', over='ignore'):
                acc = self._sum_in_order(x, self.weights)
                if mode == 'mean':
                    if self.weights is None:
                        den = self.counts.astype(np.float32)
                    else:
                        den = self._sum_in_order(np.ones((1, self.V), np.float32), self.weights)[0]
                    acc = acc / den[None, :]
            out.append(acc)
        return out[0] if single else out

    # ---- the device -------------------------------------------------------------------------------------------------------------
    def _runs(self, series):
        single = (isinstance(series, np.ndarray) or is_tensor(series)) and series.ndim == 2
        runs = [series] if single else list(series)
        if not runs:
            raise ValueError('Parcellation: no runs')
        for r in runs:
            if not (isinstance(r, np.ndarray) or is_tensor(r)):
                raise ValueError('Parcellation: a run must be a NumPy array or a torch tensor, not %s' % type(r).__name__)
            if r.ndim != 2 or r.shape[1] != self.V:
                raise ValueError('Parcellation: every run must be [T, %d], got shape %r' % (self.V, tuple(r.shape)))
            if isinstance(r, np.ndarray) and not (np.issubdtype(r.dtype, np.number) or r.dtype == bool):
                raise ValueError('Parcellation: a run of dtype %s' % r.dtype)
        return runs, single

    def _tables(self, dev):
        import torch
        key = (dev.type, dev.index)
        if key not in self._dev:
            self._dev[key] = tuple(None if a is None else torch.as_tensor(a).to(dev)
                                   for a in (self.ptr, self.idx, self.region_of, self.weights))
        return self._dev[key]

    def reduce(self, series, device=None, chunk_rows=None, mode='mean'):
        """One ``[T, V]`` run or a list of runs (NumPy arrays of any numeric dtype, or torch tensors on the host or the device;
        all converted to float32) -> float32 device tensors ``[T_i, R]``, one per run, a single tensor for a single run.

        A host run is uploaded ``chunk_rows`` rows at a time (default: as many as fit 256 MiB) and reduced slice by slice into the
        result, so the device holds one slice of the vertex-level run and the ``[T, R]`` result, never the run.  A device tensor
        is reduced where it lies.  The result does not depend on ``chunk_rows`` or on where the input lives: bit-identical, and
        equal to ``reduce_host``.  Input is not searched for non-finite values: a NaN at ``(t, v)`` gives NaN at ``(t,
        region_of[v])`` and nowhere else.  The outputs are what ``stage_windows``, ``fit_series``, ``fit_events``,
        ``stage_events``, ``decode_series`` and ``graph.connectivity_graph`` accept as runs."""
        if mode not in MODES:
            raise ValueError('Parcellation: mode must be one of %s, not %r' % (MODES, mode))
        if chunk_rows is None:
            chunk_rows = max(1, CHUNK_BYTES // (4 * self.V))
        if int(chunk_rows) != chunk_rows or chunk_rows < 1:
            raise ValueError('Parcellation: chunk_rows = %r' % (chunk_rows,))
        chunk_rows = int(chunk_rows)
        runs, single = self._runs(series)
        import torch
        from . import ops
        dev = cuda_device(device, next((r for r in runs if is_tensor(r) and r.is_cuda), None))
        m = MODES.index(mode)
        out = []
        with torch.cuda.device(dev):
            ptr, idx, _, w = self._tables(dev)
            for r in runs:
                T = int(r.shape[0])
                res = torch.empty((T, self.R), dtype=torch.float32, device=dev)
                if is_tensor(r) and r.is_cuda:
                    x = r.to(dev, torch.float32)
                    if x.stride(1) != 1 and self.V > 1:
                        x = x.contiguous()
                    ops.parcellate(x, ptr, idx, self.R, w=w, mode=m, out=res)
                else:
                    for t0 in range(0, T, chunk_rows):
                        piece = r[t0:t0 + chunk_rows]
                        if is_tensor(piece):
                            x = piece.to(torch.float32).contiguous().to(dev)
                        else:
                            x = torch.as_tensor(np.ascontiguousarray(piece, dtype=np.float32)).to(dev)
                        ops.parcellate(x, ptr, idx, self.R, w=w, mode=m, out=res[t0:t0 + chunk_rows])
                out.append(res)
        return out[0] if single else out

    def expand(self, maps, fill=0.0):
        """Region values back on the vertices: ``maps`` ``[R]`` or ``[B, R]`` (the attribution maps of ``saliency_maps``,
        ``occlusion_maps``, ``gradcam_maps``) -> ``[V]`` or ``[B, V]`` float32 with ``out[b, v] = maps[b, region_of[v]]`` and
        ``fill`` on the background.  A NumPy array gives a NumPy array (indexing on the host), a device tensor a device tensor
        (chebgcn_parcel_expand); a host tensor comes back as a host tensor."""
        tensor = is_tensor(maps)
        if not tensor:
            maps = np.asarray(maps)
        if maps.ndim not in (1, 2) or maps.shape[-1] != self.R:
            raise ValueError('Parcellation: maps must be [%d] or [B, %d], got shape %r' % (self.R, self.R, tuple(maps.shape)))
        if tensor and maps.is_cuda:
            import torch
            from . import ops
            with torch.cuda.device(maps.device):
                region_of = self._tables(maps.device)[2]
                m2 = maps.reshape(-1, self.R).to(torch.float32).contiguous()
                out = ops.parcel_expand(m2, region_of, fill=fill)
            return out[0] if maps.ndim == 1 else out
        m = maps.detach().numpy() if tensor else maps
        m2 = m.reshape(-1, self.R).astype(np.float32, copy=False)
        out = np.where(self.region_of[None, :] >= 0, m2[:, np.maximum(self.region_of, 0)], np.float32(fill)).astype(np.float32)
        out = out[0] if maps.ndim == 1 else out
        if tensor:
            import torch
            return torch.as_tensor(out)
        return out
