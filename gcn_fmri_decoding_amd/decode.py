"""Decoding a scan window by window: ``decode_series`` says which state the model sees at every time point of a run (what
predict_states.py exists for).  ``Decode`` carries the method and is a base of ``models_gcn.base_model``; ``Windows`` is what the
first conv layer reads while the shared path runs.

Why there is a shared path.  The model's input folds time into the channels, ``x[w][v][c] = s[start_w + c][v]``, and the
Chebyshev recurrence acts on every channel plane on its own: ``T_k(L~) x`` of window ``w``, channel ``c`` IS ``T_k(L~) s_t`` of
the run's time point ``t = start_w + c``.  Overlapping windows share their time points, so the first layer's recurrence needs T
planes, not W * C, and its contraction reads each window's operand straight out of that one stack
(chebgcn_contract_fwd_windows).  Layers 2 ... n see different inputs per window and run as they always do."""
import os

import numpy as np
import torch

from . import _lib, ops

OUTPUTS = ('logits', 'probabilities', 'labels')
# device bytes the shared path spends on the run's Chebyshev stack [K, T, Mp]; longer runs are decoded in chunks of time
# points that overlap by C - 1 (CHEBGCN_DECODE_STACK_MB, or the keyword ``max_stack_bytes``)
STACK_BYTES = int(float(os.environ.get('CHEBGCN_DECODE_STACK_MB', '256')) * (1 << 20))
# 'auto' leaves graphs this small to the materialised path: there csrc/fused_small.hip runs the whole first layer on chip in
# one launch, and the shared path (two launches through a stack in memory) measured no faster -- DESIGN 4.10
AUTO_MIN_VERTICES = 385


class Windows(object):
    """``model._windows`` while a batch of the shared path runs (None otherwise): the run's (or chunk's) Chebyshev stack
    ``[K, T, Mp]`` and the int32 device table of this batch's window starts inside it."""
    __slots__ = ('stack', 'T', 'starts')

    def __init__(self, stack, T, starts):
        self.stack, self.T, self.starts = stack, int(T), starts

    @property
    def B(self):
        return int(self.starts.numel())


def window_starts(T, C, starts=None, stride=1, what='decode_series'):
    """The int64 starts of the windows of ``C`` time points decoded in a run of ``T``: ``starts`` as given (any order,
    repeats allowed; every window must lie inside the run), else ``range(0, T - C + 1, stride)``.  ``ValueError`` otherwise
    (``what`` names the calling method in the message)."""
    T, C = int(T), int(C)
    if T < C:
        raise ValueError('%s: a run of T = %d time points is shorter than one window (C = %d)' % (what, T, C))
    if starts is None:
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
            raise ValueError('%s: stride must be an int >= 1, got %r' % (what, stride))
        return np.arange(0, T - C + 1, int(stride), dtype=np.int64)
    a = np.asarray(starts)
    if a.ndim != 1 or a.size == 0 or a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s: starts must be a non-empty 1-d int array, got %s %s' % (what, a.dtype, a.shape))
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() + C > T:
        raise ValueError('%s: every start must satisfy 0 <= start and start + %d <= T = %d; got %d ... %d'
                         % (what, C, T, a.min(), a.max()))
    return a


def run_list(series, what):
    """``series``, one run or a list of runs, as a non-empty list."""
    runs = list(series) if isinstance(series, (list, tuple)) else [series]
    if not runs:
        raise ValueError('%s: series is an empty list' % what)
    return runs


def check_run(r, M0, what, least=0):
    """One run as a numeric ``[T, M0]`` array or tensor of at least ``least`` time points, else a ``ValueError``."""
    if not isinstance(r, torch.Tensor):
        r = np.asarray(r)
        if not (np.issubdtype(r.dtype, np.floating) or np.issubdtype(r.dtype, np.integer)):
            raise ValueError('%s: series must be numeric, got %s' % (what, r.dtype))
    shape = tuple(int(d) for d in r.shape)
    if len(shape) != 2 or shape[1] != M0 or shape[0] < least:
        raise ValueError('%s: series must be [T, %d] (time points x vertices), got %s' % (what, M0, shape))
    return r


def check_table(v, name, M0, C, what):
    """A ``scale`` / ``shift`` table as float32 ``[M0, C]`` (None stays None), else a ``ValueError``."""
    if v is None:
        return None
    a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float32)
    if a.shape != (M0, C):
        raise ValueError('%s: %s must be [%d, %d] (vertices x channels), got %s' % (what, name, M0, C, a.shape))
    return a


def chunk_plan(starts, T, C, chunk_T):
    """How a run is cut when its stack may hold ``chunk_T >= C`` time points: a list of ``(t0, t1, idx)`` -- the chunk covers
    the time points ``[t0, t1)``, consecutive chunks overlap by ``C - 1``, and ``idx`` are the positions in ``starts`` of the
    windows decoded from it (each window belongs to exactly one chunk, which holds all of it).  Chunks without a window are
    left out."""
    T, C, chunk_T = int(T), int(C), int(chunk_T)
    if chunk_T < C:
        raise ValueError('decode_series: a chunk of %d time points does not hold a window of %d' % (chunk_T, C))
    step = chunk_T - (C - 1)
    which = np.minimum(starts // step, max(0, (T - C) // step))
    plan = []
    for j in np.unique(which):
        t0 = int(j) * step
        idx = np.nonzero(which == j)[0]
        plan.append((t0, min(T, t0 + chunk_T), idx))
    return plan


class Decode(object):
    """``decode_series`` of ``base_model``.  Uses the model's ``_inference_storage``, ``as_internal``, ``probabilities`` /
    ``prediction``, its sizes (``_M0``, ``channel``, ``K``, ``F``, ``p``, ``M``, ``batch_size``), its input order table
    ``_order_dev`` and ``training_mode``; the first conv layer reads ``_windows``."""

    last_decode_path = None         # 'shared' | 'materialised': the path the last decode_series call took

    # ---------------------------------------------------------------- arguments

    def _decode_args(self, series, starts, stride, scale, shift, share, batch_size, output, what='decode_series'):
        """Everything that can be refused before device work.  Returns (runs as arrays / tensors, their starts, batch size,
        scale, shift as float32 [M, C] or None, whether a list was given).  ``what``: the public method the messages name."""
        if output not in OUTPUTS:
            raise ValueError('%s: output must be one of %s, got %r' % (what, OUTPUTS, output))
        if not (share is True or share is False or share == 'auto'):
            raise ValueError("%s: share must be True, False or 'auto', got %r" % (what, share))
        bs = self.batch_size if batch_size is None else batch_size
        if isinstance(bs, bool) or not isinstance(bs, (int, np.integer)) or not 1 <= bs <= 65535:
            raise ValueError('%s: batch_size must be an int in [1, 65535], got %r' % (what, batch_size))
        many = isinstance(series, (list, tuple))
        runs = run_list(series, what)
        if many and starts is not None:
            if not isinstance(starts, (list, tuple)) or len(starts) != len(runs) or any(np.ndim(s) == 0 for s in starts):
                raise ValueError('%s: with a list of %d runs, starts must be a list of as many arrays' % (what, len(runs)))
        per_run = list(starts) if (many and starts is not None) else [starts] * len(runs)
        M0, C = int(self._M0), int(self.channel)
        out_runs, out_starts = [], []
        for r, st in zip(runs, per_run):
            r = check_run(r, M0, what)
            out_starts.append(window_starts(r.shape[0], C, st, stride, what))
            out_runs.append(r)
        scale, shift = check_table(scale, 'scale', M0, C, what), check_table(shift, 'shift', M0, C, what)
        return out_runs, out_starts, int(bs), scale, shift, many

    def _shared_refusal(self, B, scaled):
        """None where the shared path serves this model, else why not."""
        from . import models_gcn
        if scaled:
            return 'scale / shift act per vertex AND channel, which does not commute with the recurrence'
        cg = getattr(models_gcn, 'cgcnn')
        if not isinstance(self, cg) or not self._fusable():
            return "only filter='chebyshev5' with the standard brelu / pool methods shares its recurrence"
        if int(self.K[0]) < 2:
            return 'K[0] = 1: the first layer has no recurrence to share'
        if self.layer_precisions()[0] != 'f32':
            return 'the first layer computes in %s; the windowed contraction is fp32' % self.layer_precisions()[0]
        top = len(self.p) == 1 and isinstance(self, getattr(models_gcn, 'finetuning_cgcnn'))
        pool = 1 if (top or self._pool_maps[0] is not None) else int(self.p[0])
        if not _lib.lib().chebgcn_contract_fwd_windows_supported(int(B), int(self._M0), int(self.channel), int(self.K[0]),
                                                                 int(self.F[0]), pool):
            return 'chebgcn_contract_fwd_windows does not serve the first layer (more than 32 filters?)'
        return None

    # ---------------------------------------------------------------- the method

    def decode_series(self, series, starts=None, stride=1, scale=None, shift=None, share='auto', batch_size=None,
                      output='logits', max_stack_bytes=None, mc=None):
        """The model's output for every window of a scan.  ``series``: ``[T, M]`` (NumPy, any numeric dtype, or a torch
        tensor), time points x vertices in the vertex layout ``predict`` takes (``M = L[0].shape[0]``, after
        ``coarsening.perm_data``), or a list of such runs (a list returns a list; windows never cross runs).  Window ``w``
        is the model input ``x[v][c] = series[start_w + c][v]``, ``c < channel``.

        * ``starts``: explicit window starts (event-locked decoding: onsets plus offsets; any order, repeats allowed; a list
          of arrays for a list of runs), else ``range(0, T - channel + 1, stride)``.  ``T < channel`` or a start outside
          the run raises ``ValueError`` before anything is launched.
        * Returns float32 ``[W, classes]`` (``output='logits'`` or ``'probabilities'``) or int64 ``[W]`` (``'labels'``,
          ``prediction()``'s tie rule) in the order of the starts.
        * Evaluation mode, dropout off, no gradient; the model's variables, optimizer state, step counter and captured step
          are not touched.  Windows go through the network ``batch_size`` (default the model's) at a time; the last batch
          is run at its own size.
        * ``scale`` / ``shift`` ``[M, channel]``: every window is normalised per vertex and channel, ``x * scale + shift``
          (how the reference's NDStandardScaler treats windows).
        * ``share``: the series is staged on the device once either way.  The **shared** path runs the first layer's
          Chebyshev recurrence ONCE over the run (T planes instead of W * channel) and contracts every window out of that
          stack (chebgcn_contract_fwd_windows: the same products in the same order as the ordinary layer); runs whose
          stack ``[K, T, Mp]`` exceeds ``max_stack_bytes`` (default 256 MB) go in chunks that overlap by ``channel - 1``
          time points.  The **materialised** path builds each batch of windows on the device and runs the ordinary
          network.  ``True``: shared, ``ValueError`` if it cannot serve the model; ``False``: materialised; ``'auto'``:
          shared where it serves the model (``filter='chebyshev5'`` with the standard layers, ``K[0] > 1``, an fp32 first
          layer of at most 32 filters, no ``scale`` / ``shift``), the windows overlap, and the graph is larger than the
          atlas sizes whose first layer already runs on chip in one launch.  ``last_decode_path`` names the path taken.

        * ``mc``: ``dict(samples=32, seed=0, keep=None)`` decodes with Monte-Carlo dropout (``predict_mc``, whose keywords
          these are): every run returns an ``uncertainty.MCResult`` -- mean probabilities, labels, entropy, expected entropy,
          mutual information, votes and agreement per window -- instead of logits, and ``output`` is not used.  The windows
          are numbered in the order of the starts, on across the runs of a list; the masks depend on that number alone, so
          the result equals ``predict_mc`` on the same windows cut out by hand, on either path.  ``None`` (default): no
          sampling, everything as described above.

        The two paths agree to fp32 round-off, and bit for bit wherever the first layer of the materialised path runs the
        recurrence + contraction kernels (graphs beyond the on-chip layer's 384 vertices).  Results do not depend on
        ``batch_size`` or on the chunking as long as those keep every launch on the same kernels (include/chebgcn.h: the
        dispatchers choose by launch size)."""
        runs, run_starts, bs, scale, shift, many = self._decode_args(series, starts, stride, scale, shift, share, batch_size,
                                                                     output)
        if max_stack_bytes is not None and (isinstance(max_stack_bytes, bool) or int(max_stack_bytes) < 1):
            raise ValueError('decode_series: max_stack_bytes must be a positive int, got %r' % (max_stack_bytes,))
        mc_args = None if mc is None else self._mc_dict(mc, bs)
        if self.device.type != 'cuda':
            raise RuntimeError('decode_series: the model has no device to run on (%s)' % self.device)
        scaled = scale is not None or shift is not None
        C = int(self.channel)
        refusal = self._shared_refusal(bs, scaled)
        if share is True and refusal is not None:
            raise ValueError('decode_series(share=True): ' + refusal)
        shared = refusal is None and share is not False
        if shared and share == 'auto':
            covered = sum(len(np.unique((st[:, None] + np.arange(C)[None, :]).ravel())) for st in run_starts)
            overlapping = sum(len(st) for st in run_starts) * C > covered
            shared = overlapping and int(self._M0) >= AUTO_MIN_VERTICES
        budget = STACK_BYTES if max_stack_bytes is None else int(max_stack_bytes)
        was_training = self.training_mode
        self.training_mode = False
        results, first = [], 0
        try:
            with torch.no_grad():
                tabs = self._scale_tables(scale, shift) if scaled else None
                for run, st in zip(runs, run_starts):
                    planes = self._stage_series(run)
                    if mc_args is not None:
                        from .uncertainty import MCHead          # (here: uncertainty imports series, which imports this module)
                        self._mc = MCHead(self, len(st), mc_args[0], mc_args[1], mc_args[2], first_window=first)
                        first += len(st)
                    # (Monte-Carlo decoding: the head writes into the MCHead's buffers; there are no logits to collect)
                    res = None if mc_args is not None else torch.empty((len(st), int(self.M[-1])), dtype=torch.float32,
                                                                       device=self.device)
                    if shared:
                        self._decode_shared(planes, st, bs, res, budget)
                    else:
                        self._decode_materialised(planes, st, bs, res, tabs)
                    if mc_args is not None:
                        results.append(self._mc.result())
                        continue
                    if output == 'probabilities':
                        res = self.probabilities(res)
                    elif output == 'labels':
                        res = self.prediction(res).to(torch.int64)
                    results.append(res.cpu().numpy())
        finally:
            self.training_mode, self._windows, self._mc = was_training, None, None
        self.last_decode_path = 'shared' if shared else 'materialised'
        return results if many else results[0]

    # ---------------------------------------------------------------- device work

    def _stage_series(self, run, out=None):
        """One run ``[T, M]`` -> its planes ``[T, Mp]`` on the device in the model's internal vertex order, fp32
        (chebgcn_perm_data with one channel; the pad of every plane is zero).  ``out``: a ``[T, Mp]`` buffer to fill."""
        if isinstance(run, torch.Tensor):
            x = run.to(self.device, torch.float32).contiguous()
        else:
            x = torch.as_tensor(np.ascontiguousarray(run, np.float32)).to(self.device)
        T, M = x.shape
        out = ops.plane_empty(T, 1, M, self.device) if out is None else out.view(T, 1, -1)
        order = self._order_dev if self._order_dev is not None else torch.arange(M, dtype=torch.int32, device=self.device)
        for t0 in range(0, T, 32768):                                   # (the kernel's grid takes 65535 rows)
            ops.perm_data(x[t0:t0 + 32768].unsqueeze(2), order, out=out[t0:t0 + 32768])
        return out.view(T, out.shape[2])

    def _scale_tables(self, scale, shift):
        """``scale`` / ``shift`` ``[M, C]`` in the caller's vertex order -> ``[C, Mp]`` device planes in the internal one (zero
        in the pad, so that the pad of a normalised window stays zero)."""
        M0, C = int(self._M0), int(self.channel)
        order = np.arange(M0) if self._order is None else np.asarray(self._order)
        tabs = []
        for v, fill in ((scale, 1.0), (shift, 0.0)):
            a = np.full((M0, C), fill, np.float32) if v is None else v
            t = np.zeros((C, ops.plane_stride(M0)), np.float32)
            t[:, :M0] = a[order].T
            tabs.append(torch.as_tensor(t).to(self.device))
        return tabs

    def _decode_materialised(self, planes, starts, bs, res, tabs):
        C = int(self.channel)
        st = torch.as_tensor(starts).to(self.device)
        offs = torch.arange(C, dtype=torch.int64, device=self.device)
        for b0 in range(0, len(starts), bs):
            x = planes[st[b0:b0 + bs, None] + offs[None, :]]           # [B, C, Mp]: the windows, a strided copy
            if tabs is not None:
                x = x * tabs[0] + tabs[1]
            if self._mc is not None:
                self._mc.at(np.arange(b0, min(b0 + bs, len(starts))))
            out = self._inference_storage(self.as_internal(x), 1)
            if res is not None:
                res[b0:b0 + bs] = out

    def _decode_shared(self, planes, starts, bs, res, budget):
        lib = _lib.lib()
        T, Mp = planes.shape
        C, K, g = int(self.channel), int(self.K[0]), self.graphs[0]
        chunk_T = max(C, min(T, budget // (4 * K * Mp)))
        for t0, t1, idx in chunk_plan(starts, T, C, chunk_T):
            Tc = t1 - t0
            stack = torch.empty((K, Tc, Mp), dtype=torch.float32, device=self.device)
            x = planes[t0:t1]
            _lib.check(ops._launch('recurrence_fwd', 4.0 * g.M * Tc * K, 0.0, lambda: lib.chebgcn_recurrence_fwd(
                g.handle, ops._p(x), ops._p(stack), 1, Tc, K, ops._stream())), 'recurrence_fwd')
            rel = torch.as_tensor((starts[idx] - t0).astype(np.int32)).to(self.device)
            where = torch.as_tensor(idx.astype(np.int64)).to(self.device)
            for b0 in range(0, len(idx), bs):
                self._windows = Windows(stack, Tc, rel[b0:b0 + bs])
                if self._mc is not None:
                    self._mc.at(idx[b0:b0 + bs])
                try:
                    logits = self._inference_storage(None, 1)
                finally:
                    self._windows = None
                if res is not None:
                    res.index_copy_(0, where[b0:b0 + bs], logits)
