"""Training on scans: ``WindowSet`` is a dataset that IS windows of scans -- the runs staged once as planes, the windows an
int64 table of first rows, cut (and scaled) on the device batch by batch -- and ``Series`` carries ``stage_windows`` /
``fit_series`` and is a base of ``models_gcn.base_model``.

The reference builds ``[S, M, channel]`` on the host (utils.py: the windows cut with NumPy, stacked, an NDStandardScaler fitted
on the stack, every split transformed): a time point is stored once per window that holds it, and the normalisation lives
outside the model.  Here the series is stored once (``channel`` x less memory at stride 1), ``fit`` / ``predict`` /
``evaluate`` take the set wherever they take an array, the scaler's tables come from one pass over the series
(chebgcn_window_stats) in exactly the form ``decode_series(scale=, shift=)`` takes, and moving a window a few TRs inside its
trial is a new row table, not a new array."""
import numpy as np
import torch

from . import ops
from .decode import window_starts          # noqa: F401  (the validation stage_windows shares with decode_series)


def row_table(run_lengths, run_starts, C):
    """The windows of a list of runs as rows of their concatenation: ``(rows, lo, hi)`` int64 ``[S]`` -- the global row of each
    window's first time point (run offset + start; runs in order, the starts of a run in the caller's order) and the first /
    last row a window of that run may start at (what ``jitter_rows`` clips to)."""
    rows, lo, hi = [], [], []
    off = 0
    for T, st in zip(run_lengths, run_starts):
        st = np.asarray(st, np.int64)
        rows.append(off + st)
        lo.append(np.full(len(st), off, np.int64))
        hi.append(np.full(len(st), off + int(T) - int(C), np.int64))
        off += int(T)
    return np.concatenate(rows), np.concatenate(lo), np.concatenate(hi)


def jitter_rows(rows, lo, hi, jitter, rng):
    """Every row displaced by an integer drawn uniformly from ``[-jitter, jitter]`` out of ``rng`` (a
    ``np.random.RandomState``; the global NumPy stream is never touched), clipped to ``[lo, hi]`` so that the window stays
    inside its own run.  ``jitter = 0`` draws nothing and returns the rows."""
    rows = np.asarray(rows, np.int64)
    if isinstance(jitter, bool) or not isinstance(jitter, (int, np.integer)) or jitter < 0:
        raise ValueError('jitter must be an int >= 0, got %r' % (jitter,))
    if jitter == 0:
        return rows.copy()
    d = rng.randint(-int(jitter), int(jitter) + 1, size=rows.shape).astype(np.int64)
    return np.clip(rows + d, lo, hi)


class WindowSet(object):
    """``S`` windows of ``channel`` time points over staged runs: ``planes`` ``[Ttot, Mp]`` (every run concatenated, the owner's
    internal vertex order, zero pad), ``rows`` the int64 device table of first rows, optionally the ``[channel, Mp]`` device
    tables of a normalisation ``x * scale + shift``.  ``len()`` and ``shape == (S, M, channel)`` are those of the array it
    stands for."""

    def __init__(self, owner, planes, run_lengths, run_starts, M, C):
        self.owner, self.planes = owner, planes
        self.run_lengths = [int(t) for t in run_lengths]
        self.run_starts = [np.asarray(s, np.int64) for s in run_starts]
        self.base_rows, self.lo, self.hi = row_table(self.run_lengths, self.run_starts, C)
        self.offsets = self.lo.copy()                   # run offset of every window: start = row - offset
        self.rows_host = self.base_rows.copy()
        self.rows = torch.as_tensor(self.rows_host).to(planes.device)
        self.shape = (int(len(self.base_rows)), int(M), int(C))
        self.tables = None              # (scale, shift) device [C, Mp], internal order
        self.scaler = None              # the same as NumPy [M, C] in the caller's order
        self.stats = None               # fit_scaler(): (mean, var) float64 [M, C] in the caller's order
        self.jitter, self.jitter_rng = 0, None

    def __len__(self):
        return self.shape[0]

    @property
    def starts(self):
        """The start of every window inside its run, as currently in use (after a displacement: the displaced ones)."""
        return self.rows_host - self.offsets

    @property
    def nbytes(self):
        """Device bytes of the set: planes, row table, tables."""
        n = self.planes.numel() * 4 + self.rows.numel() * 8
        return n + (sum(t.numel() * 4 for t in self.tables) if self.tables is not None else 0)

    # ---------------------------------------------------------------- tables

    def _caller_order(self, tab):
        """A device table ``[C, Mp]`` in the internal order -> NumPy ``[M, C]`` in the caller's."""
        M = self.shape[1]
        t = tab[:, :M].cpu().numpy().T
        order = self.owner._order
        if order is None:
            return np.ascontiguousarray(t)
        out = np.empty_like(t)
        out[np.asarray(order)] = t
        return out

    def set_tables(self, scale, shift):
        """Install a normalisation: ``scale`` / ``shift`` ``[M, channel]`` in the caller's vertex order (what ``fit_scaler``
        and ``decode_series`` use), both or neither."""
        if (scale is None) != (shift is None):
            raise ValueError('stage_windows: scale and shift come together (both or neither)')
        if scale is None:
            self.tables = self.scaler = None
            return self
        scale, shift = np.asarray(scale, np.float32), np.asarray(shift, np.float32)
        self.tables = tuple(self.owner._scale_tables(scale, shift))
        self.scaler = (scale.copy(), shift.copy())
        return self

    def share_tables(self, other):
        """Install the tables of another set of the same model (the validation set takes the training set's)."""
        self.tables, self.scaler = other.tables, other.scaler
        return self

    def fit_scaler(self):
        """Mean and population variance of every (vertex, channel) over the set's windows, none of them built
        (chebgcn_window_stats), installed on the set as ``scale = 1/std``, ``shift = -mean/std`` (a zero variance: 1 and
        ``-mean``, like sklearn's StandardScaler).  Returns ``(scale, shift)`` as ``[M, channel]`` float32 in the caller's
        vertex order; ``stats`` keeps ``(mean, var)`` in float64.  Always computed on the undisplaced windows."""
        S, M, C = self.shape
        rows = torch.as_tensor(self.base_rows).to(self.planes.device)
        mean, var, scale, shift = ops.window_stats(self.planes, rows, M, C)
        self.tables = (scale, shift)
        self.scaler = (self._caller_order(scale), self._caller_order(shift))
        self.stats = (self._caller_order(mean), self._caller_order(var))
        return self.scaler

    # ---------------------------------------------------------------- windows

    def gather(self, model, idx, out=None):
        """The windows ``idx`` (int32 device indices; None: all) as ``InternalPlanes`` ``[B, channel, Mp]`` of ``model``
        (chebgcn_gather_windows), straight into ``out`` when that has the shape."""
        if model is not self.owner and not model._same_order(self.owner):
            raise ValueError('this WindowSet is staged in the internal vertex order of another model')
        S, M, C = self.shape
        scale, shift = self.tables if self.tables is not None else (None, None)
        return model.as_internal(ops.gather_windows(self.planes, self.rows, M, C, idx, scale, shift, out))

    def materialise(self):
        """The ``[S, M, channel]`` float32 array the set stands for, in the caller's vertex order, as the model sees it (the
        tables applied, in float32 like the kernel: a rounded product, then a rounded sum)."""
        S, M, C = self.shape
        series = self._caller_order(self.planes)                                        # [M, Ttot]
        x = series[:, self.rows_host[:, None] + np.arange(C)[None, :]]                 # [M, S, C]
        x = np.ascontiguousarray(x.transpose(1, 0, 2))
        if self.scaler is not None:
            x = (x * self.scaler[0][None]).astype(np.float32) + self.scaler[1][None]
        return x.astype(np.float32, copy=False)

    # ---------------------------------------------------------------- displaced starts

    def set_rows(self, rows_host):
        """Upload another row table (same length) into the device table in place."""
        self.rows_host = np.asarray(rows_host, np.int64).copy()
        self.rows.copy_(torch.as_tensor(self.rows_host))

    def refill(self):
        """Called by ``fit`` each time it refills its index deque (once per epoch): with ``jitter > 0`` every window's start
        is redrawn around its undisplaced one and the table uploaded, once.  Returns the starts now in use."""
        if self.jitter:
            self.set_rows(jitter_rows(self.base_rows, self.lo, self.hi, self.jitter, self.jitter_rng))
        return self.starts

    def reset_rows(self):
        self.jitter, self.jitter_rng = 0, None
        if not np.array_equal(self.rows_host, self.base_rows):
            self.set_rows(self.base_rows)


class Series(object):
    """``stage_windows`` / ``fit_series`` of ``base_model``.  Uses the model's ``_decode_args`` / ``_stage_series`` /
    ``_scale_tables`` (decode.Decode), its sizes and ``fit``."""

    window_scaler = None            # (scale, shift) [M, channel] fitted by fit_series(standardize=True), else None

    def _window_args(self, series, starts, scale, shift, what):
        runs, run_starts, _, scale, shift, _ = self._decode_args(series, starts, 1, scale, shift, 'auto', None, 'logits', what)
        if (scale is None) != (shift is None):
            raise ValueError('%s: scale and shift come together (both or neither)' % what)
        return runs, run_starts, scale, shift

    def _stage_window_set(self, runs, run_starts, scale, shift, what):
        if self.device.type != 'cuda':
            raise RuntimeError('%s: the model has no device to run on (%s)' % (what, self.device))
        M0, C = int(self._M0), int(self.channel)
        lengths = [int(r.shape[0]) for r in runs]
        planes = torch.empty((sum(lengths), ops.plane_stride(M0)), dtype=torch.float32, device=self.device)
        off = 0
        for r, T in zip(runs, lengths):
            self._stage_series(r, out=planes[off:off + T])
            off += T
        return WindowSet(self, planes, lengths, run_starts, M0, C).set_tables(scale, shift)

    def stage_windows(self, series, starts=None, scale=None, shift=None):
        """A ``WindowSet``: the windows ``x[v][c] = series[start + c][v]`` of one ``[T, M]`` run or a list of runs (``starts``:
        an array per run; any order, repeats allowed; None: every window, stride 1 -- ``decode_series``' rules), staged on
        the device once as planes.  ``fit`` / ``predict`` / ``evaluate`` / ``model_perf.test`` / ``model_perf.predict`` take
        it wherever they take ``[S, M, channel]`` data.  ``scale`` / ``shift`` ``[M, channel]``: every window is seen as
        ``x * scale + shift``.  Arguments are refused (``ValueError``) before anything touches the device."""
        runs, run_starts, scale, shift = self._window_args(series, starts, scale, shift, 'stage_windows')
        return self._stage_window_set(runs, run_starts, scale, shift, 'stage_windows')

    def fit_series(self, train_series, train_starts, train_labels, val_series, val_starts, val_labels, standardize=False,
                   jitter=0, jitter_seed=0, best_checkpoint_dir=None):
        """``fit`` on scans: both splits are staged as ``WindowSet``s (``stage_windows``' rules; labels one per window, runs in
        order, the starts of a run in the caller's order) and ``fit`` runs on them; returns what ``fit`` returns.

        * ``standardize``: the training set's per-vertex-and-channel ``scale = 1/std`` / ``shift = -mean/std`` are fitted on
          the device (``WindowSet.fit_scaler``), applied to both splits, kept as ``model.window_scaler`` (``[M, channel]``
          each; None without) and written into the checkpoints.  Pass them to ``decode_series(scale=, shift=)``.
        * ``jitter = j > 0``: each time ``fit`` refills its index deque (once per epoch) every training window's start is
          displaced by an integer from ``[-j, j]`` drawn out of ``np.random.RandomState(jitter_seed)`` and clipped so that the
          window stays inside its run.  Labels, validation windows and the scaler (fitted on the undisplaced windows) are
          unaffected; the global NumPy stream sees exactly the draws of ``fit``.  With ``record_fit``, ``fit_log['starts']``
          holds the starts of every refill."""
        what = 'fit_series'
        if isinstance(jitter, bool) or not isinstance(jitter, (int, np.integer)) or jitter < 0:
            raise ValueError('fit_series: jitter must be an int >= 0, got %r' % (jitter,))
        if isinstance(jitter_seed, bool) or not isinstance(jitter_seed, (int, np.integer)) or not 0 <= jitter_seed < 2 ** 32:
            raise ValueError('fit_series: jitter_seed must be an int in [0, 2**32), got %r' % (jitter_seed,))
        tr = self._window_args(train_series, train_starts, None, None, what)
        va = self._window_args(val_series, val_starts, None, None, what)
        for (runs, run_starts, _, _), labels, name in ((tr, train_labels, 'train'), (va, val_labels, 'val')):
            n = sum(len(s) for s in run_starts)
            if np.ndim(labels) != 1 or len(labels) != n:
                raise ValueError('fit_series: %s_labels must be one label per window (%d), got shape %s'
                                 % (name, n, np.shape(labels)))
        ws_train = self._stage_window_set(tr[0], tr[1], None, None, what)
        ws_val = self._stage_window_set(va[0], va[1], None, None, what)
        self.window_scaler = None
        if standardize:
            self.window_scaler = ws_train.fit_scaler()
            ws_val.share_tables(ws_train)
        ws_train.jitter, ws_train.jitter_rng = int(jitter), np.random.RandomState(int(jitter_seed))
        try:
            return self.fit(ws_train, train_labels, ws_val, val_labels, best_checkpoint_dir)
        finally:
            ws_train.reset_rows()

    # ---------------------------------------------------------------- checkpoints

    def _scaler_to_sd(self, sd):
        """``window_scaler`` into a checkpoint: one float32 tensor ``[2, M, channel]`` (scale, shift), only when there is one."""
        if self.window_scaler is not None:
            sd['window_scaler'] = torch.as_tensor(np.stack([np.asarray(t, np.float32) for t in self.window_scaler]))
        return sd

    def _scaler_from_sd(self, sd):
        """The optional key back: a checkpoint without it (every earlier one) leaves ``window_scaler`` None."""
        t = sd.get('window_scaler')
        if t is None:
            self.window_scaler = None
            return
        a = np.asarray(t, np.float32)
        want = (2, int(self._M0), int(self.channel))
        if a.shape != want:
            raise ValueError('checkpoint window_scaler has shape %s, the model wants %s' % (a.shape, want))
        self.window_scaler = (a[0].copy(), a[1].copy())
