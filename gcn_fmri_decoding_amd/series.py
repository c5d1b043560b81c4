"""Training on scans: a ``WindowSet`` is a dataset that IS windows of scans -- the runs staged once as planes, the windows a
device table, cut (and scaled) on the device batch by batch -- and ``Series`` carries ``stage_windows`` / ``fit_series`` /
``stage_events`` / ``fit_events`` and is a base of ``models_gcn.base_model``.

The reference builds ``[S, M, channel]`` on the host (utils.py: the windows cut with NumPy, stacked, an NDStandardScaler fitted
on the stack, every split transformed): a time point is stored once per window that holds it, and the normalisation lives
outside the model.  Here the series is stored once (``channel`` x less memory at stride 1), ``fit`` / ``predict`` /
``evaluate`` take the set wherever they take an array, the scaler's tables come from one pass over the series
(chebgcn_window_stats) in exactly the form ``decode_series(scale=, shift=)`` takes.  Balancing unbalanced classes (the
reference's ``sampling``) is a table as well: ``balance_plan`` says which original windows every extra window is the mean of,
and the mix gathers form them batch by batch.

``WindowSet`` holds what every set does -- tables and scaler, the owner check of ``gather``, ``balance``, ``materialise``,
``nbytes`` -- and two kinds say how a window is cut.  ``StartWindowSet``: ``channel`` consecutive rows from an int64 table of
first rows (``stage_windows(starts=)``, ``fit_series``); moving a window a few TRs inside its trial is a new row table, not a
new array, and only this kind can be displaced.  ``EventWindowSet``: a list of rows per window, ``fold`` of them averaged per
channel (the windows of an event design, ``events.match_events``: ``stage_windows(index=)`` / ``stage_events`` /
``fit_events``).

``WindowSet.augment`` makes the set stand for ``copies`` perturbed copies of itself (the reference's ``train_dataarg`` /
``drop_rate``): vertex dropout and a time shift inside the window's symmetric reflection, drawn by a counter-based generator
(``drop_vertices`` / ``time_shifts``, the NumPy restatement of the one in include/chebgcn.h), applied while a batch is gathered
(chebgcn_gather_windows_reflect, chebgcn_window_drop) and drawn anew at every ``refill``.

``WindowSet.select`` makes a VIEW: a set of the same kind over some of the runs that shares the planes and has tables of its own
(``select_runs``) -- what a fold of ``crossval.CrossValidate`` is."""
import numpy as np
import torch

from . import ops
from .decode import check_run, check_table, run_list, window_starts    # (the validation shared with decode_series)  # noqa: F401
from .runs import AUG_KEY, AUG_MUL1, AUG_MUL2, AUG_WINDOW, aug_draw     # (the generator ``stats`` draws with as well)  # noqa: F401


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _both_or_neither(scale, shift, what):
    if (scale is None) != (shift is None):
        raise ValueError('%s: scale and shift come together (both or neither)' % what)


def check_jitter(jitter, what=''):
    if not _is_int(jitter) or jitter < 0:
        raise ValueError('%sjitter must be an int >= 0, got %r' % (what, jitter))
    return int(jitter)


def check_seed(seed, name, what):
    if not _is_int(seed) or not 0 <= seed < 2 ** 32:
        raise ValueError('%s: %s must be an int in [0, 2**32), got %r' % (what, name, seed))
    return int(seed)


def run_offsets(run_lengths):
    """The first row of every run in the concatenation of the runs, int64."""
    return np.concatenate([[0], np.cumsum([int(t) for t in run_lengths])[:-1]]).astype(np.int64)


def row_table(run_lengths, run_starts, C, offsets=None):
    """The windows of a list of runs as rows of their concatenation: ``(rows, lo, hi)`` int64 ``[S]`` -- the global row of each
    window's first time point (run offset + start; runs in order, the starts of a run in the caller's order) and the first /
    last row a window of that run may start at (what ``jitter_rows`` clips to).  ``offsets``: the first row of every run where
    the runs are not the whole concatenation in order (the runs of a view, ``select_runs``)."""
    rows, lo, hi = [], [], []
    offsets = run_offsets(run_lengths) if offsets is None else offsets
    for T, st, off in zip(run_lengths, run_starts, offsets):
        st, off = np.asarray(st, np.int64), int(off)
        rows.append(off + st)
        lo.append(np.full(len(st), off, np.int64))
        hi.append(np.full(len(st), off + int(T) - int(C), np.int64))
    return np.concatenate(rows), np.concatenate(lo), np.concatenate(hi)


def select_runs(run_lengths, offsets, run_windows, runs, what='select'):
    """The table arithmetic of a view over the runs ``runs`` (positions into the set's runs, any order, no repeats) of a set
    whose runs have ``run_lengths`` time points, begin at the rows ``offsets`` of the planes and hold ``run_windows`` windows:
    ``(windows, lengths, offsets, counts)`` -- the int64 indices of the set's original windows that belong to those runs, run
    by run in the order of ``runs`` and inside a run in the set's order, and the lengths, first rows and window counts of the
    selected runs.  Host only."""
    a = np.asarray(runs)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in 'iu':
        raise ValueError('%s: runs must be a non-empty 1-D int array of run positions, got %s %s' % (what, a.dtype, a.shape))
    a = a.astype(np.int64)
    n = len(run_lengths)
    if a.min() < 0 or a.max() >= n:
        raise ValueError('%s: every run position must lie in [0, %d); got %d ... %d' % (what, n, a.min(), a.max()))
    if len(np.unique(a)) != len(a):
        raise ValueError('%s: a run is named twice in %s' % (what, a.tolist()))
    counts = np.asarray(run_windows, np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)      # the first window of every run
    windows = np.concatenate([first[r] + np.arange(counts[r], dtype=np.int64) for r in a])
    return windows, np.asarray(run_lengths, np.int64)[a], np.asarray(offsets, np.int64)[a], counts[a]


def jitter_rows(rows, lo, hi, jitter, rng):
    """Every row displaced by an integer drawn uniformly from ``[-jitter, jitter]`` out of ``rng`` (a
    ``np.random.RandomState``; the global NumPy stream is never touched), clipped to ``[lo, hi]`` so that the window stays
    inside its own run.  ``jitter = 0`` draws nothing and returns the rows."""
    rows = np.asarray(rows, np.int64)
    jitter = check_jitter(jitter)
    if jitter == 0:
        return rows.copy()
    d = rng.randint(-jitter, jitter + 1, size=rows.shape).astype(np.int64)
    return np.clip(rows + d, lo, hi)


# ---- what the augmentation draws from ``runs.aug_draw``, the generator of include/chebgcn.h restated in NumPy ----------------------
AUG_SHIFT_DRAW = 0xFFFFFFFF
AUG_COPIES_MAX = 64


def drop_vertices(seed, refill, i, D, M):
    """The ``D`` vertices (int64, in ``[0, M)``, with replacement, the caller's vertex order) that augmented window ``i`` drops
    at refill ``refill``: draw ``d`` mapped as ``(u * M) >> 32``.  ``i`` may be an array: ``[len(i), D]``."""
    i = np.asarray(i)
    u = aug_draw(seed, refill, i[..., None], np.arange(int(D), dtype=np.uint64))
    return ((u * np.uint64(int(M))) >> np.uint64(32)).astype(np.int64)


def time_shifts(seed, refill, n, C):
    """The time shifts ``r`` in ``[0, C)`` of the augmented windows ``0 .. n - 1`` at refill ``refill`` (int32 ``[n]``): draw
    ``AUG_SHIFT_DRAW`` of every window, mapped as ``(u * C) >> 32``."""
    u = aug_draw(seed, refill, np.arange(int(n), dtype=np.uint64), np.uint64(AUG_SHIFT_DRAW))
    return ((u * np.uint64(int(C))) >> np.uint64(32)).astype(np.int32)


def reflect_channels(C, r):
    """``rho(c + r)`` for ``c < C``: the source channel of every channel of a window shifted by ``r`` in ``[0, C)`` inside its
    symmetric reflection -- ``np.pad(x, C, 'symmetric')[r + C : r + 2 C]`` is ``x[rho(c + r)]``.  ``r`` may be an array
    ``[n]``: ``[n, C]``."""
    j = np.asarray(r, np.int64)[..., None] + np.arange(int(C), dtype=np.int64)
    return np.where(j < C, j, 2 * int(C) - 1 - j)


def check_augment_args(what, copies, drop_rate, time_shift, drop_value, seed):
    """The arguments of ``WindowSet.augment`` / ``fit_series(augment=...)``, refused with a ``ValueError`` or returned as
    ``(copies, drop_rate, time_shift, drop_value, seed)``."""
    if not _is_int(copies) or not 0 <= copies <= AUG_COPIES_MAX:
        raise ValueError('%s: the number of augmented copies must be an int in [0, %d], got %r' % (what, AUG_COPIES_MAX, copies))
    if isinstance(drop_rate, bool) or not isinstance(drop_rate, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(drop_rate) <= 1.0:
        raise ValueError('%s: drop_rate must be a number in [0, 1], got %r' % (what, drop_rate))
    if not isinstance(time_shift, (bool, np.bool_)):
        raise ValueError('%s: time_shift must be a bool, got %r' % (what, time_shift))
    if isinstance(drop_value, bool) or not isinstance(drop_value, (int, float, np.integer, np.floating)) \
            or not np.isfinite(float(drop_value)):
        raise ValueError('%s: drop_value must be a finite number, got %r' % (what, drop_value))
    return int(copies), float(drop_rate), bool(time_shift), float(drop_value), check_seed(seed, 'the augmentation seed', what)


SAMPLING_MAX = 16              # sources of one synthetic window at most (the mix gather holds them in registers)


def check_sampling(sampling, what, least=0):
    """``sampling`` as an int in ``[least, SAMPLING_MAX]``; a bool, a non-int or a value outside is a ``ValueError``."""
    if not _is_int(sampling) or not least <= sampling <= SAMPLING_MAX:
        raise ValueError('%s: sampling must be an int in [%d, %d], got %r' % (what, least, SAMPLING_MAX, sampling))
    return int(sampling)


def _int_vector(a, name, what, n=None):
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype.kind not in 'iu' or (n is not None and len(a) != n):
        raise ValueError('%s: %s must be a 1-D int array%s, got %s %s'
                         % (what, name, '' if n is None else ' of %d entries' % n, a.dtype, a.shape))
    return a.astype(np.int64)


def check_balance_args(what, labels, S, sampling, seed, groups, nruns, resample):
    """The arguments of ``WindowSet.balance`` / ``fit_series(sampling=...)``, refused with a ``ValueError`` or returned as
    ``(labels int64 [S], one group id per run int64 [nruns])``."""
    check_sampling(sampling, what)
    labels = _int_vector(labels, 'labels', what, S)
    check_seed(seed, 'the sampling seed', what)
    if not isinstance(resample, (bool, np.bool_)):
        raise ValueError('%s: resample must be a bool, got %r' % (what, resample))
    if groups is None:
        return labels, np.arange(nruns, dtype=np.int64)
    return labels, _int_vector(groups, 'the sampling groups (one id per run)', what, nruns)


def balance_plan(labels, groups, sampling, rng):
    """Which windows top up the small classes of an unbalanced set: ``(src, cnt, new_labels)``.

    ``labels`` int ``[S]``, ``groups`` int ``[S]`` (the scan, or subject, of every window), ``sampling`` an int in [1, 16],
    ``rng`` a ``np.random.RandomState`` (the global NumPy stream is never touched).  With ``n_c`` windows of class ``c`` and
    ``n_max`` the largest class, a class with ``2 n_c <= n_max`` gets ``n_c * (n_max // n_c - 1)`` extra windows, every other
    class none.  Window ``w`` of the balanced set is the mean of the ``cnt[w]`` windows ``src[w, :cnt[w]]``:

    * the originals keep the indices ``0 .. S-1`` (``cnt = 1``, ``src[w, 0] = w``); the extra windows follow, classes in
      ascending label order; ``new_labels`` ``[S']`` are the labels of all of them;
    * ``sampling == 1``: an extra window is ONE window of its class, drawn uniformly with replacement;
    * ``sampling >= 2``: per extra window, groups are drawn uniformly with replacement and all windows of class ``c`` of the
      drawn group appended, in window order, to a pool (a group without any adds nothing, a group drawn twice adds twice) until
      the pool holds at least ``sampling`` windows; the sources are ``sampling`` entries of the pool, drawn uniformly with
      replacement -- a synthetic window, the mean of same-class windows of a few scans.

    ``src`` is int64 ``[S', max(1, sampling)]`` (entries past ``cnt`` repeat entry 0), ``cnt`` int32 ``[S']``."""
    what = 'balance_plan'
    sampling = check_sampling(sampling, what, least=1)
    labels = _int_vector(labels, 'labels', what)
    groups = _int_vector(groups, 'groups', what, len(labels))
    S = len(labels)
    if S == 0:
        raise ValueError('%s: labels is empty' % what)
    smax = max(1, sampling)
    classes, counts = np.unique(labels, return_counts=True)                # ascending labels
    n_max = int(counts.max())
    group_ids = np.unique(groups)
    src = [np.repeat(np.arange(S, dtype=np.int64)[:, None], smax, axis=1)]
    new_labels = [labels]
    for c, n_c in zip(classes.tolist(), counts.tolist()):
        extra = n_c * (n_max // n_c - 1) if 2 * n_c <= n_max else 0
        if extra == 0:
            continue
        own = np.flatnonzero(labels == c)                                  # window order
        if sampling == 1:
            rows = own[rng.randint(0, n_c, size=extra)][:, None]
        else:
            of_group = [own[groups[own] == g] for g in group_ids]
            rows = np.empty((extra, sampling), np.int64)
            for x in range(extra):
                pool, n = [], 0
                while n < sampling:
                    t = of_group[rng.randint(0, len(group_ids))]
                    pool.append(t)
                    n += len(t)
                rows[x] = np.concatenate(pool)[rng.randint(0, n, size=sampling)]
        src.append(rows)
        new_labels.append(np.full(extra, c, np.int64))
    src = np.concatenate(src)
    cnt = np.ones(len(src), np.int32)
    cnt[S:] = sampling
    return src, cnt, np.concatenate(new_labels).astype(labels.dtype)


class WindowSet(object):
    """``S`` windows of ``channel`` time points over staged runs, the machinery both kinds of set share: ``planes``
    ``[Ttot, Mp]`` (every run concatenated, the owner's internal vertex order, zero pad), optionally the ``[channel, Mp]`` device
    tables of a normalisation ``x * scale + shift``.  ``len()`` and ``shape == (S, M, channel)`` are those of the array it
    stands for.  After ``balance()`` the set stands for ``S' >= S`` windows: the originals and, behind them, the windows
    that top up the small classes, each the mean of ``cnt`` source windows (``sources``).

    A kind names each original by an int64 KEY (``_keys()``: its first row, or its place in the index table) and says how keys
    become windows on the host (``_originals``) and on the device (``_gather``, ``_stats``), and what the mix table of a plan
    holds (``_mix_table``: ``[S', smax]`` keys)."""

    def __init__(self, owner, planes, run_lengths, run_windows, M, C, offsets=None):
        self.owner, self.planes = owner, planes
        self.run_lengths = [int(t) for t in run_lengths]
        self.run_windows = [int(n) for n in run_windows]                # windows of every run
        # the first row of every run in ``planes``: the runs one behind the other, or -- of a view (``select``) -- wherever the
        # parent staged them
        self.run_offsets = run_offsets(self.run_lengths) if offsets is None else np.asarray(offsets, np.int64).copy()
        self.offsets = np.repeat(self.run_offsets, self.run_windows)    # run offset of every window: start = row - offset
        self.shape = self.shape_base = (int(sum(self.run_windows)), int(M), int(C))   # shape_base: the originals', whatever plan
        self.tables = None              # (scale, shift) device [C, Mp], internal order
        self.scaler = None              # the same as NumPy [M, C] in the caller's order
        self.stats = None               # fit_scaler(): (mean, var) float64 [M, C] in the caller's order
        self.plan = None                # balance(): dict(src, cnt, labels, groups, sampling, resample, rng)
        self.mix_rows_host = self.mix_rows = self.mix_cnt = None   # [S', smax] keys of every source; device: int64 / int32
        self.aug = None                 # augment(): dict(copies, base_len, D, time_shift, drop_value, seed, refill, shifts)
        self.aug_shifts = self.aug_pos = None       # device int32: [copies * S'] time shifts; [M] caller vertex -> position

    def __len__(self):
        return self.shape[0]

    @property
    def nbytes(self):
        """Device bytes of the set: every device tensor it holds (planes, row or index table, mix tables, the tables of an
        augmentation) and the scaler's tables."""
        held = [t for t in vars(self).values() if isinstance(t, torch.Tensor)] + list(self.tables or ())
        return sum(t.numel() * t.element_size() for t in held)

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
        _both_or_neither(scale, shift, 'stage_windows')
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
        """Mean and population variance of every (vertex, channel) over the set's ``S`` ORIGINAL windows, none of them built
        (chebgcn_window_stats; of windows that are lists of rows chebgcn_window_stats_indexed, over the folded values as the
        gather forms them in float32), installed on the set as ``scale = 1/std``, ``shift = -mean/std`` (a zero variance: 1
        and ``-mean``, like sklearn's StandardScaler).  Returns ``(scale, shift)`` as ``[M, channel]`` float32 in the caller's
        vertex order; ``stats`` keeps ``(mean, var)`` in float64.  Always computed on the undisplaced windows, whatever plan
        is installed."""
        mean, var, scale, shift = self._stats()
        self.tables = (scale, shift)
        self.scaler = (self._caller_order(scale), self._caller_order(shift))
        self.stats = (self._caller_order(mean), self._caller_order(var))
        return self.scaler

    def _stat_planes(self):
        """``(planes, delta)`` the statistics kernels run over: the set's runs one behind the other and nothing else, and per
        run what to add to a row of ``self.planes`` to name the same row there.  The kernels sum in float64 relative to the
        FIRST row of the buffer they are given and in the order of its rows, so the statistics of a view are those of a set
        staged from its runs alone, bit for bit, only when the kernels see exactly those runs in the view's order: the set's
        own planes (a set that is no view), a slice of them (a view of consecutive runs), else a compact copy of the view's
        runs that lives for the call."""
        delta = run_offsets(self.run_lengths) - self.run_offsets
        total = int(sum(self.run_lengths))
        if (delta == delta[0]).all():
            first = int(self.run_offsets[0])
            whole = first == 0 and total == int(self.planes.shape[0])
            return (self.planes if whole else self.planes[first:first + total]), delta
        return torch.cat([self.planes[o:o + t] for o, t in zip(self.run_offsets.tolist(), self.run_lengths)]), delta

    # ---------------------------------------------------------------- views

    def windows_of(self, runs):
        """The int64 indices of the set's ORIGINAL windows that belong to the runs ``runs`` (positions into the set's runs, any
        order, no repeats): run by run in that order, inside a run in the set's order -- what slices the labels of a view."""
        return select_runs(self.run_lengths, self.run_offsets, self.run_windows, runs, 'windows_of')[0]

    def select(self, runs):
        """A view: a set of the same kind over the original windows of the runs ``runs`` (``windows_of(runs)``, in that order)
        that SHARES this set's ``planes`` -- the same tensor, nothing is copied and no kernel runs -- and has row / index
        tables of its own.  ``view.materialise()`` is ``self.materialise()[self.windows_of(runs)]``; its starts, jitter bounds
        and run lengths are those of the selected runs; it takes over this set's scaler tables (``share_tables``), and
        ``fit_scaler``, ``balance`` (``groups``: one id per SELECTED run), ``augment``, ``jitter`` / ``refill`` and
        ``set_rows`` work on it as on a set staged from those runs alone and change neither this set nor another view.  A view
        of a view is a view of the first set.  A set that carries a plan, an augmentation or displaced rows refuses
        (``ValueError``): select first, then perturb."""
        if self.plan is not None or self.aug is not None or self._displaced():
            raise ValueError('select: the set carries %s; select first, then perturb (balance(None, 0), augment(None, 0), '
                             'reset_rows())' % ('a plan' if self.plan is not None else 'an augmentation' if self.aug is not None
                                                else 'displaced rows'))
        windows, lengths, offsets, counts = select_runs(self.run_lengths, self.run_offsets, self.run_windows, runs)
        return self._view(windows, lengths, offsets, counts).share_tables(self)

    def _displaced(self):
        return False

    # ---------------------------------------------------------------- windows

    def gather(self, model, idx, out=None):
        """The windows ``idx`` (int32 device indices; None: all) as ``InternalPlanes`` ``[B, channel, Mp]`` of ``model``
        (chebgcn_gather_windows, of a balanced set chebgcn_gather_windows_mix; of windows that are lists of rows
        chebgcn_gather_windows_indexed either way), straight into ``out`` when that has the shape."""
        if model is not self.owner and not model._same_order(self.owner):
            raise ValueError('this WindowSet is staged in the internal vertex order of another model')
        scale, shift = self.tables if self.tables is not None else (None, None)
        sources = None if self.plan is None else self.plan['cnt'].mean()
        if self.aug is None:
            return model.as_internal(self._gather(idx, scale, shift, out, sources))
        # an augmented set: the copy's window (through the reflection where it is shifted), then its dropped vertices -- both on
        # the current stream, the second in place on what the first wrote
        aug = self.aug
        if idx is None:
            idx = torch.arange(self.shape[0], dtype=torch.int32, device=self.planes.device)
        if aug['time_shift']:
            x = self._gather_shifted(idx, scale, shift, out)
        else:
            x = self._gather(torch.remainder(idx, aug['base_len']), scale, shift, out, sources)
        if aug['D']:
            ops.window_drop(x, idx, self.shape[1], aug['D'], aug['seed'], aug['refill'], self.aug_pos, scale, shift,
                            aug['drop_value'])
        return model.as_internal(x)

    # ---------------------------------------------------------------- augmentation

    def augment(self, labels, copies, drop_rate=0.0, time_shift=False, drop_value=1.0, seed=0):
        """Make the set stand for ``copies`` perturbed copies of itself (the reference's ``train_dataarg`` / ``drop_rate``);
        returns the labels of the augmented set, ``np.tile(labels, copies)``.  With ``S'`` the set's length now (after
        ``balance``, if a plan is installed), ``len()`` and ``shape[0]`` become ``copies * S'``; window ``i`` is base window
        ``i % S'``, copy ``i // S'``, and EVERY copy is perturbed (``copies = 1``: fresh perturbations of the set at every
        refill).  ``copies = 0`` removes the augmentation (``labels`` may be None then).  ``shape_base`` stays the originals'.

        * vertex dropout: ``D = int(drop_rate * M)`` vertices of every window, drawn with replacement out of the ``M`` real
          ones in the caller's order, take ``drop_value`` in all channels BEFORE the tables: with tables the stored value is
          ``fl(fl(drop_value * scale) + shift)``.  The pad stays zero.  Works on every kind of set, balanced or not.
        * ``time_shift``: one ``r`` in ``[0, channel)`` per window; channel ``c`` takes source channel ``rho(c + r)``
          (``reflect_channels``): ``np.pad(x, channel, 'symmetric')[r + channel : r + 2 * channel]``.  Not on a balanced set
          (``ValueError``): the mix kernels average whole source windows.
        * the draws are ``drop_vertices(seed, refill, i, D, M)`` and ``time_shifts(seed, refill, copies * S', channel)``: a
          function of the seed, the refill number and the window's index alone -- never of the batch a window lands in.
          ``refill()`` (once per epoch of ``fit``) advances the refill number: every epoch sees new perturbations.

        Departure from the reference, on purpose: it repeats the labels but draws the SOURCE window of every copy at random,
        so labels and data come apart there; here the labels follow the base window.  Arguments are refused (``ValueError``)
        before anything touches the device.  ``materialise()`` returns the windows of the current refill."""
        copies, drop_rate, time_shift, drop_value, seed = check_augment_args('augment', copies, drop_rate, time_shift,
                                                                             drop_value, seed)
        base_len = self.shape[0] if self.aug is None else self.aug['base_len']
        if copies == 0:
            self._augment_removed(base_len)
            return None if labels is None else np.asarray(labels).copy()
        labels = np.asarray(labels)
        if labels.ndim != 1 or len(labels) != base_len:
            raise ValueError('augment: labels must be one label per window (%d), got shape %s' % (base_len, labels.shape))
        if time_shift and self.plan is not None:
            raise ValueError('augment: time_shift on a balanced set is not served (the mix kernels average whole source '
                             'windows); remove the plan (balance(None, 0)) or leave time_shift out')
        if copies * base_len > 0x7fffffff:
            raise ValueError('augment: %d copies of %d windows are more than an int32 index names' % (copies, base_len))
        self._augment_removed(base_len)
        M = self.shape[1]
        self.aug = dict(copies=copies, base_len=base_len, D=int(drop_rate * M), time_shift=time_shift, drop_value=drop_value,
                        seed=seed, refill=0, shifts=None)
        self.shape = (copies * base_len,) + self.shape[1:]
        order = self.owner._order
        if self.aug['D'] and order is not None:
            pos = np.empty(M, np.int32)
            pos[np.asarray(order)] = np.arange(M, dtype=np.int32)
            self.aug_pos = torch.as_tensor(pos).to(self.planes.device)
        self._aug_draw()
        return np.tile(labels, copies)

    def _augment_removed(self, base_len):
        if self.aug is not None:
            self.aug = self.aug_shifts = self.aug_pos = None
            self.shape = (base_len,) + self.shape[1:]
            self._aug_tables()

    def _aug_draw(self):
        """The time shifts of the current refill, drawn on the host and uploaded once, and the kind's shifted table."""
        aug = self.aug
        if not aug['time_shift']:
            return
        aug['shifts'] = time_shifts(aug['seed'], aug['refill'], self.shape[0], self.shape[2])
        if self.aug_shifts is None:
            self.aug_shifts = torch.as_tensor(aug['shifts']).to(self.planes.device)
        else:
            self.aug_shifts.copy_(torch.as_tensor(aug['shifts']))
        self._aug_tables()

    def _aug_tables(self):
        """What a kind keeps on the device for its shifted windows (dropped with the augmentation)."""

    def _aug_refill(self):
        if self.aug is not None:
            self.aug['refill'] += 1
            self._aug_draw()

    def _augmented(self, x):
        """``x`` ``[S', M, C]`` (the caller's order, before the tables) -> the ``copies * S'`` windows of the current refill."""
        aug = self.aug
        n, M, C = self.shape
        x = x[np.arange(n) % aug['base_len']]                                             # (a new array)
        if aug['time_shift']:
            x = np.take_along_axis(x, reflect_channels(C, aug['shifts'])[:, None, :], axis=2)
        if aug['D']:
            v = drop_vertices(aug['seed'], aug['refill'], np.arange(n), aug['D'], M)           # [n, D]
            x[np.arange(n)[:, None], v] = np.float32(aug['drop_value'])
        return x

    def materialise(self):
        """The ``[S, M, channel]`` float32 array the set stands for, in the caller's vertex order, as the model sees it: every
        level in float32 like the kernels -- the originals as their kind cuts them, of a balanced set the ``S'`` windows, the
        sources added in their order and divided once by ``cnt``, then the tables (a rounded product, then a rounded sum).  Of an
        augmented set the ``copies * S'`` windows of the current refill, bit for bit what ``gather`` forms: the copy's channels
        taken through the reflection, then ``drop_value`` at its dropped vertices, then the tables."""
        series = self._caller_order(self.planes)                                        # [M, Ttot]
        if self.plan is None:
            x = self._originals(series, self._keys())                                   # [M, S, C]
        else:
            tab, cnt = self.mix_rows_host, self.plan['cnt']
            x = self._originals(series, tab[:, 0])
            for j in range(1, tab.shape[1]):
                more = cnt > j
                if more.any():
                    x[:, more] = x[:, more] + self._originals(series, tab[more, j])
            mixed = cnt > 1
            x[:, mixed] = x[:, mixed] / cnt[mixed].astype(np.float32)[None, :, None]
        x = np.ascontiguousarray(x.transpose(1, 0, 2))
        if self.aug is not None:
            x = self._augmented(x)
        if self.scaler is not None:
            x = (x * self.scaler[0][None]).astype(np.float32) + self.scaler[1][None]
        return x.astype(np.float32, copy=False)

    # ---------------------------------------------------------------- balanced classes

    @property
    def sources(self):
        """``(src, cnt)`` of the plan in use (``balance_plan``), None without one."""
        return None if self.plan is None else (self.plan['src'], self.plan['cnt'])

    def _upload_mix(self, extra=None):
        """The ``[S', smax]`` mix table of the plan in use (``_mix_table``; ``extra``: rows of the extra windows that are not
        their sources' undisplaced ones), in one upload."""
        tab = self.mix_rows_host = np.ascontiguousarray(self._mix_table(extra))
        if self.mix_rows is None or tuple(self.mix_rows.shape) != tab.shape:
            self.mix_rows = torch.as_tensor(tab).to(self.planes.device)
            self.mix_cnt = torch.as_tensor(self.plan['cnt']).to(self.planes.device)
        else:
            self.mix_rows.copy_(torch.as_tensor(tab))

    def _redraw(self):
        """The plan drawn again out of its stream where ``resample`` asks for it; says whether it was."""
        plan = self.plan
        if plan is None or not plan['resample']:
            return False
        src, cnt, _ = balance_plan(plan['labels'], plan['groups'], plan['sampling'], plan['rng'])
        assert np.array_equal(cnt, plan['cnt'])                        # the counts depend on the labels alone
        plan['src'] = src
        return True

    def refill(self):
        """Called by ``fit`` each time it refills its index deque (once per epoch): redraws the plan when ``resample`` is
        set, one upload; of an augmented set the refill number advances and the time shifts are drawn again, one upload.
        Returns the starts (rows) in use."""
        if self._redraw():
            self._upload_mix()
        self._aug_refill()
        return self.starts

    def _plan_removed(self):
        pass

    def balance(self, labels, sampling, seed=0, groups=None, resample=False):
        """Top up the small classes (``balance_plan``): installs the plan and returns the ``S'`` labels of the balanced set.
        Afterwards ``len()`` and ``shape[0]`` are ``S'``, ``gather()`` forms the means on the device, ``materialise()``
        returns the ``S'`` windows and ``sources`` is ``(src, cnt)``; ``starts`` stays the ``S`` originals' starts.

        ``labels``: one int per original window.  ``sampling``: 1 re-draws windows of a small class, ``n >= 2`` (at most 16)
        forms every extra window as the mean of ``n`` same-class windows of randomly drawn groups; 0 removes the plan.
        ``groups``: one int id PER RUN -- the runs of one subject form one group; None: every run is its own.  ``seed``
        starts the balancing stream ``np.random.RandomState(seed)``, which every later draw of the plan comes out of (the
        global NumPy stream is never touched).  ``resample``: ``refill()`` redraws the plan (once per epoch of ``fit``);
        the labels do not change with it.  Arguments are refused (``ValueError``) before anything touches the device."""
        sampling = check_sampling(sampling, 'balance')
        if self.aug is not None and (sampling or self.plan is not None):
            raise ValueError('balance: the set is augmented; remove the augmentation first (augment(None, 0)) -- it goes on top '
                             'of the plan')
        if sampling == 0:
            if self.plan is not None:
                self.plan = self.mix_rows_host = self.mix_rows = self.mix_cnt = None
                self.shape = self.shape_base
                self._plan_removed()
            return None if labels is None else np.asarray(labels).copy()
        labels, run_groups = check_balance_args('balance', labels, self.shape_base[0], sampling, seed, groups,
                                                len(self.run_windows), resample)
        groups = np.repeat(run_groups, self.run_windows)
        rng = np.random.RandomState(int(seed))
        src, cnt, new_labels = balance_plan(labels, groups, sampling, rng)
        self.plan = dict(src=src, cnt=cnt, labels=labels, groups=groups, sampling=sampling, resample=bool(resample), rng=rng)
        self.shape = (int(len(src)),) + self.shape[1:]
        self.mix_rows = self.mix_cnt = None
        self._upload_mix()
        return new_labels


class StartWindowSet(WindowSet):
    """The ``WindowSet`` of ``stage_windows(starts=)``: a window is ``channel`` CONSECUTIVE rows, ``rows`` the int64 device
    table of first rows, and the only kind that can be displaced (``jitter``: every window moved a few TRs inside its run, a
    new row table, not a new array).  The mix table of a plan holds the first rows of every source."""

    def __init__(self, owner, planes, run_lengths, run_starts, M, C, offsets=None):
        run_starts = [np.asarray(s, np.int64) for s in run_starts]
        WindowSet.__init__(self, owner, planes, run_lengths, [len(s) for s in run_starts], M, C, offsets)
        self.base_rows, self.lo, self.hi = row_table(self.run_lengths, run_starts, C, self.run_offsets)
        self.rows_host = self.base_rows.copy()
        self.rows = torch.as_tensor(self.rows_host).to(planes.device)
        self.jitter, self.jitter_rng = 0, None
        self.aug_rows = None            # augment(time_shift=True): int64 device [copies * S]

    @property
    def starts(self):
        """The start of every window inside its run, as currently in use (after a displacement: the displaced ones)."""
        return self.rows_host - self.offsets

    def _keys(self):
        return self.rows_host

    def _originals(self, series, rows):
        return series[:, rows[:, None] + np.arange(self.shape[2])[None, :]]

    def _stats(self):
        planes, delta = self._stat_planes()
        rows = torch.as_tensor(self.base_rows + np.repeat(delta, self.run_windows)).to(self.planes.device)
        return ops.window_stats(planes, rows, *self.shape[1:])

    def _view(self, windows, lengths, offsets, counts):
        starts = np.split((self.base_rows - self.offsets)[windows], np.cumsum(counts)[:-1])
        return StartWindowSet(self.owner, self.planes, lengths, starts, self.shape[1], self.shape[2], offsets)

    def _displaced(self):
        return bool(self.jitter) or not np.array_equal(self.rows_host, self.base_rows)

    def _gather(self, idx, scale, shift, out, sources):
        M, C = self.shape[1:]
        if self.plan is not None:
            return ops.gather_windows_mix(self.planes, self.mix_rows, self.mix_cnt, M, C, idx, scale, shift, out, sources=sources)
        return ops.gather_windows(self.planes, self.rows, M, C, idx, scale, shift, out)

    def _gather_shifted(self, idx, scale, shift, out):
        M, C = self.shape[1:]
        return ops.gather_windows_reflect(self.planes, self.aug_rows, self.aug_shifts, M, C, idx, scale, shift, out)

    def _aug_tables(self):
        """The rows of every augmented window (the row table once per copy, repeated on the device), indexed like the shifts."""
        shifted = self.aug is not None and self.aug['time_shift']
        self.aug_rows = self.rows.repeat(self.aug['copies']) if shifted else None

    def _mix_table(self, extra):
        """The originals at their rows in use (every entry), the extra windows at ``extra`` (None: their sources'
        undisplaced rows)."""
        src, S = self.plan['src'], self.shape_base[0]
        tab = np.empty(src.shape, np.int64)
        tab[:S] = self.rows_host[:, None]
        tab[S:] = self.base_rows[src[S:]] if extra is None else extra
        return tab

    def _plan_removed(self):
        self.rows.copy_(torch.as_tensor(self.rows_host))              # (displaced originals were uploaded in the mix table only)

    # ---------------------------------------------------------------- displaced starts

    def set_rows(self, rows_host):
        """Upload another row table (same length) into the device table in place."""
        self.rows_host = np.asarray(rows_host, np.int64).copy()
        self.rows.copy_(torch.as_tensor(self.rows_host))
        if self.plan is not None:
            self._upload_mix()
        self._aug_tables()

    def refill(self):
        """``WindowSet.refill``; with ``jitter > 0`` every window's start is redrawn around its undisplaced one and the table
        uploaded, once.  Returns the starts now in use.

        Of a balanced set the originals are displaced exactly as without the plan (the same ``jitter_rng`` draws, the same
        rows); then, out of the balancing stream, the plan is redrawn when ``resample`` is set and, with ``jitter > 0``, every
        source entry of the extra windows gets a displacement of its own, clipped to the source's run; the ``[S', smax]``
        table is uploaded once."""
        if not self.jitter:
            return WindowSet.refill(self)
        rows = jitter_rows(self.base_rows, self.lo, self.hi, self.jitter, self.jitter_rng)
        if self.plan is None:
            self.set_rows(rows)
        else:
            self.rows_host = rows
            self._redraw()
            e = self.plan['src'][self.shape_base[0]:]
            self._upload_mix(jitter_rows(self.base_rows[e], self.lo[e], self.hi[e], self.jitter, self.plan['rng']))
        self._aug_refill()
        return self.starts

    def reset_rows(self):
        self.jitter, self.jitter_rng = 0, None
        if not np.array_equal(self.rows_host, self.base_rows):
            self.set_rows(self.base_rows)
        elif self.plan is not None:
            self._upload_mix()


class EventWindowSet(WindowSet):
    """The ``WindowSet`` whose windows are LISTS of rows (``stage_windows(index=, fold=)``, ``stage_events``): ``index`` is the
    int64 device table ``[S, channel * fold]`` of global rows, channel ``c`` of window ``s`` the float32 mean of the rows
    ``index[s, f * channel + c]`` (chebgcn_gather_windows_indexed).  It cannot be displaced: ``jitter`` and ``set_rows`` raise
    a ``ValueError`` -- a displaced window leaves its trial.  The mix table of a plan holds the plan's sources themselves:
    they are places in ``index``."""

    def __init__(self, owner, planes, run_lengths, run_index, M, C, fold, offsets=None):
        run_index = [np.asarray(i, np.int64) for i in run_index]
        WindowSet.__init__(self, owner, planes, run_lengths, [len(i) for i in run_index], M, C, offsets)
        self.fold = int(fold)
        self.index_host = np.ascontiguousarray(np.concatenate(run_index) + self.offsets[:, None], np.int64)
        self.index = torch.as_tensor(self.index_host).to(planes.device)
        self.aug_index = None           # augment(time_shift=True): int64 device [copies * S, C * fold]

    @property
    def jitter(self):
        return 0

    @jitter.setter
    def jitter(self, j):
        if not _is_int(j) or j != 0:
            raise ValueError('jitter: the windows of an event design cannot be displaced (a displaced window leaves its '
                             'trial), got jitter = %r' % (j,))

    def set_rows(self, rows_host):
        raise ValueError('set_rows: the windows of an event design cannot be displaced')

    @property
    def starts(self):
        """The rows every window reads, inside its run: ``[S, channel * fold]``."""
        return self.index_host - self.offsets[:, None]

    def _keys(self):
        return np.arange(self.shape_base[0])

    def _originals(self, series, which):
        """The ``fold`` pieces added in ascending order and divided once."""
        C, idx = self.shape[2], self.index_host[which]
        piece = series[:, idx[:, :C]]                                                   # [M, S, C]
        for f in range(1, self.fold):
            piece = piece + series[:, idx[:, f * C:(f + 1) * C]]
        return piece / np.float32(self.fold) if self.fold > 1 else piece

    def _stats(self):
        planes, delta = self._stat_planes()
        if planes is self.planes:
            return ops.window_stats_indexed(planes, self.index, *self.shape[1:], self.fold)
        index = torch.as_tensor(self.index_host + np.repeat(delta, self.run_windows)[:, None]).to(self.planes.device)
        return ops.window_stats_indexed(planes, index, *self.shape[1:], self.fold)

    def _view(self, windows, lengths, offsets, counts):
        index = np.split(self.starts[windows], np.cumsum(counts)[:-1])
        return EventWindowSet(self.owner, self.planes, lengths, index, self.shape[1], self.shape[2], self.fold, offsets)

    def _gather(self, idx, scale, shift, out, sources):
        M, C = self.shape[1:]
        return ops.gather_windows_indexed(self.planes, self.index, M, C, self.fold, self.mix_rows, self.mix_cnt, idx, scale,
                                          shift, out, sources=sources)

    def _mix_table(self, extra):
        return self.plan['src']

    def _gather_shifted(self, idx, scale, shift, out):
        M, C = self.shape[1:]
        return ops.gather_windows_indexed(self.planes, self.aug_index, M, C, self.fold, None, None, idx, scale, shift, out)

    def _aug_tables(self):
        """The index table of every augmented window, its columns taken through the reflection on the host --
        ``idx'[i, f * C + c] = idx[i % S, f * C + rho(c + r_i)]`` -- and uploaded once: ``[copies * S, C * fold]``, read by
        chebgcn_gather_windows_indexed like any index table."""
        if self.aug is None or not self.aug['time_shift']:
            self.aug_index = None
            return
        n, C = self.shape[0], self.shape[2]
        cols = reflect_channels(C, self.aug['shifts'])                                  # [n, C]
        cols = (np.arange(self.fold)[None, :, None] * C + cols[:, None, :]).reshape(n, self.fold * C)
        tab = np.take_along_axis(self.index_host[np.arange(n) % self.shape_base[0]], cols, axis=1)
        if self.aug_index is None or tuple(self.aug_index.shape) != tab.shape:
            self.aug_index = torch.as_tensor(np.ascontiguousarray(tab)).to(self.planes.device)
        else:
            self.aug_index.copy_(torch.as_tensor(np.ascontiguousarray(tab)))


class Series(object):
    """``stage_windows`` / ``fit_series`` / ``stage_events`` / ``fit_events`` of ``base_model``.  Uses the model's
    ``_decode_args`` / ``_stage_series`` / ``_scale_tables`` (decode.Decode), its sizes and ``fit``."""

    window_scaler = None            # (scale, shift) [M, channel] fitted by fit_series(standardize=True), else None

    def _window_args(self, series, starts, scale, shift, what):
        runs, run_starts, _, scale, shift, _ = self._decode_args(series, starts, 1, scale, shift, 'auto', None, 'logits', what)
        _both_or_neither(scale, shift, what)
        return runs, run_starts, scale, shift

    def _stage_set(self, what, kind, runs, cut, scale=None, shift=None, **more):
        """The runs staged as planes and the set ``kind`` (a ``WindowSet`` class) over them; ``cut``: per run the starts or
        the index table of its windows."""
        if self.device.type != 'cuda':
            raise RuntimeError('%s: the model has no device to run on (%s)' % (what, self.device))
        M0, C = int(self._M0), int(self.channel)
        lengths = [int(r.shape[0]) for r in runs]
        planes = torch.empty((sum(lengths), ops.plane_stride(M0)), dtype=torch.float32, device=self.device)
        off = 0
        for r, T in zip(runs, lengths):
            self._stage_series(r, out=planes[off:off + T])
            off += T
        return kind(self, planes, lengths, cut, M0, C, **more).set_tables(scale, shift)

    def _check_runs(self, series, what):
        """``series`` as a list of ``[T, M]`` runs of at least one time point each (``decode.check_run``)."""
        return [check_run(r, int(self._M0), what, least=1) for r in run_list(series, what)]

    def _index_args(self, series, index, fold, scale, shift, what):
        """The arguments of ``stage_windows(index=)``, refused or returned as ``(runs, one int64 [S_r, Cin] table per run,
        fold, scale, shift)``."""
        runs = self._check_runs(series, what)
        M0, C = int(self._M0), int(self.channel)
        if not _is_int(fold) or not 1 <= fold <= 16:
            raise ValueError('%s: fold must be an int in [1, 16], got %r' % (what, fold))
        many = isinstance(series, (list, tuple))
        tables = list(index) if (many and isinstance(index, (list, tuple))) else [index]
        if len(tables) != len(runs) or (many and not isinstance(index, (list, tuple))):
            raise ValueError('%s: index must hold one [S_r, %d] table per run (%d runs)' % (what, C * fold, len(runs)))
        out = []
        for r, t in zip(runs, tables):
            a = np.asarray(t)
            if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != C * fold or a.dtype == np.bool_ \
                    or not np.issubdtype(a.dtype, np.integer):
                raise ValueError('%s: every index table must be a non-empty int array [S_r, channel * fold = %d * %d], got %s %s'
                                 % (what, C, fold, a.dtype, a.shape))
            a = a.astype(np.int64)
            T = int(r.shape[0])
            if a.min() < 0 or a.max() >= T:
                raise ValueError('%s: every row of an index table must satisfy 0 <= row < T = %d; got %d ... %d'
                                 % (what, T, a.min(), a.max()))
            out.append(a)
        _both_or_neither(scale, shift, what)
        return runs, out, int(fold), check_table(scale, 'scale', M0, C, what), check_table(shift, 'shift', M0, C, what)

    def stage_windows(self, series, starts=None, scale=None, shift=None, index=None, fold=1):
        """A ``WindowSet``: the windows ``x[v][c] = series[start + c][v]`` of one ``[T, M]`` run or a list of runs (``starts``:
        an array per run; any order, repeats allowed; None: every window, stride 1 -- ``decode_series``' rules), staged on
        the device once as planes.  ``fit`` / ``predict`` / ``evaluate`` / ``model_perf.test`` / ``model_perf.predict`` take
        it wherever they take ``[S, M, channel]`` data.  ``scale`` / ``shift`` ``[M, channel]``: every window is seen as
        ``x * scale + shift``.  Arguments are refused (``ValueError``) before anything touches the device.

        ``index`` (instead of ``starts``): one int table ``[S_r, channel * fold]`` per run -- a window is a LIST of rows of its
        run, ``x[v][c] = mean_f series[index[s, f * channel + c]][v]`` (rows may repeat, decrease or skip; ``fold`` in
        [1, 16]).  Returns an ``EventWindowSet`` (``events.match_events`` produces such tables; ``stage_events``)."""
        what = 'stage_windows'
        if index is not None:
            if starts is not None:
                raise ValueError('stage_windows: starts and index are mutually exclusive')
            runs, run_index, fold, scale, shift = self._index_args(series, index, fold, scale, shift, what)
            return self._stage_set(what, EventWindowSet, runs, run_index, scale, shift, fold=fold)
        if not (fold == 1 and not isinstance(fold, bool)):
            raise ValueError('stage_windows: fold goes with index (windows cut by starts have fold = 1), got %r' % (fold,))
        runs, run_starts, scale, shift = self._window_args(series, starts, scale, shift, what)
        return self._stage_set(what, StartWindowSet, runs, run_starts, scale, shift)

    def _event_args(self, series, label_runs, target_name, block_dura, match_kw, what):
        """``stage_events``' arguments matched and checked: ``(runs kept, their index tables, fold, labels int64 [S], kept)``."""
        from . import events
        runs = self._check_runs(series, what)
        many = isinstance(series, (list, tuple))
        if not many:
            label_runs = [label_runs]
        try:
            ev = events.match_events(label_runs, target_name, block_dura, **match_kw)
        except (TypeError, ValueError) as e:            # (TypeError: a keyword match_events does not take, jitter= among them)
            raise ValueError('%s: %s' % (what, e))
        if len(label_runs) != len(runs):
            raise ValueError('%s: %d runs but %d event designs' % (what, len(runs), len(label_runs)))
        for r, names in zip(runs, label_runs):
            if int(r.shape[0]) != len(names):
                raise ValueError('%s: a run of %d time points with a design of %d entries' % (what, int(r.shape[0]), len(names)))
        if ev.channel != int(self.channel):
            raise ValueError('%s: the model has channel = %d, block_dura // TRstep = %d // %d = %d'
                             % (what, int(self.channel), ev.block_dura, ev.fold, ev.channel))
        if not ev.kept:
            raise ValueError('%s: no run yields a window (no trial of %r of at least block_dura = %d TRs?)'
                             % (what, list(target_name), ev.block_dura))
        if len(ev.classes) > int(self.M[-1]):
            raise ValueError('%s: %d conditions but the model has %d classes' % (what, len(ev.classes), int(self.M[-1])))
        return [runs[k] for k in ev.kept], ev.index, ev.fold, np.concatenate(ev.labels), ev.kept

    def stage_events(self, series, label_runs, target_name, block_dura, **match_kw):
        """``(window_set, labels)`` of an event design: ``events.match_events(label_runs, target_name, block_dura,
        **match_kw)`` (the reference's ``matching_fmri_data_to_trials_event``; ``match_kw``: ``start_trial``, ``hrf_delay``,
        ``flag_event``, ``TRstep``, ``rest``) decides which rows every window reads, and the runs that yield windows are
        staged as an ``EventWindowSet``.  ``series``: one ``[T, M]`` run with one design, or a list of runs with a list of
        designs, each as long as its run.  ``labels``: int64, one per window, codes into ``sorted(set(target_name))``.  The
        model's ``channel`` must equal ``block_dura // TRstep`` (``ValueError``)."""
        runs, run_index, fold, labels, _ = self._event_args(series, label_runs, target_name, block_dura, match_kw,
                                                            'stage_events')
        return self._stage_set('stage_events', EventWindowSet, runs, run_index, fold=fold), labels

    def fit_events(self, train_series, train_label_runs, val_series, val_label_runs, target_name, block_dura, standardize=False,
                   sampling=0, seed=0, groups=None, best_checkpoint_dir=None, augment=0, drop_rate=0.0, time_shift=False,
                   drop_value=1.0, augment_seed=0, **match_kw):
        """``fit`` on event designs: both splits go through ``stage_events`` and ``fit`` runs on the two sets; returns what
        ``fit`` returns.  ``fit_series``' rules: with ``standardize`` the scaler is fitted on the training set's ORIGINAL
        windows (their folded values, chebgcn_window_stats_indexed) before balancing, the validation set takes the training
        tables, and ``model.window_scaler`` goes into the checkpoints; ``sampling = n > 0`` balances the training classes
        (``WindowSet.balance``; ``seed`` starts the balancing stream, ``groups``: one id per training run GIVEN -- runs that
        yield no window are dropped from it like from the set; None: every run its own); ``augment = n > 0`` trains on ``n``
        perturbed copies of the (balanced) training set (``fit_series``' ``augment``, ``drop_rate``, ``time_shift``,
        ``drop_value``, ``augment_seed``)."""
        what = 'fit_events'
        aug = self._augment_args(what, augment, drop_rate, time_shift, drop_value, augment_seed, sampling)
        tr = self._event_args(train_series, train_label_runs, target_name, block_dura, match_kw, what)
        va = self._event_args(val_series, val_label_runs, target_name, block_dura, match_kw, what)
        train_labels, val_labels = tr[3], va[3]
        if check_sampling(sampling, what):
            if groups is not None:
                n_given = len(train_series) if isinstance(train_series, (list, tuple)) else 1
                groups = _int_vector(groups, 'the sampling groups (one id per run)', what, n_given)[tr[4]]
            check_balance_args(what, train_labels, len(train_labels), sampling, seed, groups, len(tr[0]), False)
        ws_train = self._stage_set(what, EventWindowSet, tr[0], tr[1], fold=tr[2])
        ws_val = self._stage_set(what, EventWindowSet, va[0], va[1], fold=va[2])
        return self._fit_sets(ws_train, train_labels, ws_val, val_labels, standardize, best_checkpoint_dir,
                              (sampling, seed, groups), aug)

    @staticmethod
    def _augment_args(what, copies, drop_rate, time_shift, drop_value, seed, sampling):
        """``fit_series`` / ``fit_events``' augmentation arguments checked: ``augment``'s arguments from ``copies`` on."""
        aug = check_augment_args(what, copies, drop_rate, time_shift, drop_value, seed)
        if aug[0] and aug[2] and _is_int(sampling) and sampling:
            raise ValueError('%s: time_shift together with sampling is not served (the mix kernels average whole source '
                             'windows)' % what)
        return aug

    def _fit_sets(self, ws_train, train_labels, ws_val, val_labels, standardize, best_checkpoint_dir, plan, aug=None,
                  fitted=None):
        """The tail of ``fit_series`` / ``fit_events``: the scaler fitted on the training originals and shared, the classes
        balanced (``plan``: ``balance``'s arguments from ``sampling`` on), the balanced set augmented (``aug``: ``augment``'s
        arguments from ``copies`` on), ``fit``; the training set left as it was staged.  The validation set is never
        augmented.  ``fitted``: a set whose scaler both sets take over instead (cross-validation's pool scaler)."""
        self.window_scaler = None
        if fitted is not None:
            ws_train.share_tables(fitted)
            ws_val.share_tables(fitted)
            self.window_scaler = fitted.scaler
        elif standardize:
            self.window_scaler = ws_train.fit_scaler()
            ws_val.share_tables(ws_train)
        try:
            if plan[0]:
                train_labels = ws_train.balance(train_labels, *plan)
            if aug is not None and aug[0]:
                train_labels = ws_train.augment(train_labels, *aug)
            return self.fit(ws_train, train_labels, ws_val, val_labels, best_checkpoint_dir)
        finally:
            ws_train.augment(None, 0)
            if ws_train.jitter:
                ws_train.reset_rows()
            ws_train.balance(None, 0)

    def fit_series(self, train_series, train_starts, train_labels, val_series, val_starts, val_labels, standardize=False,
                   jitter=0, jitter_seed=0, best_checkpoint_dir=None, sampling=0, sampling_seed=0, sampling_groups=None,
                   resample=False, augment=0, drop_rate=0.0, time_shift=False, drop_value=1.0, augment_seed=0):
        """``fit`` on scans: both splits are staged as ``WindowSet``s (``stage_windows``' rules; labels one per window, runs in
        order, the starts of a run in the caller's order) and ``fit`` runs on them; returns what ``fit`` returns.

        * ``standardize``: the training set's per-vertex-and-channel ``scale = 1/std`` / ``shift = -mean/std`` are fitted on
          the device (``WindowSet.fit_scaler``), applied to both splits, kept as ``model.window_scaler`` (``[M, channel]``
          each; None without) and written into the checkpoints.  Pass them to ``decode_series(scale=, shift=)``.
        * ``jitter = j > 0``: each time ``fit`` refills its index deque (once per epoch) every training window's start is
          displaced by an integer from ``[-j, j]`` drawn out of ``np.random.RandomState(jitter_seed)`` and clipped so that the
          window stays inside its run.  Labels, validation windows and the scaler (fitted on the undisplaced windows) are
          unaffected; the global NumPy stream sees exactly the draws of ``fit``.  With ``record_fit``, ``fit_log['starts']``
          holds the starts of every refill.
        * ``sampling = n > 0``: the classes of the TRAINING set are balanced (``WindowSet.balance``, ``balance_plan``): every
          class with at most half the windows of the largest is topped up, with re-drawn windows of its own at ``n = 1`` and
          with synthetic windows at ``n >= 2`` (at most 16), each the mean of ``n`` same-class windows of randomly drawn groups
          (``sampling_groups``: one id per training run, e.g. its subject; None: every run its own), formed batch by batch
          on the device (chebgcn_gather_windows_mix).  The scaler is fitted before, on the originals.  All draws come out of
          ``np.random.RandomState(sampling_seed)``; ``resample`` redraws the plan at every refill; with ``jitter`` the
          originals move exactly as without balancing and every source of an extra window gets a displacement of its own out
          of the balancing stream.  ``fit`` then runs on ``S'`` windows; with ``record_fit``, ``fit_log['sources']`` holds
          ``(src, cnt)`` of every refill.  ``sampling = 0`` is the training without any of this, on the same kernels as
          before.  Under ``dist.DataParallel`` the ranks' ``S'`` may differ (they depend on each shard's labels); ``fit``'s
          check of equal training-set sizes then fires -- balance shards that come out equal, or balance before sharding.
        * ``augment = n > 0`` (at most 64): ``fit`` trains on ``n`` perturbed copies of the training set
          (``WindowSet.augment``; the reference's ``train_dataarg``), installed after the scaler is fitted (on the originals)
          and after balancing.  ``drop_rate``: ``int(drop_rate * M)`` vertices of every window, drawn with replacement, take
          ``drop_value`` in all channels before the scaler (chebgcn_window_drop).  ``time_shift``: every window is shifted by
          ``r`` in ``[0, channel)`` inside its symmetric reflection (chebgcn_gather_windows_reflect; not together with
          ``sampling``).  The draws are a function of ``(augment_seed, refill number, window index)`` alone and are redrawn
          at every refill: no copy is ever stored.  Labels follow the base window (the reference draws the source of a copy
          at random and repeats the labels: there they come apart).  With ``record_fit``, ``fit_log['augment']`` holds
          ``(refill number, shifts or None)`` of every refill.  ``augment = 0`` launches none of the new kernels."""
        what = 'fit_series'
        aug = self._augment_args(what, augment, drop_rate, time_shift, drop_value, augment_seed, sampling)
        check_jitter(jitter, 'fit_series: ')
        check_seed(jitter_seed, 'jitter_seed', what)
        tr = self._window_args(train_series, train_starts, None, None, what)
        va = self._window_args(val_series, val_starts, None, None, what)
        for (runs, run_starts, _, _), labels, name in ((tr, train_labels, 'train'), (va, val_labels, 'val')):
            n = sum(len(s) for s in run_starts)
            if np.ndim(labels) != 1 or len(labels) != n:
                raise ValueError('fit_series: %s_labels must be one label per window (%d), got shape %s'
                                 % (name, n, np.shape(labels)))
        if check_sampling(sampling, what):
            train_labels, _ = check_balance_args(what, train_labels, len(train_labels), sampling, sampling_seed,
                                                 sampling_groups, len(tr[0]), resample)
        ws_train = self._stage_set(what, StartWindowSet, tr[0], tr[1])
        ws_val = self._stage_set(what, StartWindowSet, va[0], va[1])
        ws_train.jitter, ws_train.jitter_rng = int(jitter), np.random.RandomState(int(jitter_seed))
        return self._fit_sets(ws_train, train_labels, ws_val, val_labels, standardize, best_checkpoint_dir,
                              (sampling, sampling_seed, sampling_groups, resample), aug)

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
