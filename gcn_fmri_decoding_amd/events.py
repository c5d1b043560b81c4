"""Event designs to windows: ``match_events`` turns the per-TR condition names of every run into the table of rows each
trial-aligned window reads -- the reference's ``matching_fmri_data_to_trials_event`` (utils.py:423-525) without the data.

The reference indexes the scan itself (NumPy fancy indexing, ``np.split``, ``take(mode='clip')``, ``array_split`` + ``mean``)
and returns ``[S, M, block_dura // TRstep]`` arrays.  Every one of those steps only SELECTS rows of the run, so the same rules
applied to ``arange(T)`` give, per window, the ``block_dura`` rows it is made of; ``stage_windows(index=, fold=)`` cuts the
windows out of the staged scan on the device from that table (chebgcn_gather_windows_indexed).  NumPy only."""
import warnings

import numpy as np

FOLD_MAX = 16                  # TRstep at most (the indexed gather holds fold in [1, 16])


class EventWindows(object):
    """What ``match_events`` returns.

    * ``kept``: the indices of the runs that yield windows (a run with no trial left is skipped), ascending;
    * ``index``: per kept run int64 ``[S_r, block_dura]`` -- the rows OF THAT RUN every window reads.  With ``fold > 1`` channel
      ``c`` of a window is the mean of the rows ``index[s, f * channel + c]``, ``f < fold``;
    * ``labels``: per kept run int64 ``[S_r]``, codes into ``classes = sorted(set(target_name))`` (sklearn's LabelEncoder);
    * ``trial_dura``: the shortest trial of the last kept run (the reference's ``Trial_dura``), 0 when no run is kept;
    * ``fold = TRstep``, ``channel = block_dura // TRstep``, ``block_dura``."""

    def __init__(self, kept, index, labels, trial_dura, fold, channel, block_dura, classes):
        self.kept, self.index, self.labels = kept, index, labels
        self.trial_dura, self.fold, self.channel, self.block_dura = int(trial_dura), int(fold), int(channel), int(block_dura)
        self.classes = classes

    def __len__(self):
        return int(sum(len(l) for l in self.labels))


def _int(v, name, least=None, most=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) \
            or (least is not None and v < least) or (most is not None and v > most):
        span = '' if least is None else (' >= %d' % least if most is None else ' in [%d, %d]' % (least, most))
        raise ValueError('match_events: %s must be an int%s, got %r' % (name, span, v))
    return int(v)


def match_events(label_runs, target_name, block_dura, start_trial=0, hrf_delay=0, flag_event=0, TRstep=1, rest='rest'):
    """The windows of an event design, as rows: an ``EventWindows``.

    ``label_runs``: one sequence of per-TR condition names per run.  ``target_name``: the conditions to keep.  The rules are
    those of the reference's ``matching_fmri_data_to_trials_event`` (utils.py:423-525), rule for rule:

    * ``hrf_delay > 0``: the design is shifted right with ``np.roll`` (:435-437), which wraps around the end of the run;
      a value <= 0 shifts nothing (the reference tests ``> 0``);
    * a TR is kept when its condition is in ``target_name`` (:438).  ``start_trial > 0``: the mask and the mask of the design
      rolled by ``start_trial`` are ANDed (:446-447: every trial loses its first TRs); ``start_trial < 0``: they are ORed and
      every ``rest`` entry takes the rolled label (:443-445: every trial starts earlier).  A kept TR whose label is not in
      ``target_name`` is a ``ValueError`` (the reference's LabelEncoder raises there, :457);
    * the run is COMPRESSED to the kept TRs (:451-452) and then split where the encoded label changes (:460-461): two trials
      of the same condition separated only by dropped TRs merge into one block, and a window may straddle the gap;
    * the last block is dropped when it is shorter than ``block_dura`` or than 4 TRs (:467-469); a run with no block left is
      skipped (:470-474);
    * a block of ``dura >= block_dura`` TRs gives ``dura // block_dura`` windows of consecutive kept TRs, the remainder is
      dropped (:499-502); a shorter block gives ONE window whose last TR repeats (``take(mode='clip')``, :494-498);
    * every window carries the label of its block's first TR (:498, :502), encoded as ``LabelEncoder().fit(target_name)``
      encodes it: the index into ``sorted(set(target_name))``;
    * ``TRstep > 1``: the window's time axis is cut into ``TRstep`` consecutive pieces that are averaged (:520-521): the
      table keeps all ``block_dura`` rows and ``fold = TRstep``.  ``block_dura % TRstep != 0`` is a ``ValueError`` (the
      reference's ``np.array_split`` would average ragged pieces).

    ``flag_event`` only silences the reference's warning about trials shorter than 5 TRs (:475-476), here a
    ``warnings.warn``.  Every malformed argument is a ``ValueError``."""
    block_dura = _int(block_dura, 'block_dura', 1)
    start_trial = _int(start_trial, 'start_trial')
    hrf_delay = _int(hrf_delay, 'hrf_delay')
    TRstep = _int(TRstep, 'TRstep', 1, FOLD_MAX)
    if isinstance(flag_event, (bool, np.bool_)):
        flag_event = int(flag_event)
    flag_event = _int(flag_event, 'flag_event', 0, 1)
    if block_dura % TRstep != 0:
        raise ValueError('match_events: block_dura = %d is not a multiple of TRstep = %d (the sub-windows would be ragged)'
                         % (block_dura, TRstep))
    if not isinstance(rest, str):
        raise ValueError('match_events: rest must be a condition name (str), got %r' % (rest,))
    if isinstance(target_name, str) or not hasattr(target_name, '__len__') or len(target_name) == 0 \
            or not all(isinstance(n, str) for n in target_name):
        raise ValueError('match_events: target_name must be a non-empty sequence of condition names (str), got %r'
                         % (target_name,))
    classes = sorted(set(str(n) for n in target_name))
    if isinstance(label_runs, (str, np.ndarray)) or not hasattr(label_runs, '__len__') or len(label_runs) == 0:
        raise ValueError('match_events: label_runs must be a non-empty list with one sequence of condition names per run')
    designs = []
    for r, names in enumerate(label_runs):
        a = np.asarray(names)
        if isinstance(names, str) or a.ndim != 1 or a.size == 0 or a.dtype.kind not in 'USO' \
                or (a.dtype.kind == 'O' and not all(isinstance(n, str) for n in a)):
            raise ValueError('match_events: run %d of label_runs must be a non-empty 1-d sequence of condition names (str), '
                             'got %s %s' % (r, a.dtype, a.shape))
        designs.append(a.astype(str))

    kept, index, labels = [], [], []
    trial_dura = 0
    for r, names in enumerate(designs):
        code = np.full(len(names), -1, np.int64)                # the encoded label of every TR, -1: not a target
        for i, n in enumerate(classes):
            code[names == n] = i
        is_rest = names == rest
        if hrf_delay > 0:
            code, is_rest = np.roll(code, hrf_delay), np.roll(is_rest, hrf_delay)
        mask = code >= 0
        if start_trial != 0:
            code_shift = np.roll(code, start_trial)
            if start_trial < 0:
                mask = np.logical_or(code_shift >= 0, mask)
                code[is_rest] = code_shift[is_rest]
            else:
                mask = np.logical_and(code_shift >= 0, mask)
        rows = np.flatnonzero(mask).astype(np.int64)            # the compressed run: what every later step indexes
        sel = code[rows]
        if (sel < 0).any():
            raise ValueError("match_events: run %d keeps a TR (start_trial = %d) whose condition %r is not in target_name"
                             % (r, start_trial, str(names[rows[np.flatnonzero(sel < 0)[0]]])))
        cuts = np.flatnonzero(np.diff(sel)) + 1
        blocks = np.split(rows, cuts)
        firsts = np.concatenate([[0], cuts]).astype(np.int64)
        duras = [len(b) for b in blocks]
        if duras[-1] < block_dura or duras[-1] < 4:
            duras = duras[:-1]
        if not duras:
            continue
        trial_dura = min(duras)
        if trial_dura < 5 and not flag_event:
            warnings.warn('match_events: run %d has trials of only %d TRs; recheck the event design' % (r, trial_dura))
        idx, lab = [], []
        for ti, dura in enumerate(duras):
            chunks = dura // block_dura
            if chunks < 1:
                idx.append(blocks[ti][np.minimum(np.arange(block_dura), dura - 1)][None, :])
                lab.append(sel[firsts[ti]:firsts[ti] + 1])
            else:
                idx.append(blocks[ti][:chunks * block_dura].reshape(chunks, block_dura))
                lab.append(np.repeat(sel[firsts[ti]], chunks))
        kept.append(r)
        index.append(np.ascontiguousarray(np.concatenate(idx), np.int64))
        labels.append(np.concatenate(lab).astype(np.int64))
    return EventWindows(kept, index, labels, trial_dura, TRstep, block_dura // TRstep, block_dura, classes)


def host_windows(run, index, fold=1):
    """The windows ``index`` (``[S, channel * fold]`` rows of ``run`` ``[T, M]``) as float32 ``[S, M, channel]``, formed like
    chebgcn_gather_windows_indexed forms them: the ``fold`` pieces added in float32 in ascending order, one rounded division
    when ``fold > 1``."""
    run = np.asarray(run, np.float32)
    index = np.asarray(index, np.int64)
    C = index.shape[1] // int(fold)
    x = run[index[:, :C]]                                       # [S, C, M]
    for f in range(1, int(fold)):
        x = x + run[index[:, f * C:(f + 1) * C]]
    if fold > 1:
        x = x / np.float32(fold)
    return np.ascontiguousarray(x.transpose(0, 2, 1), np.float32)
