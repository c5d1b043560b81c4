"""Subject-level splits of a list of runs: ``subject_folds`` holds out test subjects and draws the train / validation folds of
the rest -- the rule of the reference's ``subject_cross_validation_split_trials_event``
(HCP_task_fmri_gcn_test8.py:1168, 1272, 1299-1304: ``train_test_split`` over the subjects, then ``ShuffleSplit`` over the
remaining ones), restated on ``np.random.RandomState`` so that it does not move with scikit-learn.  Host only, NumPy only; the
global NumPy stream is never touched.

Departure from the reference, on purpose: where its ``train_test_split`` fails it falls back to "all subjects for training and
testing" (:1273-1276) -- test subjects the model was trained on.  Here a split that cannot be made is a ``ValueError``."""
import math

import numpy as np

SCHEMES = ('shuffle', 'kfold')


class SubjectFolds(object):
    """What ``subject_folds`` returns.  Subjects are numbered in order of first appearance in ``groups``; every ``*_runs`` entry
    is an int64 array of positions into the runs given, the subjects of the set in the split's order and the runs of one
    subject in the order given.

    * ``subjects``: the subject ids, by number; ``run_subjects`` int64: the subject number of every run;
    * ``test_subjects`` / ``test_runs``; ``pool_subjects`` / ``pool_runs`` (every subject that is not a test subject);
    * ``fold_subjects`` / ``folds``: per fold ``(train, val)``;
    * ``scheme``, ``seed``."""

    def __init__(self, subjects, run_subjects, test_subjects, pool_subjects, fold_subjects, scheme, seed):
        self.subjects, self.run_subjects = list(subjects), np.asarray(run_subjects, np.int64)
        self.scheme, self.seed = scheme, int(seed)
        self.test_subjects = np.asarray(test_subjects, np.int64)
        self.pool_subjects = np.asarray(pool_subjects, np.int64)
        self.fold_subjects = [(np.asarray(t, np.int64), np.asarray(v, np.int64)) for t, v in fold_subjects]
        self.test_runs, self.pool_runs = self.runs_of(self.test_subjects), self.runs_of(self.pool_subjects)
        self.folds = [(self.runs_of(t), self.runs_of(v)) for t, v in self.fold_subjects]

    def __len__(self):
        return len(self.folds)

    def runs_of(self, subjects):
        """The runs of ``subjects`` (numbers): subject by subject in the order given, a subject's runs in the order given."""
        runs = [np.flatnonzero(self.run_subjects == s) for s in np.asarray(subjects, np.int64)]
        return np.concatenate(runs).astype(np.int64) if runs else np.zeros(0, np.int64)


def number_subjects(groups, n_runs=None, what='subject_folds'):
    """``(subjects, run_subjects)``: the distinct ids of ``groups`` (one int or str per run) in order of first appearance and
    the number of every run's subject, int64.  ``groups = None``: every one of the ``n_runs`` runs is its own subject."""
    if groups is None:
        if isinstance(n_runs, bool) or not isinstance(n_runs, (int, np.integer)) or n_runs < 1:
            raise ValueError('%s: without groups the number of runs must be given (n_runs, an int >= 1), got %r' % (what, n_runs))
        return list(range(int(n_runs))), np.arange(int(n_runs), dtype=np.int64)
    if isinstance(groups, (str, bytes)):
        raise ValueError('%s: groups must hold one subject id per run, got %r' % (what, groups))
    try:
        a = np.asarray(groups)
    except Exception:
        a = None
    if a is None or a.ndim != 1 or a.size == 0 or a.dtype.kind not in 'iuUS' or (n_runs is not None and len(a) != int(n_runs)):
        raise ValueError('%s: groups must hold one subject id (int or str) per run%s, got %s'
                         % (what, '' if n_runs is None else ' (%d runs)' % int(n_runs),
                            'an object of type %s' % type(groups).__name__ if a is None else '%s %s' % (a.dtype, a.shape)))
    ids, first, inverse = np.unique(a, return_index=True, return_inverse=True)
    rank = np.empty(len(ids), np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(ids))
    subjects = [ids[i].item() for i in np.argsort(first, kind='stable')]
    return subjects, rank[np.asarray(inverse).reshape(-1)].astype(np.int64)


def _share(v, name, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) < 1.0:
        raise ValueError('%s: %s must be a number in [0, 1), got %r' % (what, name, v))
    return float(v)


def check_fold_args(n_folds, test_size, val_size, seed, scheme, what='subject_folds'):
    """Everything about a split that can be refused without knowing the subjects; returns the arguments as plain values."""
    if scheme not in SCHEMES:
        raise ValueError('%s: scheme must be one of %s, got %r' % (what, SCHEMES, scheme))
    if isinstance(n_folds, (bool, np.bool_)) or not isinstance(n_folds, (int, np.integer)) or n_folds < 1:
        raise ValueError('%s: n_folds must be an int >= 1, got %r' % (what, n_folds))
    test_size, val_size = _share(test_size, 'test_size', what), _share(val_size, 'val_size', what)
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
        raise ValueError('%s: the split seed must be an int in [0, 2**32) (np.random.RandomState), got %r' % (what, seed))
    return int(n_folds), test_size, val_size, int(seed), scheme


def subject_folds(groups, n_folds=10, test_size=0.2, val_size=0.1, seed=123, scheme='shuffle', n_runs=None):
    """Hold out test subjects, then draw ``n_folds`` train / validation splits of the remaining ones: a ``SubjectFolds``.

    ``groups``: one subject id per run (ints or strings); None: each of the ``n_runs`` runs is its own subject.  With ``n``
    subjects and ``rs = np.random.RandomState(seed)``: ``n_test = ceil(test_size * n)``, ``p = rs.permutation(n)``,
    ``test = p[:n_test]``, ``pool = p[n_test:]`` (``test_size = 0``: no test subject).

    * ``scheme='shuffle'`` (the reference's): ``n_val = ceil(val_size * len(pool))`` and per fold one
      ``q = rs.permutation(len(pool))``, ``val = pool[q[:n_val]]``, ``train = pool[q[n_val:]]`` -- what scikit-learn's
      ``train_test_split(range(n), test_size=, random_state=rs)`` followed by ``ShuffleSplit(n_folds, test_size=val_size,
      random_state=rs).split(pool)`` on the same ``rs`` give;
    * ``scheme='kfold'``: one ``q = rs.permutation(len(pool))``; ``np.array_split(q, n_folds)`` are the validation parts, so
      every pool subject validates exactly once, and a fold trains on the rest in ``q``'s order (``val_size`` plays no part;
      ``n_folds = len(pool)`` leaves one subject out).

    ``ValueError``: a non-empty test set or a pool of fewer than 2 subjects (where the reference falls back to training and
    testing on everyone, :1273-1276), a validation side of fewer than 1 subject
    (``val_size = 0``) or a training side of fewer than 1, ``n_folds < 1``, ``'kfold'`` with more folds than pool subjects,
    sizes outside [0, 1), a seed outside ``RandomState``'s range.  Nothing falls back to an overlapping split."""
    what = 'subject_folds'
    n_folds, test_size, val_size, seed, scheme = check_fold_args(n_folds, test_size, val_size, seed, scheme, what)
    subjects, run_subjects = number_subjects(groups, n_runs, what)
    n = len(subjects)
    rs = np.random.RandomState(seed)
    n_test = int(math.ceil(test_size * n))
    p = rs.permutation(n)
    test, pool = p[:n_test], p[n_test:]
    if len(pool) < 2 or len(test) == 1:
        raise ValueError('%s: %d subjects with test_size = %r give %d test subjects and a pool of %d; a test set that is not '
                         'empty and the pool need 2 each (the reference trains and tests on all subjects here: refused)'
                         % (what, n, test_size, len(test), len(pool)))
    folds = []
    if scheme == 'shuffle':
        n_val = int(math.ceil(val_size * len(pool)))
        if n_val < 1 or len(pool) - n_val < 1:
            raise ValueError('%s: val_size = %r of a pool of %d subjects gives %d validation and %d training subjects; both '
                             'sides need 1' % (what, val_size, len(pool), n_val, len(pool) - n_val))
        for _ in range(n_folds):
            q = rs.permutation(len(pool))
            folds.append((pool[q[n_val:]], pool[q[:n_val]]))
    else:
        if n_folds > len(pool):
            raise ValueError('%s: kfold with n_folds = %d over a pool of %d subjects' % (what, n_folds, len(pool)))
        if n_folds < 2:
            raise ValueError('%s: kfold with n_folds = 1 leaves no subject to train on' % what)
        q = rs.permutation(len(pool))
        parts = np.array_split(q, n_folds)
        for f, part in enumerate(parts):
            rest = np.concatenate([x for g, x in enumerate(parts) if g != f])
            folds.append((pool[rest], pool[part]))
    return SubjectFolds(subjects, run_subjects, test, pool, folds, scheme, seed)
