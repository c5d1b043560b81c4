"""Subject-level cross-validation on ONE staged copy of the scans: ``cross_validate_series`` / ``cross_validate_events`` of
``base_model`` (``CrossValidate`` is a base of it) and what they return, ``CVResult``.

The reference's main experiment (HCP_task_fmri_gcn_test8.py: ``build_graph_cnn_subject_validation`` :1849-2010 over
``subject_cross_validation_split_trials_event`` :1159-1394) holds out test subjects, draws ``n_folds`` train / validation
splits of the rest, fits one scaler and runs ``model_perf.test`` once per fold, on ``n_folds + 1`` scaled copies of the data.
Here every run is staged once (``stage_events`` / ``stage_windows``), ``splits.subject_folds`` decides the folds, and a fold is
a pair of views (``WindowSet.select``): row tables over the same planes.  There is no kernel of its own in this: a fold runs
the training step and the gather, statistics and mix kernels the sets already have, bit for bit what ``fit_events`` /
``fit_series`` on the fold's runs compute."""
import os

import numpy as np
import torch

from . import ops, splits
from .series import EventWindowSet, StartWindowSet, _int_vector, check_jitter, check_sampling, check_seed

SCALERS = ('pool', 'fold')


class FoldResult(object):
    """One fold of a ``CVResult``: ``train_runs`` / ``val_runs`` (positions into the runs kept), ``fit_accuracies`` /
    ``fit_losses`` / ``t_step`` (what ``fit`` returned), ``train`` / ``test`` ``(accuracy, f1, loss)`` of ``evaluate`` on the
    training originals and on the test set, ``test_logits`` float32 ``[W_test, classes]`` of the same restored variables,
    ``window_scaler`` and ``checkpoint_dir`` (what ``model_perf.predict`` and the ``*_maps`` restore from)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class CVResult(object):
    """What ``cross_validate_series`` / ``cross_validate_events`` return: ``split`` (the ``splits.SubjectFolds`` over the runs
    kept), ``labels`` (one per window of the staged set), ``test_labels``, ``folds`` (a ``FoldResult`` each).  Without a test
    set ``test_labels`` and every fold's ``test`` / ``test_logits`` are None."""

    def __init__(self, split, labels, test_labels, folds):
        self.split, self.labels, self.test_labels, self.folds = split, labels, test_labels, folds

    def summary(self):
        """The reference's report (:2008-2010) as a dict: the mean over the folds of the training accuracy
        (``train_accuracy``), of the test accuracy (``test_accuracy``, None without a test set) and of the PEAK validation
        accuracy of every fold's ``fit`` (``val_accuracy``), and the population standard deviation of each (``*_std``)."""
        out = {}
        cols = (('train_accuracy', [f.train[0] for f in self.folds]),
                ('test_accuracy', [f.test[0] for f in self.folds] if self.test_labels is not None else None),
                ('val_accuracy', [np.max(f.fit_accuracies) for f in self.folds]))
        for name, v in cols:
            out[name] = None if v is None else float(np.mean(v))
            out[name + '_std'] = None if v is None else float(np.std(v))
        return out

    def ensemble(self):
        """The folds as an ensemble on the test set: ``(MCResult, accuracy in percent)`` -- ``ops.mc_reduce``
        (chebgcn_mc_reduce) over the stacked ``test_logits`` ``[n_folds, W_test, classes]``, the folds' models in place of
        dropout samples: mean probabilities, labels, entropy, expected entropy, mutual information, votes, agreement."""
        from .uncertainty import MCResult
        if self.test_labels is None:
            raise ValueError('ensemble: the cross-validation held out no test set')
        z = np.stack([np.asarray(f.test_logits, np.float32) for f in self.folds])
        if not 1 <= z.shape[0] <= ops.MC_SAMPLES_MAX or not 1 <= z.shape[2] <= ops.MC_CLASSES_MAX:
            raise ValueError('ensemble: %d folds of %d classes are outside what chebgcn_mc_reduce serves (%d members, %d '
                             'classes)' % (z.shape[0], z.shape[2], ops.MC_SAMPLES_MAX, ops.MC_CLASSES_MAX))
        red = ops.mc_reduce(torch.as_tensor(z).to(torch.device('cuda', torch.cuda.current_device())))
        res = MCResult((k, v.cpu().numpy()) for k, v in red.items())
        res['labels'] = res['labels'].astype(np.int64)
        return res, 100.0 * float(np.mean(res['labels'] == np.asarray(self.test_labels)))


class CrossValidate(object):
    """``cross_validate_series`` / ``cross_validate_events`` of ``base_model``.  Uses ``series.Series`` (``_event_args``,
    ``_window_args``, ``_stage_set``, ``_fit_sets``), the model's ``evaluate``, ``_gather_padded`` / ``_inference_storage``
    and its ``dir_name``."""

    def _cv_args(self, what, n_given, groups, n_folds, test_size, val_size, split_seed, scheme, standardize, scaler, fold_seed,
                 sampling, seeds):
        """What both methods check alike, before any device work; returns the subject id of every run given (an array)."""
        if self._dp is not None:
            raise NotImplementedError('%s: under dist.DataParallel (folds over ranks) is not served' % what)
        n_folds = splits.check_fold_args(n_folds, test_size, val_size, split_seed, scheme, what)[0]
        if not isinstance(standardize, (bool, np.bool_)):
            raise ValueError('%s: standardize must be a bool, got %r' % (what, standardize))
        if scaler not in SCALERS:
            raise ValueError('%s: scaler must be one of %s, got %r' % (what, SCALERS, scaler))
        if fold_seed is not None:
            check_seed(fold_seed, 'fold_seed', what)
            check_seed(fold_seed + n_folds - 1, 'fold_seed + the last fold', what)
        check_sampling(sampling, what)
        for name, v in seeds:
            check_seed(v, name, what)
            check_seed(v + n_folds - 1, name + ' + the last fold', what)
        splits.number_subjects(groups, n_given, what)
        return np.arange(n_given) if groups is None else np.asarray(groups)

    def _cv_split(self, what, subject_of_run, kept, n_folds, test_size, val_size, split_seed, scheme):
        """The folds over the runs kept (a subject left without runs drops out before the split)."""
        try:
            return splits.subject_folds(subject_of_run[np.asarray(kept, np.int64)], n_folds, test_size, val_size, split_seed,
                                        scheme)
        except ValueError as e:
            raise ValueError('%s: %s' % (what, e))

    def _cv_logits(self, data):
        """The logits of every window of ``data``, batch by batch as ``predict`` runs them (the last batch padded to
        ``batch_size``): float32 ``[S, classes]``."""
        data_dev = self.stage(data)
        size = data_dev.shape[0]
        out = np.empty((size, int(self.M[-1])), np.float32)
        was_training = self.training_mode
        self.training_mode = False
        try:
            for begin in range(0, size, self.batch_size):
                end = min(begin + self.batch_size, size)
                idx = torch.as_tensor(np.arange(begin, end), dtype=torch.int32).to(self.device)
                x = self.as_internal(self._gather_padded(data_dev, idx, self.batch_size))
                with torch.no_grad():
                    out[begin:end] = self._inference_storage(x, 1)[:end - begin].float().cpu().numpy()
        finally:
            self.training_mode = was_training
        return out

    def _cv_folds(self, full, labels, split, standardize, scaler, fold_seed, target_names, plan_of, aug_of, jitter_of=None):
        """The folds of ``split`` over the views of ``full``: per fold what ``model_perf.test`` does -- ``fit`` on the fold's
        (train view, val view) through ``_fit_sets``, then ``evaluate`` on the training view's originals and on the test
        view -- under ``<dir_name>/fold<f>``.  ``plan_of(f, train_runs)`` / ``aug_of(f)`` / ``jitter_of(f)``: fold ``f``'s
        arguments of ``balance`` (from ``sampling`` on), of ``augment`` (from ``copies`` on) and ``(jitter, rng)``."""
        labels = np.asarray(labels)
        fitted = None
        if standardize and scaler == 'pool':
            fitted = full.select(split.pool_runs)
            fitted.fit_scaler()
        test = test_labels = None
        if len(split.test_runs):
            test, test_labels = full.select(split.test_runs), labels[full.windows_of(split.test_runs)]
        base_dir, folds = self.dir_name, []
        try:
            for f, (train_runs, val_runs) in enumerate(split.folds):
                self.dir_name = os.path.join(base_dir, 'fold%d' % f)
                train, val = full.select(train_runs), full.select(val_runs)
                train_labels, val_labels = labels[full.windows_of(train_runs)], labels[full.windows_of(val_runs)]
                if jitter_of is not None:
                    train.jitter, train.jitter_rng = jitter_of(f)
                if fold_seed is not None:
                    np.random.seed(fold_seed + f)
                accuracies, losses, t_step = self._fit_sets(train, train_labels, val, val_labels,
                                                            standardize and scaler == 'fold', None, plan_of(f, train_runs),
                                                            aug_of(f), fitted=fitted)
                res = FoldResult(train_runs=train_runs, val_runs=val_runs, fit_accuracies=accuracies, fit_losses=losses,
                                 t_step=t_step, test=None, test_logits=None, checkpoint_dir=self._get_path('checkpoints'))
                res.train = tuple(self.evaluate(train, train_labels, target_name=target_names)[1:])
                if test is not None:
                    test.share_tables(train)
                    res.test = tuple(self.evaluate(test, test_labels, target_name=target_names)[1:])
                    res.test_logits = self._cv_logits(test)
                res.window_scaler = self.window_scaler
                folds.append(res)
        finally:
            self.dir_name = base_dir
        return CVResult(split, labels, test_labels, folds)

    def cross_validate_events(self, series, label_runs, target_name, block_dura, groups=None, n_folds=10, test_size=0.2,
                              val_size=0.1, split_seed=123, scheme='shuffle', standardize=False, scaler='pool', fold_seed=None,
                              target_names=None, sampling=0, seed=0, augment=0, drop_rate=0.0, time_shift=False, drop_value=1.0,
                              augment_seed=0, **match_kw):
        """The reference's subject-level cross-validation (``subject_cross_validation_split_trials_event`` +
        ``model_perf.test`` per fold) on event designs, every run staged ONCE: returns a ``CVResult``.

        ``series`` / ``label_runs`` / ``target_name`` / ``block_dura`` / ``match_kw``: ``stage_events``' (all runs of all
        subjects).  ``groups``: one subject id (int or str) per run GIVEN (None: every run its own subject); runs that yield no
        window drop out of it as in ``fit_events``, a subject left without runs drops out before the split.
        ``splits.subject_folds(groups, n_folds, test_size, val_size, split_seed, scheme)`` decides the test subjects and the
        folds; every set of a fold is a view of the one staged set (``WindowSet.select``).

        * ``standardize``: with ``scaler='pool'`` (the reference, :1290) one scaler is fitted on the windows of all non-test
          subjects and shared by every view; with ``scaler='fold'`` each fold fits its own on its training view
          (``fit_events``' rule: no validation subject leaks into it).  Either way ``model.window_scaler`` is set per fold
          and goes into that fold's checkpoints.
        * per fold ``f``: ``fit`` on (train view, val view) with the plan (``sampling``, ``seed + f``, the subjects of the
          training runs as groups) and the augmentation (``augment``, ``drop_rate``, ``time_shift``, ``drop_value``,
          ``augment_seed + f``) on the training view only, removed afterwards also when ``fit`` raises; then ``evaluate`` on
          the training view's originals and on the test view (``target_names`` is its ``target_name``), from the latest
          checkpoint as always.  ``fold_seed``: an int calls ``np.random.seed(fold_seed + f)`` before the fold's ``fit``;
          None leaves the global stream alone, as the reference does.
        * during fold ``f`` the model's ``dir_name`` is ``<dir_name>/fold<f>``: one checkpoint directory per fold
          (``FoldResult.checkpoint_dir``); ``dir_name`` is restored afterwards, also on an exception.

        Every argument is checked before anything touches the device; under ``dist.DataParallel``:
        ``NotImplementedError``."""
        what = 'cross_validate_events'
        n_given = len(series) if isinstance(series, (list, tuple)) else 1
        subject_of_run = self._cv_args(what, n_given, groups, n_folds, test_size, val_size, split_seed, scheme, standardize,
                                       scaler, fold_seed, sampling, (('seed', seed), ('augment_seed', augment_seed)))
        aug = self._augment_args(what, augment, drop_rate, time_shift, drop_value, augment_seed, sampling)
        runs, run_index, fold, labels, kept = self._event_args(series, label_runs, target_name, block_dura, match_kw, what)
        split = self._cv_split(what, subject_of_run, kept, n_folds, test_size, val_size, split_seed, scheme)
        full = self._stage_set(what, EventWindowSet, runs, run_index, fold=fold)
        return self._cv_folds(full, labels, split, standardize, scaler, fold_seed, target_names,
                              lambda f, train_runs: (sampling, seed + f, split.run_subjects[train_runs]),
                              lambda f: aug[:4] + (augment_seed + f,))

    def cross_validate_series(self, series, starts, labels, groups=None, n_folds=10, test_size=0.2, val_size=0.1,
                              split_seed=123, scheme='shuffle', standardize=False, scaler='pool', fold_seed=None,
                              target_names=None, sampling=0, seed=0, augment=0, drop_rate=0.0, time_shift=False, drop_value=1.0,
                              augment_seed=0, jitter=0, jitter_seed=0, resample=False):
        """``cross_validate_events`` for windows cut by starts: ``series`` / ``starts`` / ``labels`` as ``fit_series`` takes
        one split's (a list of runs, an array of starts per run or None, one label per window), ``groups`` one subject id per
        run.  ``jitter`` displaces fold ``f``'s training windows out of ``np.random.RandomState(jitter_seed + f)``
        (``fit_series``' rule), ``resample`` redraws the plan at every refill; everything else as there."""
        what = 'cross_validate_series'
        n_given = len(series) if isinstance(series, (list, tuple)) else 1
        subject_of_run = self._cv_args(what, n_given, groups, n_folds, test_size, val_size, split_seed, scheme, standardize,
                                       scaler, fold_seed, sampling,
                                       (('seed', seed), ('augment_seed', augment_seed), ('jitter_seed', jitter_seed)))
        aug = self._augment_args(what, augment, drop_rate, time_shift, drop_value, augment_seed, sampling)
        jitter = check_jitter(jitter, what + ': ')
        if not isinstance(resample, (bool, np.bool_)):
            raise ValueError('%s: resample must be a bool, got %r' % (what, resample))
        runs, run_starts, _, _ = self._window_args(series, starts, None, None, what)
        n = sum(len(s) for s in run_starts)
        if np.ndim(labels) != 1 or len(labels) != n:
            raise ValueError('%s: labels must be one label per window (%d), got shape %s' % (what, n, np.shape(labels)))
        if sampling:
            labels = _int_vector(labels, 'labels', what, n)
        split = self._cv_split(what, subject_of_run, np.arange(len(runs)), n_folds, test_size, val_size, split_seed, scheme)
        full = self._stage_set(what, StartWindowSet, runs, run_starts)
        return self._cv_folds(full, labels, split, standardize, scaler, fold_seed, target_names,
                              lambda f, train_runs: (sampling, seed + f, split.run_subjects[train_runs], bool(resample)),
                              lambda f: aug[:4] + (augment_seed + f,),
                              lambda f: (jitter, np.random.RandomState(jitter_seed + f)))
